"""CPU tests (no GPU): the loader's program check (ta_program_check, terran_amd/csrc/model_load.hip) -- everything about a
packed program that does not depend on an input shape is accepted or refused here, before a device is touched.

Every program the packer and the tests' hand-built helpers make passes; one small valid program, broken in exactly one way per
case by editing its packed records through pack.layout's dtypes, is refused with TA_E_INVALID and a message that names the defect.
`python -m tests.test_program_check_cpu --dump-blobs <dir>` writes every blob of the refusal cases, and 2 000 copies of the valid
one with one random 32-bit field of a random op or tensor record overwritten, to <dir>: the input of tools/program_check_main.cpp
(host sanitizers)."""
import os

import numpy as np
import pytest

from terran_amd import lib, pack
from terran_amd.pack import layout
from tests import util

KIND = pack.MODEL_OPENPOSE


# ---- well-formed programs -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('precision', sorted(layout.PRECISIONS))
@pytest.mark.parametrize('net', ['openpose', 'arcface', 'retinaface'])
@pytest.mark.parametrize('wild', [False, True], ids=['seeded', 'wild'])
def test_packed_networks_pass(states, net, precision, wild):
    sd = states(('wild_' if wild else '') + net)
    lib.check_program(getattr(pack, 'pack_' + net)(sd, precision))


def test_layerwise_detector_and_pack_switches_pass(states, monkeypatch):
    sd = states('retinaface')
    lib.check_program(pack.pack_retinaface(sd, 'f16x3', fused=False))
    for switch in pack.PACK_SWITCHES:
        monkeypatch.setenv(switch, '1')
        lib.check_program(pack.pack_retinaface(sd, 'f16x3'))
        lib.check_program(pack.pack_arcface(states('arcface'), 'f16x3'))
        monkeypatch.delenv(switch)


def test_hand_built_test_programs_pass():
    """The programs the GPU tests run, built by the same helpers (a small layer of every kind stands for the bench-sized ones)."""
    V = lib.CONV_VARIANTS
    layers = [dict(c1=192, cout=128, k=7), dict(c1=256, cout=256, k=7, groups=2), dict(c1=128, cout=128, k=3, stride=2, res=True, out2=True),
              dict(c1=128, cout=128, k=3, act=2), dict(c1=64, cout=64, k=3, act=1, pool=True),
              dict(c1=128, cout=38, k=1, out_total=192, out_off=128, cout_p=40)]
    for L in layers:
        for precision in ('f32', 'f16x3', 'bf16x3'):
            lib.check_program(util.conv_case_program(L, V['auto'], False, precision, False)[0])
        if L['cout'] % 32 == 0 and 'out_total' not in L:
            lib.check_program(util.conv_case_program(L, V['split_2x2'], False, 'f16x3', True)[0])
    lib.check_program(util.conv_case_program(layers[0], V['generic'], True, 'f32', False)[0])
    lib.check_program(util.fc_program(V['auto'], 'f16x3')[0])
    lib.check_program(util.pinned_variant_program(V['split_2x4']))        # refused by the forward (a launch record), not by the loader
    for L in (dict(c1=256, cout=256, k=3, act=2), dict(c1=256, cout=256, k=3, res=True), dict(c1=128, cout=128, k=5, act=1),
              dict(c1=256, cout=256, k=3, groups=2, act=1)):
        for precision in ('f16x3', 'f16x2'):
            for variant in ('split_2x2', 'win_2x2', 'auto'):
                lib.check_program(util.window_program(L, V[variant], precision, util.window_weights(L)))
    for C, cout, stride, split_out in ((64, 128, 2, False), (256, 256, 1, True), (96, 40, 1, False)):
        lib.check_program(util.dwpw_block_program(C, cout, stride, split_out))
    lib.check_program(util.two_conv_program())
    lib.check_program(_f16_program())


# ---- refusals -------------------------------------------------------------------------------------------------------------------
class Blob:
    """The bytes of a packed program with its three tables open for editing."""

    def __init__(self, blob):
        self.buf = bytearray(blob)
        self.hdr = np.frombuffer(self.buf, layout.HEADER_DT, 1)
        h = self.hdr[0]
        self.tensors = np.frombuffer(self.buf, layout.TENSOR_DT, int(h['n_tensors']), int(h['tensors_off']))
        self.ops = np.frombuffer(self.buf, layout.OP_DT, int(h['n_ops']), int(h['ops_off']))
        self.tables_end = int(h['ops_off']) + self.ops.nbytes
        self.weights_bytes = int(h['weights_bytes'])

    def bytes(self):
        return bytes(self.buf)


def _f16_program():
    return util.two_conv_program('f16', c=64)


def _lanes3():
    """util.lane_sharing_program with its last conv reading the main stream's tensor: a closed branch, accepted."""
    b = Blob(util.lane_sharing_program().blob())
    b.ops[2]['in'] = b.ops[1]['in']
    return b


def _detector(states):
    return Blob(pack.pack_retinaface(states('retinaface'), 'f32', fused=False).blob())


def _fused_detector(states):
    return Blob(pack.pack_retinaface(states('retinaface'), 'f32').blob())


def _op(field, value, op=1, base=None):
    def make(states):
        b = Blob((base or util.two_conv_program)().blob())
        b.ops[op][field] = value(b) if callable(value) else value
        return b
    return make


def _tensor(field, value, tensor, base=None):
    def make(states):
        b = Blob((base or util.two_conv_program)().blob())
        b.tensors[tensor][field] = value
        return b
    return make


def _hdr(field, value):
    def make(states):
        b = Blob(util.two_conv_program().blob())
        b.hdr[0][field] = value(b) if callable(value) else value
        return b
    return make


def _edit(fn, base=None):
    def make(states):
        b = base(states) if base else Blob(util.two_conv_program().blob())
        fn(b)
        return b
    return make


def _set(b, table, index, **fields):
    for k, v in fields.items():
        getattr(b, table)[index][k] = v


def _first(b, typ):
    return int(np.flatnonzero(b.ops['type'] == typ)[0])


def _dw_slice(b):
    b.ops[_first(b, pack.OP_DWCONV)]['in_ch_off'] = 4


def _front_not_shape_only(b):
    assert b.ops[0]['type'] == pack.OP_RFSTEM
    b.tensors[b.hdr[0]['input_tensor']]['alias_of'] = -1


def _outputs0(b):
    b.hdr[0]['outputs'][0] = b.hdr[0]['n_tensors']


past = lambda b: b.weights_bytes                          # noqa: E731  (an offset at the end of the weight region)
dwpw64 = lambda: util.dwpw_block_program(64, 64, 1, False)   # noqa: E731

# (id, blob maker, what the message must say)
REFUSALS = [
    # the loader's own
    ('magic', _hdr('magic', 0), 'magic'),
    ('version', _hdr('version', 8), 'version'),
    ('counts_no_ops', _hdr('n_ops', 0), 'bad counts'),
    ('counts_outputs', _hdr('n_outputs', 17), 'bad counts'),
    ('counts_input', _hdr('input_tensor', lambda b: b.hdr[0]['n_tensors']), 'bad counts'),
    ('truncated_tensors', _hdr('tensors_off', lambda b: len(b.buf) - 10), 'tensor table'),
    ('truncated_ops', _hdr('ops_off', lambda b: len(b.buf) - 10), 'op table'),
    ('truncated_weights', _hdr('weights_bytes', lambda b: b.weights_bytes + 1), 'weights'),
    ('negative_table_offset', _hdr('tensors_off', -20), 'tensor table'),
    ('w_off_past', _op('w_off', past), 'w_off'),
    ('bias_off_past', _op('bias_off', past), 'bias_off'),
    ('prelu_off_past', _op('prelu_off', past), 'prelu_off'),
    ('scale2_off_past', _op('scale2_off', past), 'scale2_off'),
    ('shift2_off_past', _op('shift2_off', past), 'shift2_off'),
    ('wus_off_not_behind_bias', _op('wus_off', lambda b: b.ops[1]['wus_off'] + 4), 'wus_off'),
    ('front_w_off_past', _edit(lambda b: _set(b, 'ops', 0, w_off=b.weights_bytes), lambda s: _fused_detector(s)), 'w_off'),
    ('dwpw_scale2_off_past', _op('scale2_off', past, base=dwpw64), 'scale2_off'),
    ('dwpw_shift2_off_past', _op('shift2_off', past, base=dwpw64), 'shift2_off'),
    ('depthwise_w_off_past', _edit(lambda b: _set(b, 'ops', _first(b, pack.OP_DWCONV), w_off=b.weights_bytes), _detector), 'w_off'),
    ('depthwise_bias_off_past', _edit(lambda b: _set(b, 'ops', _first(b, pack.OP_DWCONV), bias_off=b.weights_bytes), _detector), 'bias_off'),
    ('unscale_off_past', _edit(lambda b: _set(b, 'tensors', 1, unscale_off=b.weights_bytes)), 'activation scales'),
    ('prelu_without_slopes', _op('act', pack.ACT_PRELU), 'PReLU'),
    ('second_output_without_affine', _op('out2', 1), 'second output'),
    ('border_bias_on_1x1', _edit(lambda b: _set(b, 'ops', 1, variant=1 << 16, kh=1, kw=1)), 'border-bias'),
    ('unscale_on_input', _tensor('unscale_off', 0, 0), 'activation scales'),
    ('unscale_misaligned', _tensor('unscale_off', 2, 1), 'activation scales'),
    ('output_out_of_range', _edit(_outputs0), 'output 0'),
    ('tensor_index', _op('out', 99), 'tensor index'),
    ('lane_3', _edit(lambda b: _set(b, 'ops', 1, variant=3 << 17), lambda s: _lanes3()), 'shares tensors'),
    ('lane_with_k_split', _edit(lambda b: _set(b, 'ops', 1, variant=(1 << 17) | (2 << 8)), lambda s: _lanes3()), 'shares tensors'),
    ('lane_result_read_outside', lambda s: Blob(util.lane_sharing_program().blob()), 'shares tensors'),
    ('lane_input_overwritten', _edit(lambda b: _set(b, 'ops', 2, out=b.ops[1]['in']), lambda s: _lanes3()), 'shares tensors'),
    ('lane_two_writers', _edit(lambda b: _set(b, 'ops', 2, variant=2 << 17, out=b.ops[1]['out']), lambda s: _lanes3()), 'shares tensors'),
    # formerly the planner's and the executor's
    ('grouped', _op('groups', 2), 'grouped convolution'),
    ('pooled', _op('pool', 1), 'max-pool fusion'),
    ('dwpw_slice', _op('in_ch_off', 4, base=dwpw64), 'dw+pw block'),
    ('dwpw_no_halo', _tensor('halo', 0, 1, base=dwpw64), 'needs an input halo'),
    ('front_op', _edit(_front_not_shape_only, lambda s: _fused_detector(s)), 'front op'),
    ('halo_below_pad', _tensor('halo', 0, 0), 'needs halo 1, tensor has 0'),
    ('non_conv_on_half_floats', _tensor('fmt', pack.FMT_F16, 2, base=dwpw64), 'only convs'),
    ('format_against_channels', _tensor('fmt', pack.FMT_F16, 2), 'format 3 with 32 channels'),
    ('too_few_k_slabs', _op('n_slabs', 1), 'too few K slabs'),
    ('f16_input_of_another_mode', _op('prec', 3, base=_f16_program), 'half-float tensor feeds'),
    ('depthwise_slice', _edit(_dw_slice, _detector), 'channel slice'),
    ('unknown_op_type', _op('type', 9), 'unknown op type 9'),
    ('reads_unset_tensor', _op('in', 2), 'unset tensor'),
    ('field_out_of_range', _op('stride', 0), 'out of range'),
]


def _refused(blob, kind=KIND):
    with pytest.raises(lib.TerranAmdError) as e:
        lib.check_program(blob, kind)
    assert e.value.code == lib.E_INVALID
    return str(e.value)


@pytest.mark.parametrize('name,make,says', REFUSALS, ids=[r[0] for r in REFUSALS])
def test_one_defect_is_refused_with_its_name(states, name, make, says):
    b = make(states)
    msg = _refused(b.bytes(), int(b.hdr[0]['kind']))
    assert says in msg, msg
    if name not in ('magic', 'version') and not name.startswith(('counts', 'truncated', 'negative', 'output', 'unscale', 'lane_result', 'front')):
        assert 'op ' in msg or 'tensor ' in msg, msg                  # the record is named where it is known


def test_the_bases_of_the_refusals_pass(states):
    for b in (Blob(util.two_conv_program().blob()), Blob(dwpw64().blob()), Blob(_f16_program().blob()), _lanes3(), _detector(states)):
        lib.check_program(b.bytes(), int(b.hdr[0]['kind']))
    f16 = Blob(_f16_program().blob())
    assert f16.tensors[1]['fmt'] == pack.FMT_F16 and f16.ops[1]['prec'] == 4      # what 'f16_input_of_another_mode' breaks


def test_wrong_kind_cut_blobs_and_null_are_refused():
    blob = util.two_conv_program().blob()
    assert 'kind' in _refused(blob, pack.MODEL_ARCFACE)
    b = Blob(blob)
    assert b.tables_end <= int(b.hdr[0]['weights_off']) < len(blob)
    for n in range(0, int(b.hdr[0]['weights_off']) + 64, 64):             # header, tensor table, op table: cut at every 64 bytes
        _refused(blob[:n])
    assert 'too small' in _refused(b'')
    with pytest.raises(ValueError):
        lib.check_program(blob)                                        # bytes do not say which model they are for
    err = lib.C.create_string_buffer(256)
    assert lib.load().ta_program_check(KIND, None, 0, err, len(err)) == lib.E_INVALID and b'null' in err.value
    assert lib.load().ta_program_check(KIND, blob, len(blob), None, 0) == lib.OK     # the message is optional


def dump_blobs(out, states):
    """What tools/program_check_main.cpp is run on: every refusal case, the cut blobs, 2 000 one-field corruptions of the valid blob."""
    os.makedirs(out, exist_ok=True)
    for name, make, _ in REFUSALS:
        with open(os.path.join(out, 'refused_%s.tam' % name), 'wb') as f:
            f.write(make(states).bytes())
    blob = util.two_conv_program().blob()
    for n in range(0, len(blob), 64):
        if n <= Blob(blob).tables_end + 64:
            with open(os.path.join(out, 'cut_%05d.tam' % n), 'wb') as f:
                f.write(blob[:n])
    rng = np.random.default_rng(2024)
    for i in range(2000):
        b = Blob(blob)
        h = b.hdr[0]
        off, n, size = ((h['ops_off'], h['n_ops'], layout.OP_DT.itemsize) if rng.random() < 0.7 else
                        (h['tensors_off'], h['n_tensors'], layout.TENSOR_DT.itemsize))
        at = int(off) + int(rng.integers(n)) * size + 4 * int(rng.integers(size // 4))
        word = rng.choice([int(rng.integers(0, 2 ** 32)), int(rng.integers(0, 256)), 2 ** 31 - 1, 2 ** 31, 2 ** 32 - 1])
        b.buf[at:at + 4] = int(word).to_bytes(4, 'little')
        with open(os.path.join(out, 'fuzz_%04d.tam' % i), 'wb') as f:
            f.write(b.bytes())


if __name__ == '__main__':                                  # python -m tests.test_program_check_cpu --dump-blobs DIR
    import sys
    from terran_amd import weights
    assert len(sys.argv) == 3 and sys.argv[1] == '--dump-blobs', 'usage: python -m tests.test_program_check_cpu --dump-blobs DIR'
    dump_blobs(sys.argv[2], lambda name: getattr(weights, 'make_%s_state' % name)())
