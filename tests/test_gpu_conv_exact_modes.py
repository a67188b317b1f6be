"""-m gpu: the dense conv kernels in the three tolerance modes ('f16', 'f16x2', 'bf16'), bit for bit, one pinned kernel at a time.

tests/test_gpu_conv_exact.py holds the f32 / f16x3 / bf16x3 instances of these kernels to one bit pattern; this file does the same
for the instances that were reached through tolerances only: the 64-channel slab walk, the `rows64` weight image and the four
TA_FMT_F16 stores of 'f16', the two-product MFMA sequence of 'f16x2' in the streamed and window kernels, the hi-only reads of 'bf16'.
The programs of family 'exact' (tests/exact_programs.py, module text: the per-mode rule) hold values no rounding of the mode changes,
so every tensor is np.array_equal to plain float64 arithmetic; test_rounded_operands runs the family whose operands or results exceed
the mode's bit counts, against a reference that applies the mode's one rounding exactly.  tests/test_exact_programs_cpu.py holds both
references against torch.  DESIGN.md section 4 maps each mode-specific code path to the test ids of this file.
"""
import numpy as np
import pytest

from tests import exact_programs as ep
from tests.util import run_exact

pytestmark = pytest.mark.gpu
MODES = ep.TOLERANCE_MODES


@pytest.fixture(scope='module')
def ctx():
    from terran_amd import lib
    c = lib.Context(0)
    yield c
    c.close()


_refs = {}              # (program key, size) -> the reference: the weights depend on the key (mode included), not on variant or io


def check(ctx, net, key, sizes, stride, what):
    """The tensors have the formats the program was built for; one forward per size: the counts are net.counts, every named tensor
    equals the reference.  -> {size: (out, out2)}."""
    ep.assert_formats(net)
    outs = {}
    for size in sizes:
        fr = ep.mode_frames(net, size, stride)
        ctx.conv_counts(reset=True)
        _refs[key, size] = run_exact(ctx, net, fr, net.names, what, ref=_refs.get((key, size)))
        assert ctx.conv_counts() == net.counts, (what, size, ctx.conv_counts(), net.counts)
        outs[size] = tuple(net.model.read(k) for k in ('out', 'out2') if k in net.tid)
    net.model.free()
    return outs


def ref_key(net, *key):
    """What the reference of a program depends on: its weights (the key), the mode and the format of each of its tensors (a store
    rounds by its format)."""
    return key + (net.precision, tuple(net.P.tensor_formats()))


EPI_ITEMS = [(case, v, p) for p in MODES for case in ep.all_cases(p) for v in ep.VARIANTS if ep.conv_programs(case, v, p)]
UP2_ITEMS = [(case, v, p) for p in MODES for case in ep.UP2_CASES for v in ep.VARIANTS if ep.up2_programs(case, v, p)]
ROUNDED_ITEMS = [(case, v, p) for p in MODES for case in ep.ROUNDED_CASES for v in ep.VARIANTS if ep.rounded_programs(case, v, p)]


@pytest.mark.parametrize('case,variant,precision', EPI_ITEMS, ids=['%s-%s-%s' % i for i in EPI_ITEMS])
def test_epilogue(ctx, case, variant, precision):
    """Every epilogue of the case on the pinned kernel, with float32 and with the mode's own shortcut / outputs, at every size."""
    for epi, io, sizes in ep.conv_programs(case, variant, precision):
        net = ep.epilogue_net(precision, case, variant, epi, io)
        check(ctx, net, ref_key(net, 'epilogue', case, epi), sizes, ep.all_cases(precision)[case].get('stride', 1),
              '%s %s %s %s %s' % (case, variant, precision, epi, io))


@pytest.mark.parametrize('case,variant,precision', UP2_ITEMS, ids=['%s-%s-%s' % i for i in UP2_ITEMS])
def test_shortcut_upsampled_x2(ctx, case, variant, precision):
    for epi, io, sizes in ep.up2_programs(case, variant, precision):
        net = ep.up2_net(precision, case, variant, epi, io)
        check(ctx, net, ref_key(net, 'up2', case, epi), sizes, 1, 'up2 %s %s %s %s %s' % (case, variant, precision, epi, io))


@pytest.mark.parametrize('precision', MODES)
@pytest.mark.parametrize('variant', ep.KSPLIT_VARIANTS)
@pytest.mark.parametrize('case', sorted(ep.KSPLIT_CASES))
def test_k_split(ctx, case, variant, precision):
    """K in 2 and 4 ranges: splitk_reduce_kernel runs the whole epilogue and, with the mode's own io, stores the mode's format ('f16':
    TA_FMT_F16 from both range counts)."""
    for epi, ks, io in ep.ksplit_programs(case, precision):
        net = ep.ksplit_net(precision, case, variant, epi, ks, io)
        sizes = ep.KSPLIT_SIZES + ((ep.AFFINE_SIZE,) if ep.KSPLIT_EPILOGUES[epi].get('affine') else ())
        check(ctx, net, ref_key(net, 'ksplit', case, epi, ks), sizes, 1, 'k_split %d %s %s %s %s %s' % (ks, case, variant, precision, epi, io))


@pytest.mark.parametrize('case,variant,precision', ROUNDED_ITEMS, ids=['%s-%s-%s' % i for i in ROUNDED_ITEMS])
def test_rounded_operands(ctx, case, variant, precision):
    """The family that exceeds the mode's bit counts: the reference rounds where the mode does (a TA_FMT_F16 store to 11 bits, x_hi of
    'f16x2', both operands of 'bf16') and nowhere else.  The 40-channel case is the direct drain, K in 2 and 4 ranges the reduce kernel."""
    for epi, io, ks in ep.rounded_programs(case, variant, precision):
        net = ep.rounded_net(precision, case, variant, epi, io, ks)
        check(ctx, net, ref_key(net, 'rounded', case, epi, ks), ep.ROUNDED_SIZES, 1, 'rounded %s %s %s %s %s k_split %d' % (case, variant, precision, epi, io, ks))


AGREE_SIZES = ((3, 5, 3), (3, 9, 10))


@pytest.mark.parametrize('precision', MODES)
@pytest.mark.parametrize('case', ['c64_3x3', 'c128_3x3', 'c64to128_1x1_s2', 'c192to128_7x7', 'c64to64_1x1'])
def test_variants_agree(ctx, case, precision):
    """'out' and 'out2' of every kernel that can run the case are the same bits (the mode's own tensors where it has them)."""
    c = ep.all_cases(precision)[case]
    for epi in c['epi']:
        got = {}
        for v in ep.VARIANTS:
            listed = [(io, sizes) for e, io, sizes in ep.conv_programs(case, v, precision) if e == epi]
            if listed:
                io, sizes = listed[-1]
                net = ep.epilogue_net(precision, case, v, epi, io)
                got[v] = check(ctx, net, ref_key(net, 'epilogue', case, epi), [s for s in AGREE_SIZES if s in sizes], c.get('stride', 1),
                               'agree %s %s %s %s' % (case, v, precision, epi))
        first = next(iter(got))
        assert len(got) > 1
        for v, outs in got.items():
            for size, tensors in outs.items():
                assert all(np.array_equal(a, b) for a, b in zip(tensors, got[first][size])), (case, epi, precision, v, 'differs from', first, size)


@pytest.mark.parametrize('variant', ep.VARIANTS)
def test_f16x2_equals_f16x3_where_x_lo_is_zero(ctx, variant):
    """One 'exact' case per kernel: the activations have 11 bits, so x_lo = 0 and the two-product mode's 'out' is the three-product
    mode's, bit for bit, on the same weights (lo halves in use) and frames."""
    from terran_amd import lib
    case, epi, size = 'c128_3x3', 'plain', (3, 9, 10)
    io = [io for e, io, s in ep.conv_programs(case, variant, 'f16x2') if e == epi][-1]
    outs = []
    for precision in ('f16x2', 'f16x3'):
        net = ep.epilogue_net(precision, case, variant, epi, io, like='f16x2')
        ep.assert_formats(net)
        m = lib.Model(ctx, net.P)
        frames = ctx.upload(ep.mode_frames(net, size))
        ctx.conv_counts(reset=True)
        m.forward_frames(frames)
        assert ctx.conv_counts() == net.counts, (precision, ctx.conv_counts(), net.counts)
        outs.append(m.read('out'))
        frames.free()
        m.free()
    assert np.array_equal(*outs)
    assert np.any(outs[0] != np.rint(outs[0]))          # the w_lo * x_hi product shows: multiples of 2^-11
