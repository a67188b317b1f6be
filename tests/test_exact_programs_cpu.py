"""CPU tests (no GPU): the programs of tests/exact_programs.py are what tests/test_gpu_layers_exact.py takes them for.

- their float64 reference equals torch-CPU float64 conv2d / max_pool2d (floor) / slicing on every builder and shape the GPU
  module runs;
- the exactness rule (16 significant bits; 2^24 for float32-only outputs) holds for all of them, and `reference` does refuse
  a program that breaks it;
- the packer really stores the operands of the depthwise / pool / copy cases as float32, bf16 pairs and half-float pairs in
  the three precisions (a later packer change must not quietly turn these into float32-only tests), gives both sides of every
  pool and copy one exponent, and keeps every tensor of the half-float mode inside the half-float range: a TA_E_RANGE on the
  GPU would be a mistake of the test, not a finding;
- the loader's program check accepts every program;
- the conv output-stage programs of tests/test_gpu_conv_exact.py (epilogue_net, up2_net, ksplit_net): reference == torch, the
  exactness rule through the whole chain, data on which one wrong offset / slope / class / K range / shift changes the answer,
  the formats each listing assumes, and a per-channel un-scale that is not one value throughout;
- the programs of the tolerance modes (tests/test_gpu_conv_exact_modes.py): the 'exact' family equals plain torch float64 and obeys the
  per-mode rule, the 'rounded' family equals a second statement of the roundings made of torch.half / torch.bfloat16 casts and does
  round something; formats, 64-channel slab counts, lo halves in the packed rows, and the deliberate mistakes of ep.MODE_MISTAKES.
"""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from terran_amd import lib, pack
from tests import exact_programs as ep

FMT_OF = {'f32': pack.FMT_F32, 'bf16x3': pack.FMT_SPLIT, 'f16x3': pack.FMT_SPLIT16}


def _cast(v, dt):
    return v.to(torch.float32).to(dt).to(torch.float64)


def _cast_pair(v, dt):
    hi = _cast(v, dt)
    return hi + _cast(v - hi, dt)


def _stored(net, name, y, ch_off, fmts):
    """What tensor `name` gives back after y was stored into it: casts at the packer's per-channel exponents."""
    e = torch.from_numpy(np.ldexp(1.0, net.P.scales[net.tid[name]][ch_off:ch_off + y.shape[1]].astype(np.int32)))[None, :, None, None]
    f = fmts[net.tid[name]]
    s = y * e
    s = _cast(s, torch.half) if f == pack.FMT_F16 else (_cast_pair(s, torch.half) if f == pack.FMT_SPLIT16 else
                                                       (_cast_pair(s, torch.bfloat16) if f == pack.FMT_SPLIT else _cast(s, torch.float32)))
    return s / e


def torch_replay(net, fr, rounded=False):
    """The same recipe on torch-CPU float64 ops.  rounded: a program of a tolerance mode, with the mode's roundings as torch casts --
    the activation operand (half / bfloat16 of the stored value), the weight operand (hi word, or the pair) and every store."""
    x0 = torch.zeros((fr.shape[0], 4) + fr.shape[1:3], dtype=torch.float64)
    x0[:, :3] = torch.from_numpy(fr.astype(np.float64)).permute(0, 3, 1, 2).flip(1)
    t = {'input': x0}
    T = lambda a: torch.from_numpy(np.asarray(a, np.float64))
    for op, src, dst, a in net.steps:
        x = t[src]
        if op == 'conv':
            cout, cin = a['W'].shape[:2]
            Wt = T(a['W'])
            if rounded:
                assert a['in_affine'] is None and a['groups'] == 1 and not a['in_ch_off']
                mode, fmts = a['precision'], net.P.tensor_formats()
                dt = torch.bfloat16 if mode.startswith('bf16') else torch.half
                e_in = torch.from_numpy(np.ldexp(1.0, net.P.scales[net.tid[src]].astype(np.int32)))
                if mode in ('f16', 'f16x2', 'bf16'):
                    x = _cast(x * e_in[None, :, None, None], dt) / e_in[None, :, None, None]
                e_w = torch.from_numpy(np.ldexp(1.0, net.P._fold[a['op']]['wexp'][:cout].astype(np.int32)))[:, None, None, None] / e_in[None, :cin, None, None]
                Wt = (_cast(Wt * e_w, dt) if mode in ('f16', 'bf16') else _cast_pair(Wt * e_w, dt)) / e_w
            xin = x[:, a['in_ch_off']:a['in_ch_off'] + cin * a['groups']]
            if a['in_affine'] is not None:                             # the affine first, the zero padding after it
                xin = xin * T(a['in_affine'][0])[None, :, None, None] + T(a['in_affine'][1])[None, :, None, None]
            y = F.conv2d(xin, Wt, T(a['b']), stride=a['stride'], padding=a['pad'], groups=a['groups'])
            y = F.prelu(y, T(a['prelu'])) if a['prelu'] is not None else (F.relu(y) if a['relu'] else y)
            y = F.max_pool2d(y, 2, 2) if a['pool'] else y
            if a['res'] is not None:
                r = t[a['res']][:, a['res_ch_off']:a['res_ch_off'] + cout]
                if a['res_up2']:
                    r = F.interpolate(r, scale_factor=2, mode='nearest')[:, :, :y.shape[2], :y.shape[3]]
                y = y + r
            if a['out2'] is not None:
                z = y * T(a['scale2'])[None, :, None, None] + T(a['shift2'])[None, :, None, None]
                if rounded:
                    z = _stored(net, a['out2'], z, a['out2_ch_off'], fmts)
                full = t[a['out2']].clone() if a['out2'] in t else torch.zeros((y.shape[0], net.P.tensors[net.tid[a['out2']]][0]) + y.shape[2:], dtype=torch.float64)
                full[:, a['out2_ch_off']:a['out2_ch_off'] + cout] = z
                t[a['out2']] = full
            if rounded:
                y = _stored(net, dst, y, a['out_ch_off'], fmts)
            if dst in t or cout != net.P.tensors[net.tid[dst]][0]:
                full = t[dst].clone() if dst in t else torch.zeros((y.shape[0], net.P.tensors[net.tid[dst]][0]) + y.shape[2:], dtype=torch.float64)
                full[:, a['out_ch_off']:a['out_ch_off'] + cout] = y
                y = full
        elif op == 'dwconv':
            C = a['W'].shape[0]
            y = F.conv2d(x[:, :C], T(a['W']), T(a['b']), stride=a['stride'], padding=1, groups=C)
            y = F.relu(y) if a['relu'] else y
        elif op == 'maxpool':
            y = F.max_pool2d(x, 2, 2)
        elif op == 'copych':
            y = t[dst].clone()
            y[:, a['out_off']:a['out_off'] + a['ch']] = x[:, a['in_off']:a['in_off'] + a['ch']]
        elif op == 'dwpw':
            C = a['Wd'].shape[0]
            mid = F.relu(F.conv2d(x[:, :C], T(a['Wd']), T(a['bd']), stride=a['stride'], padding=1, groups=C))
            t[dst + ':mid'] = mid
            y = F.relu(F.conv2d(mid, T(a['Wp']), T(a['bp'])))
        elif op == 'rfstem':
            (Ws, bs), rest = a['blocks'][0], a['blocks'][1:]
            y = F.relu(F.conv2d(x[:, :3], T(Ws), T(bs), stride=2, padding=1))
            for i, (Wd, bd, Wp, bp) in enumerate(rest):
                y = F.relu(F.conv2d(y, T(Wd), T(bd), stride=1 + i, padding=1, groups=Wd.shape[0]))
                y = F.relu(F.conv2d(y, T(Wp), T(bp)))
        t[dst] = y
    return {k: v.numpy() for k, v in t.items()}


def check(net, shapes, n=2, seed=100):
    """Reference == torch on every shape, and what the half-float mode stores stays in its range.  -> the last reference.
    A shape is (h, w) of `n` frames, or (n, h, w)."""
    lib.check_program(net.P)                                       # packs the program: net.P.scales / mid_scales exist from here on
    for shape in shapes:
        h, w = shape[-2:]
        fr = ep.frames(seed + h * 31 + w, shape[0] if len(shape) == 3 else n, h, w)
        ref = ep.reference(net, fr)
        want = torch_replay(net, fr)
        assert set(ref) == set(want)
        for k in ref:
            assert ref[k].shape == want[k].shape and np.array_equal(ref[k], want[k]), (k, h, w)
        if net.precision == 'f16x3':
            for name, tid in net.tid.items():
                if name in ref and (net.read_by_an_op(name) or tid not in net.P.f32_only):
                    in_half_range(ref[name], net.P.scales[tid], name)
            for name, oi in net.mid_ops.items():
                in_half_range(ref[name + ':mid'], net.P.mid_scales[oi], name + ':mid')
    return ref


def in_half_range(v, a, what):
    """Integers stored times 2^a[c] as a half-float pair: the largest fits, and the lowest bit (2^a) is no subnormal's."""
    top = np.abs(v).max(axis=(0, 2, 3)) * np.ldexp(1.0, a[:v.shape[1]].astype(np.int32))
    assert top.max() <= ep.F16_MAX and a.min() >= -24, (what, float(top.max()), int(a.min()))


def formats(net):
    f = net.P.tensor_formats()
    return {name: f[t] for name, t in net.tid.items()}


@pytest.mark.parametrize('precision', ep.PRECISIONS)
@pytest.mark.parametrize('C', ep.DW_CHANNELS)
def test_dwconv_programs(precision, C):
    net = ep.dwconv_net(precision, C)
    ref = check(net, ep.DW_SHAPES)
    f = formats(net)
    names = ['dw_s%d_r%d' % v for v in ep.DW_VARIANTS]
    for name in names + (['src'] if C else []):
        assert f[name] == (FMT_OF[precision] if C % 32 == 0 and C else pack.FMT_F32), (name, f)
    # the weights have negative taps: the ReLU matters, and what is kept uses the lo words of both pair formats
    assert ref['dw_s1_r0'].min() < 0 and np.array_equal(ref['dw_s1_r1'], np.maximum(ref['dw_s1_r1'], 0))
    if C >= 32:
        assert _needs_lo(ref['src']) and _needs_lo(ref['dw_s1_r0'])
    assert all(np.all(net.P.tensor_scales()[net.tid[k]] == 0) for k in names)        # plain depthwise tensors are stored unscaled


def _needs_lo(v, bits=11):
    """Some value has more than the 11 bits of a half float's hi word (so more than the 8 of a bf16's as well)."""
    v = np.abs(v[v != 0]).astype(np.int64)
    return bool(np.any(v // (v & -v) >= 1 << bits))


@pytest.mark.parametrize('precision', ep.PRECISIONS)
@pytest.mark.parametrize('in_halo', [0, 1])
@pytest.mark.parametrize('C', ep.POOL_CHANNELS)
def test_maxpool_programs(precision, C, in_halo):
    net = ep.maxpool_net(precision, C, in_halo)
    ref = check(net, ep.POOL_SHAPES)
    f = formats(net)
    src = 'input' if C == 4 else 'src'
    want = FMT_OF[precision] if C % 32 == 0 else pack.FMT_F32
    assert f[src] == want and f['pooled'] == want, f
    assert net.P.tensors[net.tid[src]][1] == in_halo and net.P.tensors[net.tid['pooled']][1] == 1
    s = net.P.tensor_scales()
    assert np.array_equal(s[net.tid[src]], s[net.tid['pooled']])
    if C != 4:
        assert (ref['pooled'].max(axis=(0, 2, 3)) < 0).any()       # all-negative windows (11 x 13 frames): a max that starts at 0 shows
        assert _needs_lo(ref['pooled'])
    if C != 4 and precision == 'f16x3':                             # the shared exponent is the pinned one, not a second estimate
        natural = ep.maxpool_net(precision, C, in_halo)
        natural.P.forced_scale.clear()
        assert np.all(s[net.tid['pooled']] == ep.PINNED_EXPONENT) and np.any(natural.P.tensor_scales()[net.tid['pooled']] != ep.PINNED_EXPONENT)


@pytest.mark.parametrize('precision', ep.PRECISIONS)
@pytest.mark.parametrize('case', sorted(ep.COPY_CASES))
def test_copych_programs(precision, case):
    c_src, c_dst, in_off, out_off, ch = ep.COPY_CASES[case][:5]
    net = ep.copych_net(precision, *ep.COPY_CASES[case])
    ref = check(net, ep.COPY_SHAPES)
    f = formats(net)
    whole_blocks = (in_off | out_off | ch) % 32 == 0
    assert (case == 'offset4_falls_back_to_f32') == (not whole_blocks)
    want = FMT_OF[precision] if whole_blocks else pack.FMT_F32
    assert f['src'] == want and f['dst'] == want, f
    s = net.P.tensor_scales()
    assert np.array_equal(s[net.tid['src']][in_off:in_off + ch], s[net.tid['dst']][out_off:out_off + ch])
    if precision == 'f16x3':
        outside = np.r_[0:out_off, out_off + ch:c_dst]                 # ... the source's pinned one; the other channels keep theirs
        assert np.all(s[net.tid['dst']][out_off:out_off + ch] == ep.PINNED_EXPONENT) and np.any(s[net.tid['dst']][outside] != ep.PINNED_EXPONENT)
    # the copy changes the destination, and only there
    before = ep.conv_ref(ref['input'], net.steps[0][3]['W'], net.steps[0][3]['b'], 1, 1)
    keep = np.ones(c_dst, bool)
    keep[out_off:out_off + ch] = False
    assert np.array_equal(ref['dst'][:, keep], before[:, keep]) and not np.array_equal(ref['dst'], before)
    assert _needs_lo(ref['src'])


@pytest.mark.parametrize('precision', ep.PRECISIONS)
def test_convpool_program(precision):
    net = ep.convpool_net(precision)
    ref = check(net, ep.CONVPOOL_SHAPES)
    assert np.array_equal(ref['fused'], ref['pooled']) and ref['fused'].max() > 2048
    f = formats(net)
    assert f['src'] == FMT_OF[precision] and f['full'] == FMT_OF[precision] and f['fused'] == f['pooled'] == pack.FMT_F32
    s = net.P.tensor_scales()
    assert np.array_equal(s[net.tid['full']], s[net.tid['pooled']])


@pytest.mark.parametrize('precision', ['f32', 'f16x3'])
@pytest.mark.parametrize('C,cout,stride', ep.DWPW_CASES)
def test_dwpw_programs(precision, C, cout, stride):
    net = ep.dwpw_net(precision, C, cout, stride)
    refs = {}
    for shape in ep.dwpw_shapes(C) + ((ep.DWPW_MANY_TILES[(C, cout, stride)],) if (C, cout, stride) in ep.DWPW_MANY_TILES else ()):
        refs[shape] = check(net, [shape], seed=700)                 # the frames test_dwpw runs
        if precision == 'f16x3':                                    # the range guard watches the float32 store of 'block' as well
            in_half_range(refs[shape]['block'], net.P.scales[net.tid['block']], 'block')
    ref = refs[(2, 5, 7) if C > 256 else (2, 9, 16)]
    assert formats(net)['src'] == pack.FMT_F32
    assert ref['block'].max() > 2048 and (ref['block'] == 0).any() and (ref['block:mid'] == 0).any()      # both ReLUs cut something
    assert (ref['block'] > 0).any(axis=(0, 2, 3)).all() and (ref['block:mid'] > 0).any(axis=(0, 2, 3)).all()      # ... but no channel whole
    Wp = net.steps[-1][3]['Wp'][:, :, 0, 0]
    assert Wp.any(axis=0).all() and np.array_equal(Wp, np.rint(Wp)) and np.abs(Wp).max() == 2      # every input channel reaches an output


# ---- dw+pw: what the sizes and cases reach, proved from the mirror of the kernels' tiling (ep.dwpw_grid) ---------------------------
def _dwpw_M(shape, stride):
    n, h, w = shape
    return n * ((h - 1) // stride + 1) * ((w - 1) // stride + 1)


def test_dwpw_grid_mirror_deals_every_tile_once():
    """ep.dwpw_grid (the mirror of ta_xcd_tile and the block -> (cout tile, pixel tile) arithmetic): every tile of every launch listed
    has exactly one block, the other blocks of the grid return; an XCD's tiles are consecutive."""
    for C, cout, stride in ep.DWPW_CASES:
        shapes = ep.dwpw_shapes(C) + ((ep.DWPW_MANY_TILES[(C, cout, stride)],) if (C, cout, stride) in ep.DWPW_MANY_TILES else ())
        for shape in shapes:
            for lean in (True, False):
                g = ep.dwpw_grid(cout, _dwpw_M(shape, stride), lean)
                live = sorted(t for t in g['tiles'] if t[1] >= 0)
                assert live == [(ct, pt) for ct in range(g['n_ct']) for pt in range(g['n_pt'])], (C, cout, stride, shape, lean)
                assert g['BN'] * g['n_ct'] == -(-cout // 32) * 32 and g['blocks'] % 8 == 0
                for xcd in range(8):
                    mine = [pt for b, (ct, pt) in enumerate(g['tiles']) if b & 7 == xcd and ct == 0 and pt >= 0]
                    assert mine == list(range(mine[0], mine[0] + len(mine))) if mine else g['n_pt'] < 8
    assert [ep.dwpw_tile(c, True) for c in (24, 40, 64, 128, 256)] == [(32, 128), (64, 64), (64, 64), (128, 64), (128, 64)]
    assert [ep.dwpw_tile(c, False) for c in (24, 40, 64, 128, 256)] == [(32, 128), (64, 128), (64, 128), (128, 128), (128, 128)]


def test_dwpw_sizes_reach_the_tile_edges():
    """Stride-1 cases of both pixel tiles of the lean kernel (BM 64 and 128) and of the generic kernel (BM 128) run DWPW_SHAPES, whose M
    are whole tiles (exactly 1, 2 and 4 of 64; 1 and 2 of 128), one pixel either side of 64 and of 128, and a tile that holds the end
    of one image and the start of the next, both of an odd Ho Wo."""
    s1 = [(C, cout) for C, cout, stride in ep.DWPW_CASES if stride == 1 and C <= 256]
    assert {ep.dwpw_tile(cout, True)[1] for _, cout in s1} == {64, 128} and {ep.dwpw_tile(cout, False)[1] for _, cout in s1} == {128}
    assert {ep.dwpw_tile(cout, True)[0] for _, cout in s1} == {32, 64, 128}
    shapes = ep.dwpw_shapes(64)
    Ms = [_dwpw_M(s, 1) for s in shapes]
    assert {63, 64, 65, 127, 128, 129, 256} <= set(Ms), Ms
    for BM, whole in ((64, {1, 2, 4}), (128, {1, 2})):
        assert whole <= {M // BM for M in Ms if M % BM == 0}, (BM, Ms)
        # a tile with the last pixel of image 0 and the first of image 1, Ho Wo odd
        assert any(n >= 2 and h * w % 2 == 1 and h * w % BM and (h * w - 1) // BM == h * w // BM for n, h, w in shapes), BM
    assert (2, 7, 9) in shapes and (2, 5, 13) in shapes        # 63 + 1 in a tile of 64; 65 + 63 in a tile of 128


def test_dwpw_many_tiles_cases_deal_rounds_and_a_remainder():
    """More than 8 pixel tiles in the lean and in the generic kernel: ta_xcd_tile with base >= 1 and rem > 0, so that XCDs own
    different numbers of tiles; n_pt = 9 at BM = 128 and 17 at BM = 64 (stride 1), and a stride-2 case on an odd x even map."""
    seen, tiles = set(), set()
    for (C, cout, stride), shape in ep.DWPW_MANY_TILES.items():
        assert (C, cout, stride) in ep.DWPW_CASES
        n, h, w = shape
        M = _dwpw_M(shape, stride)
        for lean in (True, False):
            g = ep.dwpw_grid(cout, M, lean)
            assert g['n_pt'] > 8 and g['n_pt'] >> 3 >= 1 and g['n_pt'] & 7, (C, cout, stride, lean, g['n_pt'])
            assert any(pt < 0 for _, pt in g['tiles'])                # some blocks of the last round have no tile
            seen.add((stride, g['BM'], g['n_pt'], lean))
            tiles.add((stride, g['BN'], lean))
        if stride == 2:
            assert ((h - 1) // 2 + 1) % 2 == 1 and ((w - 1) // 2 + 1) % 2 == 0
    assert {(1, 128, 9, True), (1, 64, 17, True), (1, 128, 9, False)} <= seen, seen
    assert any(s == 2 and lean for s, _, _, lean in seen) and any(s == 2 and not lean for s, _, _, lean in seen)
    assert {g for _, g, _, lean in seen if lean} == {64, 128}          # both pixel tiles of the lean kernel
    assert {(1, 32, True), (1, 64, True), (1, 128, True), (2, 64, True), (2, 128, True)} <= tiles, tiles      # every instance of it, both strides


BIG_C = [c for c in ep.DWPW_CASES if c[0] > 256]


def test_dwpw_big_c_cases_reach_the_table_tail_loop():
    """C = 320: 800 granules, the tail loop loads bias values only; C = 1024: 2560 granules, seven passes of it over tap rows 3 .. 8
    and the bias.  Both take rf_dwpw_kernel (lean_ok), within the LDS of a CU; one case has two cout tiles."""
    assert {c[0] for c in BIG_C} == {320, 1024} and max(c[0] for c in ep.DWPW_CASES if c not in BIG_C) == 256
    for C, cout, stride in BIG_C:
        assert ep.dwpw_lean_ok('f16x3', C, cout) and not ep.dwpw_lean_ok('f32', C, cout)
        assert ep.dwpw_lean_lds(C, cout) <= ep.LDS_PER_CU
        trips = {(row, ep.dwpw_table_loader(C, row, c)[1]) for row in range(10) for c in range(0, C, 4)}
        assert 10 * C // 4 > ep.DWPW_TABLE_FIRST and any(t for _, t in trips)
        if C == 320:
            assert {row for row, t in trips if t} == {9} and {t for _, t in trips} == {0, 1}
            assert ep.dwpw_table_loader(C, 9, 192) == (768, 1) and ep.dwpw_table_loader(C, 9, 188)[1] == 0
        else:
            assert {row for row, t in trips if t} == set(range(3, 10)) and {t for _, t in trips} == set(range(8))
            assert ep.dwpw_table_loader(C, 3, 0) == (768, 1) and ep.dwpw_table_loader(C, 9, C - 1) == (2559, 7)
    assert max(ep.dwpw_lean_lds(C, cout) for C, cout, _ in BIG_C) == 2 * (128 + 64) * 128 + 40 * 1024      # 88 KB: the (1024, 128) case
    assert not ep.dwpw_lean_ok('f16x3', 1056, 64)
    assert {(C, cout) for C, cout, _ in BIG_C} >= {(320, 64), (1024, 64), (1024, 128)}
    assert 2 in {ep.dwpw_grid(cout, 70, True)['n_ct'] for _, cout, _ in BIG_C}
    # the shipped network's blocks never get there
    assert all(10 * C // 4 <= ep.DWPW_TABLE_FIRST for C, _, _ in ep.DWPW_CASES if C <= 256)


def _dwpw_sample(C):
    """(row of the depthwise table, channel): channel 0, the last, one in every 32-channel slab (the tap walks the nine), and the
    values whose granules lie at, just before and beyond 768, at every pass of the tail loop, and the last granule."""
    out = {(0, 0), (8, C - 1), (9, 0), (9, C - 1)}
    out |= {((s * 5 + 1) % 9, s * 32 + (s * 11 + 3) % 32) for s in range(C // 32)}
    out |= {(9, s * 32 + (s * 7 + 5) % 32) for s in range(C // 32)}
    out |= {(row, row * 37 % C) for row in range(10)}
    for g in [ep.DWPW_TABLE_FIRST - 1] + list(range(ep.DWPW_TABLE_FIRST, 10 * C // 4, 256)) + [10 * C // 4 - 1]:
        if g < 10 * C // 4:
            row, c = divmod(g * 4, C)
            out |= {(row, c), (row, c + 3)}
    return sorted(out)


@pytest.mark.parametrize('C,cout,stride', BIG_C + [(256, 256, 1), (64, 24, 1)])
def test_dwpw_every_sampled_channel_reaches_the_output(C, cout, stride):
    """One depthwise tap, then one depthwise bias, changed by 1 for a channel: the reference output must change each time.  (A channel
    whose 1x1 weights are all zero, or whose rows the ReLU cuts everywhere, would be no test of that channel's taps, bias or slab.)"""
    net = ep.dwpw_net('f32', C, cout, stride)
    a = net.steps[-1][3]
    n, h, w = ep.dwpw_shapes(C)[0]
    fr = ep.frames(700 + h * 31 + w, n, h, w)
    ref = ep.reference(net, fr)['block']
    sample = _dwpw_sample(C)
    assert {c // 32 for _, c in sample} == set(range(C // 32)) and {r for r, _ in sample} == set(range(10))
    if C > 256:
        trips = {ep.dwpw_table_loader(C, row, c)[1] for row, c in sample}
        assert trips == set(range(2 if C == 320 else 8)), trips
    for row, c in sample:
        key, at = ('bd', (c,)) if row == 9 else ('Wd', (c, 0, row // 3, row % 3))
        keep = a[key][at]
        for delta in ((1.0,) if row == 9 else (1.0, -1.0)):            # (a tap of a pixel that is 0 there: try the other sign as well)
            a[key][at] = keep + delta
            changed = not np.array_equal(ep.reference(net, fr)['block'], ref)
            a[key][at] = keep
            if changed:
                break
        assert changed, (C, 'bias' if row == 9 else 'tap %d' % row, c)
    assert np.array_equal(ep.reference(net, fr)['block'], ref)


# ---- the fused front: what RFSTEM_FUSED_SHAPES reach, proved from ep.rfstem_fused_geometry ------------------------------------------
def test_rfstem_fused_shapes_reach_the_tile_edges():
    shapes = ep.RFSTEM_FUSED_SHAPES
    assert len(shapes) <= 10 and all(h <= 49 and w <= 245 for _, h, w in shapes)
    assert set(ep.RFSTEM_SHAPES) <= set(ep.RFSTEM_ALL_SHAPES) and set(shapes) <= set(ep.RFSTEM_ALL_SHAPES)
    assert len(set(ep.RFSTEM_ALL_SHAPES)) == len(ep.RFSTEM_ALL_SHAPES)
    G = {s: ep.rfstem_fused_geometry(s[1], s[2]) for s in shapes}
    assert ep.rfstem_fused_geometry(24, 120)['origin'](1, 1) == (24 - 5, 120 - 5) and ep.rfstem_fused_geometry(24, 120)['origin'](0, 0) == (-5, -5)
    tiles = {s: (g['tiles_y'], g['tiles_x']) for s, g in G.items()}
    whole = {s: g for s, g in G.items() if g['oh'] % ep.RFS_OY == 0 and g['ow'] % ep.RFS_OX == 0}
    # exactly one tile and exactly 2 x 2
    assert {tiles[s] for s in whole} == {(1, 1), (2, 2)}
    # one row and one column more than whole tiles, and one less
    assert any((g['oh'], g['ow']) == (7, 31) for g in G.values()) and any(g['oh'] % 6 == 5 and g['ow'] % 30 == 29 for g in G.values())
    # every row misalignment at a width of exactly one tile, mw odd and even; mh odd and even at the tile's last output row: output
    # row oh - 1 reads row 2 oh - 1 of the 16-channel map, which is outside the map (staged as zero) when mh is odd
    one = {s: g for s, g in whole.items() if tiles[s] == (1, 1)}
    assert {3 * w % 4 for _, _, w in one} == {0, 1, 2, 3}
    assert {g['mw'] % 2 for g in one.values()} == {0, 1} and {g['mh'] % 2 for g in one.values()} == {0, 1}
    assert {2 * g['oh'] - 1 < g['mh'] for g in one.values()} == {True, False} and {2 * g['ow'] - 1 < g['mw'] for g in one.values()} == {True, False}
    # the second image of a batch starts off a dword, at two residues at least
    assert len({h * w * 3 % 4 for n, h, w in shapes if n >= 2} - {0}) >= 2
    # x_inside: at W = 244 no tile, at W = 245 tile column 1 of three alone
    at = {w: [G[s]['x_inside'](bx) for bx in range(G[s]['tiles_x'])] for s in shapes for w in [s[2]] if w in (244, 245)}
    assert at == {244: [False, False, False], 245: [False, True, False]}, at
    assert all(not g['x_inside'](bx) for s, g in G.items() if s[2] < 244 for bx in range(g['tiles_x']))
    # smaller than one window (33 rows x 129 pixels from (-5, -5)), and three tile rows
    assert (1, 5, 7) in shapes and any(g['tiles_y'] == 3 for g in G.values())
    # the unfused 14 x 62 tiling keeps its own shapes
    assert ep.RFSTEM_ALL_SHAPES[:len(ep.RFSTEM_SHAPES)] == ep.RFSTEM_SHAPES


@pytest.mark.parametrize('fused', [False, True])
def test_rfstem_programs(fused):
    net = ep.rfstem_net('f32', fused)
    lib.check_program(net.P)
    for n, h, w in ep.RFSTEM_ALL_SHAPES:
        fr = ep.frames(50 + h, n, h, w)
        ref, want = ep.reference(net, fr), torch_replay(net, fr)
        assert np.array_equal(ref['front'], want['front'])
        q = 4 if fused else 2
        assert ref['front'].shape == (n, 32 if fused else 16, (h + q - 1) // q, (w + q - 1) // q)
        assert (ref['front'] > 0).mean() > 0.3                      # the ReLUs leave most of the map alive
    assert ref['front'].max() > 1 << 12


def test_second_trip_programs():
    for k, (hw, total) in ep.SECOND_TRIP.items():
        assert ep.GRID_CAP < total < ep.GRID_CAP * 1.02, k
    h, w = ep.SECOND_TRIP['dwconv'][0]
    net = ep.dwconv_net('f32', 32, variants=((1, 1),))
    assert ep.reference(net, ep.frames(1, 1, h, w))['dw_s1_r1'][0, 0].size * 8 == ep.SECOND_TRIP['dwconv'][1]
    h, w = ep.SECOND_TRIP['maxpool'][0]
    net = ep.maxpool_net('f32', 64, 0, with_sink=False)
    assert ep.reference(net, ep.frames(1, 1, h, w))['pooled'][0, 0].size * 16 == ep.SECOND_TRIP['maxpool'][1]
    h, w = ep.SECOND_TRIP['copych'][0]
    net = ep.copych_net('f32', 32, 64, 0, 0, 32, with_sink=False)
    assert ep.reference(net, ep.frames(1, 1, h, w))['src'][0, 0].size * 8 == ep.SECOND_TRIP['copych'][1]
    for net in (ep.dwconv_net('f32', 32, variants=((1, 1),)), ep.maxpool_net('f32', 64, 0, with_sink=False),
                ep.copych_net('f32', 32, 64, 0, 0, 32, with_sink=False)):
        check(net, [(6, 5)])


@pytest.mark.parametrize('kind', [pack.MODEL_RETINAFACE, pack.MODEL_OPENPOSE, pack.MODEL_ARCFACE])
def test_preprocess_programs_load(kind):
    lib.check_program(ep.preprocess_net(kind).P)
    fr = ep.frames(3, 1, 17, 23)
    assert set(np.unique(fr)) == set(range(256))                    # every byte value occurs
    x = ep.input_ref(fr)
    assert np.array_equal(x[0, :3, 4, 5], fr[0, 4, 5, ::-1]) and not x[:, 3].any()


def test_the_reference_refuses_what_is_not_exact():
    """17 significant bits in a tensor the packer may split, and 2^24 in a float32 one."""
    fr = np.full((1, 5, 5, 3), 255, np.uint8)
    net = ep.Net('bf16x3')
    net.tensor('big', 32, 0)
    net.conv('input', 'big', np.full((32, 3, 1, 1), 90.0), np.zeros(32))              # 3 * 90 * 255 = 68850 >= 2^16
    with pytest.raises(AssertionError, match='not exact'):
        ep.reference(net, fr)
    net = ep.Net('f32')
    net.tensor('big', 32, 0, f32=True)
    net.conv('input', 'big', np.full((32, 3, 1, 1), 90.0), np.zeros(32))              # float32 only and read by nothing: fine
    ep.reference(net, fr)
    net.tensor('bigger', 32, 0, f32=True)
    net.conv('big', 'bigger', np.full((32, 32, 1, 1), 8.0), np.zeros(32))             # ... but now it is read (and 'bigger' passes 2^24)
    with pytest.raises(AssertionError, match='not exact'):
        ep.reference(net, fr)


# ---- the conv output stage: the programs of tests/test_gpu_conv_exact.py -----------------------------------------------------------
def stage_programs():
    """(id, builder(precision, variant, io), the variants and ios it is listed under per precision, frame sizes, conv stride)."""
    out = []
    for case, c in ep.CONV_CASES.items():
        for epi in c['epi']:
            listed = {p: [(v, io) for v in ep.VARIANTS for e_, io, _ in ep.conv_programs(case, v, p) if e_ == epi] for p in ep.PRECISIONS}
            sizes = ep.case_sizes(case, ep.EPILOGUES[epi].get('affine'))
            out.append(('epilogue-%s-%s' % (case, epi), lambda p, v, io, case=case, epi=epi: ep.epilogue_net(p, case, v, epi, io),
                        listed, sizes, c.get('stride', 1)))
    for case in ep.UP2_CASES:
        for epi in ep.UP2_EPILOGUES:
            listed = {p: [(v, io) for v in ep.VARIANTS for e_, io, _ in ep.up2_programs(case, v, p) if e_ == epi] for p in ep.PRECISIONS}
            out.append(('up2-%s-%s' % (case, epi), lambda p, v, io, case=case, epi=epi: ep.up2_net(p, case, v, epi, io), listed, ep.case_sizes(case), 1))
    for case in ep.KSPLIT_CASES:
        for epi, ks, _ in ep.ksplit_programs(case, 'f32'):
            listed = {p: [(v, io) for v in ep.KSPLIT_VARIANTS for e_, k_, io in ep.ksplit_programs(case, p) if (e_, k_) == (epi, ks)]
                      for p in ep.PRECISIONS}
            sizes = ep.KSPLIT_SIZES + ((ep.AFFINE_SIZE,) if ep.KSPLIT_EPILOGUES[epi].get('affine') else ())
            out.append(('ksplit%d-%s-%s' % (ks, case, epi), lambda p, v, io, case=case, epi=epi, ks=ks: ep.ksplit_net(p, case, v, epi, ks, io),
                        listed, sizes, 1))
    return out


STAGE = stage_programs()
_stage_refs = {}


def stage_refs(i):
    """The references of STAGE[i] at every size, from its strictest listing: nothing pinned to float32 where a listing leaves it so
    (every limit is then 16 bits), held against torch."""
    if i not in _stage_refs:
        name, build, listed, sizes, stride = STAGE[i]
        v, io = listed['bf16x3'][-1]
        net = build('bf16x3', v, io)
        refs = []
        for size in sizes:
            fr = ep.frames(ep.frame_seed(size), *ep.frame_size(size, stride))
            ref, want = ep.reference(net, fr), torch_replay(net, fr)
            assert set(ref) == set(want) >= set(net.names)
            for k in ref:
                assert ref[k].shape == want[k].shape and np.array_equal(ref[k], want[k]), (name, k, size)
            assert (ref['out'].shape[0],) + ref['out'].shape[2:] == tuple(size)
            refs.append((fr, ref))
        _stage_refs[i] = (net, refs)
    return _stage_refs[i]


@pytest.mark.parametrize('i', range(len(STAGE)), ids=[s[0] for s in STAGE])
def test_conv_stage_reference_equals_torch_and_is_exact(i):
    """float64 reference == torch float64 conv2d / prelu / nearest x2 / slicing at every listed size; `reference` asserts the
    exactness rule through the whole chain on the way.  The stage does something: ReLU / PReLU meet negative sums, the shortcut and
    both outputs use more bits than one hi word holds."""
    net, refs = stage_refs(i)
    a = [s for s in net.steps if s[1] == 'src' and s[2] == 'out'][0][3]
    big = max(refs, key=lambda r: r[1]['out'][:, 0].size)[1]               # the 3 x 9 x 10 map
    assert _needs_lo(big['out']) and _needs_lo(big['src'], 8)          # ('src' stays below 2^11: the sink convs read 'out', which does not)
    if a['prelu'] is not None:
        assert len(set(a['prelu'].tolist())) == 5
    if a['relu']:
        assert (big['out'] == 0).any()
    if a['res'] is not None:
        sc = big['shortcut']
        assert all(len(np.unique(sc[0, c])) > 1 for c in range(sc.shape[1])) or sc[0, 0].size == 1     # not constant across the map


@pytest.mark.parametrize('i', range(len(STAGE)), ids=[s[0] for s in STAGE])
def test_conv_stage_data_discriminates(i):
    """A reference with one deliberate mistake differs from the true one at every size where the feature is reachable: a green GPU
    run cannot come from a shortcut that happened to be constant, slopes that happened to be equal, a shift of zero, ..."""
    net, refs = stage_refs(i)
    a = [s for s in net.steps if s[1] == 'src' and s[2] == 'out'][0][3]
    has = {'up2_unshifted': bool(a['res_up2']), 'res_ch_off+4': a['res'] is not None, 'out2_ch_off+8': a['out2'] is not None,
           'prelu_shifted': a['prelu'] is not None, 'corner_as_edge': a['in_affine'] is not None, 'k_range_dropped': a['k_split'] > 1,
           'no_shift2': a['out2'] is not None}
    assert set(has) == set(ep.MISTAKES)
    for fr, ref in refs:
        for mistake in ep.MISTAKES:
            reachable = has[mistake] and not (mistake == 'up2_unshifted' and ref['out'].shape[2:] == (1, 1))
            if not reachable:
                continue
            wrong = ep.reference(net, fr, mistake=mistake)
            assert any(not np.array_equal(wrong[k], ref[k]) for k in ('out', 'out2') if k in ref), (mistake, fr.shape)
        if a['in_affine'] is not None:                                  # the packer's folded form means the same
            folded = ep.reference(net, fr, mistake='fold')
            assert all(np.array_equal(folded[k], ref[k]) for k in ref), fr.shape
    if a['in_affine'] is not None:
        Wf, b16 = pack.fold_input_affine(a['W'], a['b'], *a['in_affine'])
        assert np.array_equal(Wf, np.rint(Wf)) and np.array_equal(b16, np.rint(b16)) and len(np.unique(b16, axis=0)) == 16


@pytest.mark.parametrize('precision', ep.PRECISIONS)
@pytest.mark.parametrize('i', range(len(STAGE)), ids=[s[0] for s in STAGE])
def test_conv_stage_programs_load_as_listed(i, precision):
    """Every (variant, io) a program is listed under: the loader's check accepts it, its tensors have the formats the listing assumes
    (so the pinned kernel is eligible and the lean drain is where lean_expected says), the half-float mode stays inside its range, and
    the per-channel un-scale of the conv under test is not one value throughout."""
    name, build, listed, sizes, stride = STAGE[i]
    _, refs = stage_refs(i)
    assert listed[precision], name
    for v, io in listed[precision]:
        net = build(precision, v, io)
        lib.check_program(net.P)
        f = formats(net)
        oi = net.conv_ops['out']
        op = net.P.ops[oi]
        staged = (op['out_ch_off'] | op['res_ch_off'] | op['out2_ch_off']) % 8 == 0
        assert f['src'] == (pack.FMT_F32 if v == 'generic' or not staged else FMT_OF[precision]), (name, v, io, f)
        assert v == 'generic' or staged
        for k in ('shortcut', 'out', 'out2'):
            if k in f:
                want = FMT_OF[precision] if io == 'split' and net.P.tensors[net.tid[k]][0] % 32 == 0 else pack.FMT_F32
                assert f[k] == want, (name, v, io, k, f)
        if precision != 'f16x3':
            continue
        for fr, ref in refs:
            for k, tid in net.tid.items():
                if k in ref:
                    in_half_range(ref[k], net.P.scales[tid], k)
        cout = op['cout']
        a_out = net.P._exponents(net.P.scales, op, 'out')[:cout]
        us = a_out - net.P._fold[oi]['wexp'][:cout]
        assert len(np.unique(us)) >= 2, (name, v, io)
        if io == 'split':
            assert len(np.unique(a_out)) >= 2, (name, v, io, a_out)


# ---- the tolerance modes: the programs of tests/test_gpu_conv_exact_modes.py -------------------------------------------------------
FMT_OF_MODE = {'f16': pack.FMT_F16, 'f16x2': pack.FMT_SPLIT16, 'bf16': pack.FMT_SPLIT}


def mode_programs(mode):
    """(id, net of the last listed (variant, io), sizes, stride) of every 'exact' program of `mode`."""
    out = []
    for case, c in ep.all_cases(mode).items():
        for epi in c['epi']:
            listed = [(v, io, sizes) for v in ep.VARIANTS for e_, io, sizes in ep.conv_programs(case, v, mode) if e_ == epi]
            if not listed:                                          # ('f16' has no grouped conv, so that case has no listing at all)
                assert mode == 'f16' and c.get('groups', 1) > 1
                break
            v, io, _ = listed[-1]
            out.append(('epilogue-%s-%s' % (case, epi), ep.epilogue_net(mode, case, v, epi, io), ep.case_sizes(case, ep.EPILOGUES[epi].get('affine'), mode), c.get('stride', 1)))
    for case in ep.UP2_CASES:
        for epi in ep.UP2_EPILOGUES:
            v, io = [(v, io) for v in ep.VARIANTS for e_, io, _ in ep.up2_programs(case, v, mode) if e_ == epi][-1]
            out.append(('up2-%s-%s' % (case, epi), ep.up2_net(mode, case, v, epi, io), ep.case_sizes(case, False, mode), 1))
    for case in ep.KSPLIT_CASES:
        for epi, ks, io in ep.ksplit_programs(case, mode):
            if io == 'split':
                out.append(('ksplit%d-%s-%s' % (ks, case, epi), ep.ksplit_net(mode, case, 'split_2x2', epi, ks, io), ep.KSPLIT_SIZES, 1))
    return out


def conv_under_test(net):
    return net.P.ops[net.conv_ops['out']], [s for s in net.steps if s[1] == 'src' and s[2] == 'out'][0][3]


@pytest.mark.parametrize('mode', ep.TOLERANCE_MODES)
def test_mode_exact_family(mode):
    """reference == plain torch float64 (so no rounding of the mode changed a value; `reference` asserts the per-mode rule per tensor
    on the way); the tensors have the mode's own formats; 'f16': n_slabs == taps * cin / 64 and a rows64 image; 'f16x2': every packed
    weight row of the conv under test has a non-zero lo half; the mistakes of the mode change the answer."""
    flipped, f16_named = set(), set()
    for name, net, sizes, stride in mode_programs(mode):
        lib.check_program(net.P)
        op, a = conv_under_test(net)
        f = formats(net)
        for size in sizes:
            fr = ep.mode_frames(net, size, stride)
            ref, want = ep.reference(net, fr), torch_replay(net, fr)
            for k in ref:
                assert np.array_equal(ref[k], want[k]), (mode, name, k, size)
            assert not net.rounding.changed
            for mistake in ep.MODE_MISTAKES:
                wrong = ep.reference(net, fr, mistake=mistake)
                if any(not np.array_equal(wrong[k], ref[k]) for k in ('out', 'out2') if k in ref):
                    flipped.add(mistake)
        assert f['src'] in (FMT_OF_MODE[mode], pack.FMT_F32), (name, f)
        for k in ('src', 'shortcut', 'out', 'out2'):
            if f.get(k) == FMT_OF_MODE[mode]:
                f16_named.add(k)
        taps, cin = op['kh'] * op['kw'], op['cin']
        if mode == 'f16' and f['src'] == pack.FMT_F16:
            assert op['n_slabs'] == taps * cin // 64 and net.P._fold[net.conv_ops['out']]['rows64'].shape[0] == op['n_slabs'], name
        if mode == 'f16x2':
            k, size = net.P.w._at[op['w_off']]                         # the packed image itself: [slab][coutp][hi x32 | lo x32] half words
            rows = np.frombuffer(net.P.w.chunks[k], np.uint16).reshape(op['n_slabs'], op['coutp'], 64)
            assert size == rows.nbytes and np.all(((rows[:, :op['cout'], 32:] & 0x7FFF) != 0).any(axis=(0, 2))), name
    assert f16_named == {'src', 'shortcut', 'out', 'out2'}, (mode, f16_named)
    # every listing of every program, not only the one walked above: the formats are the ones meant (tensor_formats() against
    # net.want_formats), and each drain of DESIGN.md's table meets the mode's own format in 'out', 'out2' and 'shortcut'
    own, met = FMT_OF_MODE[mode], {}
    nets = [(('lean' if net.counts.get('lean_epilogue') else 'staged') if io == 'split' and staged else ('direct' if io == 'split' else None), v, net)
            for case, c in ep.all_cases(mode).items() for v in ep.VARIANTS for staged in [c.get('out_off', 0) % 8 == 0]
            for epi, io, _ in ep.conv_programs(case, v, mode) for net in [ep.epilogue_net(mode, case, v, epi, io)]]
    nets += [('lean' if net.counts.get('lean_epilogue') else 'staged' if io == 'split' else None, v, net) for case in ep.UP2_CASES for v in ep.VARIANTS
             for epi, io, _ in ep.up2_programs(case, v, mode) for net in [ep.up2_net(mode, case, v, epi, io)]]
    nets += [('reduce%d' % ks if io == 'split' else None, v, net) for case in ep.KSPLIT_CASES for v in ep.KSPLIT_VARIANTS
             for epi, ks, io in ep.ksplit_programs(case, mode) for net in [ep.ksplit_net(mode, case, v, epi, ks, io)]]
    for drain, v, net in nets:
        got = ep.assert_formats(net)
        if drain:                                                     # the mode's own io: what the drain stores and adds is in the format
            blk = 64 if mode == 'f16' else 32                         # (the 40-channel case: its own 40-wide 'out2' cannot be of whole blocks)
            whole = [k for k in ('shortcut', 'out', 'out2') if k in got and net.P.tensors[net.tid[k]][0] % blk == 0]
            assert all(got[k] == own for k in whole), (mode, drain, v, got)
            for k in whole:
                if True:
                    met.setdefault((drain, 'sym' if v in ('generic', 'pipe64') else 'split'), set()).add(k)
    every = {'shortcut', 'out', 'out2'}
    assert met[('direct', 'sym')] == every and met[('staged', 'sym')] == every and met[('staged', 'split')] == every, met
    assert met[('lean', 'split')] == every and met[('reduce2', 'split')] == every and met[('reduce4', 'split')] == every, met
    want = {'f16': {'slab64_second_half_swapped'}, 'f16x2': {'x_lo_kept', 'w_lo_dropped'}, 'bf16': set()}[mode]
    assert flipped >= want - {'x_lo_kept'}, (mode, flipped)       # (x_lo_kept needs an x_lo: the rounded family below)


@pytest.mark.parametrize('mode', ep.TOLERANCE_MODES)
def test_mode_rounded_family(mode):
    """reference == the torch-cast statement of the mode's roundings, something IS rounded in every program (the stored value in 'f16',
    an operand in 'f16x2' / 'bf16'), and the mode's mistakes change the answer."""
    flipped = set()
    for case in ep.ROUNDED_CASES:
        for v in ep.VARIANTS:
            for epi, io, ks in ep.rounded_programs(case, v, mode):
                net = ep.rounded_net(mode, case, v, epi, io, ks)
                lib.check_program(net.P)
                ep.assert_formats(net)
                changed = set()
                for size in ep.ROUNDED_SIZES:
                    fr = ep.mode_frames(net, size)
                    ref, want = ep.reference(net, fr), torch_replay(net, fr, rounded=True)
                    for k in ref:
                        assert np.array_equal(ref[k], want[k]), (mode, case, v, epi, ks, k, size)
                    changed |= net.rounding.changed
                    for mistake in ep.MODE_MISTAKES:
                        wrong = ep.reference(net, fr, mistake=mistake)
                        if any(not np.array_equal(wrong[k], ref[k]) for k in net.names):
                            flipped.add(mistake)
                what = {'f16': ('out', 'store'), 'f16x2': ('src', 'read by f16x2'), 'bf16': ('src', 'read by bf16')}[mode]
                assert what in changed, (mode, case, v, epi, ks, changed)
    want = {'f16': {'store_truncated'}, 'f16x2': {'x_lo_kept', 'w_lo_dropped'}, 'bf16': set()}[mode]
    assert flipped >= want, (mode, flipped)


def test_the_mode_rule_refuses_what_the_mode_rounds():
    """An 'exact' program on frames of the whole 0 .. 255 breaks the bit counts: `reference` says so."""
    net = ep.epilogue_net('bf16', 'c64_3x3', 'split_1x4', 'plain', 'split')
    net.pixel_shift = 0
    with pytest.raises(AssertionError, match='exactness rule'):
        ep.reference(net, ep.frames(5, 3, 9, 10))
