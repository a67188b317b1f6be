"""-m gpu: the HBM-bound layer kernels (csrc/layers.hip) and the format helpers of csrc/act_format.h, bit for bit.

Every other arithmetic test of the network kernels allows max|got - ref| <= tol * max|ref| on Gaussian data: the right judge for
an MFMA's summation order, a weak one for kernels that move and combine numbers (a dropped lo word, a wrong pixel in a weak
channel, a halo that is written, a neighbour of a channel slice overwritten, a second grid-stride trip that never runs, an
exponent that differs between the two sides of a raw copy are all small against a tensor's largest value).  The programs of
tests/exact_programs.py hold only integers that every storage format carries exactly, so each comparison below is
np.array_equal against their float64 reference (tests/test_exact_programs_cpu.py holds that reference against torch, and the
programs to the exactness rule: 16 significant bits, 2^24 for float32-only outputs).

The RetinaFace front runs in 'f32' only: alone in a program it has no half-float op beside it, so the packer stores its output
unscaled and the other precisions would run the very same launch.
"""
import numpy as np
import pytest

from terran_amd import pack
from tests import exact_programs as ep
from tests.util import run_exact as run, same

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def ctx():
    from terran_amd import lib
    c = lib.Context(0)
    yield c
    c.close()


# ---- preprocess -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('mode', ['retinaface', 'openpose', 'arcface_crops'])
def test_preprocess(ctx, mode):
    """All three modes into the halo-padded 4-channel input tensor: RetinaFace BGR 0..255; OpenPose RGB x / 255 - 0.5, the division
    correctly rounded on both sides; ArcFace planar BGR crops (x - 127.5) 2^-7, exact.  The 4th channel is 0."""
    from terran_amd import lib
    kind = {'retinaface': pack.MODEL_RETINAFACE, 'openpose': pack.MODEL_OPENPOSE, 'arcface_crops': pack.MODEL_ARCFACE}[mode]
    m = lib.Model(ctx, ep.preprocess_net(kind).P)
    shapes = [(112, 112)] if mode == 'arcface_crops' else [(1, 1), (1, 7), (5, 1), (17, 23)]
    seen = set()
    for n in (1, 3):
        for h, w in shapes:
            fr = ep.frames(200 + 10 * n + h, n, h, w)
            seen |= set(np.unique(fr).tolist())
            x = np.transpose(fr, (0, 3, 1, 2)).astype(np.float32)                    # (n, 3, h, w) in the order of the frame's bytes
            if mode == 'arcface_crops':
                m.forward_crops(np.ascontiguousarray(np.transpose(fr, (0, 3, 1, 2))))     # planar crops: channel c is network channel c
                want = (x - np.float32(127.5)) * np.float32(2.0 ** -7)
                assert np.array_equal(want.astype(np.float64), (x.astype(np.float64) - 127.5) / 128.0)
            else:
                frames = ctx.upload(fr)
                m.forward_frames(frames)
                want = x[:, ::-1] if mode == 'retinaface' else x / np.float32(255) - np.float32(0.5)
            got = m.read('input')
            same(got[:, :3], want, '%s %dx%dx%d' % (mode, n, h, w))
            assert got.shape[1] == 4 and not got[:, 3].any()
    assert seen == set(range(256))
    m.free()


# ---- depthwise 3x3 --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('precision', ep.PRECISIONS)
@pytest.mark.parametrize('C', ep.DW_CHANNELS, ids=lambda c: 'C%d' % c if c else 'on_input')
def test_dwconv(ctx, precision, C):
    """Stride 1 and 2, ReLU on and off, weights with negative taps, on maps from 1 x 1 up; with C = 32 / 64 both operands are in
    the precision's pair format (ta_ld4 and ta_st4)."""
    net = ep.dwconv_net(precision, C)
    names = ['dw_s%d_r%d' % v for v in ep.DW_VARIANTS] + (['src'] if C else ['input'])
    for h, w in ep.DW_SHAPES:
        run(ctx, net, ep.frames(300 + h * 31 + w, 2, h, w), names, 'dwconv C%d %s' % (C, precision))
    net.model.free()


# ---- 2x2 max-pool ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('precision', ep.PRECISIONS)
@pytest.mark.parametrize('in_halo', [0, 1], ids=['halo0', 'halo1'])
@pytest.mark.parametrize('C', ep.POOL_CHANNELS, ids=lambda c: 'C%d' % c)
def test_maxpool(ctx, precision, C, in_halo):
    """Floor: the last row / column of an odd map must not leak in.  Windows that are negative throughout (channels 5, 13, ...
    of the selector).  The pooled tensor has halo 1; the 3 x 3 conv behind it is exact only if that halo is still zero."""
    net = ep.maxpool_net(precision, C, in_halo)
    for h, w in ep.POOL_SHAPES:
        ref = run(ctx, net, ep.frames(400 + h * 31 + w, 2, h, w), ['input' if C == 4 else 'src', 'pooled', 'after'], 'maxpool C%d %s' % (C, precision))
        assert ref['pooled'].shape[2:] == (h // 2, w // 2)
    net.model.free()


# ---- channel-slice copy ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('precision', ep.PRECISIONS)
@pytest.mark.parametrize('case', sorted(ep.COPY_CASES))
def test_copych(ctx, precision, case):
    """A slice between tensors of different channel totals and halos, into a destination a conv has written before: the copied
    channels are the source's, every other channel is still the conv's, the halo is still zero (3 x 3 conv behind it).  Offsets
    that are multiples of 32 leave both tensors in the precision's pair format; one that is not falls back to float32."""
    net = ep.copych_net(precision, *ep.COPY_CASES[case])
    fmt = net.P.tensor_formats()
    want = pack.FMT_F32 if case == 'offset4_falls_back_to_f32' else pack.SPLIT_FMT[pack.PRECISIONS[precision]]
    assert fmt[net.tid['src']] == fmt[net.tid['dst']] == want
    for h, w in ep.COPY_SHAPES:
        run(ctx, net, ep.frames(500 + h * 31 + w, 2, h, w), ['src', 'dst', 'after'], 'copych %s %s' % (case, precision))
    net.model.free()


# ---- conv + fused pool ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('precision', ep.PRECISIONS)
def test_conv_with_fused_pool_equals_conv_then_pool(ctx, precision):
    """Program.conv(pool=True), 32 -> 64 channels, against the same conv followed by OP_MAXPOOL (bit-identical) and against the
    float64 reference, on conv outputs of 2 x 2, 5 x 7, 8 x 8 and 9 x 16."""
    net = ep.convpool_net(precision)
    for h, w in ep.CONVPOOL_SHAPES:
        run(ctx, net, ep.frames(600 + h * 31 + w, 2, h, w), ['src', 'full', 'pooled', 'fused'], 'conv+pool %s' % precision)
        assert np.array_equal(net.model.read('fused'), net.model.read('pooled'))
    net.model.free()


# ---- depthwise + pointwise block ------------------------------------------------------------------------------------------------
def _dwpw(ctx, monkeypatch, precision, C, cout, stride, shapes):
    """The block on every frame size of `shapes` with the lean and the generic kernel (TA_DWPW_GENERIC): both equal to the exact
    reference, computed once per size; ctx.kernel_work() names the kernel that ran."""
    refs = {}
    for generic in (False, True):
        if generic:
            monkeypatch.setenv('TA_DWPW_GENERIC', '1')
        else:
            monkeypatch.delenv('TA_DWPW_GENERIC', raising=False)
        net = ep.dwpw_net(precision, C, cout, stride)
        for n, h, w in shapes:
            ctx.kernel_work(reset=True)
            refs[n, h, w] = run(ctx, net, ep.frames(700 + h * 31 + w, n, h, w), ['src', 'block'], 'dwpw %s generic=%d' % (precision, generic), ref=refs.get((n, h, w)))
            kernels = sorted(k for k in ctx.kernel_work() if 'dwpw' in k)
            lean = precision == 'f16x3' and not generic
            assert lean == (ep.dwpw_lean_ok(precision, C, cout) and not generic)
            assert kernels and all(k.startswith('rf_dwpw_kernel' if lean else 'conv_dwpw') for k in kernels), kernels
        net.model.free()


@pytest.mark.parametrize('precision', ['f32', 'f16x3'])
@pytest.mark.parametrize('C,cout,stride', ep.DWPW_CASES)
def test_dwpw(ctx, monkeypatch, precision, C, cout, stride):
    """The (C, cout, stride) of test_rf_dwpw_kernel_equals_the_generic_kernel, both kernels (TA_DWPW_GENERIC): not only equal to each
    other but equal to the exact reference.  ep.DWPW_SHAPES: odd maps, whole pixel tiles of 64 and of 128 (M = 64, 128, 256), one pixel
    either side of them, tiles that hold the end of one odd image and the start of the next.  The cases of 320 and 1024 input channels
    (on one 5 x 7 map) are the only runs of the loop that loads the depthwise table beyond its first 768 granules, with 88 KB of LDS at
    (1024, 128); in 'f16x3' they must run rf_dwpw_kernel itself.  tests/test_exact_programs_cpu.py proves all of this from the
    mirror of the kernels' tiling, and that every sampled input channel reaches the output."""
    _dwpw(ctx, monkeypatch, precision, C, cout, stride, ep.dwpw_shapes(C))


@pytest.mark.parametrize('precision', ['f32', 'f16x3'])
@pytest.mark.parametrize('C,cout,stride', sorted(ep.DWPW_MANY_TILES))
def test_dwpw_many_tiles(ctx, monkeypatch, precision, C, cout, stride):
    """More than 8 pixel tiles: ta_xcd_tile deals whole rounds and a remainder over the 8 XCDs, as in every launch of the real
    detector (9 tiles of 128 pixels, 17 or 18 of 64; stride 2 on an odd x even map)."""
    shape = ep.DWPW_MANY_TILES[C, cout, stride]
    n, h, w = shape
    M = n * ((h - 1) // stride + 1) * ((w - 1) // stride + 1)
    for lean in (True, False):
        g = ep.dwpw_grid(cout, M, lean)
        assert g['n_pt'] > 8 and g['n_pt'] & 7, g['n_pt']
    _dwpw(ctx, monkeypatch, precision, C, cout, stride, [shape])


# ---- RetinaFace front -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('shape', ep.RFSTEM_ALL_SHAPES, ids=lambda s: 'x'.join(map(str, s)))
def test_rfstem(ctx, shape):
    """rf_stem_kernel, unfused and fused with the next block, with sparse +-1 integer weights.  ep.RFSTEM_SHAPES are the edges of the
    unfused kernel's 14 x 62 tiles of the half-resolution map.  ep.RFSTEM_FUSED_SHAPES are those of rf_stem_kernel<true>, which writes
    6 x 30 tiles of the quarter-resolution map (a 24 x 120 step in frame pixels, window from frame row 24 by - 5, column 120 bx - 5):
    21..24 x 117..120 exactly one tile at every row misalignment 3 W mod 4, with mh and mw odd (the tile's last row / column reads a
    16-channel pixel outside the map: staged as zero) and even; 25 x 121 and 43 x 235 one more and one less than whole tiles;
    48 x 240 exactly 2 x 2; 47 x 245 the smallest width at which a tile takes the unmasked x_inside copy and 49 x 244 the largest
    at which none does (three tile rows); batches whose second image starts 2 and 3 bytes off a dword; 5 x 7 smaller than a window.
    tests/test_exact_programs_cpu.py proves each from ep.rfstem_fused_geometry."""
    for fused in (False, True):
        net = ep.rfstem_net('f32', fused)
        run(ctx, net, ep.frames(50 + shape[1], *shape), ['front'], 'rfstem fused=%d' % fused)
        net.model.free()


# ---- the second trip of the grid-stride loops -----------------------------------------------------------------------------------
@pytest.mark.parametrize('kernel', sorted(ep.SECOND_TRIP))
def test_second_trip_of_the_grid_stride_loop(ctx, kernel):
    """grid_for caps a launch at 2048 x 256 threads; with a few more work items than that the loop's second trip has to run."""
    (h, w), total = ep.SECOND_TRIP[kernel]
    fr = ep.frames(800, 1, h, w)
    if kernel == 'preprocess':
        net, names, items = ep.preprocess_net(pack.MODEL_RETINAFACE), ['input'], 1 * h * w
    elif kernel == 'dwconv':
        net, names, items = ep.dwconv_net('f32', 32, variants=((1, 1),)), ['dw_s1_r1'], 1 * h * w * (32 // 4)
    elif kernel == 'maxpool':
        net, names, items = ep.maxpool_net('f32', 64, 0, with_sink=False), ['pooled'], 1 * (h // 2) * (w // 2) * (64 // 4)
    else:
        net, names, items = ep.copych_net('f32', 32, 64, 0, 0, 32, with_sink=False), ['dst'], 1 * h * w * (32 // 4)
    assert items == total and total > 524288
    run(ctx, net, fr, names, 'second trip: ' + kernel)
    net.model.free()
