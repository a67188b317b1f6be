"""-m gpu: the oldest device code of the recognition path at its edges -- the aligned crop (csrc/arcface_post.hip
warp_kernel), the row normalisation and the cosine matrix of the same file, the resize and paste kernels of resident frames
(csrc/frames.hip) and their Pillow-bicubic resize (ta_frames_resize_bicubic on the kernels of csrc/resample.hip).

References: real Pillow through tests/golden/align.npz (tests/golden/make_golden_align.py) for the warp and the bicubic
resize; beyond the fixture their numpy restatements, which tests/test_align_cpu.py holds bit for bit to the fixture and to
live Pillow; float64 numpy for the normalisation and the cosine; oracle.facade.cv2_resize_linear for `Frames.resize` (cv2
itself is absent here, so parity with cv2 stays UNPINNED, as in tests/test_gpu_pipeline.py); a numpy model for the paste.
"""
import numpy as np
import pytest

from oracle import arcface_pre, facade
from tests import align_cases
from tests.test_gpu_pipeline import EMB_TOL

pytestmark = pytest.mark.gpu

COS_ATOL = 2.4e-7      # the kernel accumulates in float64 and rounds once to float32 a value of magnitude at most 2: at most
                       # 2^-23 = 1.2e-7; the margin is a factor of two
L2_ATOL = 1e-6         # a lane's partial sum is at most 8 rounded products and adds, six butterfly adds follow: the sum is
                       # within about 15 x 2^-24 relative; the square root halves that, two more roundings come from the
                       # square root and the division: below 8e-7 of a component of size at most 1


@pytest.fixture(scope='module')
def ctx():
    from terran_amd import runtime
    return runtime.get_context(0)


@pytest.fixture(scope='module')
def arc(states):
    from terran_amd import ArcFace
    return ArcFace(device=0, state=states('arcface'), precision='f32')


@pytest.fixture(scope='module')
def warp_cases():
    return {name: (src, matrix, crop) for name, src, matrix, crop in align_cases.warp_cases()}


# ---- the aligned crop -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', align_cases.WARP_NAMES)
def test_warp_equals_pillow_on_the_fixture(arc, warp_cases, name):
    """One face from a 1-image batch per case: the reject test and its fill, the clamped taps, the last-row branch, sources of
    one pixel in a dimension, rotations, magnification and minification -- bit for bit Pillow's crop."""
    src, matrix, crop = warp_cases[name]
    frames = arc.ctx.upload(src[None])
    try:
        feats, crops = arc.embed_faces(frames, [0], [matrix], return_crops=True)
    finally:
        frames.free()
    assert crops.shape == (1, 3, 112, 112) and crops.dtype == np.uint8
    assert np.array_equal(crops[0], align_cases.bgr_chw(crop))
    assert np.isfinite(feats).all()
    np.testing.assert_allclose(np.linalg.norm(feats, axis=1), 1.0, atol=1e-5)


def test_warp_many_faces_from_several_batches(arc):
    """48 faces in ONE launch, cut from three resident batches of different sizes (2x37x53, 1x113x111, 3x1x64) through the
    per-face source table.  48 x 12 544 crop pixels are more than the launch's 2048 x 256 threads, so this is the case that
    runs the kernel's grid-stride loop.  Every crop equals the restatement on that face's own image; the embeddings are
    those of the crops; the same faces in reversed order give the reversed crops."""
    batches, src, idx, mats = align_cases.many_faces()
    n = len(mats)
    assert n == 48 and n * 112 * 112 > 2048 * 256
    assert {(int(s), int(f)) for s, f in zip(src, idx)} == \
        {(s, f) for s, (m, _, _) in enumerate(align_cases.MANY_BATCHES) for f in range(m)}
    cover = align_cases.branch_coverage(src, mats)                   # conditions on the inputs, not on the kernel
    assert cover['mixed'] >= 5 and cover['all_fill'] >= 1 and cover['last_row'] >= 1 and cover['before_left'] >= 1, cover
    ref = np.stack([align_cases.bgr_chw(arcface_pre.pil_affine_bilinear(batches[s][f], a)) for s, f, a in zip(src, idx, mats)])
    fill = (ref == 0).all(axis=1)
    assert sum(bool(f.any() and not f.all()) for f in fill) >= 5 and sum(bool(f.all()) for f in fill) >= 1
    frames = [arc.ctx.upload(b) for b in batches]
    try:
        feats, crops = arc.embed_faces_multi(frames, src, idx, mats, return_crops=True)
        feats_r, crops_r = arc.embed_faces_multi(frames, src[::-1], idx[::-1], mats[::-1], return_crops=True)
    finally:
        for f in frames:
            f.free()
    wrong = [k for k in range(n) if not np.array_equal(crops[k], ref[k])]
    assert not wrong, 'faces %s differ from the restatement' % wrong
    assert np.array_equal(crops_r, crops[::-1])
    again = arc.embed_crops(crops)
    diff = float(np.abs(feats - again).max())
    print('many faces: max |embed_faces_multi - embed_crops| = %.3g (bar %g)' % (diff, EMB_TOL))
    assert np.isfinite(feats).all() and diff <= EMB_TOL
    assert float(np.abs(feats_r - again[::-1]).max()) <= EMB_TOL


# ---- the row normalisation --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('n', [1, 3, 5, 9])
def test_l2norm_rows_and_the_tail_of_a_block(arc, n):
    """One wavefront per row, four rows per block: n = 1, 3, 5, 9 leave the last block partly empty (`row >= n`).  The
    kernel's `nrm == 0` guard needs an all-zero embedding, which no input reaches through the ABI: not tested."""
    x = align_cases.noise(500 + n, n, 3, 112, 112)
    raw = arc.embed_crops(x, normalize=False).astype(np.float64)
    got = arc.embed_crops(x, normalize=True)
    norms = np.sqrt((raw * raw).sum(1))
    assert got.shape == (n, 512) and got.dtype == np.float32 and (norms > 0).all()
    diff = float(np.abs(got - raw / norms[:, None]).max())
    print('l2norm n=%d: max |kernel - float64| = %.3g (bound %g)' % (n, diff, L2_ATOL))
    assert diff <= L2_ATOL


# ---- the cosine matrix ------------------------------------------------------------------------------------------------------
def _scaled_rows(rng, n, dim):
    """Normal rows, each scaled by its own factor between 1e-3 and 1e3."""
    return (rng.normal(size=(n, dim)) * 10.0 ** rng.uniform(-3, 3, (n, 1))).astype(np.float32)


@pytest.mark.parametrize('dim', [1, 3, 63, 64, 65, 512, 1000])
def test_cosine_vs_float64(ctx, dim):
    """Dimensions around the 64-lane stride, pair counts around the four pairs of a block, unnormalised rows."""
    rng = np.random.default_rng(600 + dim)
    worst = 0.0
    for na, nb in [(1, 1), (1, 5), (3, 3), (7, 2), (33, 17)]:
        a, b = _scaled_rows(rng, na, dim), _scaled_rows(rng, nb, dim)
        got = ctx.cosine_distance(a, b)
        ref = arcface_pre.cosine_distance(a, b)
        assert got.shape == (na, nb) and got.dtype == np.float32
        worst = max(worst, float(np.abs(got - ref).max()))
        np.testing.assert_allclose(got, ref, rtol=0, atol=COS_ATOL, err_msg='dim %d, %d x %d' % (dim, na, nb))
    print('cosine dim=%d: max |kernel - float64| = %.3g (bound %g)' % (dim, worst, COS_ATOL))


def test_cosine_exact_cases_zero_rows_and_empty_sides(ctx):
    rng = np.random.default_rng(610)
    a = _scaled_rows(rng, 6, 65)
    assert np.abs(np.diag(ctx.cosine_distance(a, a))).max() <= COS_ATOL
    np.testing.assert_allclose(np.diag(ctx.cosine_distance(a, -a)), 2.0, rtol=0, atol=COS_ATOL)
    hot = np.zeros((3, 65), np.float32)
    hot[0, 0], hot[1, 63], hot[2, 64] = 3.0, 0.25, 1e3
    d = ctx.cosine_distance(hot, hot)
    assert (d[~np.eye(3, dtype=bool)] == 1.0).all() and (np.diag(d) == 0.0).all()
    # a zero row: NaN where the oracle has it, and nowhere else
    z, b = a.copy(), _scaled_rows(rng, 5, 65)
    z[2] = 0.0
    b[4] = 0.0
    got = ctx.cosine_distance(z, b)
    with np.errstate(divide='ignore', invalid='ignore'):
        ref = arcface_pre.cosine_distance(z, b)
    nan = np.isnan(ref)
    assert nan.sum() == 6 + 5 - 1 and np.array_equal(np.isnan(got), nan)
    np.testing.assert_allclose(got[~nan], ref[~nan], rtol=0, atol=COS_ATOL)
    # an empty side: an empty matrix, no error
    for na, nb in [(0, 5), (6, 0), (0, 0)]:
        got = ctx.cosine_distance(np.zeros((na, 65), np.float32), np.zeros((nb, 65), np.float32))
        assert got.shape == (na, nb) and got.dtype == np.float32


# ---- Frames.resize ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('shape', [(1, 1, 1), (1, 1, 37), (1, 37, 1), (1, 2, 2), (3, 97, 131)])
def test_frames_resize_edges(ctx, shape):
    """Bit for bit the cv2 restatement (parity with cv2 itself UNPINNED: cv2 is absent here).  Sources of one pixel in a
    dimension (the clamped fraction of the column table), a batch of 3 (the image stride), targets of the same size, 1 x 1,
    8 x each side, ceil(side / 8) and 33 x 200; 3 x 97 x 131 -> 420 x 420 is 529 200 pixels, more than the launch's
    2048 x 256 threads: the grid-stride loop."""
    n, h, w = shape
    imgs = align_cases.noise(700 + h + w, n, h, w, 3)
    targets = [(h, w), (1, 1), (8 * h, 8 * w), (-(-h // 8), -(-w // 8)), (33, 200)]
    if n == 3:
        targets.append((420, 420))
        assert n * 420 * 420 > 2048 * 256
    fr = ctx.upload(imgs)
    try:
        for dh, dw in targets:
            out = fr.resize(dh, dw)
            try:
                got = out.download()
            finally:
                out.free()
            ref = np.stack([facade.cv2_resize_linear(im, (dw, dh)) for im in imgs])
            assert got.shape == ref.shape and np.array_equal(got, ref), (shape, dh, dw)
    finally:
        fr.free()


# ---- Frames.resize_bicubic --------------------------------------------------------------------------------------------------
def _bicubic(ctx, imgs, w, h):
    fr = ctx.upload(imgs)
    try:
        out = fr.resize_bicubic(h, w)
        try:
            return out.download()
        finally:
            out.free()
    finally:
        fr.free()


def test_frames_resize_bicubic_equals_pillow_on_the_fixture(ctx):
    """Reduction by 8 (33 coefficients per output pixel), enlargement, sources of one pixel in a dimension, each pass
    skipped in turn and the copy: bit for bit Pillow's Image.resize."""
    for src, (w, h), expected in align_cases.bicubic_cases():
        got = _bicubic(ctx, src[None], w, h)
        assert got.shape == (1, h, w, 3) and np.array_equal(got[0], expected), (src.shape, w, h)


def test_frames_resize_bicubic_batch_and_grid_stride(ctx):
    """A batch of 3 (the per-image offsets of the horizontal result and of the output), and one 600 x 450 image to
    900 x 600: 15 tiles of 64 pixels across, 29 groups of 16 rows in the horizontal pass and 150 groups of 4 rows in the
    vertical one, the last tile of each partly empty."""
    imgs = align_cases.noise(800, 3, 80, 96, 3)
    got = _bicubic(ctx, imgs, 12, 10)
    for k in range(3):
        assert np.array_equal(got[k], arcface_pre.pil_resize_bicubic(imgs[k], (12, 10))), k
    big = align_cases.noise(801, 450, 600, 3)
    assert 900 * 600 > 2048 * 256
    assert np.array_equal(_bicubic(ctx, big[None], 900, 600)[0], arcface_pre.pil_resize_bicubic(big, (900, 600)))


def _whole_frames(ctx, imgs, w, h):
    """Frames.resample of one whole-frame region per image, BICUBIC."""
    from terran_amd import lib
    regions = np.zeros(len(imgs), lib.RESAMPLE_DT)
    regions['frame'], regions['x1'], regions['y1'] = np.arange(len(imgs)), imgs.shape[2], imgs.shape[1]
    fr = ctx.upload(imgs)
    try:
        out = fr.resample(regions, h, w, lib.BICUBIC)
        try:
            return out.download()
        finally:
            out.free()
    finally:
        fr.free()


def test_frames_resize_bicubic_equals_resample_of_whole_frames(ctx):
    """The two entries of the shared resampler agree: every case of the fixture, and a batch of 3."""
    cases = [(src[None], size) for src, size, _ in align_cases.bicubic_cases()] + [(align_cases.noise(810, 3, 21, 34, 3), (9, 40))]
    for imgs, (w, h) in cases:
        got = _bicubic(ctx, imgs, w, h)
        assert got.shape == (len(imgs), h, w, 3) and np.array_equal(got, _whole_frames(ctx, imgs, w, h)), (imgs.shape, w, h)


@pytest.mark.parametrize('shape,size', align_cases.BICUBIC_EDGE_CASES, ids=lambda v: 'x'.join(map(str, v)))
def test_frames_resize_bicubic_tile_edges_skipped_passes_and_the_lds_switch(ctx, shape, size):
    """Batches of 2 against the restatement of Pillow.  align_cases.BICUBIC_TILE_EDGES: one pixel and row past, exactly on and
    one short of the 64-pixel tile, the 16 source rows of a horizontal group and the 4 output rows of a vertical one.
    BICUBIC_SKIPS: the vertical pass skipped, the horizontal one skipped, both (the result is the input).  BICUBIC_LDS_SWITCH:
    127 and 129 coefficients per output column, 2045 and 2049 per output row -- the last counts staged in LDS and the first
    read from global memory (tests/test_resample_cpu.py holds the planned tables to these counts)."""
    (n, h, w), (oh, ow) = shape, size
    imgs = align_cases.noise(820 + h + w, n, h, w, 3)
    got = _bicubic(ctx, imgs, ow, oh)
    assert got.shape == (n, oh, ow, 3)
    for k in range(n):
        assert np.array_equal(got[k], arcface_pre.pil_resize_bicubic(imgs[k], (ow, oh))), k
    if (oh, ow) == (h, w):
        assert np.array_equal(got, imgs)


def test_frames_resize_bicubic_of_an_empty_batch(ctx):
    fr = ctx.upload(np.zeros((0, 5, 7, 3), np.uint8))
    try:
        out = fr.resize_bicubic(3, 4)
        try:
            assert out.shape == (0, 3, 4, 3)
        finally:
            out.free()
    finally:
        fr.free()


def test_frames_resize_bicubic_refusals(ctx):
    from terran_amd import lib
    imgs = align_cases.noise(830, 2, 5, 7, 3)
    fr = ctx.upload(imgs)
    try:
        for h, w in [(0, 4), (3, -1)]:
            with pytest.raises(lib.TerranAmdError) as e:
                fr.resize_bicubic(h, w)
            assert e.value.code == lib.E_INVALID and 'frames_resize_bicubic:' in str(e.value), (h, w)
            assert np.array_equal(fr.download(), imgs)
    finally:
        fr.free()


# ---- Frames.paste -----------------------------------------------------------------------------------------------------------
def test_frames_paste_corners_edges_and_refusals(ctx):
    """The canvas is an uploaded pattern without zeros, and after every paste the WHOLE canvas is compared with a numpy model:
    what a paste must not touch is checked as unchanged, not as zero."""
    from terran_amd import lib
    model = (align_cases.noise(900, 3, 40, 50, 3) | 1).astype(np.uint8)
    src_np = align_cases.noise(901, 2, 5, 7, 3)
    dot_np = align_cases.noise(902, 1, 1, 1, 3)
    full_np = align_cases.noise(903, 1, 40, 50, 3)
    canvas, src, dot, full = (ctx.upload(a) for a in (model, src_np, dot_np, full_np))
    try:
        for top, left in [(0, 0), (0, 50 - 7), (40 - 5, 0), (40 - 5, 50 - 7)]:        # top + h == H and left + w == W exactly
            canvas.paste(src, 1, 2, top, left)
            model[2, top:top + 5, left:left + 7] = src_np[1]
            assert np.array_equal(canvas.download(), model), (top, left)
        canvas.paste(dot, 0, 0, 39, 49)
        model[0, 39, 49] = dot_np[0, 0, 0]
        assert np.array_equal(canvas.download(), model)
        canvas.paste(full, 0, 1, 0, 0)
        model[1] = full_np[0]
        assert np.array_equal(canvas.download(), model)
        for args in [(1, 2, -1, 0), (1, 2, 0, -1), (1, 2, 40 - 5 + 1, 0), (1, 2, 0, 50 - 7 + 1), (2, 2, 0, 0), (1, 3, 0, 0)]:
            with pytest.raises(lib.TerranAmdError):
                canvas.paste(src, *args)
            assert np.array_equal(canvas.download(), model), args
    finally:
        for f in (canvas, src, dot, full):
            f.free()


def test_frames_paste_grid_stride(ctx):
    """450 x 400 x 3 = 540 000 bytes, more than the launch's 2048 x 256 threads of one byte each: the grid-stride loop."""
    big = align_cases.noise(904, 1, 450, 400, 3)
    model = (align_cases.noise(905, 2, 450, 400, 3) | 1).astype(np.uint8)
    assert 450 * 400 * 3 > 2048 * 256
    canvas, src = ctx.upload(model), ctx.upload(big)
    try:
        canvas.paste(src, 0, 1, 0, 0)
        model[1] = big[0]
        assert np.array_equal(canvas.download(), model)
    finally:
        canvas.free()
        src.free()
