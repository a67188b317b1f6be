"""-m gpu: tiled pose estimation.  The merge (ta_poses_merge) against the model of tests/pose_tiles_model.py, bit for bit and with no
tolerance anywhere, at the wave, workgroup and bit-word seams of its kernels, past a 32-bit squared distance, at every boundary of
its definition, through its capacity protocol and its errors; OpenPose.estimate_tiles and TiledEstimation against the same steps
made by hand with the calls that existed before; and the one-tile identity."""
import ctypes as C

import numpy as np
import pytest

from tests import pose_tiles_model as pm

pytestmark = pytest.mark.gpu

NAMES = ('counts', 'keypoints', 'scores', 'source')
CASES = pm.boundary_cases()


@pytest.fixture(scope='module')
def ctx():
    from terran_amd import lib
    c = lib.Context(0)
    yield c
    c.close()


def same(got, want):
    for a, b, what in zip(got, want, NAMES):
        assert a.dtype == b.dtype and a.shape == b.shape, (what, a.dtype, b.dtype, a.shape, b.shape)
        assert np.array_equal(a, b), (what, int(np.argmax(np.any((a != b).reshape(len(a), -1), axis=1))))


def check(ctx, groups, n_frames, kp, sc, params=(0.1, 0.5, 3, 0), stats=None, want=None):
    if want is None:
        want = pm.merge_model(groups, n_frames, kp, sc, *params, stats=stats)
    got = ctx.poses_merge(pm.records(groups), n_frames, kp, sc, *params)
    same(got, want)
    return got


# ---- the seams ---------------------------------------------------------------------------------------------------------------------
SEAM_COUNTS = (65, 0, 1, 63, 2049, 64, 1025)          # per frame; frame 1 is empty between two that are not
SEAM_PARAMS = [(0.1, 0.5, 3, 0), (0.1, 0.5, 3, 12), (0.25, 1.0, 1, 0), (0.05, 0.3, 6, 7)]


@pytest.fixture(scope='module')
def seams():
    """Seven frames with SEAM_COUNTS candidates, each frame's dealt out to up to three groups with their own origins, rectangles and
    interior bits; clusters of near-duplicates whose copies land in different groups or in one, in the even frames a quarter of them
    exact copies with equal scores.  The model's answers are computed once per parameter set and shared."""
    rng = np.random.default_rng(11)
    groups, parts, first = [], [], 0
    for f, n in enumerate(SEAM_COUNTS):
        extent = 2400 if n > 1000 else 600
        kp, sc = pm.clustered_poses(rng, n, extent, exact=f % 2 == 0)
        groups += pm.split(rng, f, first, kp, extent)
        parts.append((kp, sc))
        first += n
    kp, sc = np.concatenate([p[0] for p in parts]), np.concatenate([p[1] for p in parts])
    answers = {}

    def model(params):
        if params not in answers:
            stats = {}
            answers[params] = (pm.merge_model(groups, len(SEAM_COUNTS), kp, sc, *params, stats=stats), stats)
        return answers[params]
    return groups, kp, sc, model


@pytest.mark.parametrize('params', SEAM_PARAMS)
def test_merge_seams(ctx, seams, params):
    groups, kp, sc, model = seams
    want, stats = model(params)
    counts = want[0]
    print('radius %g agree %g min_shared %d edge %d: %s -> %s' % (params + (stats, counts.tolist())))
    assert stats['candidates'] == sum(SEAM_COUNTS) and stats['suppressed'] > 100 and (stats['cut'] > 0) == (params[3] > 0)
    assert stats['empty'] > 0 and counts[1] == 0 and (counts[[0, 4, 6]] > 0).all()
    check(ctx, groups, len(SEAM_COUNTS), kp, sc, params, want=want)


def test_merge_in_batches_of_frames(ctx, seams, monkeypatch):
    """The matrices of a call are cut in batches of frames that fit a budget of scratch memory: with room for one frame's at a time
    the answer is the same."""
    groups, kp, sc, model = seams
    monkeypatch.setenv('TA_PM_MATRIX_BYTES', str(2049 * 33 * 8))
    check(ctx, groups, len(SEAM_COUNTS), kp, sc, SEAM_PARAMS[0], want=model(SEAM_PARAMS[0])[0])


def test_no_32_bit_distance(ctx):
    """The same skeleton (100 x 300, so a joint may lie 17 pixels off) in four groups: as it is; 65536 pixels to the right (by its
    coordinates), dx * dx = 2^32; 65536 pixels down (by its group's origin); 3 pixels to the right.  The far ones stay, the near one
    goes; a 32-bit squared distance would be 0 for the far ones and remove them."""
    rng = np.random.default_rng(2)
    a = np.stack([rng.integers(1000, 1100, 18), rng.integers(2000, 2300, 18), np.ones(18, np.int64)], axis=1).astype(np.int32)
    right, near = a.copy(), a.copy()
    right[:, 0] += 65536
    near[:, 0] += 3
    groups = [pm.group(0, 0, 1), pm.group(0, 1, 1), pm.group(0, 2, 1, oy=65536), pm.group(0, 3, 1)]
    kp, sc = np.stack([a, right, a, near]), np.array([0.9, 0.8, 0.7, 0.6])
    counts, okp, _, src = check(ctx, groups, 1, kp, sc)
    assert counts.tolist() == [3] and src.tolist() == [0, 1, 2]
    assert np.array_equal(okp[2, :, 1], a[:, 1] + 65536) and np.array_equal(okp[1, :, 0], a[:, 0] + 65536)
    # and at the largest coordinates the call takes, on both sides of the bound
    far = a.copy()
    far[:, 0] += (1 << 22) - 1 - far[:, 0].max()
    groups = [pm.group(0, 0, 1), pm.group(0, 1, 1, ox=(1 << 22) - 1, oy=-(1 << 22) + 1), pm.group(0, 2, 1, ox=(1 << 22) - 1, oy=-(1 << 22) + 1)]
    counts, _, _, src = check(ctx, groups, 1, np.stack([far, a, near]), sc[:3])
    assert src.tolist() == [0, 1]                      # rows 1 and 2 are 3 pixels apart after the same origin; row 0 is far from both


# ---- the boundary cases of the CPU file on the device ----------------------------------------------------------------------------------
@pytest.mark.parametrize('name', sorted(CASES))
def test_boundary_case_on_the_device(ctx, name):
    groups, n_frames, kp, sc, params, source = CASES[name]
    got = check(ctx, groups, n_frames, kp, sc, params)
    assert got[3].tolist() == source


# ---- capacity protocol and errors ----------------------------------------------------------------------------------------------------
def raw_merge(ctx, groups, n_frames, kp, sc, capacity, outputs=True):
    from terran_amd import lib
    g = pm.records(groups)
    counts = np.full(max(n_frames, 1), -1, np.int32)
    cap = max(capacity, 1)
    okp, osc, src = np.full((cap, 18, 3), -7, np.int32), np.full(cap, np.nan, np.float64), np.full(cap, -1, np.int32)
    req = C.c_int32(-1)
    out = [lib.ptr(a) if outputs else None for a in (okp, osc, src)]
    rc = ctx.lib.ta_poses_merge(ctx.h, lib.ptr(g) if len(g) else None, len(g), n_frames, lib.ptr(kp), lib.ptr(sc), len(sc), 0.1, 0.5, 3, 0,
                                int(capacity), lib.ptr(counts), *out, C.byref(req))
    return rc, counts[:n_frames], okp, osc, src, int(req.value)


def test_merge_capacity_protocol(ctx):
    from terran_amd import lib
    rng = np.random.default_rng(8)
    kp, sc = pm.clustered_poses(rng, 200, 500)
    groups = pm.split(rng, 0, 0, kp[:120], 500) + pm.split(rng, 2, 120, kp[120:], 500)
    want = pm.merge_model(groups, 3, kp, sc)
    total = int(want[0].sum())
    assert 0 < total < 200 and want[0][1] == 0
    rc, counts, okp, osc, src, required = raw_merge(ctx, groups, 3, kp, sc, total - 1)
    assert rc == lib.E_CAPACITY and required == total and np.array_equal(counts, want[0])
    assert (okp == -7).all() and np.isnan(osc).all() and (src == -1).all()                # nothing was written
    rc, counts, okp, osc, src, required = raw_merge(ctx, groups, 3, kp, sc, total)
    assert rc == lib.OK and required == total
    same((counts, okp, osc, src), want)
    rc, counts, _, _, _, required = raw_merge(ctx, groups, 3, kp, sc, 0, outputs=False)
    assert rc == lib.E_CAPACITY and required == total and np.array_equal(counts, want[0])
    rc, counts, _, _, _, required = raw_merge(ctx, [], 3, kp, sc, 0, outputs=False)          # nothing to merge
    assert rc == lib.OK and required == 0 and counts.tolist() == [0, 0, 0]
    same(ctx.poses_merge(pm.records(groups), 3, kp, sc, capacity=1), want)                   # the wrapper grows and retries
    # a negative capacity counts as 0: short when there is a pose, enough when there is none
    rc, counts, _, _, _, required = raw_merge(ctx, groups, 3, kp, sc, -1, outputs=False)
    assert rc == lib.E_CAPACITY and required == total and np.array_equal(counts, want[0])
    rc, counts, _, _, _, required = raw_merge(ctx, [pm.group(0, 0, 4)], 1, np.zeros((4, 18, 3), np.int32), np.zeros(4), -1, outputs=False)
    assert rc == lib.OK and required == 0 and counts.tolist() == [0]


def test_merge_errors(ctx):
    from terran_amd import lib
    n = lib.MERGE_MAX_PER_FRAME + 1                      # the limit is checked on the host, before any launch
    kp, sc = np.zeros((n, 18, 3), np.int32), np.zeros(n)
    with pytest.raises(lib.TerranAmdError, match=str(lib.MERGE_MAX_PER_FRAME)) as e:
        ctx.poses_merge(pm.records([pm.group(0, 0, n - 5), pm.group(0, n - 5, 5)]), 1, kp, sc)
    assert e.value.code == lib.E_OVERFLOW
    assert ctx.poses_merge(pm.records([pm.group(0, 0, n - 1)]), 1, kp[:n - 1], sc[:n - 1])[0].tolist() == [0]     # the limit itself: all empty
    kp, sc = kp[:10].copy(), sc[:10]
    kp[:, :3] = 1
    ok = [pm.group(0, 0, 2)]
    wild_x, wild_y, absent = kp.copy(), kp.copy(), kp.copy()
    wild_x[3, 5, 0], wild_y[3, 17, 1], absent[3, 9] = 1 << 22, -(1 << 22), (1 << 22, 0, 0)
    for groups, args, kw, what in (
            ([pm.group(1, 0, 2), pm.group(0, 2, 2)], kp, {}, 'sorted'), ([pm.group(0, 0, 3), pm.group(0, 2, 2)], kp, {}, 'belongs to groups'),
            ([pm.group(2, 0, 2)], kp, {}, 'frame 2'), ([pm.group(-1, 0, 2)], kp, {}, 'frame -1'), ([pm.group(0, 8, 3)], kp, {}, 'not inside'),
            ([pm.group(0, -1, 3)], kp, {}, 'not inside'),
            (ok, kp, dict(radius=-0.5), 'radius'), (ok, kp, dict(radius=float('inf')), 'radius'), (ok, kp, dict(radius=float('nan')), 'radius'),
            (ok, kp, dict(agree=0.0), 'agree'), (ok, kp, dict(agree=1.5), 'agree'), (ok, kp, dict(agree=float('nan')), 'agree'),
            (ok, kp, dict(min_shared=0), 'min_shared'), (ok, kp, dict(min_shared=19), 'min_shared'), (ok, kp, dict(edge=-1), 'edge'),
            ([pm.group(0, 0, 2, ox=1 << 22)], kp, {}, 'origin'), ([pm.group(0, 0, 2, oy=-(1 << 22))], kp, {}, 'origin'),
            ([pm.group(0, 0, 5)], wild_x, {}, 'row 3'), ([pm.group(0, 0, 5)], wild_y, {}, 'row 3'), ([pm.group(0, 0, 5)], absent, {}, 'row 3')):
        with pytest.raises(lib.TerranAmdError, match=what) as e:
            ctx.poses_merge(pm.records(groups), 2, args, sc, **kw)
        assert e.value.code == lib.E_INVALID, what
    assert ctx.poses_merge(pm.records([pm.group(0, 0, 3)]), 2, wild_x, sc)[0].tolist() == [3, 0]   # a row in no group is not looked at
    with pytest.raises(ValueError, match='scores'):
        ctx.poses_merge(pm.records(ok), 1, kp, sc[:4])


# ---- estimate_tiles and the facade against the steps by hand -----------------------------------------------------------------------------
def arrays(per_image):
    flat = [p for poses in per_image for p in poses]
    kp = np.stack([p['keypoints'] for p in flat]) if flat else np.zeros((0, 18, 3), np.int32)
    return np.array([len(poses) for poses in per_image], np.int32), kp, np.array([p['score'] for p in flat], np.float64)


def by_hand_case(zoom):
    """zoom 0.5: two coded frames of 256 x 384 blown up to 512 x 768 (`synth.upscale_for_resize`: every 2 x 2 block holds one coded
    pixel), tile 384, overlap 128 -- origins y 0, 128; x 0, 256, 384, all even, so a tile halved by the device IS a 192-pixel crop of
    the coded frame and the network sees people in it -- and a whole-frame pass at short side 256, which halves the frame exactly as
    well.  zoom 1.5: the coded frames themselves, tile 192, overlap 64, whole-frame pass at 184: coded frames do not survive an
    enlargement, so every candidate comes from the whole-frame pass; the case stays for the enlarging resize and its chunks.
    -> (frames, tile, overlap, short side of the whole-frame pass, the origins expected)"""
    from terran_amd import synth
    coded = synth.pose_code_frames(60, 2, 256, 384, 6)
    if zoom == 0.5:
        return synth.upscale_for_resize(coded, 512, 768), 384, 128, 256, [[y, x] for y in (0, 128) for x in (0, 256, 384)]
    return coded, 192, 64, 184, [[y, x] for y in (0, 64) for x in (0, 128, 192)]


@pytest.mark.parametrize('zoom', [0.5, 1.5])
def test_estimate_tiles_equals_the_steps_by_hand(ctx, states, zoom):
    """Two frames cut in twelve tiles (chunks of 7 and 5) and a whole-frame pass (`by_hand_case`).  Expected: the tiles cropped on the
    host, uploaded and run through `OpenPose.call_frames` at short side int(tile * zoom) -- its own resize and its own
    ta_openpose_run, with the scale it works out itself -- the whole frames through `call_frames`, `tiles.pose_groups`, the model of
    the merge.  At zoom 0.5 real tile poses go through the resize and the division by the scale: at least 4 of them and at least 1
    suppression are asserted on the by-hand candidates.

    The network is the seeded one with the decoder channels (`states('openpose_decoder')`) on coded frames: the plain seeded
    network (`states('openpose')` on `synth.frames`) assembles no person at any seed or size (terran_amd/weights.py says why; the
    oracle's pose path gave 0 poses for seeds 20 .. 31 at 256 x 384, tile 192, zoom 1.5)."""
    from terran_amd import OpenPose, TiledEstimation, tiles
    fr, T, overlap, short_side, expected_origins = by_hand_case(zoom)
    H, W = fr.shape[1:3]
    te = TiledEstimation(tile=T, overlap=overlap, zoom=zoom, full_frame=True, short_side=short_side, device=0, state=states('openpose_decoder'),
                         max_tiles=7)
    mctx = te._ctx()
    origins = tiles.tile_grid(H, W, T, overlap)
    assert origins.tolist() == expected_origins
    crops = np.stack([fr[f, y:y + T, x:x + T] for f in range(2) for y, x in origins])
    by_tile = OpenPose(device=0, short_side=int(T * zoom), state=states('openpose_decoder'), ctx=mctx)
    parts = []
    for lo in range(0, len(crops), 7):
        up = mctx.upload(crops[lo:lo + 7])
        parts.append(arrays(by_tile.call_frames(up)))
        up.free()
    tile_counts = np.concatenate([p[0] for p in parts])
    up = mctx.upload(fr)
    parts.append(arrays(te.model.call_frames(up)))
    groups = tiles.pose_groups(2, H, W, origins, T, T, tile_counts, parts[-1][0])
    kp, sc = np.concatenate([p[1] for p in parts]), np.concatenate([p[2] for p in parts])
    stats = {}
    want = pm.merge_model(groups, 2, kp, sc, 0.1, 0.5, 3, 0, stats)
    counts = want[0]
    print('zoom %g: %d tile poses, %s -> %s' % (zoom, tile_counts.sum(), stats, counts.tolist()))
    assert counts.sum() >= 4
    if zoom == 0.5:
        assert tile_counts.sum() >= 4 and stats['suppressed'] >= 1
        assert kp[:tile_counts.sum(), :, :2].max() > T // 2                              # tile coordinates, not those of the halved tile
    same(te.model.estimate_tiles(up, T, overlap, zoom, short_side, 0, 0.1, 0.5, 3, 7), want[:3])
    for images in (fr, up, [fr[1], fr[0][:H - 56], fr[0]]):
        got = te(images)
        if isinstance(images, list):
            assert len(got) == 3 and isinstance(got[1], list)
            got = [got[2], got[0]]                                                      # a mixed-size list answers in input order
        assert all(p['keypoints'].dtype == np.int32 and p['keypoints'].shape == (18, 3) and isinstance(p['score'], np.float64)
                   for poses in got for p in poses)
        same(arrays(got), want[:3])
    one = te(fr[0])
    assert len(one) == counts[0] and np.array_equal(np.stack([p['keypoints'] for p in one]), want[1][:counts[0]])
    up.free()
    by_tile.model.free()


def test_one_tile_is_call_frames(ctx, states):
    """A frame no larger than the tile, zoom = 184 / min(H, W) = 0.5, no whole-frame pass: the poses of `OpenPose.call_frames`, with
    the same keypoints and scores, in the model's order (one group per frame: nothing is compared), none lost.  The frames are coded
    184 x 248 frames blown up to 368 x 496, which the halving resize returns exactly: the network sees people."""
    from terran_amd import TiledEstimation, synth, tiles
    H, W = 368, 496
    fr = synth.upscale_for_resize(synth.pose_code_frames(61, 2, 184, 248, 4), H, W)
    zoom = 184 / min(H, W)
    te = TiledEstimation(tile=512, overlap=0.25, zoom=zoom, full_frame=False, device=0, state=states('openpose_decoder'))
    frames = te._ctx().upload(fr)
    try:
        counts, kp, sc = arrays(te.model.call_frames(frames))
        assert counts.sum() >= 4 and kp[:, :, :2].max() > 248                              # the frame's coordinates, not the network's
        want = pm.merge_model(tiles.pose_groups(2, H, W, [[0, 0]], H, W, counts), 2, kp, sc)
        assert np.array_equal(want[0], counts) and sorted(want[3].tolist()) == list(range(counts.sum()))     # none is lost
        same(te.model.estimate_tiles(frames, 512, 0.25, zoom), want[:3])
        same(arrays(te(frames)), want[:3])
    finally:
        frames.free()
