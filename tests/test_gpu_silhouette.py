"""-m gpu: silhouettes from skeletons.  ta_poses_paint against tests/silhouette_model.py with np.array_equal and no tolerance
anywhere: single capsules over every seam of the kernel's geometry (a tile is 16 rows of 16 groups of 4 pixels, a wave 4 rows, a
row's groups are cut where its bytes are dword aligned), the inclusive boundary, once-per-pose blending and list order, absent
joints, the alphas, clear, untouched frames, a crowd in one tile, the matrix cut into batches and runs of poses, a random case,
every error; then the public calls end to end against the compositions of the project's existing models.

Boxes and tables are what the header says, so nothing here is tuned to the kernel: tolerances do not exist."""
import numpy as np
import pytest

from tests import combine_model as C
from tests import resample_model as R
from tests import silhouette_model as sm
from tests import tone_model as T
from tests import vis_blur_model as B

pytestmark = pytest.mark.gpu

NONE = (0, 0, 0)                # no share of the size: every radius is min_radius


@pytest.fixture(scope='module')
def ctx():
    from terran_amd import lib
    c = lib.Context(0)
    yield c
    c.close()


def noise(seed, n, h, w):
    return np.random.default_rng(seed).integers(0, 256, (n, h, w, 3), dtype=np.uint8)


def run(ctx, host, counts, kp, rgba, permille=(90, 90, 50), min_radius=2, clear=False):
    frames = ctx.upload(host)
    try:
        ctx.poses_paint(frames, counts, kp, rgba, permille, min_radius, clear)
        return frames.download()
    finally:
        frames.free()


def check(ctx, host, counts, kp, rgba, permille=(90, 90, 50), min_radius=2, clear=False):
    kp, rgba = np.asarray(kp, np.int32).reshape(-1, 18, 3), np.asarray(rgba, np.uint8).reshape(-1, 4)
    got = run(ctx, host, counts, kp, rgba, permille, min_radius, clear)
    want = sm.paint(host.copy(), counts, kp, rgba, permille, min_radius, clear)
    assert got.dtype == np.uint8 and got.shape == want.shape
    assert np.array_equal(got, want), np.argwhere((got != want).any(-1))[:8]
    return got


def capsule(a, b):
    return sm.pose_row({3: a, 4: b})        # the LIMB segment (3, 4)


# ---- single capsules over the seams, 2 x 80 x 96 -----------------------------------------------------------------------------------
# rows of 288 bytes are dword aligned: tile columns meet at x = 59 | 60, tile rows at y = 15 | 16, 31 | 32, ...; waves at rows 3 | 4
CAPSULES = [
    ((50, 8), (70, 9), 3),          # the tile seam in x
    ((57, 2), (62, 2), 0),          # ... with r = 0: a one-pixel line over it
    ((20, 10), (25, 22), 2),        # the tile seam in y
    ((30, 1), (31, 6), 1),          # the 64-lane boundary between rows 3 and 4
    ((0, 40), (12, 40), 4),         # the left edge
    ((90, 50), (95, 60), 5),        # the right edge
    ((40, 0), (52, 3), 3),          # the top edge
    ((10, 79), (30, 75), 2),        # the bottom edge
    ((-30, -20), (15, 30), 4),      # an end at negative coordinates
    ((80, 70), (140, 120), 6),      # an end beyond the frame
    ((-9, 60), (-3, 66), 2),        # wholly outside: nothing
    ((70, 30), (70, 30), 7),        # A == B: the disc
]


def test_single_capsules_over_every_seam(ctx):
    host = noise(1, 2, 80, 96)
    rng = np.random.default_rng(2)
    for a, b, r in CAPSULES:                            # each alone, so that a wrong one is named
        ink = tuple(int(v) for v in rng.integers(0, 256, 3)) + (int(rng.integers(1, 256)),)
        got = check(ctx, host, [0, 1], capsule(a, b)[None], [ink], NONE, r)
        assert np.array_equal(got[0], host[0])
    # ... and all of them in one call, the two frames in opposite orders
    kp = np.stack([capsule(a, b) for a, b, _ in CAPSULES])
    inks = np.concatenate([rng.integers(0, 256, (len(kp), 3)), rng.integers(1, 256, (len(kp), 1))], 1)
    check(ctx, host, [len(kp), len(kp)], np.concatenate([kp, kp[::-1]]), np.concatenate([inks, inks[::-1]]), NONE, 3)


def test_the_boundary_row_is_covered_exactly(ctx):
    host = noise(3, 2, 80, 96)
    row = capsule((-16000, 10), (16000, 10))
    got = check(ctx, host, [1], row[None], [(255, 0, 0, 255)], NONE, 5)     # cross^2 = r^2 L2 in rows 5 and 15
    painted = (got[0] == (255, 0, 0)).all(-1) & (host[0] != (255, 0, 0)).any(-1)
    assert painted[5:16].all() and not painted[:5].any() and not painted[16:].any()
    # the size makes the radius as well: M = 32000, 1 permille of it is 32; 0 permille leaves min_radius
    got = check(ctx, host, [1], row[None], [(0, 255, 0, 255)], (1000, 1000, 1), 5)
    assert (got[0, :43] == (0, 255, 0)).all() and not (got[0, 43] == (0, 255, 0)).all(-1).any()


def test_odd_widths_walk_every_phase(ctx):
    """Rows of 3 * 75 = 225 and 3 * 37 = 111 bytes start at every address mod 4: heads, tails and groups that straddle."""
    for h, w in ((37, 75), (19, 37), (5, 3), (3, 1)):
        host = noise(h, 2, h, w)
        rng = np.random.default_rng(w)
        kp = np.stack([sm.person(rng, rng.integers(0, w), rng.integers(0, h), rng.integers(10, 40), absent=0.2) for _ in range(12)])
        inks = rng.integers(0, 256, (12, 4))
        check(ctx, host, [7, 5], kp, inks)
        check(ctx, host, [7, 5], kp, inks, clear=True)
        check(ctx, host, [1], capsule((-5, h // 2), (w + 5, h // 2))[None], [(9, 8, 7, 200)], NONE, 1)


# ---- once per pose, list order, absent joints, alpha ------------------------------------------------------------------------------
def test_crossing_limbs_blend_once_and_order_counts(ctx):
    host = noise(4, 2, 80, 96)
    crossing = sm.pose_row({3: (10, 10), 4: (70, 60), 6: (10, 60), 7: (70, 10)})        # (3, 4) and (6, 7) cross at (40, 35)
    got = check(ctx, host, [1], crossing[None], [(0, 100, 255, 128)], NONE, 4)
    assert tuple(got[0, 35, 40]) == tuple(sm.blend(host[0, 35, 40], (0, 100, 255), 128))
    other = sm.person(np.random.default_rng(5), 45, 40, 60)
    kp, inks = np.stack([crossing, other]), np.array([(255, 0, 0, 128), (0, 0, 255, 128)], np.uint8)
    ab = check(ctx, host, [2], kp, inks, (90, 90, 50), 4)
    ba = check(ctx, host, [2], kp[::-1], inks[::-1], (90, 90, 50), 4)
    assert not np.array_equal(ab, ba)


def test_absent_joints_and_the_alphas(ctx):
    host = noise(6, 2, 80, 96)
    rng = np.random.default_rng(7)
    rows = np.stack([sm.person(rng, 30 + 12 * k, 40, 50, absent=0.4) for k in range(4)])      # absent joints keep garbage within +-16000
    assert (rows[..., 2] == 0).any() and (np.abs(rows[rows[..., 2] == 0][:, :2]) > 200).any()
    rows[0, 5] = (-16383, 16383, 0)
    check(ctx, host, [2, 2], rows, rng.integers(1, 255, (4, 4)))
    nobody = rows.copy()
    nobody[..., 2] = 0
    assert np.array_equal(check(ctx, host, [2, 2], nobody, rng.integers(1, 255, (4, 4))), host)
    got = check(ctx, host, [2, 2], rows, [(1, 2, 3, 0), (4, 5, 6, 255), (7, 8, 9, 0), (7, 8, 9, 0)])
    assert np.array_equal(got[1], host[1]) and (got[0] == (4, 5, 6)).all(-1).any()
    cov = sm.pose_coverage(rows[1], 80, 96)
    assert (got[0][cov] == (4, 5, 6)).all() and np.array_equal(got[0][~cov], host[0][~cov])


# ---- clear, untouched frames -----------------------------------------------------------------------------------------------------
def test_clear(ctx):
    host = noise(8, 3, 80, 96)
    none = np.zeros((0, 18, 3), np.int32), np.zeros((0, 4), np.uint8)
    got = check(ctx, host, [0, 0, 0], *none, clear=True)
    assert not got.any()
    got = check(ctx, host, [0, 0], *none, clear=True)                          # the later frame is unchanged to the byte
    assert not got[:2].any() and np.array_equal(got[2], host[2])
    assert np.array_equal(check(ctx, host, [], *none, clear=True), host)
    rng = np.random.default_rng(9)
    rows = np.stack([sm.person(rng, 20 + 25 * k, 40, 60) for k in range(3)])
    got = check(ctx, host, [2, 1], rows, rng.integers(1, 256, (3, 4)), clear=True)
    assert got[:2].any() and np.array_equal(got[2], host[2])
    got = check(ctx, host, [0, 3], rows, np.full((3, 4), 255), clear=True)
    assert not got[0].any() and set(np.unique(got[1])) == {0, 255}


def test_untouched_frames(ctx):
    host = noise(10, 3, 80, 96)
    rows = np.stack([sm.person(np.random.default_rng(11), 48, 40, 60)])
    got = check(ctx, host, [0, 1], rows, [(200, 100, 0, 77)])
    assert np.array_equal(got[0], host[0]) and np.array_equal(got[2], host[2]) and not np.array_equal(got[1], host[1])
    assert np.array_equal(check(ctx, host, [0, 0, 0], np.zeros((0, 18, 3)), np.zeros((0, 4))), host)
    assert np.array_equal(check(ctx, host, [], np.zeros((0, 18, 3)), np.zeros((0, 4))), host)


# ---- a crowd the binning must survive ----------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def crowd():
    rng = np.random.default_rng(12)
    packed = np.zeros((600, 18, 3), np.int32)            # every joint inside the tile x 64 .. 123, y 16 .. 31
    packed[..., 0] = rng.integers(64, 124, (600, 18))
    packed[..., 1] = rng.integers(16, 32, (600, 18))
    packed[..., 2] = rng.random((600, 18)) < 0.5
    spread = np.stack([sm.person(rng, rng.integers(0, 256), rng.integers(0, 256), rng.integers(8, 60), absent=0.1) for _ in range(600)])
    kp = np.concatenate([packed, spread])[rng.permutation(1200)]
    rgba = rng.integers(0, 256, (1200, 4), dtype=np.uint8)
    host = noise(13, 1, 256, 256)
    return host, kp, rgba, sm.paint(host.copy(), [1200], kp, rgba, (90, 90, 50), 1)


def test_a_crowd_in_one_tile(ctx, crowd):
    host, kp, rgba, want = crowd
    assert np.array_equal(run(ctx, host, [1200], kp, rgba, (90, 90, 50), 1), want)


def test_the_matrix_cut_into_batches_and_runs(ctx, crowd, monkeypatch):
    """A 256 x 256 frame has 5 x 16 tiles; 1200 poses are 19 words a tile.  8 x 300 bytes hold 3 words a tile: seven runs of
    192 poses, launch after launch, and the answer is the same."""
    host, kp, rgba, want = crowd
    monkeypatch.setenv('TA_PP_MATRIX_BYTES', str(8 * 300))
    assert np.array_equal(run(ctx, host, [1200], kp, rgba, (90, 90, 50), 1), want)
    # ... and whole frames that share no batch: 3 frames of 4 words a tile under a budget of 7 words a tile
    monkeypatch.setenv('TA_PP_MATRIX_BYTES', str(8 * 80 * 7))
    three = noise(14, 4, 256, 256)
    check(ctx, three, [256, 200, 256], kp[:712], rgba[:712], (90, 90, 50), 1, clear=True)
    monkeypatch.delenv('TA_PP_MATRIX_BYTES')


# ---- a random case ---------------------------------------------------------------------------------------------------------------
def test_random_poses(ctx):
    host = noise(15, 3, 120, 200)
    rng = np.random.default_rng(16)
    kp = np.stack([sm.person(rng, rng.integers(-10, 210), rng.integers(-10, 130), rng.integers(6, 90), absent=0.25) for _ in range(120)])
    rgba = rng.integers(0, 256, (120, 4))
    for permille, min_radius in (((90, 90, 50), 0), ((0, 1000, 37), 7), ((1000, 0, 500), 0), ((3, 250, 0), 7)):
        check(ctx, host, [40, 40, 40], kp, rgba, permille, min_radius)


# ---- validation ------------------------------------------------------------------------------------------------------------------
def test_every_error_leaves_the_frames_alone(ctx):
    from terran_amd import lib
    host = noise(17, 2, 80, 96)
    rows = np.stack([sm.person(np.random.default_rng(18), 48, 40, 60)] * 2)
    inks = np.full((2, 4), 200, np.uint8)
    frames = ctx.upload(host)
    L, I = lib.E_INVALID, np.int32

    def raw(counts, kp, rgba, n_poses, permille=(90, 90, 50), min_radius=2, clear=1, n_frames=None):
        counts, permille = np.asarray(counts, I), np.asarray(permille, I)
        return ctx.lib.ta_poses_paint(ctx.h, frames.h, len(counts) if n_frames is None else n_frames, lib.ptr(counts) if len(counts) else None,
                                      lib.ptr(kp) if kp is not None else None, lib.ptr(rgba) if rgba is not None else None, n_poses,
                                      lib.ptr(permille), min_radius, clear)
    try:
        wild = rows.copy()
        wild[1, 9] = (16384, 0, 0)                      # an absent joint counts
        low = rows.copy()
        low[0, 0, 1] = -16384
        many = np.zeros((16385, 18, 3), I)
        cases = [('negative count', raw([3, -1], rows, inks, 2), L), ('sum', raw([1, 2], rows, inks, 2), L), ('sum', raw([1], rows, inks, 2), L),
                 ('frames', raw([1, 1, 0], rows, inks, 2), L), ('null keypoints', raw([1, 1], None, inks, 2), L),
                 ('null rgba', raw([1, 1], rows, None, 2), L), ('null counts', raw([], rows, inks, 2, n_frames=2), L),
                 ('permille', raw([1, 1], rows, inks, 2, (90, 1001, 50)), L), ('permille', raw([1, 1], rows, inks, 2, (-1, 90, 50)), L),
                 ('min_radius', raw([1, 1], rows, inks, 2, min_radius=-1), L), ('min_radius', raw([1, 1], rows, inks, 2, min_radius=4097), L),
                 ('coordinate', raw([1, 1], wild, inks, 2), L), ('coordinate', raw([1, 1], low, inks, 2), L),
                 ('negative n_poses', raw([0, 0], rows, inks, -1), L),
                 ('overflow', raw([16385, 0], many, np.zeros((16385, 4), np.uint8), 16385), lib.E_OVERFLOW)]
        for what, rc, want in cases:
            assert rc == want, what
        assert np.array_equal(frames.download(), host)
        with pytest.raises(lib.TerranAmdError):
            ctx.poses_paint(frames, [1, 2], rows, inks)
        with pytest.raises(ValueError):
            ctx.poses_paint(frames, [1, 1], rows, inks[:1])
        with pytest.raises(ValueError):
            ctx.poses_paint(frames, [1, 1], rows, inks, radius_permille=(90, 90))
        assert np.array_equal(frames.download(), host)
        # the limits themselves pass
        edge = rows.copy()
        edge[0, 0] = (16383, -16383, 1)
        assert raw([1, 1], edge, inks, 2, (1000, 0, 1000), 4096, 0) == lib.OK
        assert raw([], None, None, 0, n_frames=0) == lib.OK and raw([0, 0], None, None, 0, clear=0) == lib.OK
    finally:
        frames.free()


# ---- end to end, 2 x 128 x 160 ----------------------------------------------------------------------------------------------------
def pose(row, **more):
    return dict(keypoints=np.asarray(row, np.float64), score=1.0, **more)


@pytest.fixture(scope='module')
def scene():
    rng = np.random.default_rng(19)
    rows = [[sm.person(rng, 40, 70, 100), sm.person(rng, 75, 64, 90, absent=0.2)], [sm.person(rng, 120, 80, 80), sm.person(rng, 150, 20, 70), sm.pose_row({4: (9, 9)})]]
    host = noise(20, 2, 128, 160)
    counts, kp = [2, 3], np.stack(rows[0] + rows[1])
    return host, [[pose(r) for r in f] for f in rows], counts, kp, sm.masks(host.shape, counts, kp)


def test_pose_masks(ctx, scene):
    from terran_amd import vis
    host, poses, counts, kp, matte = scene
    frames = ctx.upload(host)
    for source in (frames, host.shape, (2, 128, 160)):
        m = vis.pose_masks(source, poses, ctx=ctx)
        assert m.shape == (2, 128, 160, 3) and np.array_equal(m.download(), matte)
        m.free()
    m = vis.pose_masks(frames, poses, head=0.2, torso=0.0, limb=0.03, min_radius=1)
    assert np.array_equal(m.download(), sm.masks(host.shape, counts, kp, (200, 0, 30), 1))
    m.free()
    small = ctx.upload(host[:1, :64, :64])
    ms = vis.pose_masks([frames, small], poses + [poses[0]])            # a mixed-size list, frames counted through
    assert np.array_equal(ms[0].download(), matte) and np.array_equal(ms[1].download(), matte[:1, :64, :64])
    assert np.array_equal(frames.download(), host)
    for b in ms + [small, frames]:
        b.free()


def test_blur_poses_is_the_composition_of_the_models(ctx, scene):
    from terran_amd import vis
    host, poses, counts, kp, matte = scene
    for kw, model in ((dict(), B.blur_regions), (dict(radius=2.5), B.blur_regions), (dict(method='pixelate'), R.pixelate_regions),
                      (dict(method='pixelate', block=5), R.pixelate_regions)):
        regions, _ = vis.pack_pose_blur(poses, host.shape, **kw)
        assert [tuple(int(q[k]) for k in ('frame', 'x0', 'y0', 'x1', 'y1')) for q in regions] == [(f, x0, y0, x1, y1) for f, _, x0, y0, x1, y1 in
                                                                                               sm.boxes(counts, kp, 128, 160)]
        want = C.paste_mask(host, model(host.copy(), regions), matte.astype(np.int64))
        frames = ctx.upload(host)
        assert vis.blur_poses(frames, poses, **kw) is frames
        got = frames.download()
        frames.free()
        assert np.array_equal(got, want), kw
        assert np.array_equal(got[matte == 0], host[matte == 0]) and not np.array_equal(got, host)
    one = vis.anonymize_poses(host[1], poses[1], method='pixelate')
    regions, _ = vis.pack_pose_blur(poses, host.shape, method='pixelate')
    assert np.array_equal(one, C.paste_mask(host, R.pixelate_regions(host.copy(), regions), matte.astype(np.int64))[1])
    frames = ctx.upload(host[:1])
    vis.blur_poses(frames, [poses[0]])
    assert np.array_equal(vis.anonymize_poses(host[0], poses[0]), frames.download()[0])
    frames.free()


def test_spotlight_poses(ctx, scene):
    from terran_amd import vis
    host, poses, counts, kp, matte = scene
    frames = ctx.upload(host)
    vis.spotlight_poses(frames, poses, dim=0.4)
    want = C.paste_mask(np.stack([T.brightness(f, 0.4) for f in host]), host, matte.astype(np.int64))
    assert np.array_equal(frames.download(), want)
    frames.free()


def test_paint_poses_keeps_a_persons_colour(ctx):
    from terran_amd import tracking, vis
    rng = np.random.default_rng(21)
    a, b = sm.person(rng, 40, 70, 100), sm.person(rng, 115, 64, 90)
    clip = []
    for t in range(3):
        pa, pb = a.copy(), b.copy()
        pa[:, 0] += 3 * t
        pb[:, 1] -= 2 * t
        clip.append([pose(pa), pose(pb)] if t != 1 else [pose(pb), pose(pa)])        # the list order says nothing
    tracking.reset_pose_track_ids()
    tracking.PoseTracker(max_gap=1, ctx=ctx).update(clip)
    ids = [[p['pose_track'] for p in f] for f in clip]
    assert ids[0][0] == ids[1][1] == ids[2][0] != ids[0][1] == ids[1][0] == ids[2][1]
    vis.POSE_COLORMAP = vis.build_colormap()
    host = noise(22, 3, 128, 160)
    frames = ctx.upload(host)
    vis.paint_poses(frames, clip)
    got = frames.download()
    frames.free()
    vis.POSE_COLORMAP = vis.build_colormap()
    counts, kp, rgba = vis.pack_silhouettes(clip, 'track', 128)
    assert np.array_equal(got, sm.paint(host.copy(), counts, kp, rgba))
    ca, cb = vis.PALETTE[0], vis.PALETTE[1]
    for t in range(3):
        for row, ink in ((a, ca), (b, cb)):
            x, y = int(row[1, 0]) + (3 * t if row is a else 0), int(row[1, 1]) - (0 if row is a else 2 * t)
            assert tuple(got[t, y, x]) == tuple(sm.blend(host[t, y, x], ink, 128))      # the neck, in its track's colour
    # opaque, one colour, in place on a list of batches
    one, two = ctx.upload(host[:1]), ctx.upload(host[1:])
    vis.paint_poses([one, two], clip, colors=(9, 8, 7), alpha=255)
    want = sm.paint(host.copy(), counts, kp, np.tile(np.array([9, 8, 7, 255], np.uint8), (6, 1)))
    assert np.array_equal(one.download(), want[:1]) and np.array_equal(two.download(), want[1:])
    one.free()
    two.free()
