"""No GPU: the silhouette rule of ta_poses_paint as tests/silhouette_model.py states it -- the numpy int64 test against the exact
fraction, the symmetries of the rule, the radius rule, the class tables -- and the host half of the public calls
(vis.pack_silhouettes' colours, vis.pose_boxes / pack_pose_blur's regions, the argument checks)."""
import numpy as np
import pytest

from terran_amd import lib, vis
from tests import silhouette_model as sm


def random_segments(rng, n):
    """Segments around a 24 x 24 frame: every octant, A == B, r = 0, ends outside the frame."""
    out = []
    octants = [(1, 0), (1, 1), (0, 1), (-1, 1), (-1, 0), (-1, -1), (0, -1), (1, -1)]
    for k in range(n):
        ax, ay = (int(v) for v in rng.integers(-10, 34, 2))
        if k % 7 == 0:
            bx, by = ax, ay                                                   # the disc
        elif k % 7 == 1:
            sx, sy = octants[(k // 7) % 8]
            ln = int(rng.integers(1, 30))
            bx, by = ax + sx * ln, ay + sy * ln                               # the eight exact directions
        else:
            bx, by = (int(v) for v in rng.integers(-10, 34, 2))
        r = 0 if k % 5 == 0 else int(rng.integers(0, 9))
        out.append((ax, ay, bx, by, r))
    return out


def test_the_two_formulations_agree():
    rng = np.random.default_rng(7)
    segs = random_segments(rng, 320)
    dirs = set()
    for s in segs:
        ax, ay, bx, by, r = s
        dirs.add((np.sign(bx - ax), np.sign(by - ay)))
        got = sm.shape_coverage(s, 24, 24)
        want = np.array([[sm.covered_fraction(x, y, *s) for x in range(24)] for y in range(24)])
        assert np.array_equal(got, want), s
    assert len(dirs) == 9                                                     # eight octants and A == B
    assert any(s[4] == 0 and s[:2] != s[2:4] for s in segs) and any(min(s[:4]) < 0 or max(s[:4]) > 23 for s in segs)


def test_the_boundary_is_inclusive():
    # A = (-16000, 10), B = (16000, 10), r = 5: row 15 has cross^2 = r^2 L2 exactly, row 16 does not
    s = (-16000, 10, 16000, 10, 5)
    x = np.arange(96)
    assert sm.covered(x, 15, *s).all() and sm.covered(x, 5, *s).all() and not sm.covered(x, 16, *s).any() and not sm.covered(x, 4, *s).any()
    assert sm.covered_fraction(40, 15, *s) and not sm.covered_fraction(40, 16, *s)
    # the caps: t <= 0 and t >= L2 are disc tests, inclusive
    assert sm.covered(7, 10, 10, 10, 20, 10, 3) and not sm.covered(6, 10, 10, 10, 20, 10, 3)
    assert sm.covered(23, 10, 10, 10, 20, 10, 3) and not sm.covered(24, 10, 10, 10, 20, 10, 3)
    assert sm.covered(10, 10, 10, 10, 10, 10, 0) and not sm.covered(11, 10, 10, 10, 10, 10, 0)        # r = 0: the joint's own pixel


def test_a_pose_is_the_or_of_its_shapes():
    rng = np.random.default_rng(3)
    row = sm.person(rng, 30, 34, 50, absent=0.2)
    row[:, :2] = np.where(row[:, 2:3] != 0, row[:, :2], 0)
    shapes = sm.shapes_of(row)
    present = int((row[:, 2] != 0).sum())
    segments = sum(1 for a, b, _ in sm.SEGMENTS if row[a, 2] and row[b, 2])
    assert len(shapes) == present + segments
    want = np.zeros((64, 64), bool)
    for y in range(64):
        for x in range(64):
            want[y, x] = any(sm.covered_fraction(x, y, *s) for s in shapes)
    assert np.array_equal(sm.pose_coverage(row, 64, 64), want) and want.any() and not want.all()
    assert not sm.pose_coverage(np.zeros((18, 3), np.int32), 8, 8).any()      # no present joint: nothing


def test_swapping_the_ends_changes_nothing():
    rng = np.random.default_rng(11)
    for ax, ay, bx, by, r in random_segments(rng, 120):
        assert np.array_equal(sm.shape_coverage((ax, ay, bx, by, r), 24, 24), sm.shape_coverage((bx, by, ax, ay, r), 24, 24))


def test_translation_changes_nothing():
    rng = np.random.default_rng(12)
    x, y = np.arange(24)[None, :], np.arange(24)[:, None]
    for ax, ay, bx, by, r in random_segments(rng, 120):
        ox, oy = (int(v) for v in rng.integers(-8000, 8000, 2))
        assert np.array_equal(sm.covered(x, y, ax, ay, bx, by, r), sm.covered(x + ox, y + oy, ax + ox, ay + oy, bx + ox, by + oy, r))


def test_the_radius_rule():
    one = sm.pose_row({4: (7, 9)})
    assert sm.size_of(one) == 0 and sm.radii(one, (90, 90, 50), 2) == (2, 2, 2) and sm.radii(one, (1000, 0, 5), 0) == (0, 0, 0)
    assert sm.size_of(np.zeros((18, 3), np.int32)) is None and sm.radii(np.zeros((18, 3), np.int32)) is None
    # the larger side counts, absent joints do not
    row = sm.pose_row({0: (10, 0), 1: (10, 199), 2: (60, 5)})
    row[9] = (9000, -9000, 0)
    assert sm.size_of(row) == 199
    # truncation: 199 * 90 / 1000 = 17.91 -> 17; 200 * 90 / 1000 = 18 exactly; 199 * 50 / 1000 = 9.95 -> 9
    assert sm.radii(row, (90, 90, 50), 2) == (17, 17, 9)
    row[1, 1] = 200
    assert sm.radii(row, (90, 90, 50), 2) == (18, 18, 10)
    assert sm.radii(row, (90, 90, 50), 12) == (18, 18, 12) and sm.radii(row, (0, 1000, 4), 0) == (0, 200, 0)      # 200 * 4 / 1000 = 0.8 -> 0
    # a single joint paints the disc of min_radius
    assert sm.pose_coverage(one, 20, 20, (90, 90, 50), 2).sum() == 13


def test_the_classes_of_all_joints_and_segments():
    head, torso = {0, 14, 15, 16, 17}, {1, 2, 5, 8, 11}
    for j in range(18):
        assert sm.JOINT_CLASS[j] == (sm.HEAD if j in head else sm.TORSO if j in torso else sm.LIMB)
    want = {(0, 1): sm.HEAD, (0, 14): sm.HEAD, (14, 16): sm.HEAD, (0, 15): sm.HEAD, (15, 17): sm.HEAD,
            (1, 2): sm.TORSO, (1, 5): sm.TORSO, (1, 8): sm.TORSO, (1, 11): sm.TORSO, (8, 11): sm.TORSO}
    assert len(sm.SEGMENTS) == 18 and len(set((a, b) for a, b, _ in sm.SEGMENTS)) == 18
    assert [(a, b) for a, b, _ in sm.SEGMENTS[:17]] == [tuple(int(v) for v in c) for c in vis.POSE_CONNECTIONS] and sm.SEGMENTS[17][:2] == (8, 11)
    assert sum(1 for _, _, c in sm.SEGMENTS if c == sm.LIMB) == 8
    for a, b, c in sm.SEGMENTS:
        assert c == want.get((a, b), sm.LIMB)
    # the library's tables are the model's
    assert tuple(vis.SILHOUETTE_JOINT_CLASS) == sm.JOINT_CLASS
    assert [(int(a), int(b), int(c)) for (a, b), c in zip(vis.SILHOUETTE_SEGMENTS, vis.SILHOUETTE_SEGMENT_CLASS)] == list(sm.SEGMENTS)
    # a class's radius is what its shapes get: three joints, one of each class, far apart
    row = sm.pose_row({0: (0, 0), 1: (1000, 0), 3: (0, 1000)})
    assert sorted(s[4] for s in sm.shapes_of(row, (10, 20, 30), 0)) == [10, 10, 20, 30]           # discs 0, 1, 3 and the segment (0, 1)


def test_float64_misjudges_a_pixel_int64_does_not():
    """Found by search over d = (n, -1), r = 2 n, p = (n + 1, 2 n - 1): cross = -(2 n^2 + 1), so cross^2 = r^2 L2 + 1 with
    both near 2^58, where float64 keeps multiples of 64.  Everything lies within the checked range: coordinates below 2^14 in
    size, the pixel inside a 16384 x 16384 frame, r = 2 n the size of a skeleton that spans 2 n pixels at 1000 permille."""
    found = []
    for n in range(16300, 16390):
        a, b, r = (-16383, -16382), (-16383 + n, -16383), 2 * n
        p = (a[0] + n + 1, a[1] + 2 * n - 1)
        if max(abs(v) for v in a + b) >= 1 << 14 or not (0 <= p[0] < 16384 and 0 <= p[1] < 16384) or r >= 1 << 15:
            continue
        exact = bool(sm.covered(p[0], p[1], *a, *b, r))
        assert exact == sm.covered_fraction(p[0], p[1], *a, *b, r)
        if bool(sm.covered_float(p[0], p[1], *a, *b, r, np.float64)) != exact:
            found.append((n, a, b, r, p))
    assert found and found[-1][0] == 16383                 # the largest n the range admits
    n, a, b, r, p = found[-1]
    qx, qy, dx, dy = p[0] - a[0], p[1] - a[1], b[0] - a[0], b[1] - a[1]
    cross, L2 = qx * dy - qy * dx, dx * dx + dy * dy
    assert 0 < qx * dx + qy * dy < L2 and cross * cross == r * r * L2 + 1 and cross * cross > 1 << 57
    assert not sm.covered(p[0], p[1], *a, *b, r) and sm.covered_float(p[0], p[1], *a, *b, r, np.float64)
    # the same through the whole rule: a skeleton whose LIMB segment (3, 4) is that capsule, its size 32764, limb share 1000
    row = sm.pose_row({3: a, 4: b, 7: (a[0] + r, -16383)})
    assert sm.radii(row, (0, 0, 1000), 0)[2] == r
    assert not any(sm.covered(p[0], p[1], *s) for s in sm.shapes_of(row, (0, 0, 1000), 0))
    assert any(sm.covered_float(p[0], p[1], *s) for s in sm.shapes_of(row, (0, 0, 1000), 0))


def test_paint_blends_once_per_pose_in_list_order():
    crossing = sm.pose_row({3: (2, 2), 4: (20, 20), 6: (2, 20), 7: (20, 2)})       # (3, 4) and (6, 7) cross at (11, 11)
    frames = np.full((1, 24, 24, 3), 200, np.uint8)
    got = sm.paint(frames.copy(), [1], crossing[None], [(0, 100, 255, 128)], (0, 0, 0), 1)
    assert tuple(got[0, 11, 11]) == tuple(sm.blend(np.array([200, 200, 200], np.uint8), (0, 100, 255), 128))
    assert len(np.unique(got[0].reshape(-1, 3), axis=0)) == 2                      # painted once, or not at all
    other = sm.pose_row({3: (2, 11), 4: (20, 11)})
    kp, inks = np.stack([crossing, other]), np.array([(255, 0, 0, 128), (0, 0, 255, 128)], np.uint8)
    ab = sm.paint(frames.copy(), [2], kp, inks, (0, 0, 0), 1)
    ba = sm.paint(frames.copy(), [2], kp[::-1], inks[::-1], (0, 0, 0), 1)
    assert not np.array_equal(ab, ba)
    # alpha 255 replaces, alpha 0 changes nothing, clear zeroes the listed frames only
    two = np.full((2, 24, 24, 3), 9, np.uint8)
    got = sm.paint(two.copy(), [1], other[None], [(1, 2, 3, 255)], (0, 0, 0), 1, clear=True)
    assert tuple(got[0, 11, 11]) == (1, 2, 3) and got[0, 0, 0].sum() == 0 and np.array_equal(got[1], two[1])
    assert np.array_equal(sm.paint(two.copy(), [1], other[None], [(1, 2, 3, 0)], (0, 0, 0), 1), two)
    assert np.array_equal(sm.masks((1, 24, 24), [1], other[None], (0, 0, 0), 1)[0, :, :, 0] == 255, sm.pose_coverage(other, 24, 24, (0, 0, 0), 1))


# ---- the host half of the public calls -------------------------------------------------------------------------------------------
def pose(row, **more):
    return dict(keypoints=np.asarray(row, np.float64), **more)


def test_pack_silhouettes_colours():
    row = sm.pose_row({0: (5, 5), 1: (5, 20)})
    vis.POSE_COLORMAP = vis.build_colormap()
    clip = [[pose(row, pose_track=7), pose(row, pose_track=3)], [pose(row, pose_track=3), pose(row, pose_track=7), pose(row, pose_track=9)]]
    counts, kp, rgba = vis.pack_silhouettes(clip, 'track', 128)
    assert counts.dtype == np.int32 and kp.dtype == np.int32 and rgba.dtype == np.uint8
    assert list(counts) == [2, 3] and kp.shape == (5, 18, 3) and np.array_equal(kp[0], row)
    assert tuple(rgba[0]) == tuple(rgba[3]) == vis.PALETTE[0] + (128,) and tuple(rgba[1]) == tuple(rgba[2]) == vis.PALETTE[1] + (128,)
    assert tuple(rgba[4, :3]) == vis.PALETTE[2]
    # ... and in a later call
    assert tuple(vis.pack_silhouettes([[pose(row, pose_track=3)]], 'track')[2][0]) == vis.PALETTE[1] + (255,)
    # the fallbacks: pose_track before track before the index in the frame
    vis.POSE_COLORMAP = vis.build_colormap()
    rgba = vis.pack_silhouettes([[pose(row, pose_track=5, track=6), pose(row, track=5), pose(row), pose(row, track=2)]], 'track')[2]
    assert tuple(rgba[0, :3]) == tuple(rgba[1, :3]) == vis.PALETTE[0]          # id 5 either way
    assert tuple(rgba[2, :3]) == tuple(rgba[3, :3]) == vis.PALETTE[1]          # index 2 and track 2 are the same key
    # None, one colour, one per pose, alpha per pose
    assert np.array_equal(vis.pack_silhouettes(clip)[2], np.full((5, 4), 255, np.uint8))
    assert np.array_equal(vis.pack_silhouettes(clip, (1, 2, 3), 9)[2], np.tile(np.array([1, 2, 3, 9], np.uint8), (5, 1)))
    per = np.arange(15).reshape(5, 3)
    got = vis.pack_silhouettes(clip, per, np.arange(5))[2]
    assert np.array_equal(got[:, :3], per) and list(got[:, 3]) == [0, 1, 2, 3, 4]
    # truncation as pack_poses truncates; an absent joint is (0, 0, 0) whatever it held
    odd = np.array(row, np.float64)
    odd[0, :2] = (5.9, -3.9)
    odd[9] = (np.nan, 1e9, 0)
    kp = vis.pack_silhouettes([pose(odd)])[1]
    assert tuple(kp[0, 0]) == (5, -3, 1) and tuple(kp[0, 9]) == (0, 0, 0)
    assert vis.pack_silhouettes([[], []])[1].shape == (0, 18, 3)
    for bad in (dict(colors='name'), dict(colors=(1, 2)), dict(colors=(1, 2, 256)), dict(alpha=256), dict(alpha=0.5), dict(alpha=[1, 2])):
        with pytest.raises(ValueError):
            vis.pack_silhouettes(clip, **bad)
    wild = np.array(row, np.float64)
    wild[1, 0] = 16384
    with pytest.raises(ValueError):
        vis.pack_silhouettes([pose(wild)])


def test_blur_poses_region_boxes():
    rng = np.random.default_rng(5)
    rows = [sm.person(rng, 40, 60, 80), sm.person(rng, 150, 30, 60, absent=0.3), sm.pose_row({4: (3, 3)}), np.zeros((18, 3), np.int32),
            sm.pose_row({0: (-50, -50), 1: (-40, -45)}), sm.person(rng, 100, 120, 90)]
    per_frame = [[pose(r) for r in rows[:4]], [pose(r) for r in rows[4:]]]
    counts, kp, _ = vis.pack_silhouettes(per_frame)
    want = sm.boxes(counts, kp, 128, 160, (90, 90, 50), 2)
    assert vis.pose_boxes(per_frame, (128, 160)) == want
    assert [(f, i) for f, i, *_ in want] == [(0, 0), (0, 1), (0, 2), (1, 1)]      # no joint, and off the frame: left out
    assert want[2][2:] == (1, 1, 6, 6)                                              # one joint: min_radius round it
    # a box holds everything the silhouette covers
    cov = sm.pose_coverage(rows[0], 128, 160)
    ys, xs = np.nonzero(cov)
    f, i, x0, y0, x1, y1 = want[0]
    assert x0 <= xs.min() and xs.max() < x1 and y0 <= ys.min() and ys.max() < y1
    regions, pixelate = vis.pack_pose_blur(per_frame, (2, 128, 160, 3))
    assert not pixelate and regions.dtype == lib.BLUR_DT and len(regions) == 4
    for q, (f, _, x0, y0, x1, y1) in zip(regions, want):
        assert (q['frame'], q['x0'], q['y0'], q['x1'], q['y1'], q['shape']) == (f, x0, y0, x1, y1, lib.BLUR_BOX)
        assert q['radius'] == np.float32(max(x1 - x0, y1 - y0) / 8)
    regions, pixelate = vis.pack_pose_blur(per_frame, (128, 160), method='pixelate')
    assert pixelate and regions.dtype == lib.PIXELATE_DT and [int(b) for b in regions['block']] == [max(1, max(x1 - x0, y1 - y0) // 8) for *_, x0, y0, x1, y1 in want]
    assert list(vis.pack_pose_blur(per_frame, (128, 160), radius=3.5)[0]['radius']) == [3.5] * 4
    assert list(vis.pack_pose_blur(per_frame, (128, 160), method='pixelate', block=6)[0]['block']) == [6] * 4
    # other shares widen the boxes
    assert vis.pose_boxes(per_frame, (128, 160), head=0.2, min_radius=0) == sm.boxes(counts, kp, 128, 160, (200, 90, 50), 0)


def test_argument_checks_need_no_device():
    row = sm.pose_row({0: (5, 5), 1: (5, 20)})
    per_frame = [[pose(row)]]
    for kw in (dict(method='mosaic'), dict(method='pixelate', radius=2.0), dict(method='gaussian', block=4), dict(method='pixelate', block=0),
               dict(radius=-1.0), dict(head=1.5), dict(limb=-0.1), dict(min_radius=4097), dict(min_radius=1.5)):
        with pytest.raises(ValueError):
            vis.pack_pose_blur(per_frame, (32, 32), **kw)
    img = np.zeros((32, 32, 3), np.uint8)
    for call in (lambda: vis.pose_masks((1, 32, 32), per_frame, device=[0, 1]), lambda: vis.paint_poses(None, per_frame, device=[0]),
                 lambda: vis.blur_poses(None, per_frame, device=(0, 1)), lambda: vis.spotlight_poses(None, per_frame, device=[0]),
                 lambda: vis.anonymize_poses(img, per_frame[0], device=[0, 1])):
        with pytest.raises(ValueError, match='device list'):
            call()
    with pytest.raises(ValueError):
        vis.anonymize_poses(img.astype(np.float32), per_frame[0])
    with pytest.raises(ValueError):
        vis.anonymize_poses(img, per_frame[0], method='mosaic')
    import terran_amd
    for name in ('pose_masks', 'paint_poses', 'blur_poses', 'spotlight_poses', 'anonymize_poses'):
        assert getattr(terran_amd, name) is getattr(vis, name)
    L = lib.load()
    assert L.ta_poses_paint(None, None, 0, None, None, None, 0, None, 2, 0) == lib.E_INVALID
