"""-m gpu: tracks filled across missed frames and joints.  ta_tracks_fill against the model of tests/fill_model.py with
np.array_equal and no tolerance anywhere: the cases computed by hand, 1, 7 and 18 points a row, a frame that gains 300 (and 70)
rows at once -- across the 64-lane and the workgroup-chunk seams of the ranking --, seeded clips at max_gap 0, 5 and 30 with
coordinates at the ends of the range, every error with the outputs untouched, the capacity query, the empty cases; and the public
calls end to end: PoseTracker -> fill_pose_tracks -> pose_masks, fill_face_tracks -> blur_faces."""
import numpy as np
import pytest

from tests import fill_model as fm

pytestmark = pytest.mark.gpu

NAMES = ('out_counts', 'out_points', 'out_source')


@pytest.fixture(scope='module')
def ctx():
    from terran_amd import lib
    c = lib.Context(0)
    yield c
    c.close()


def same(got, want):
    for a, b, what in zip(got, want, NAMES):
        b = np.asarray(b, np.int32).reshape((-1,) + a.shape[1:])
        assert a.dtype == np.int32 and a.shape == b.shape, (what, a.dtype, a.shape, b.shape)
        assert np.array_equal(a, b), (what, int(np.argmax((a != b).reshape(-1))))


def check(ctx, counts, points, prev, max_gap=5, mark=2):
    want = fm.fill_model(counts, points, prev, max_gap, mark)
    got = ctx.tracks_fill(counts, points, prev, max_gap, mark)
    same(got, want)
    return got


@pytest.mark.parametrize('case', fm.hand_cases(), ids=lambda c: c[0])
def test_hand_cases(ctx, case):
    _, call, max_gap, mark, want = case
    same(ctx.tracks_fill(*call, max_gap, mark), want)
    check(ctx, *call, max_gap, mark)


@pytest.mark.parametrize('tracks,n_points', [(300, 18), (70, 18), (300, 1), (70, 7)])
def test_a_frame_that_gains_every_row_at_once(ctx, tracks, n_points):
    counts, points, prev = fm.seam_clip(tracks, n_points)
    oc, op, src = check(ctx, counts, points, prev, 1, 9)
    assert oc.tolist() == [tracks] * 3 and src[tracks:2 * tracks, 1].tolist() == list(range(tracks, 2 * tracks))
    assert set(np.unique(op[tracks:2 * tracks, :, 2]).tolist()) == {0, 9}
    oc, op, src = check(ctx, counts, points, prev, 0, 9)                # a link of two frames is too long for max_gap 0
    assert oc.tolist() == counts.tolist() and np.array_equal(src, np.repeat(np.arange(2 * tracks), 2).reshape(-1, 2))


# (seed, extreme) per max_gap: the first case of each walks between the two ends of the coordinate range
@pytest.mark.parametrize('max_gap', [0, 5, 30])
@pytest.mark.parametrize('seed,extreme,n_points', [(1, True, 18), (2, False, 18), (3, False, 7)])
def test_seeded_clips(ctx, max_gap, seed, extreme, n_points):
    counts, points, prev = fm.seeded_clip(100 * max_gap + seed, n_points=n_points, extreme=extreme)
    if extreme:
        assert points[:, :, :2].max() == (1 << 22) - 1 and points[:, :, :2].min() == 1 - (1 << 22)
    oc, op, src = check(ctx, counts, points, prev, max_gap, 2)
    print('rows', len(points), '->', len(op), 'points filled', int((op[:, :, 2] == 2).sum()))
    assert (len(op) > len(points)) == (max_gap > 0)


# ---- errors and empty cases ----------------------------------------------------------------------------------------------------------
def raw_fill(ctx, counts, points, prev, n_points=None, n_frames=None, n_rows=None, max_gap=5, mark=2, capacity=None, outputs=True, oc=True, room=64):
    """The bare call into buffers of `room` rows filled with -7; `capacity` is what the call is told (default: the room)."""
    from terran_amd import lib
    import ctypes as C
    p = lambda a: lib.ptr(a) if a is not None and len(a) else None
    n_frames = (len(counts) if counts is not None else 0) if n_frames is None else n_frames
    n_rows = (len(points) if points is not None else 0) if n_rows is None else n_rows
    n_points = points.shape[1] if n_points is None else n_points
    capacity = room if capacity is None else capacity
    assert capacity <= room
    out_counts, out_points = np.full(max(n_frames, 1), -7, np.int32), np.full((room, max(n_points, 1), 3), -7, np.int32)
    out_source, n_out = np.full((room, 2), -7, np.int32), C.c_int32(-7)
    rc = ctx.lib.ta_tracks_fill(ctx.h, n_frames, p(counts), p(points), n_points, p(prev), n_rows, max_gap, mark, lib.ptr(out_counts) if oc else None,
                                lib.ptr(out_points) if outputs else None, lib.ptr(out_source) if outputs else None, capacity, C.byref(n_out))
    return rc, out_counts, out_points, out_source, n_out.value


def untouched(*arrays):
    return all((a == -7).all() for a in arrays)


def test_errors(ctx):
    from terran_amd import lib
    i32 = lambda *v: np.array(v, np.int32)
    counts, prev = i32(2, 0, 1, 1), i32(-1, -1, 0, 2)
    points = np.ones((4, 3, 3), np.int32)
    big = 1 << 22

    def wild(arr, index, value):
        out = arr.copy()
        out[index] = value
        return out

    cases = [
        (dict(counts=i32(2, -1, 2, 1)), 'negative'), (dict(counts=i32(2, 0, 1, 2)), 'sum'), (dict(n_rows=3), 'sum'), (dict(n_frames=3), 'sum'),
        (dict(points=None, n_rows=4, n_points=3), 'null'), (dict(prev=None), 'null'), (dict(counts=None, n_frames=4), 'null'),
        (dict(outputs=False), 'null output'), (dict(oc=False), 'null output'),
        (dict(n_points=0), 'n_points'), (dict(n_points=19), 'n_points'), (dict(max_gap=-1), 'max_gap'), (dict(max_gap=31), 'max_gap'),
        (dict(mark=0), 'mark'), (dict(mark=256), 'mark'),
        (dict(points=wild(points, (3, 0, 0), big)), 'row 3'), (dict(points=wild(points, (0, 2, 1), -big)), 'row 0'),
        (dict(points=wild(wild(points, (1, 1, 2), 0), (1, 1, 0), big)), 'row 1'),               # an absent point counts too
        (dict(prev=i32(-1, -1, 0, -2)), 'prev[3]'), (dict(prev=i32(-1, -1, 0, 4)), 'prev[3]'), (dict(prev=i32(-1, -1, 0, 3)), 'prev[3]'),
        (dict(prev=i32(-1, 0, -1, -1)), 'prev[1]'),                                            # the same frame
        (dict(prev=i32(-1, -1, 3, -1)), 'prev[2]'),                                            # a later frame
        (dict(prev=i32(-1, -1, 0, 0)), 'two rows'),
    ]
    for change, what in cases:
        a = dict(counts=counts, points=points, prev=prev)
        a.update(change)
        rc, oc, op, src, n_out = raw_fill(ctx, **a)
        assert rc == lib.E_INVALID and what in ctx.last_error(), (what, rc, ctx.last_error())
        assert untouched(oc, op, src) and n_out in (-7, 5), (what, n_out)         # only a null output comes as far as the count
    # the call itself: row 0 -> row 2 skips frame 1; the bound is 2^22 - 1 in size, and the third value of a point is free
    ok = wild(wild(points, (3, 0, 0), big - 1), (0, 2, 1), 1 - big)
    ok[2, 1, 2] = 1 << 30
    assert check(ctx, counts, ok, prev, 30, 255)[0].tolist() == [2, 1, 1, 1]
    # the capacity: too small by one, and asked for with nothing to write to
    rc, oc, op, src, n_out = raw_fill(ctx, counts, points, prev, capacity=4)
    assert rc == lib.E_OVERFLOW and 'out_capacity' in ctx.last_error() and n_out == 5 and untouched(oc, op, src)
    rc, oc, op, src, n_out = raw_fill(ctx, counts, points, prev, capacity=0, outputs=False, oc=False)
    assert rc == lib.E_OVERFLOW and n_out == 5
    rc, oc, op, src, n_out = raw_fill(ctx, counts, points, prev, capacity=5)
    assert rc == lib.OK and n_out == 5 and oc.tolist() == [2, 1, 1, 1] and (op[:5] != -7).all() and (src[:5] != -7).all() and untouched(op[5:], src[5:])
    with pytest.raises(lib.TerranAmdError) as e:
        ctx.tracks_fill(counts, points, prev, 40)
    assert e.value.code == lib.E_INVALID
    with pytest.raises(ValueError, match='prev'):
        ctx.tracks_fill(counts, points, prev[:3])
    with pytest.raises(ValueError, match='points'):
        ctx.tracks_fill(counts, points.reshape(4, 9), prev)


def test_the_limit_per_frame(ctx):
    from terran_amd import lib
    n = lib.FILL_MAX_PER_FRAME
    assert n == fm.MAX_PER_FRAME == 16384
    one = np.ones((n + 2, 1, 3), np.int32)
    one[:, 0, 0] = np.arange(n + 2)
    rc, oc, op, src, n_out = raw_fill(ctx, np.array([n + 1, 1], np.int32), one, np.full(n + 2, -1, np.int32), room=n + 8)
    assert rc == lib.E_OVERFLOW and '16384' in ctx.last_error() and untouched(oc, op, src) and n_out == -7
    link = np.full(n + 2, -1, np.int32)
    link[n + 1] = 0
    rc, oc, op, src, n_out = raw_fill(ctx, np.array([1, n, 1], np.int32), one, link, room=n + 8)
    assert rc == lib.E_OVERFLOW and 'would have 16385' in ctx.last_error() and untouched(oc, op, src) and n_out == -7
    # one row fewer: the frame is full, and its last row is the synthesized one
    link = np.full(n + 1, -1, np.int32)
    link[n] = 0
    oc, op, src = ctx.tracks_fill([1, n - 1, 1], one[:n + 1], link, 1, 2)
    assert oc.tolist() == [1, n, 1] and src[n].tolist() == [0, n] and op[n, 0].tolist() == [n // 2, 1, 2]
    assert np.array_equal(op[:n, 0, 0], np.arange(n)) and np.array_equal(src[:n, 0], np.arange(n))


def test_empty_cases(ctx):
    from terran_amd import lib
    none = np.zeros(0, np.int32)
    oc, op, src = ctx.tracks_fill(none, none.reshape(0, 18, 3), none)
    assert oc.shape == (0,) and op.shape == (0, 18, 3) and src.shape == (0, 2)
    rc, oc, op, src, n_out = raw_fill(ctx, None, None, None, n_points=7, capacity=0, outputs=False, oc=False)
    assert rc == lib.OK and n_out == 0
    rc, oc, op, src, n_out = raw_fill(ctx, np.zeros(3, np.int32), None, None, n_points=7, capacity=0, outputs=False)
    assert rc == lib.OK and n_out == 0 and oc.tolist() == [0, 0, 0]
    rows = np.ones((3, 2, 3), np.int32)
    same(check(ctx, [1, 0, 2], rows, [-1, -1, -1]), ([1, 0, 2], rows, [[0, 0], [1, 1], [2, 2]]))     # no links


# ---- end to end ----------------------------------------------------------------------------------------------------------------------
def walker(frames=5, step=3):
    """One person of 18 joints inside 64 x 96 who moves `step` pixels to the right a frame: [(18, 3) int32 per frame]."""
    shape = np.array([[24, 8], [24, 16], [16, 17], [12, 26], [10, 36], [32, 17], [36, 26], [38, 36], [19, 34], [18, 45], [17, 56],
                      [29, 34], [30, 45], [31, 56], [22, 6], [26, 6], [19, 8], [29, 8]], np.int32)
    out = []
    for t in range(frames):
        kp = np.ones((18, 3), np.int32)
        kp[:, :2] = shape + [10 + step * t, 2]
        out.append(kp)
    return out


def test_end_to_end_tracker_fill_masks(ctx):
    from terran_amd import PoseTracker, fill_pose_tracks, tracking, vis
    rows = walker()
    rows[3][4, 2] = 0                                   # and the right wrist is lost a frame after the person is
    clip = [[{'keypoints': r.copy(), 'score': np.float64(0.5 + 0.1 * t)}] for t, r in enumerate(rows)]
    clip[2] = []
    tracking.reset_pose_track_ids()
    ids = PoseTracker(max_gap=1, radius=0.3, ctx=ctx).update(clip)
    assert [v.tolist() for v in ids] == [[0], [0], [], [0], [0]]
    got = fill_pose_tracks(clip, max_gap=2, ctx=ctx)
    want = fill_pose_tracks(clip, max_gap=2, ctx=fm.ModelContext())
    assert [len(f) for f in got] == [1] * 5 and got[2][0]['filled'] is True and got[2][0]['pose_track'] == 0 and got[2][0]['score'] == 0.6
    for f, g in zip(got, want):
        for p, q in zip(f, g):
            assert p.keys() == q.keys() and all(np.array_equal(p[k], q[k]) for k in p)
    # 6 pixels in two frames: the middle is where the person was; the wrist, from frame 1 to frame 4, is a third and two thirds
    middle = walker()[2]
    middle[:, 2] = 2
    assert np.array_equal(got[2][0]['keypoints'], middle)
    assert got[3][0]['keypoints'][4].tolist() == walker()[3][4, :2].tolist() + [2]
    masks = vis.pose_masks((5, 64, 96), got, ctx=ctx).download()
    assert np.array_equal(masks, vis.pose_masks((5, 64, 96), want, ctx=ctx).download())
    assert masks[2].any() and np.array_equal(masks[2], vis.pose_masks((1, 64, 96), [[{'keypoints': walker()[2]}]], ctx=ctx).download()[0])
    assert not vis.pose_masks((5, 64, 96), clip, ctx=ctx).download()[2].any()


def test_face_twin_fill_then_blur(ctx):
    from terran_amd import fill_face_tracks, vis
    rng = np.random.default_rng(8)
    host = rng.integers(0, 256, (5, 64, 96, 3), dtype=np.uint8)
    lm = np.array([[6, 8], [16, 8], [11, 13], [7, 18], [15, 18]], np.float32)

    def face(t, track):
        at = np.array([8 + 5 * t, 10 + 2 * t], np.float32)
        return {'bbox': np.concatenate([at, at + [22, 27]]).astype(np.float32), 'landmarks': lm + at, 'score': np.float32(0.9 - 0.1 * t), 'track': track}

    clip = [[face(0, 4)], [face(1, 4), {'bbox': np.array([60, 30, 80, 50], np.float32), 'landmarks': lm + [60, 30], 'score': np.float32(0.3)}],
            [], [], [face(4, 4)]]
    got = fill_face_tracks(clip, max_gap=2, ctx=ctx)
    want = fill_face_tracks(clip, max_gap=2, ctx=fm.ModelContext())
    assert [len(f) for f in got] == [1, 2, 1, 1, 1]
    for f, g in zip(got, want):
        for p, q in zip(f, g):
            assert p.keys() == q.keys() and all(np.array_equal(p[k], q[k]) for k in p)
    # frame 1 -> frame 4, (13, 12) -> (28, 18): 5 and 2 a frame
    assert got[2][0]['bbox'].tolist() == [18, 14, 40, 41] and got[3][0]['bbox'].tolist() == [23, 16, 45, 43]
    assert got[2][0]['filled'] and got[2][0]['track'] == 4 and got[2][0]['bbox'].dtype == got[2][0]['landmarks'].dtype == np.int32
    assert [len(f) for f in fill_face_tracks(clip, max_gap=1, ctx=ctx)] == [1, 2, 0, 0, 1]
    blurred = vis.blur_faces(ctx.upload(host), got, ctx=ctx).download()
    assert np.array_equal(blurred, vis.blur_faces(ctx.upload(host), want, ctx=ctx).download())
    bare = vis.blur_faces(ctx.upload(host), clip, ctx=ctx).download()
    assert np.array_equal(bare[2], host[2]) and np.array_equal(bare[3], host[3])
    for t in (2, 3):
        x0, y0, x1, y1 = got[t][0]['bbox'].tolist()
        changed = (blurred[t] != host[t]).any(-1)
        assert changed[y0:y1, x0:x1].mean() > 0.9 and not changed[:, x1 + 1:].any() and not changed[:, :x0].any()
    assert np.array_equal(blurred[[0, 1, 4]], bare[[0, 1, 4]])
