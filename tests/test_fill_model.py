"""No GPU: the rule of ta_tracks_fill as tests/fill_model.py states it, pinned on cases computed by hand -- the rounding and its
halves, the window of a joint, the ends of a chain, a link that is too long, the order of synthesized rows, every refusal, that
filling a filled clip adds nothing -- and the host halves of fill_pose_tracks / fill_face_tracks on the model: faces packed and
unpacked, ids to prev, copies and not aliases, the duplicate id."""
import numpy as np
import pytest

from tests import fill_model as fm


def same(got, want):
    for a, b, what in zip(got, want, ('out_counts', 'out_points', 'out_source')):
        b = np.asarray(b, np.int32).reshape((-1,) + a.shape[1:])
        assert a.dtype == np.int32 and a.shape == b.shape, (what, a.dtype, a.shape, b.shape)
        assert np.array_equal(a, b), (what, a.tolist(), b.tolist())


@pytest.mark.parametrize('case', fm.hand_cases(), ids=lambda c: c[0])
def test_hand_cases(case):
    _, call, max_gap, mark, want = case
    same(fm.fill_model(*call, max_gap, mark), want)


def test_the_rounding_is_to_nearest_with_halves_up():
    for v0, v1, k, dt in ((0, 10, 1, 3), (0, -10, 1, 3), (0, 1, 1, 2), (0, -1, 1, 2), (-3, 4, 5, 31), (7, 7, 1, 2), ((1 << 22) - 1, 1 - (1 << 22), 30, 31)):
        exact2 = 2 * v0 * dt + 2 * (v1 - v0) * k                    # 2 dt times the exact value
        got = fm.interpolate(v0, v1, k, dt)
        assert 2 * dt * got - dt <= exact2 < 2 * dt * got + dt, (v0, v1, k, dt, got)
        assert abs(2 * (v1 - v0) * k + dt) < 1 << 29


def test_refusals():
    counts, points, prev = fm.seeded_clip(3, n_frames=6, tracks=5, n_points=3)
    fm.fill_model(counts, points, prev, 5, 2)

    def wild(arr, index, value):
        out = arr.copy()
        out[index] = value
        return out

    b = int(np.argmax(prev >= 0))                       # a row with a predecessor
    assert b < len(prev) - 1 and counts[-1] > 0
    twice = wild(prev, len(prev) - 1, prev[b])          # the last row takes b's predecessor as well
    cases = [
        dict(counts=wild(counts, 0, -1)), dict(counts=wild(counts, 0, counts[0] + 1)), dict(points=points[:, :0]),
        dict(points=np.zeros((len(points), 19, 3), np.int32)), dict(max_gap=-1), dict(max_gap=31), dict(mark=0), dict(mark=256),
        dict(points=wild(points, (0, 0, 0), 1 << 22)), dict(points=wild(wild(points, (1, 2, 2), 0), (1, 2, 1), -(1 << 22))),
        dict(prev=wild(prev, b, -2)), dict(prev=wild(prev, b, len(prev))), dict(prev=wild(prev, b, b)),
        dict(prev=wild(prev, 0, len(prev) - 1)), dict(prev=twice),
    ]
    for change in cases:
        a = dict(counts=counts, points=points, prev=prev, max_gap=5, mark=2)
        a.update(change)
        with pytest.raises(ValueError):
            fm.fill_model(**a)
    same_frame = fm.call_of([np.ones((2, 1, 3))], 1) + (np.array([-1, 0]),)
    with pytest.raises(ValueError, match='earlier frame'):
        fm.fill_model(*same_frame)
    # the bound itself is 2^22 - 1 in size, and the ranges' ends are taken
    fm.fill_model(counts, wild(points, (0, 0, 0), (1 << 22) - 1), prev, 0, 1)
    fm.fill_model(counts, wild(points, (0, 0, 1), 1 - (1 << 22)), prev, 30, 255)
    # the limit per frame: on the way in, and on the way out
    n = fm.MAX_PER_FRAME
    one = np.ones((n + 2, 1, 3), np.int32)
    with pytest.raises(ValueError, match='input rows'):
        fm.fill_model([n + 1, 1], one, np.full(n + 2, -1))
    out = np.full(n + 2, -1)
    out[n + 1] = 0
    with pytest.raises(ValueError, match='output rows'):
        fm.fill_model([1, n, 1], one, out)
    assert fm.fill_model([1, n - 1, 1], one[:n + 1], np.roll(out, -1)[:n + 1])[0].tolist() == [1, n, 1]


def test_filling_a_filled_clip_adds_nothing():
    counts, points, prev = fm.seeded_clip(11, n_frames=20, tracks=12, n_points=4, row_drop=0.3, point_drop=0.3)
    for max_gap in (0, 2, 5):
        oc, op, src = fm.fill_model(counts, points, prev, max_gap, 2)
        assert (len(op) > len(points)) == (max_gap > 0) and ((op[:, :, 2] == 2).sum() > 0) == (max_gap > 0)
        # ids kept: a row follows the row of its chain in the nearest frame before it, synthesized ones included
        root = np.arange(len(prev))
        for r in range(len(prev)):
            root[r] = root[prev[r]] if prev[r] >= 0 else r
        ids, at = [], 0
        for c in oc:
            ids.append([int(root[b]) for _, b in src[at:at + c]])
            at += c
        again = fm.fill_model(oc, op, fm.prev_of_ids(ids), max_gap, 3)
        same(again, (oc, op, np.repeat(np.arange(len(op)), 2)))


def test_empty_cases():
    none = np.zeros(0, np.int32)
    oc, op, src = fm.fill_model(none, none.reshape(0, 7, 3), none)
    assert oc.shape == (0,) and op.shape == (0, 7, 3) and src.shape == (0, 2)
    oc, op, src = fm.fill_model([0, 0], none.reshape(0, 18, 3), none)
    assert oc.tolist() == [0, 0] and len(op) == 0
    rows = np.ones((3, 2, 3), np.int32)
    same(fm.fill_model([1, 0, 2], rows, [-1, -1, -1]), ([1, 0, 2], rows, [[0, 0], [1, 1], [2, 2]]))


# ---- the host halves of the public calls -----------------------------------------------------------------------------------------------
def test_prev_of_ids():
    prev = fm.prev_of_ids([[4, None, 9], [], [9, -1, 4, 7], [np.int64(7), 4]])
    assert prev.dtype == np.int32 and prev.tolist() == [-1, -1, -1, 2, -1, 0, -1, 6, 5]
    assert fm.prev_of_ids([]).shape == (0,) and fm.prev_of_ids([[], []]).shape == (0,)
    with pytest.raises(ValueError, match='frame 1 carries id 3 twice'):
        fm.prev_of_ids([[3], [3, 5, 3]])
    fm.prev_of_ids([[None, None, -1, -1]])              # no id, as often as it likes


def test_faces_pack_and_unpack():
    from terran_amd import tracking
    face = {'bbox': np.array([10.9, 20.2, 30.5, 41.0], np.float32), 'landmarks': np.arange(10, dtype=np.float32).reshape(5, 2) + 0.75}
    p = tracking.pack_face(face)
    assert p.dtype == np.int32 and p.shape == (7, 3) and (p[:, 2] == 1).all()
    assert p[:2, :2].tolist() == [[10, 20], [30, 41]] and p[2:, :2].tolist() == np.arange(10).reshape(5, 2).tolist()
    bbox, lm = tracking.unpack_face(p)
    assert bbox.dtype == lm.dtype == np.int32 and bbox.tolist() == [10, 20, 30, 41] and lm.shape == (5, 2) and lm[4].tolist() == [8, 9]


def clip_of_poses():
    a = np.zeros((18, 3), np.int32)
    a[:6] = [[10 * j, 5 * j, 1] for j in range(6)]
    b = a.copy()
    b[:, :2] += [8, -4]
    b[3, 2] = 0                                         # joint 3 is lost where the track comes back
    c = b.copy()
    c[:, :2] += [2, 2]
    c[3, 2] = 1
    other = a.copy()
    other[:, :2] += 300
    return [[{'keypoints': a, 'score': np.float64(0.9), 'pose_track': 7, 'text': 'ann', 'extra': [1]}, {'keypoints': other, 'score': np.float64(0.5)}],
            [{'keypoints': other.copy(), 'score': np.float64(0.4), 'pose_track': None}],
            [{'keypoints': b, 'score': np.float64(0.6), 'pose_track': 7}],
            [{'keypoints': c, 'score': np.float64(0.8), 'pose_track': 7, 'text': 'bob'}]]


def test_fill_pose_tracks_on_the_model():
    from terran_amd import fill_pose_tracks
    clip = clip_of_poses()
    before = [[{k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in p.items()} for p in f] for f in clip]
    got = fill_pose_tracks(clip, max_gap=2, mark=5, ctx=fm.ModelContext())
    assert [len(f) for f in got] == [2, 2, 1, 1]
    new = got[1][1]                                     # behind the frame's own skeleton
    assert new['filled'] is True and new['pose_track'] == 7 and new['score'] == 0.6 and new['text'] == 'ann' and 'extra' not in new
    want = clip[0][0]['keypoints'].copy()
    want[:6, :2] += [4, -2]
    want[:6, 2] = 5
    want[3, :2] = [30 + 3, 15 - 1]                      # joint 3: from frame 0 to frame 3, (30, 15) -> (40, 13): a third of the way
    assert new['keypoints'].dtype == np.int32 and np.array_equal(new['keypoints'], want)
    assert got[2][0]['keypoints'][3].tolist() == [30 + 7, 15 - 1, 5]         # ... and two thirds, in the row that lacked it
    assert 'filled' not in got[2][0] and got[3][0]['text'] == 'bob'
    # the input is as it was, and nothing of the output is the input's
    for f, g, h in zip(clip, before, got):
        for p, q in zip(f, g):
            assert p.keys() == q.keys() and all(np.array_equal(p[k], q[k]) for k in p)
        for p, r in zip(f, h):
            assert r is not p and r['keypoints'] is not p['keypoints'] and not np.shares_memory(r['keypoints'], p['keypoints'])
    got[0][0]['keypoints'][:] = -1
    assert clip[0][0]['keypoints'][1].tolist() == [10, 5, 1]
    # max_gap 0 fills nothing; a device list is refused as PoseTracker refuses it; one id twice in a frame
    assert [len(f) for f in fill_pose_tracks(clip, max_gap=0, ctx=fm.ModelContext())] == [2, 1, 1, 1]
    with pytest.raises(ValueError, match='device list'):
        fill_pose_tracks(clip, device=[0, 1])
    clip[0][1]['pose_track'] = 7
    with pytest.raises(ValueError, match='twice'):
        fill_pose_tracks(clip, ctx=fm.ModelContext())


def test_fill_face_tracks_on_the_model():
    from terran_amd import fill_face_tracks
    lm = np.array([[12, 12], [18, 12], [15, 15], [13, 18], [17, 18]], np.float32)
    f0 = {'bbox': np.array([10, 10, 20, 20], np.float32), 'landmarks': lm, 'score': np.float32(0.9), 'track': 3, 'text': 'ann', 'cluster': 2}
    f2 = {'bbox': np.array([14, 10, 25, 21], np.float32), 'landmarks': lm + [4, 1], 'score': np.float32(0.7), 'track': 3}
    got = fill_face_tracks([[f0], [], [f2]], ctx=fm.ModelContext())
    assert [len(f) for f in got] == [1, 1, 1]
    mid = got[1][0]
    assert mid['filled'] is True and mid['track'] == 3 and mid['text'] == 'ann' and mid['cluster'] == 2 and mid['score'] == np.float32(0.7)
    assert mid['bbox'].dtype == np.int32 and mid['bbox'].tolist() == [12, 10, 23, 21]            # 22.5 and 20.5 round up
    assert mid['landmarks'].dtype == np.int32 and mid['landmarks'].tolist() == (lm + [2, 1]).astype(int).tolist()
    # the faces a frame had are returned as they were, in arrays of their own
    assert got[0][0]['bbox'].dtype == np.float32 and np.array_equal(got[0][0]['bbox'], f0['bbox']) and got[0][0]['bbox'] is not f0['bbox']
    assert 'filled' not in got[0][0] and 'filled' not in f0 and got[2][0]['track'] == 3
    with pytest.raises(ValueError, match='device list'):
        fill_face_tracks([[f0]], device=(0, 1))
