"""No GPU: the two statements of the tracking rule (tests/track_model.py) against each other, pairs worked out by hand, and
PoseTracker's host half against a stand-in context whose poses_track is the model."""
import numpy as np
import pytest

from terran_amd import tracking
from tests import track_model as tm


class ModelContext:
    """What PoseTracker needs of a context, answered by the model."""

    def __init__(self):
        self.calls = []

    def poses_track(self, frames_per_sequence, history_frames, pose_counts, keypoints, closed=None, radius_permille=100, min_shared=3, max_gap=0):
        self.calls.append((list(frames_per_sequence), list(history_frames), radius_permille, min_shared, max_gap))
        return tm.track_model(frames_per_sequence, history_frames, pose_counts, keypoints, closed, radius_permille, min_shared, max_gap)


@pytest.fixture(autouse=True)
def fresh_ids():
    tracking.reset_pose_track_ids()


@pytest.mark.parametrize('seed', [0, 1, 2])
def test_walk_and_rounds_agree_on_seeded_crowds(seed):
    rng = np.random.default_rng(seed)
    crowd, _ = tm.walkers(rng, 40, 6, step=6, extent=160, body=30)       # dense: people compete for predecessors
    crowd = tm.drop(tm.drop(crowd, 2, 7), 4, 40)                         # a thinner frame and an empty one
    other, _ = tm.walkers(rng, 9, 3, step=2, extent=100)
    counts, kp = tm.call_of(crowd + other)
    closed = (rng.random(len(kp)) < 0.1).astype(np.uint8)
    total = 0
    for radius, min_shared, max_gap in ((100, 3, 0), (300, 5, 2), (1000, 1, 5)):
        walk = tm.track_model([6, 3], [1, 0], counts, kp, closed, radius, min_shared, max_gap)
        rounds = tm.track_rounds_model([6, 3], [1, 0], counts, kp, closed, radius, min_shared, max_gap)
        assert all(np.array_equal(a, b) for a, b in zip(walk, rounds[:3])) and rounds[3] >= 1
        prev, root, links = walk
        taken = prev[prev >= 0]
        assert len(set(taken.tolist())) == len(taken) and not closed[taken].any()       # one successor each, none for a closed row
        assert (prev[:counts[0]] == -1).all() and links[0] == 0                         # the history frame looks for nobody
        assert all(root[r] == (r if prev[r] < 0 else root[prev[r]]) for r in range(len(kp)))
        assert links.sum() == (prev >= 0).sum()
        total += int(links.sum())
    assert total > 100


def test_pairs_by_hand():
    # a: joints 0, 1, 2 on a line, size 100; b the same moved by (3, 4) on two joints and by (0, 5) on the third: D = 75, s = 3
    a = tm.pose_row({0: (0, 0), 1: (100, 0), 2: (50, 10), 5: (7, 7)})
    b = tm.pose_row({0: (3, 4), 1: (103, 4), 2: (50, 15), 9: (7, 7)})
    assert tm.pair(a, b, 1, 50, 3) == (True, 75 * (tm.LCM // 3))         # 75 * 10^6 <= 2500 * 1 * 10^4 * 3, met exactly
    b[2, 1] = 16                                                         # D = 86
    assert tm.pair(a, b, 1, 50, 3) == (False, 86 * (tm.LCM // 3))
    b[2, 1] = 15
    b[1, 0] = 104                                                        # D = 25 + 32 + 25 = 82, one unit of a coordinate more
    assert tm.pair(a, b, 1, 50, 3)[0] is False
    # g = 3 triples the bound: D = 225 is met exactly, 226 is not
    b = tm.pose_row({0: (9, 12), 1: (100, 0), 2: (50, 10)})
    assert tm.pair(a, b, 3, 50, 3) == (True, 225 * (tm.LCM // 3)) and tm.pair(a, b, 2, 50, 3)[0] is False
    b[1, 1] = 1
    assert tm.pair(a, b, 3, 50, 3) == (False, 226 * (tm.LCM // 3))
    # too few shared joints; an absent joint on top of its partner does not count
    assert tm.pair(a, b, 3, 50, 4)[0] is False
    c = a.copy()
    c[5, 2] = 0
    assert tm.pair(a, c, 1, 50, 4) == (False, 0) and tm.pair(a, a, 1, 50, 4) == (True, 0)
    # M is the larger of the two sizes: a small skeleton beside a large one
    small = tm.pose_row({0: (0, 0), 1: (10, 0), 2: (5, 1)})
    assert tm.size(tm.joints(small)) == 10 and tm.pair(small, small, 1, 50, 3) == (True, 0)
    assert tm.pair(a, tm.pose_row({}), 1)[1] is None


def person(x, y, **keys):
    """A skeleton of size 40 at (x, y)."""
    d = {'keypoints': tm.pose_row({0: (x, y), 1: (x, y + 20), 2: (x - 20, y + 20), 5: (x + 20, y + 20), 8: (x - 8, y + 40)})}
    d.update(keys)
    return d


def tracker(**kw):
    kw.setdefault('ctx', ModelContext())
    return tracking.PoseTracker(**kw)


def test_ids_persist_and_are_numbered_in_row_order():
    t = tracker(max_gap=0)
    first = t.update([[person(100, 100), person(300, 100)]])
    assert [v.tolist() for v in first] == [[0, 1]] and first[0].dtype == np.int64
    frame = [person(302, 101), person(500, 100), person(101, 99)]
    assert t.update(frame).tolist() == [1, 2, 0]
    assert [p['pose_track'] for p in frame] == [1, 2, 0] and type(frame[0]['pose_track']) is int
    assert t.ctx.calls[-1] == ([2], [1], 100, 3, 0)
    other = tracker(max_gap=0)                         # the counter is the process's, not the tracker's
    assert other.update([person(0, 0)]).tolist() == [3]
    tracking.reset_pose_track_ids(10)
    assert other.update([person(900, 900)]).tolist() == [10]


def test_a_person_returns_within_max_gap_and_not_after():
    for away, back in ((2, True), (3, False)):
        tracking.reset_pose_track_ids()
        t = tracker(max_gap=2)
        assert t.update([person(100, 100), person(400, 400)]).tolist() == [0, 1]
        for _ in range(away):
            assert t.update([person(400, 400)]).tolist() == [1]
        assert t.update([person(401, 401), person(101, 100)]).tolist() == [1, 0 if back else 2]


def clip(seed=4, n=12, frames=12):
    rng = np.random.default_rng(seed)
    crowd, _ = tm.walkers(rng, n, frames, step=4, extent=200, body=40)
    crowd = tm.drop(tm.drop(crowd, 5, 4), 6, 2)
    return [[{'keypoints': r.copy()} for r in f] for f in crowd]


@pytest.mark.parametrize('batch', [1, 5, 7])
def test_one_call_equals_batches(batch):
    whole = clip()
    want = tracker(max_gap=2, radius=0.3).update(whole)
    assert len(set(np.concatenate(want).tolist())) < sum(map(len, want)) // 2       # people are followed
    tracking.reset_pose_track_ids()
    parts, t = clip(), tracker(max_gap=2, radius=0.3)
    got = []
    for at in range(0, len(parts), batch):
        got += t.update(parts[at:at + batch])
    assert all(np.array_equal(a, b) for a, b in zip(got, want)) and len(got) == len(want)
    assert [p['pose_track'] for f in parts for p in f] == [p['pose_track'] for f in whole for p in f]
    assert len(t._history) == 3


def test_carry_hands_a_name_on_and_overwrites_nothing():
    t = tracker(max_gap=1)
    t.update([[person(100, 100, text='ada', track=7), person(400, 100, text='bob')]])
    second = [person(102, 100), person(401, 100, text='robert', cluster=3)]
    t.update([second])
    assert second[0]['text'] == 'ada' and second[0]['track'] == 7 and 'cluster' not in second[0]
    assert second[1]['text'] == 'robert' and 'track' not in second[1]
    third = [person(402, 101), person(800, 800)]
    t.update(third)                                    # the single-frame form
    assert third[0]['text'] == 'robert' and third[0]['cluster'] == 3 and 'text' not in third[1]
    # ada was not seen in the third frame; one frame of gap later she is still ada
    fourth = [person(103, 101)]
    t.update(fourth)
    assert fourth[0]['text'] == 'ada' and fourth[0]['pose_track'] == 0
    only = tracker(max_gap=0, carry=('text',))
    only.update([person(0, 0, text='x', track=1)])
    nxt = [person(1, 0)]
    only.update(nxt)
    assert nxt[0]['text'] == 'x' and 'track' not in nxt[0]


def test_both_forms_and_parameters():
    t = tracker(max_gap=4, radius=0.1234, min_shared=2)
    one = t.update([person(10, 10)])
    assert isinstance(one, np.ndarray) and one.tolist() == [0]
    many = t.update([[person(11, 10)], [], [person(12, 11)]])
    assert [v.tolist() for v in many] == [[0], [], [0]]
    assert t.update([]).tolist() == []                 # one frame with nobody in it
    assert t.update(()).tolist() == [] and t.ctx.calls[-1] == ([6], [5], 123, 2, 4)


def test_refuses_a_device_list_and_ragged_input():
    with pytest.raises(ValueError):
        tracking.PoseTracker(device=[0, 1])
    t = tracker()
    with pytest.raises(ValueError):
        t.update([[person(0, 0)], person(5, 5)])
    assert t.ctx.calls == [] and t._history == []


def test_factory():
    from terran_amd import Estimation, PoseTracking, pose_tracking

    class Video:
        framerate = 30

    est = Estimation(lazy=True)
    a = pose_tracking(video=Video(), estimator=est, radius=0.2, ctx=ModelContext())
    assert isinstance(a, PoseTracking) and a.estimator is est and a.tracker.max_gap == 6 and a.tracker.radius_permille == 200
    assert pose_tracking(estimator=est).tracker.max_gap == 5 and pose_tracking(estimator=est, max_gap=1).tracker.max_gap == 1
    with pytest.raises(ValueError):
        pose_tracking(estimator=lambda frames: frames)
    # PoseTracking behind any estimator-like callable
    frames = [[person(10, 10)], [person(11, 11), person(300, 300)]]
    pt = PoseTracking(estimator=lambda batch: [frames[k] for k in batch], tracker=tracker(max_gap=0))
    got = pt([0, 1])
    assert [[p['pose_track'] for p in f] for f in got] == [[0], [0, 1]]
