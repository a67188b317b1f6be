"""-m gpu: skeleton tracking.  ta_poses_track against the model of tests/track_model.py with np.array_equal and no tolerance
anywhere: every edge of the predicate, the order and its ties, costs at the top of the range, a chain that takes one round per
link, availability over frames, sequences, seeded moving crowds at the wave and workgroup seams with the scratch matrix cut to
one frame a batch, the per-frame limit, every error, the empty cases; PoseTracker's split invariance on the device, and
PoseTracking end to end behind the pose network."""
import numpy as np
import pytest

from tests import track_model as tm

pytestmark = pytest.mark.gpu

NAMES = ('prev', 'root', 'links')


@pytest.fixture(scope='module')
def ctx():
    from terran_amd import lib
    c = lib.Context(0)
    yield c
    c.close()


def same(got, want):
    for a, b, what in zip(got, want, NAMES):
        assert a.dtype == b.dtype == np.int32 and a.shape == b.shape, (what, a.dtype, b.dtype, a.shape, b.shape)
        assert np.array_equal(a, b), (what, int(np.argmax(a != b)))


def check(ctx, fps, hist, counts, kp, closed=None, radius=100, min_shared=3, max_gap=0, want=None):
    if want is None:
        want = tm.track_rounds_model(fps, hist, counts, kp, closed, radius, min_shared, max_gap)
    got = ctx.poses_track(fps, hist, counts, kp, closed, radius, min_shared, max_gap)
    same(got, want[:3])
    return got


def sequences(seqs):
    """[[rows of frame 0, rows of frame 1, ...] per sequence] -> (frames_per_sequence, no history, pose_counts, keypoints)."""
    counts, kp = tm.call_of([f for s in seqs for f in s])
    return np.array([len(s) for s in seqs], np.int32), np.zeros(len(seqs), np.int32), counts, kp


def apart(a, b, g):
    """Rows a and b as a sequence of their own, g frames apart (empty frames between)."""
    return [[a]] + [[]] * (g - 1) + [[b]]


# ---- edges of the predicate ----------------------------------------------------------------------------------------------------
# radius 50 permille, min_shared 3, max_gap 2.  A3: three joints, size 100; they moved by D in all: the bound is
# 2500 * g * 10^4 * 3 / 10^6 = 75 g.  A: a fourth joint, the bound is 100 g
A3 = {0: (0, 0), 1: (100, 0), 2: (50, 10)}
A = {0: (0, 0), 1: (100, 0), 2: (50, 10), 5: (7, 7)}
SMALL = {0: (0, 0), 1: (10, 0), 2: (5, 1)}             # size 10: its own bound is 0.75 g
POINT = {0: (5, 5), 1: (5, 5), 2: (5, 5)}              # size 0


def moved(js, by, also=None):
    out = {j: (x + by.get(j, (0, 0))[0], y + by.get(j, (0, 0))[1]) for j, (x, y) in js.items()}
    out.update(also or {})
    return tm.pose_row(out)


ABSENT_ON_TOP = moved(A, {})
ABSENT_ON_TOP[2, 2] = 0                                # joint 2 absent, its coordinates on top of the partner's
# (a row, b row, g, linked?)
EDGES = [
    (tm.pose_row(A3), moved(A3, {0: (3, 4), 1: (3, 4), 2: (0, 5)}), 1, True),            # D = 75: met exactly
    (tm.pose_row(A), moved(A, {0: (3, 4), 1: (3, 4), 2: (0, 5), 5: (5, 1)}), 1, False),  # s = 4: D = 101 against 100
    (tm.pose_row(A3), moved(A3, {0: (3, 4), 1: (3, 4), 2: (1, 5)}), 1, False),           # D = 76
    (tm.pose_row(A3), moved(A3, {0: (9, 12)}), 3, True),                                 # g = max_gap + 1: D = 225 = 75 * 3
    (tm.pose_row(A3), moved(A3, {0: (9, 12), 1: (0, 1)}), 3, False),                     # D = 226
    (tm.pose_row(A3), moved(A3, {0: (9, 12)}), 2, False),                                # the same move a frame earlier: 225 > 150
    (tm.pose_row(A), moved(A, {}), 4, False),                                          # beyond the gap, whatever the cost
    (tm.pose_row({j: A[j] for j in (0, 1, 2)}), moved(A, {}), 1, True),                # s = min_shared
    (tm.pose_row({j: A[j] for j in (0, 1)}), moved(A, {}), 1, False),                  # one less
    (tm.pose_row(A), ABSENT_ON_TOP, 1, True),                                          # 0, 1, 5 are shared: s = 3
    (tm.pose_row({j: A[j] for j in (0, 1, 2)}), ABSENT_ON_TOP, 1, False),              # the absent joint does not count: s = 2
    (tm.pose_row(SMALL), moved(SMALL, {0: (1, 0)}), 1, False),                         # D = 1 > 0.75
    (tm.pose_row(SMALL), moved(SMALL, {0: (1, 0)}, {9: (100, 1)}), 1, True),           # M from the larger skeleton, b: size 100
    (moved(SMALL, {}, {9: (100, 1)}), moved(SMALL, {0: (1, 0)}), 1, True),             # ... and a
    (tm.pose_row(POINT), tm.pose_row(POINT), 1, True),                                 # size 0 matches D = 0
    (tm.pose_row(POINT), moved(POINT, {0: (0, 1), 1: (0, 1), 2: (0, 1)}), 3, False),   # and nothing else: M = 0, D = 3
]


def test_edges_of_the_predicate(ctx):
    call = sequences([apart(a, b, g) for a, b, g, _ in EDGES])
    prev, root, links = check(ctx, *call, None, 50, 3, 2)
    last, b_rows = np.cumsum(call[0]) - 1, 2 * np.arange(len(EDGES)) + 1            # a sequence's last frame holds its b
    assert (prev[b_rows] >= 0).tolist() == [e[3] for e in EDGES] == (links[last] > 0).tolist()
    assert all(p in (-1, r - 1) for p, r in zip(prev[b_rows], b_rows)) and (prev[b_rows - 1] == -1).all()
    assert tm.pair(EDGES[1][0], EDGES[1][1], 1, 50, 3)[1] == 101 * (tm.LCM // 4)
    # the ends of the parameters' ranges
    a, b = tm.pose_row(A), moved(A, {0: (100, 0)})
    assert (check(ctx, *sequences([apart(a, b, 1)]), None, 1000, 1, 0)[0] >= 0).tolist() == [False, True]
    assert (check(ctx, *sequences([apart(a, b, 31), apart(a, b, 32)]), None, 1, 4, 30)[2] > 0).sum() == 0
    assert (check(ctx, *sequences([apart(a, a, 31), apart(a, a, 32)]), None, 1, 4, 30)[2] > 0).tolist() == [False] * 31 + [True] + [False] * 33
    every = tm.pose_row({j: (10 * j, j * j) for j in range(18)})
    assert check(ctx, *sequences([apart(every, every, 1)]), None, 1, 18, 0)[0].tolist() == [-1, 0]


# ---- the order -------------------------------------------------------------------------------------------------------------------
LEFT, RIGHT = (0, 1, 2), (3, 4, 5)                      # two skeletons that share no joint never link to each other


def tri(x, y, joints_=LEFT, size=60):
    return tm.pose_row({joints_[0]: (x, y), joints_[1]: (x + size, y), joints_[2]: (x, y + size)})


def both(x, y):
    r = tri(x, y, LEFT)
    r += tri(x, y, RIGHT)
    return r


def test_order_and_ties(ctx):
    # two equally cheap predecessors in one frame: the lower row; the cheaper one wherever it stands
    seqs = [[[tri(98, 100), tri(102, 100)], [tri(100, 100)]],
            [[tri(97, 100), tri(102, 100)], [tri(100, 100)]],
            # two predecessors in different frames with equal cost (they share no joint and do not link): the smaller g
            [[tri(98, 100, LEFT)], [tri(102, 100, RIGHT)], [both(100, 100)]],
            [[tri(102, 100, RIGHT)], [tri(98, 100, LEFT)], [both(100, 100)]],
            # ... and the cheaper one, though it is further back
            [[tri(99, 100, LEFT)], [tri(102, 100, RIGHT)], [both(100, 100)]],
            # two rows want one predecessor: the cheaper pair, and of equal ones the lower b
            [[tri(100, 100)], [tri(103, 100), tri(98, 100)]],
            [[tri(100, 100)], [tri(102, 100), tri(98, 100)]]]
    prev, root, links = check(ctx, *sequences(seqs), None, 100, 3, 1)
    assert prev.tolist() == [-1, -1, 0, -1, -1, 4, -1, -1, 7, -1, -1, 10, -1, -1, 12, -1, -1, 15, -1, 18, -1]
    assert root.tolist() == [0, 1, 0, 3, 4, 4, 6, 7, 7, 9, 10, 10, 12, 13, 12, 15, 16, 15, 18, 18, 20]


def test_costs_at_the_top_of_the_range(ctx):
    """One shared joint that moved by about (2^15, 2^15) between skeletons as large as the range allows, two frames apart at
    radius 1000: D is 2 * 32764^2 against 32765^2 + 32763^2, two more, and the costs, D * 12 252 240, lie above 2^54.  (The
    header's bound of 2^60 is loose: a cost is at most 12 252 240 * 2^31 < 2^55 whatever s is, so costs near 2^59 do not exist;
    and float64 cannot tie two costs, which differ by at least 12 252 240 / 18.)  float32 ties them -- restated here -- and the
    cheaper one stands at the HIGHER row, so any tie links the wrong one.  The kernel keeps int64 throughout."""
    far = (16383, 16383)
    a0 = tm.pose_row({0: (-16383, -16381), 5: far})
    a1 = tm.pose_row({0: (-16382, -16382), 5: far})
    b = tm.pose_row({0: (16382, 16382), 7: (-16383, -16383)})
    cost = [tm.pair(a, b, 2, 1000, 1) for a in (a0, a1)]
    assert cost[0][0] and cost[1][0] and cost[1][1] < cost[0][1] and cost[0][1] - cost[1][1] == 2 * tm.LCM and cost[1][1] > 1 << 54
    f32 = [np.float32(tm.LCM) * (np.float32(dx) ** 2 + np.float32(dy) ** 2) for dx, dy in ((32765, 32763), (32764, 32764))]
    f64 = [float(tm.LCM) * (float(dx) ** 2 + float(dy) ** 2) for dx, dy in ((32765, 32763), (32764, 32764))]
    print('costs', [c[1] for c in cost], 'float32', f32, 'float64', f64)
    assert f32[0] == f32[1] and f64[1] < f64[0]
    assert not tm.pair(a1, b, 1, 1000, 1)[0]            # a frame apart the bound is half as wide
    prev, _, _ = check(ctx, *sequences([[[a0, a1], [], [b]], [[a1, a0], [], [b]], [[a0, a1], [b]]]), None, 1000, 1, 1)
    assert prev.tolist() == [-1, -1, 1, -1, -1, 3, -1, -1, -1]
    # the mirror image, at the other end of the range
    prev, _, _ = check(ctx, *sequences([[[-a0, -a1], [], [-b]]]), None, 1000, 1, 1)
    assert prev.tolist() == [-1, -1, 1]


def chain(length, size):
    """The worst case of the rounds, as in the link's tests: skeletons of frame 0 (A) and of frame 1 (B) alternate on a line,
    A0 B0 A1 B1 ..., and the gaps between neighbours fall by one pixel a step, so every A prefers the B on its right and every B
    the A on its right: only the last pair is mutually best, and committing it frees the pair before it."""
    gap = lambda k: 2 * length + 50 - k
    at, a, b = 0, [], []
    for i in range(length):
        a.append(tri(at, 0, size=size))
        at += gap(2 * i)
        b.append(tri(at, 0, size=size))
        if i + 1 < length:
            at += gap(2 * i + 1)
    return [a, b]


def test_a_chain_takes_one_round_per_link(ctx):
    length = 40
    call = sequences([chain(length, 2 * length + 50), chain(3, 56)])
    want = tm.track_rounds_model(*call, None, 1000, 3, 0)
    assert want[3] == length + 1
    prev, _, links = check(ctx, *call, None, 1000, 3, 0, want)
    assert prev[length:2 * length].tolist() == list(range(length)) and links.tolist() == [0, length, 0, 3]


# ---- availability ------------------------------------------------------------------------------------------------------------------
def test_availability(ctx):
    a, b1, b2 = both(100, 100), tri(101, 100, LEFT), tri(100, 101, RIGHT)
    seqs = [[[a], [b1], [b2]],                           # a is taken at frame 1: not available at frame 2
            [[a], [], [b2]],                             # not taken: still there a frame later
            [[a], [], [], [b2]],                         # until the gap runs out
            [[a], [b2]], [[a], [b2]]]                    # the second one's a is closed on input
    fps, hist, counts, kp = sequences(seqs)
    hist[3:] = 1
    closed = np.zeros(len(kp), np.uint8)
    closed[-2] = 1
    prev, root, links = check(ctx, fps, hist, counts, kp, closed, 100, 3, 1)
    assert prev.tolist() == [-1, 0, -1, -1, 3, -1, -1, -1, 7, -1, -1]
    assert root.tolist() == [0, 0, 2, 3, 3, 5, 6, 7, 7, 9, 10]
    # a closed row in a frame that is no history: it takes a predecessor and gives none
    closed = np.array([0, 1, 0], np.uint8)
    prev, _, _ = check(ctx, [3], [0], [1, 1, 1], np.stack([a, both(101, 100), both(102, 100)]), closed, 100, 3, 0)
    assert prev.tolist() == [-1, 0, -1]


# ---- sequences ---------------------------------------------------------------------------------------------------------------------
def test_sequences_are_independent(ctx):
    f0, f1 = [tri(10, 10), tri(200, 10)], [tri(201, 11), tri(11, 11)]
    counts, kp = tm.call_of([f0, f1])
    assert check(ctx, [2], [0], counts, kp)[0].tolist() == [-1, -1, 1, 0]
    assert check(ctx, [1, 1], [0, 0], counts, kp)[0].tolist() == [-1, -1, -1, -1]
    assert check(ctx, [2], [2], counts, kp)[0].tolist() == [-1, -1, -1, -1]          # all history


# ---- seeded crowds -----------------------------------------------------------------------------------------------------------------
CROWD_SIZES = (63, 64, 65, 255, 256, 257)
CROWD_PARAMS = (400, 3, 2)


def crowd_sequences():
    """One sequence of five frames per size: a dense moving crowd, people missing in frame 1, an empty frame 3."""
    rng = np.random.default_rng(11)
    seqs = []
    for n in CROWD_SIZES:
        frames, _ = tm.walkers(rng, n, 5, step=8, extent=int(20 * np.sqrt(n)) + 80, body=40)
        seqs.append(tm.drop(tm.drop(frames, 1, n // 5), 3, n))
    return seqs


def per_sequence(call, got):
    """The answer cut by sequence, rows relative to the sequence's first."""
    fps, _, counts, _ = call
    f = np.concatenate([[0], np.cumsum(fps)])
    r = np.concatenate([[0], np.cumsum(counts)])
    out = []
    for k in range(len(fps)):
        lo, hi = r[f[k]], r[f[k + 1]]
        prev, root = got[0][lo:hi], got[1][lo:hi]
        out.append((np.where(prev >= 0, prev - lo, -1).astype(np.int32), (root - lo).astype(np.int32), got[2][f[k]:f[k + 1]]))
    return out


@pytest.fixture(scope='module')
def crowd():
    seqs = crowd_sequences()
    call = sequences(seqs)
    call[1][:] = (0, 1, 0, 2, 0, 1)
    rng = np.random.default_rng(12)
    closed = (rng.random(len(call[3])) < 0.05).astype(np.uint8)
    want = tm.track_rounds_model(*call, closed, *CROWD_PARAMS)
    return seqs, call, closed, want


def test_crowds(ctx, crowd):
    seqs, call, closed, want = crowd
    assert want[3] >= 3 and want[2].sum() * 2 > len(call[3])                         # people compete, and most are followed
    check(ctx, *call, closed, *CROWD_PARAMS, want=want)
    # whole sequences in another order: every sequence's own answer
    order = [4, 1, 5, 0, 3, 2]
    fo = np.concatenate([[0], np.cumsum(call[0])])
    ro = np.concatenate([[0], np.cumsum(call[2])])
    rows = np.concatenate([np.arange(ro[fo[k]], ro[fo[k + 1]]) for k in order])
    moved_call = sequences([seqs[k] for k in order])
    moved_call[1][:] = call[1][order]
    got = ctx.poses_track(*moved_call, closed[rows], *CROWD_PARAMS)
    theirs, ours = per_sequence(moved_call, got), per_sequence(call, want)
    for slot, k in enumerate(order):
        same(theirs[slot], ours[k])


def test_crowds_one_frame_per_scratch_batch(ctx, crowd, monkeypatch):
    """Any frame's matrices alone exceed 8 bytes, so every frame is its own batch."""
    _, call, closed, want = crowd
    monkeypatch.setenv('TA_PT_MATRIX_BYTES', '8')
    check(ctx, *call, closed, *CROWD_PARAMS, want=want)
    monkeypatch.setenv('TA_PT_MATRIX_BYTES', '40000')   # and a few frames a batch, sequences cut in the middle
    check(ctx, *call, closed, *CROWD_PARAMS, want=want)


# ---- PoseTracker on the device -------------------------------------------------------------------------------------------------------
class ModelContext:
    def poses_track(self, *a):
        return tm.track_model(*a)


def clip(frames=12):
    rng = np.random.default_rng(21)
    crowd, _ = tm.walkers(rng, 30, frames, step=4, extent=260, body=40)
    crowd = tm.drop(tm.drop(crowd, 4, 9), 5, 3)
    return [[{'keypoints': r.copy()} for r in f] for f in crowd]


def test_tracker_split_invariance_on_the_device(ctx):
    from terran_amd import PoseTracker, tracking
    ids = []
    for context, batch in ((ModelContext(), 12), (ctx, 12), (ctx, 1), (ctx, 5)):
        tracking.reset_pose_track_ids()
        t, frames, got = PoseTracker(max_gap=2, radius=0.3, ctx=context), clip(), []
        for at in range(0, 12, batch):
            got += t.update(frames[at:at + batch])
        ids.append(np.concatenate(got))
    assert all(np.array_equal(ids[0], v) and v.dtype == np.int64 for v in ids[1:])
    assert len(set(ids[0].tolist())) < len(ids[0]) // 4


# ---- the limit -----------------------------------------------------------------------------------------------------------------------
def raw_track(ctx, fps, hist, counts, kp, closed=None, n_frames=None, n_poses=None, radius=100, min_shared=3, max_gap=0, outputs=True):
    from terran_amd import lib
    p = lambda a: lib.ptr(a) if a is not None and len(a) else None
    n_frames = len(counts) if n_frames is None else n_frames
    n_poses = (len(kp) if kp is not None else 0) if n_poses is None else n_poses
    prev, root = np.full(max(n_poses, 1), -7, np.int32), np.full(max(n_poses, 1), -7, np.int32)
    links = np.full(max(n_frames, 1), -7, np.int32)
    rc = ctx.lib.ta_poses_track(ctx.h, len(fps), p(fps), p(hist), n_frames, p(counts), p(kp), p(closed), n_poses, radius, min_shared, max_gap,
                                lib.ptr(prev) if outputs else None, lib.ptr(root) if outputs else None, lib.ptr(links))
    return rc, prev, root, links


def test_the_limit_per_frame(ctx):
    from terran_amd import lib
    n = lib.TRACK_MAX_PER_FRAME
    assert n == tm.MAX_PER_FRAME == 4096
    rng = np.random.default_rng(5)
    people, _ = tm.walkers(rng, 6, 2, step=3, extent=300)
    frames = []
    for f in people:                                    # six people among rows that hold no joint
        rows = np.zeros((n, 18, 3), np.int32)
        rows[rng.choice(n, 6, replace=False)] = f
        frames.append(rows)
    counts, kp = tm.call_of(frames)
    prev, _, links = check(ctx, [2], [0], counts, kp, None, 200, 3, 0)
    assert links.tolist() == [0, 6]
    one = np.ones(1, np.int32)
    rc, prev, root, links = raw_track(ctx, one, 0 * one, one * (n + 1), np.zeros((n + 1, 18, 3), np.int32))
    assert rc == lib.E_OVERFLOW and '4096' in ctx.last_error()
    assert (prev == -7).all() and (root == -7).all() and (links == -7).all()         # checked before any launch


# ---- errors and empty cases ------------------------------------------------------------------------------------------------------------
def test_errors(ctx):
    from terran_amd import lib
    i32 = lambda *v: np.array(v, np.int32)
    fps, hist, counts = i32(2, 1), i32(1, 0), i32(1, 2, 1)
    kp = np.zeros((4, 18, 3), np.int32)
    kp[:, :, 2] = 1
    big, small = 1 << 14, -(1 << 14)

    def wild(arr, index, value):
        out = arr.copy()
        out[index] = value
        return out

    cases = [
        (dict(fps=i32(-1, 4)), 'negative'), (dict(counts=i32(5, -2, 1)), 'negative'),
        (dict(fps=i32(2, 2)), 'sum'), (dict(n_frames=4), 'sum'), (dict(counts=i32(1, 2, 2)), 'sum'), (dict(n_poses=3), 'sum'),
        (dict(hist=i32(3, 0)), 'history_frames'), (dict(hist=i32(1, -1)), 'history_frames'),
        (dict(kp=None, n_poses=4), 'null'), (dict(outputs=False), 'null'), (dict(counts=None, n_frames=3), 'null'),
        (dict(radius=0), 'radius_permille'), (dict(radius=1001), 'radius_permille'), (dict(min_shared=0), 'min_shared'),
        (dict(min_shared=19), 'min_shared'), (dict(max_gap=-1), 'max_gap'), (dict(max_gap=31), 'max_gap'),
        (dict(kp=wild(kp, (3, 0, 0), big)), 'pose row 3'), (dict(kp=wild(kp, (0, 17, 1), small)), 'pose row 0'),
        (dict(kp=wild(wild(kp, (1, 14, 2), 0), (1, 14, 0), big)), 'pose row 1'),               # an absent joint counts too
    ]
    for change, what in cases:
        a = dict(fps=fps, hist=hist, counts=counts, kp=kp, closed=None, n_frames=None, n_poses=None, radius=100, min_shared=3, max_gap=0, outputs=True)
        a.update(change)
        rc, prev, root, links = raw_track(ctx, **a)
        assert rc == lib.E_INVALID and what in ctx.last_error(), (what, rc, ctx.last_error())
        assert (prev == -7).all() and (root == -7).all() and (links == -7).all()
    # the bound itself is 2^14 - 1 in size, and the third value of a joint is free
    ok = wild(wild(kp, (3, 0, 0), big - 1), (0, 17, 1), small + 1)
    ok[2, 5, 2] = 1 << 30
    check(ctx, fps, hist, counts, ok, None, 1000, 1, 0)
    with pytest.raises(lib.TerranAmdError) as e:
        ctx.poses_track(fps, hist, counts, kp, None, 100, 3, 40)
    assert e.value.code == lib.E_INVALID
    with pytest.raises(ValueError, match='history'):
        ctx.poses_track(fps, hist[:1], counts, kp)
    with pytest.raises(ValueError, match='closed'):
        ctx.poses_track(fps, hist, counts, kp, np.zeros(3, np.uint8))


def test_empty_cases(ctx):
    from terran_amd import lib
    none = np.zeros(0, np.int32)
    prev, root, links = ctx.poses_track(none, none, none, none.reshape(0, 18, 3))
    assert len(prev) == len(root) == len(links) == 0
    rc, _, _, links = raw_track(ctx, none, none, none, None, outputs=False)
    assert rc == lib.OK and (links == -7).all()
    rows = np.stack([tri(10, 10), tri(11, 10), tri(12, 10)])
    # sequences without frames, frames without rows, a sequence that is all history, one frame alone
    prev, root, links = check(ctx, [0, 3, 0, 2, 1], [0, 0, 0, 2, 0], [0, 1, 0, 0, 1, 1], rows)
    assert prev.tolist() == [-1, -1, -1] and root.tolist() == [0, 1, 2] and links.tolist() == [0] * 6
    prev, root, links = check(ctx, [4], [0], [1, 0, 1, 1], rows, None, 100, 3, 1)
    assert prev.tolist() == [-1, 0, 1] and root.tolist() == [0, 0, 0] and links.tolist() == [0, 0, 1, 1]
    rc, prev, root, links = raw_track(ctx, np.array([2], np.int32), np.array([0], np.int32), np.array([0, 0], np.int32), None)
    assert rc == lib.OK and links[:2].tolist() == [0, 0]


# ---- end to end --------------------------------------------------------------------------------------------------------------------------
def test_end_to_end_behind_the_pose_network(states):
    """The coded frames of the link's end-to-end test (the decoder weights assemble people on them), the first one shifted by
    one cell of the coded maps a frame -- 8 pixels at the network's input, 24 in the frame; the code is per cell, so a smaller
    shift carries nobody -- through Estimation on the seeded weights and PoseTracking: the ids equal the model's on the
    estimator's own output, and people are followed."""
    from terran_amd import Estimation, PoseTracker, PoseTracking, synth, tracking
    fr = synth.upscale_for_resize(synth.pose_code_frames(60, 2, 96, 128, 3), 288, 384)
    clip_ = np.stack([np.roll(fr[0], 24 * k, axis=1) for k in range(4)])
    est = Estimation(short_side=96, device=0, state=states('openpose_decoder'))
    tracking.reset_pose_track_ids()
    got = PoseTracking(estimator=est, tracker=PoseTracker(max_gap=1, radius=0.3, device=0))(clip_)
    assert len(got) == 4 and sum(map(len, got)) >= 4
    tracking.reset_pose_track_ids()
    again = [[{'keypoints': np.array(p['keypoints'])} for p in f] for f in got]
    want = PoseTracker(max_gap=1, radius=0.3, ctx=ModelContext()).update(again)
    ids = [[p['pose_track'] for p in f] for f in got]
    print('people', [len(f) for f in got], 'ids', ids)
    assert ids == [w.tolist() for w in want]
    assert len(set(k for f in ids for k in f)) < sum(map(len, ids))                   # somebody is followed
    # one frame alone continues the clip
    nxt = PoseTracking(estimator=est, tracker=PoseTracker(max_gap=1, radius=0.3, device=0))(np.roll(fr[0], 96, axis=1))
    assert isinstance(nxt, list) and all('pose_track' in p for p in nxt)
