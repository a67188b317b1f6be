"""The model of skeleton tracking (no GPU import): what ta_poses_track must answer, bit for bit.

`track_model` restates what include/terran_amd.h says of ta_poses_track, literally and for clarity, not for speed: per frame in
ascending order, every qualifying pair with an open predecessor, sorted by (cost, g, a, b), walked once.  `track_rounds_model` is
an independent second statement: the mutual-best rounds the device runs.  Both work on Python ints, so no width or rounding of
any number format enters.  The builders below make the frames the CPU and the GPU tests share.
"""
import numpy as np

LCM = 12252240                      # lcm(1 .. 18)
COORD_LIMIT = 1 << 14
MAX_PER_FRAME = 4096


def joints(kp_row):
    """The present joints of one (18, 3) row as {joint: (x, y)} in Python ints."""
    return {j: (int(kp_row[j][0]), int(kp_row[j][1])) for j in range(18) if int(kp_row[j][2]) != 0}


def size(js):
    """The larger side of the extent of a {joint: (x, y)}; 0 with no joint."""
    if not js:
        return 0
    xs, ys = [p[0] for p in js.values()], [p[1] for p in js.values()]
    return max(max(xs) - min(xs), max(ys) - min(ys))


def pair(a_row, b_row, g, radius_permille=100, min_shared=3):
    """Two (18, 3) rows g frames apart -> (qualifies, cost); the cost is None when no joint is shared."""
    a, b = joints(a_row), joints(b_row)
    shared = [j for j in a if j in b]
    s = len(shared)
    if s == 0:
        return False, None
    m = max(size(a), size(b))
    d = sum((a[j][0] - b[j][0]) ** 2 + (a[j][1] - b[j][1]) ** 2 for j in shared)
    return s >= min_shared and d * 1000000 <= radius_permille ** 2 * g * m * m * s, d * (LCM // s)


def _layout(frames_per_sequence, history_frames, pose_counts, keypoints, closed):
    fps = [int(v) for v in np.asarray(frames_per_sequence).reshape(-1)]
    hist = [int(v) for v in np.asarray(history_frames).reshape(-1)]
    pc = [int(v) for v in np.asarray(pose_counts).reshape(-1)]
    kp = np.asarray(keypoints, np.int64).reshape(-1, 18, 3)
    assert len(fps) == len(hist) and sum(fps) == len(pc) and sum(pc) == len(kp)
    assert all(0 <= h <= f for h, f in zip(hist, fps))
    shut = [False] * len(kp) if closed is None else [bool(v) for v in np.asarray(closed).reshape(-1)]
    assert len(shut) == len(kp)
    off = np.concatenate([[0], np.cumsum(pc)]).astype(int).tolist()
    return fps, hist, pc, kp, shut, off


def frame_pairs(kp, off, t, first, max_gap, radius_permille, min_shared):
    """Every qualifying pair into frame t of a sequence that starts at frame `first`, as (cost, g, a, b) with global rows.  A
    numpy prefilter keeps the explicit loop to the pairs that can qualify: enough shared joints, and the shared joint that
    moved least within the bound on the mean (the mean is no smaller than the least; all of it far inside int64)."""
    out = []
    for g in range(1, max_gap + 2):
        ta = t - g
        if ta < first:
            break
        a0, a1 = off[ta], off[ta + 1]
        if a0 == a1:
            continue
        size_a = np.array([size(joints(r)) for r in kp[a0:a1]], np.int64)
        for b in range(off[t], off[t + 1]):
            if not kp[b, :, 2].any():                   # no joint: it shares none
                continue
            shared = (kp[a0:a1, :, 2] != 0) & (kp[b, :, 2] != 0)
            d = ((kp[a0:a1, :, :2] - kp[b, :, :2]) ** 2).sum(2)
            least = np.where(shared, d, 1 << 40).min(1)
            m = np.maximum(size_a, size(joints(kp[b])))
            can = (shared.sum(1) >= min_shared) & (least * 1000000 <= radius_permille ** 2 * g * m * m)
            for a in np.nonzero(can)[0]:
                ok, c = pair(kp[a0 + a], kp[b], g, radius_permille, min_shared)
                if ok:
                    out.append((c, g, a0 + int(a), b))
    return out


def _greedy(pairs, succ, prev):
    for _, _, a, b in sorted(pairs):
        if succ[a] is None and prev[b] < 0:
            succ[a], prev[b] = b, a


def _rounds(pairs, succ, prev):
    n = 0
    while True:
        n += 1
        best_a, best_b = {}, {}
        for c, g, a, b in pairs:
            if succ[a] is not None or prev[b] >= 0:
                continue
            if b not in best_a or (c, g, a) < best_a[b]:
                best_a[b] = (c, g, a)
            if a not in best_b or (c, b) < best_b[a]:
                best_b[a] = (c, b)
        commits = [(k[2], b) for b, k in best_a.items() if best_b[k[2]][1] == b]
        if not commits:
            return n
        for a, b in commits:
            succ[a], prev[b] = b, a


def _run(frames_per_sequence, history_frames, pose_counts, keypoints, closed, radius_permille, min_shared, max_gap, by_rounds):
    fps, hist, pc, kp, shut, off = _layout(frames_per_sequence, history_frames, pose_counts, keypoints, closed)
    succ = [True if c else None for c in shut]          # None: open
    prev = [-1] * len(kp)
    links, rounds, first = [0] * len(pc), 0, 0
    for n, h in zip(fps, hist):
        for t in range(first + h, first + n):
            pairs = frame_pairs(kp, off, t, first, max_gap, radius_permille, min_shared)
            if by_rounds:
                rounds = max(rounds, _rounds(pairs, succ, prev))
            else:
                _greedy(pairs, succ, prev)
            links[t] = sum(1 for b in range(off[t], off[t + 1]) if prev[b] >= 0)
        first += n
    root = list(range(len(kp)))
    for r in range(len(kp)):                            # a predecessor lies in an earlier row
        if prev[r] >= 0:
            root[r] = root[prev[r]]
    out = (np.array(prev, np.int32).reshape(-1), np.array(root, np.int32).reshape(-1), np.array(links, np.int32).reshape(-1))
    return out + (rounds,) if by_rounds else out


def track_model(frames_per_sequence, history_frames, pose_counts, keypoints, closed=None, radius_permille=100, min_shared=3, max_gap=0):
    """The rule: -> (prev (P,), root (P,), links (n_frames,)) int32."""
    return _run(frames_per_sequence, history_frames, pose_counts, keypoints, closed, radius_permille, min_shared, max_gap, False)


def track_rounds_model(frames_per_sequence, history_frames, pose_counts, keypoints, closed=None, radius_permille=100, min_shared=3, max_gap=0):
    """The same answer by mutual-best rounds -> (prev, root, links, the largest number of rounds a frame ran)."""
    return _run(frames_per_sequence, history_frames, pose_counts, keypoints, closed, radius_permille, min_shared, max_gap, True)


# ---- frames ------------------------------------------------------------------------------------------------------------
def pose_row(js):
    """{joint index: (x, y)} -> one (18, 3) int32 row with those joints present."""
    r = np.zeros((18, 3), np.int32)
    for j, (x, y) in js.items():
        r[j] = (x, y, 1)
    return r


def walkers(rng, n, frames, step=3, extent=600, body=40, present=0.8):
    """A crowd that moves: n people on an extent x extent canvas, each a fixed shape of 18 joints within `body` pixels of its
    centre; every frame the centre moves up to `step` pixels on each axis, every joint jitters by a pixel, is present with
    probability `present` (absent joints hold random coordinates that must be ignored), and the rows are shuffled.
    -> (list of (n, 18, 3) int32 arrays, list of (n,) arrays: the person each row is)."""
    centre = rng.integers(body, extent - body, (n, 1, 2))
    shape = rng.integers(-body // 2, body // 2 + 1, (n, 18, 2))
    out, who = [], []
    for _ in range(frames):
        kp = np.zeros((n, 18, 3), np.int32)
        kp[:, :, :2] = centre + shape + rng.integers(-1, 2, (n, 18, 2))
        kp[:, :, 2] = rng.random((n, 18)) < present
        gone = kp[:, :, 2] == 0
        kp[:, :, :2][gone] = rng.integers(0, extent, (int(gone.sum()), 2))
        order = rng.permutation(n)
        out.append(kp[order])
        who.append(order)
        centre = centre + rng.integers(-step, step + 1, (n, 1, 2))
    return out, who


def drop(poses, frame, k):
    """The same frames with the first k rows of `frame` taken out: people who were not found there."""
    return [p[k:] if f == frame else p for f, p in enumerate(poses)]


def call_of(frames):
    """A list of (n, 18, 3) arrays (or of lists of rows) -> (pose_counts, keypoints)."""
    frames = [np.asarray(f, np.int32).reshape(-1, 18, 3) for f in frames]
    return np.array([len(f) for f in frames], np.int32), (np.concatenate(frames) if frames else np.zeros((0, 18, 3), np.int32))
