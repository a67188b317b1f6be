"""The model of track filling (no GPU import): what ta_tracks_fill must answer, bit for bit.

`fill_model` restates what include/terran_amd.h says of ta_tracks_fill, literally and for clarity, not for speed: chains as lists
of rows, every output row looking along its chain for the nearest rows that have the point.  It works on Python ints, so no
width or rounding of any number format enters; every condition the library refuses is a ValueError here.  `prev_of_ids` is the
function the public calls use (terran_amd/tracking.py) and `ModelContext` stands in for a context in them, so their host halves
run without a device.  The builders below make the clips the CPU and the GPU tests share.
"""
import numpy as np

from terran_amd.tracking import prev_of_ids      # noqa: F401  (numpy only)

COORD_LIMIT = 1 << 22
MAX_PER_FRAME = 16384


def interpolate(v0, v1, k, dt):
    """v0 + floor((2 (v1 - v0) k + dt) / (2 dt)) on Python ints, whose // is the floor division."""
    return v0 + (2 * (v1 - v0) * k + dt) // (2 * dt)


def fill_model(counts, points, prev, max_gap=5, mark=2):
    """-> (out_counts (n_frames,) int32, out_points (n_out, n_points, 3) int32, out_source (n_out, 2) int32)."""
    counts = [int(v) for v in np.asarray(counts).reshape(-1)]
    points = np.asarray(points)
    prev = [int(v) for v in np.asarray(prev).reshape(-1)]
    if points.ndim != 3 or points.shape[2] != 3:
        raise ValueError('points must be (rows, n_points, 3)')
    n_rows, n_points = points.shape[0], points.shape[1]
    if not 1 <= n_points <= 18:
        raise ValueError('n_points outside 1 .. 18')
    if not 0 <= max_gap <= 30:
        raise ValueError('max_gap outside 0 .. 30')
    if not 1 <= mark <= 255:
        raise ValueError('mark outside 1 .. 255')
    if any(c < 0 for c in counts):
        raise ValueError('a negative count')
    if sum(counts) != n_rows or len(prev) != n_rows:
        raise ValueError('the counts do not sum to the rows')
    if any(c > MAX_PER_FRAME for c in counts):
        raise ValueError('overflow: more than %d input rows in one frame' % MAX_PER_FRAME)
    pts = [[(int(x), int(y), int(p)) for x, y, p in row] for row in points.tolist()]
    if any(abs(x) >= COORD_LIMIT or abs(y) >= COORD_LIMIT for row in pts for x, y, _ in row):
        raise ValueError('a coordinate at or above 2^22 in size')
    frame = [f for f, c in enumerate(counts) for _ in range(c)]
    first_row = [sum(counts[:f]) for f in range(len(counts) + 1)]
    nxt = [-1] * n_rows
    for b, a in enumerate(prev):
        if a == -1:
            continue
        if a < 0 or a >= n_rows or frame[a] >= frame[b]:
            raise ValueError('prev[%d] = %d is neither -1 nor a row of an earlier frame' % (b, a))
        if nxt[a] != -1:
            raise ValueError('two rows with the same prev %d' % a)
        nxt[a] = b
    G = max_gap + 1

    def before(row, t, j):
        """The nearest row of the chain at or behind `row` that has point j (all of them lie in frames before t), or None."""
        while row != -1:
            if pts[row][j][2] != 0:
                return row
            row = prev[row]
        return None

    def after(row, j):
        while row != -1:
            if pts[row][j][2] != 0:
                return row
            row = nxt[row]
        return None

    def filled(r0, r1, t, j):
        if r0 is None or r1 is None:
            return (0, 0, 0)
        t0, t1 = frame[r0], frame[r1]
        if t1 - t0 > G:
            return (0, 0, 0)
        return (interpolate(pts[r0][j][0], pts[r1][j][0], t - t0, t1 - t0), interpolate(pts[r0][j][1], pts[r1][j][1], t - t0, t1 - t0), mark)

    out_counts, out_points, out_source = [], [], []
    for t, c in enumerate(counts):
        rows = 0
        for r in range(first_row[t], first_row[t + 1]):             # the real rows, in input order
            row = []
            for j in range(n_points):
                if pts[r][j][2] != 0:
                    row.append(pts[r][j])
                else:
                    row.append(filled(before(prev[r], t, j), after(nxt[r], j), t, j))
            out_points.append(row)
            out_source.append((r, r))
            rows += 1
        for b in range(n_rows):                         # the links that span t and add rows, by b ascending
            a = prev[b]
            if a == -1 or not frame[a] < t < frame[b] or frame[b] - frame[a] > G:
                continue
            out_points.append([filled(before(a, t, j), after(b, j), t, j) for j in range(n_points)])
            out_source.append((a, b))
            rows += 1
        if rows > MAX_PER_FRAME:
            raise ValueError('overflow: more than %d output rows in one frame' % MAX_PER_FRAME)
        out_counts.append(rows)
    return (np.array(out_counts, np.int32).reshape(-1), np.array(out_points, np.int32).reshape(-1, n_points, 3),
            np.array(out_source, np.int32).reshape(-1, 2))


class ModelContext:
    """What the public calls need of a context, answered by the model."""

    def tracks_fill(self, counts, points, prev, max_gap=5, mark=2):
        return fill_model(counts, points, prev, max_gap, mark)


# ---- builders ---------------------------------------------------------------------------------------------------------------------
def call_of(frames, n_points):
    """[rows of frame 0 (k, n_points, 3), ...] -> (counts, points)."""
    counts = np.array([len(f) for f in frames], np.int32)
    parts = [np.asarray(f, np.int32).reshape(-1, n_points, 3) for f in frames]
    return counts, (np.concatenate(parts) if parts else np.zeros((0, n_points, 3), np.int32))


def one_point_track(observations, n_frames=None):
    """{frame: (x, y) or None (the row is there, its point absent)} -> (counts, points, prev) of one track with one point."""
    n_frames = max(observations) + 1 if n_frames is None else n_frames
    counts, rows, prev = np.zeros(n_frames, np.int32), [], []
    for t in sorted(observations):
        o = observations[t]
        counts[t] = 1
        prev.append(len(rows) - 1)
        rows.append([[0, 0, 0]] if o is None else [[o[0], o[1], 1]])
    return counts, np.array(rows, np.int32).reshape(-1, 1, 3), np.array(prev, np.int32)


def seam_clip(tracks, n_points):
    """3 frames x `tracks` tracks whose middle frame is empty: every track gains its row there."""
    rng = np.random.default_rng(tracks)
    a = rng.integers(-500, 500, (tracks, n_points, 3)).astype(np.int32)
    b = a + rng.integers(-9, 10, a.shape).astype(np.int32)
    a[:, :, 2] = 1
    b[:, :, 2] = rng.integers(0, 2, (tracks, n_points)) * 3         # some points absent at the far end, the third value free
    order = rng.permutation(tracks)                                 # the rows of the last frame in another order than their tracks
    prev = np.concatenate([np.full(tracks, -1), order]).astype(np.int32)
    return np.array([tracks, 0, tracks], np.int32), np.concatenate([a, b[order]]), prev


def seeded_clip(seed, n_frames=32, tracks=40, n_points=18, row_drop=0.15, point_drop=0.15, extreme=False):
    """`tracks` random walks over `n_frames` frames, rows and points dropped at random, rows shuffled within a frame -> (counts,
    points, prev); prev links every row to the track's last row before it, whatever the distance.  `extreme`: the walks keep to
    the two ends of the coordinate range, +-(2^22 - 1), which rows of both signs reach."""
    rng = np.random.default_rng(seed)
    per = int(rng.integers(max(1, tracks // 2), tracks + 1))
    if extreme:
        top = COORD_LIMIT - 1
        pos = np.where(rng.integers(0, 2, (per, n_points, 2)) == 1, top, -top).astype(np.int64)
    else:
        pos = rng.integers(-3000, 3000, (per, n_points, 2)).astype(np.int64)
    frames, last, prev, at = [], [-1] * per, [], 0
    for t in range(n_frames):
        if extreme:
            step = rng.integers(0, 2, pos.shape) * rng.integers(0, 2 * (COORD_LIMIT - 1) + 1, pos.shape)
            pos = np.clip(np.where(pos > 0, pos - step, pos + step), -(COORD_LIMIT - 1), COORD_LIMIT - 1)
        else:
            pos = pos + rng.integers(-7, 8, pos.shape)
        here = [k for k in rng.permutation(per).tolist() if rng.random() >= row_drop]
        rows = np.zeros((len(here), n_points, 3), np.int32)
        for i, k in enumerate(here):
            rows[i, :, :2] = pos[k]
            rows[i, :, 2] = rng.random(n_points) >= point_drop
            prev.append(last[k])
            last[k] = at + i
        frames.append(rows)
        at += len(here)
    counts, points = call_of(frames, n_points)
    return counts, points, np.array(prev, np.int32).reshape(-1)


def chain(frames_of_rows, rows):
    """One track: rows[i] (n_points, 3) lies alone in frame frames_of_rows[i] -> (counts, points, prev)."""
    counts = np.zeros(max(frames_of_rows) + 1, np.int32)
    counts[list(frames_of_rows)] = 1
    return counts, np.array(rows, np.int32), np.arange(-1, len(rows) - 1, dtype=np.int32)


def hand_cases():
    """The cases computed by hand: (name, (counts, points, prev), max_gap, mark, (out_counts, out_points, out_source) as lists)."""
    far = one_point_track({0: (0, 0), 3: (10, -10)})
    up, down = one_point_track({0: (0, 0), 2: (1, 1)}), one_point_track({0: (0, 0), 2: (-1, -1)})
    # five rows in five frames; point 1 is there at the ends only: (0, 0) and (8, 40), four frames apart
    five = chain(range(5), [[[5, 5, 1], [0, 0, 1]], [[5, 5, 1], [9, 9, 0]], [[5, 5, 1], [9, 9, 0]], [[5, 5, 1], [9, 9, 0]], [[5, 5, 1], [8, 40, 1]]])
    kept = [[5, 5, 1], [0, 0, 0]]
    # point 1 absent at both ends of a chain of three; point 0 absent in the middle, its third value free where present
    ends = chain(range(3), [[[0, 0, 7], [3, 3, 0]], [[8, 8, 0], [4, 4, 1]], [[4, 2, 9], [5, 5, 0]]])
    # frames 0, 4, 5 at max_gap 2: the link 0 -> 4 is too long for rows, and for point 1, absent at frame 4, across it
    long_ = chain((0, 4, 5), [[[0, 0, 1], [0, 0, 1]], [[8, 8, 1], [1, 1, 0]], [[9, 9, 1], [10, 10, 1]]])
    # two tracks miss frame 1 and stand in frame 2 in the other order: the synthesized rows follow b
    two = (np.array([2, 0, 2], np.int32), np.array([[[0, 0, 1]], [[100, 100, 1]], [[104, 100, 1]], [[0, 6, 1]]], np.int32),
           np.array([-1, -1, 1, 0], np.int32))
    return [
        ('frames 0 and 3', far, 2, 2, ([1, 1, 1, 1], [[[0, 0, 1]], [[3, -3, 2]], [[7, -7, 2]], [[10, -10, 1]]], [[0, 0], [0, 1], [0, 1], [1, 1]])),
        ('frames 0 and 3, max_gap 1', far, 1, 2, ([1, 0, 0, 1], [[[0, 0, 1]], [[10, -10, 1]]], [[0, 0], [1, 1]])),
        ('half up', up, 1, 200, ([1, 1, 1], [[[0, 0, 1]], [[1, 1, 200]], [[1, 1, 1]]], [[0, 0], [0, 1], [1, 1]])),
        ('half down', down, 1, 1, ([1, 1, 1], [[[0, 0, 1]], [[0, 0, 1]], [[-1, -1, 1]]], [[0, 0], [0, 1], [1, 1]])),
        ('joint gone for three rows, max_gap 3', five, 3, 2,
         ([1] * 5, [five[1][0].tolist(), [[5, 5, 1], [2, 10, 2]], [[5, 5, 1], [4, 20, 2]], [[5, 5, 1], [6, 30, 2]], five[1][4].tolist()],
          [[r, r] for r in range(5)])),
        ('joint gone for three rows, max_gap 2', five, 2, 2,
         ([1] * 5, [five[1][0].tolist(), kept, kept, kept, five[1][4].tolist()], [[r, r] for r in range(5)])),
        ('absent at the ends', ends, 5, 2,
         ([1] * 3, [[[0, 0, 7], [0, 0, 0]], [[2, 1, 2], [4, 4, 1]], [[4, 2, 9], [0, 0, 0]]], [[r, r] for r in range(3)])),
        ('a link too long', long_, 2, 2,
         ([1, 0, 0, 0, 1, 1], [long_[1][0].tolist(), [[8, 8, 1], [0, 0, 0]], long_[1][2].tolist()], [[r, r] for r in range(3)])),
        ('ordered by b', two, 5, 2,
         ([2, 2, 2], [[[0, 0, 1]], [[100, 100, 1]], [[102, 100, 2]], [[0, 3, 2]], [[104, 100, 1]], [[0, 6, 1]]],
          [[0, 0], [1, 1], [1, 2], [0, 3], [2, 2], [3, 3]])),
    ]
