"""The model of tiled pose estimation's merge (no GPU import): what ta_poses_merge must answer, bit for bit.

`merge_model` restates section by section what include/terran_amd.h says of ta_poses_merge, written for clarity and not for
speed: explicit loops, Python ints (which cannot overflow) for every integer, Python floats (IEEE doubles) for the three
multiplies the definition allows.  Nothing here looks at the kernel.
"""
import numpy as np

GROUP_FIELDS = ('frame', 'first', 'count', 'ox', 'oy', 'x0', 'y0', 'x1', 'y1', 'interior')
LIMIT = 1 << 22


def group(frame, first, count, ox=0, oy=0, rect=(0, 0, 0, 0), interior=0):
    """One group as a dict (what merge_model takes; a lib.POSE_GROUP_DT record works as well)."""
    return dict(frame=frame, first=first, count=count, ox=ox, oy=oy, x0=rect[0], y0=rect[1], x1=rect[2], y1=rect[3], interior=interior)


def records(groups):
    """A list of such dicts -> the lib.POSE_GROUP_DT array (imports the binding: only the GPU tests call this)."""
    from terran_amd import lib
    out = np.zeros(len(groups), lib.POSE_GROUP_DT)
    for i, g in enumerate(groups):
        for k in GROUP_FIELDS:
            out[i][k] = g[k]
    return out


class Candidate:
    """One candidate after the map: its row, group, mapped joints, presence mask, np, extent and s2."""

    def __init__(self, row, gi, g, kp):
        self.row, self.group = row, gi
        ox, oy = int(g['ox']), int(g['oy'])
        self.joints, self.mask = [], 0
        for j in range(18):
            x, y, p = (int(v) for v in kp[j])
            assert abs(x) < LIMIT and abs(y) < LIMIT, 'a coordinate at or above 2^22'
            if p != 0:
                self.joints.append((x + ox, y + oy, p))
                self.mask |= 1 << j
            else:
                self.joints.append((0, 0, 0))
        self.np = bin(self.mask).count('1')
        if self.np:
            xs = [q[0] for q in self.joints if q[2] != 0]
            ys = [q[1] for q in self.joints if q[2] != 0]
            self.bx0, self.bx1, self.by0, self.by1 = min(xs), max(xs), min(ys), max(ys)
            self.s2 = (self.bx1 - self.bx0 + 1) * (self.by1 - self.by0 + 1)

    def cut(self, g, edge):
        inner = int(g['interior'])
        return bool((inner & 1 and self.bx0 < int(g['x0']) + edge) or (inner & 2 and self.by0 < int(g['y0']) + edge) or
                    (inner & 4 and self.bx1 >= int(g['x1']) - edge) or (inner & 8 and self.by1 >= int(g['y1']) - edge))


def duplicates(a, b, r2, agree, min_shared, shortcut=True):
    """The pair relation of the header, in its operation order.  `shortcut` (tests/test_pose_tiles_cpu.py holds the two settings
    together): extents that lie `gap` > 0 pixels apart along an axis, gap * gap > limit, hold no joint pair within the limit --
    each end of a pair lies in its candidate's extent -- so matched = 0, which is below agree * shared > 0."""
    if a.group == b.group:
        return False
    limit = r2 * float(max(a.s2, b.s2))                      # one double multiply
    if shortcut:
        gap = max(a.bx0 - b.bx1, b.bx0 - a.bx1, a.by0 - b.by1, b.by0 - a.by1)
        if gap > 0 and float(gap * gap) > limit:
            return False
    both = a.mask & b.mask
    shared = bin(both).count('1')
    if shared < min_shared:
        return False
    matched = 0
    for j in range(18):
        if (both >> j) & 1:
            dx, dy = a.joints[j][0] - b.joints[j][0], a.joints[j][1] - b.joints[j][1]
            if float(dx * dx + dy * dy) <= limit:               # an exact integer below 2^49
                matched += 1
    return float(matched) >= agree * float(shared)           # one double multiply


def merge_model(groups, n_frames, keypoints, scores, radius=0.1, agree=0.5, min_shared=3, edge=0, stats=None):
    """-> (counts (n_frames,) int32, keypoints (T, 18, 3) int32, scores (T,) float64, source (T,) int32).  `stats`: a dict that
    receives 'candidates' (rows in a group), 'empty' (no present joint), 'cut' (dropped by the edge rule) and 'suppressed'."""
    keypoints = np.asarray(keypoints, np.int32).reshape(-1, 18, 3)
    scores = np.asarray(scores, np.float64).reshape(-1)
    radius, agree, min_shared, edge = float(radius), float(agree), int(min_shared), int(edge)
    r2 = radius * radius                                     # once
    per_frame = [[] for _ in range(n_frames)]
    seen, n_cand, n_empty, n_cut = set(), 0, 0, 0
    for gi, g in enumerate(groups):
        assert abs(int(g['ox'])) < LIMIT and abs(int(g['oy'])) < LIMIT
        for row in range(int(g['first']), int(g['first']) + int(g['count'])):
            assert row not in seen, 'a row in two groups'
            seen.add(row)
            n_cand += 1
            c = Candidate(row, gi, g, keypoints[row])
            if c.np == 0:
                n_empty += 1
            elif edge > 0 and c.cut(g, edge):
                n_cut += 1
            else:
                per_frame[int(g['frame'])].append(c)
    counts, kept_all = np.zeros(n_frames, np.int32), []
    for f in range(n_frames):
        # descending np, descending score (-0.0 == 0.0 for Python floats), ascending row
        order = sorted(per_frame[f], key=lambda c: (-c.np, -float(scores[c.row]), c.row))
        kept = []
        for c in order:
            if not any(duplicates(k, c, r2, agree, min_shared) for k in kept):
                kept.append(c)
        counts[f] = len(kept)
        kept_all += kept
    if stats is not None:
        stats.update(candidates=n_cand, empty=n_empty, cut=n_cut, suppressed=n_cand - n_empty - n_cut - len(kept_all))
    src = np.array([c.row for c in kept_all], np.int32)
    kp = np.array([c.joints for c in kept_all], np.int32).reshape(-1, 18, 3)
    return counts, kp, scores[src], src


# ---- synthetic candidates ----------------------------------------------------------------------------------------------------------
SCORES = (0.5, 0.75, 1.0, 1.5, 2.25, -0.0, 0.0)


def clustered_poses(rng, n, extent, exact=False):
    """n skeletons in clusters of 1 to 4 near-duplicates, as overlapping tiles produce them: a person of 20 .. 120 by 40 .. 300
    pixels somewhere in `extent` x `extent`, every copy with its own random missing joints (now and then all of them) and a jitter
    per joint that straddles 0.1 x the square root of the person's extent; scores from a handful of values, so that ties are
    common.  exact: a quarter of the copies are exact copies, score included.  -> (keypoints (n, 18, 3) int32, scores (n,)
    float64) in random order, in the coordinates of the frame: `split` deals them out to groups."""
    kps, scs = [], []
    while len(kps) < n:
        k = min(int(rng.integers(1, 5)), n - len(kps))
        w, h = int(rng.integers(20, 121)), int(rng.integers(40, 301))
        x0, y0 = int(rng.integers(0, max(1, extent - w))), int(rng.integers(0, max(1, extent - h)))
        base = np.stack([rng.integers(x0, x0 + w, 18), rng.integers(y0, y0 + h, 18), np.ones(18, np.int64)], axis=1)
        reach = 0.1 * np.sqrt(w * h)
        first = None
        for _ in range(k):
            if exact and first is not None and rng.random() < 0.25:
                kps.append(first[0].copy()), scs.append(first[1])
                continue
            kp = base.copy()
            kp[:, :2] += np.rint(rng.uniform(-1.2, 1.2, (18, 2)) * reach * rng.choice([0.3, 1.0])).astype(np.int64)
            drop = rng.random(18) < rng.choice([0.0, 0.2, 0.6, 1.0], p=[0.3, 0.4, 0.25, 0.05])
            kp[drop] = 0
            sc = float(rng.choice(SCORES))
            kps.append(kp), scs.append(sc)
            if first is None:
                first = (kp, sc)
    p = rng.permutation(n)
    return np.array(kps, np.int32).reshape(-1, 18, 3)[p], np.array(scs, np.float64)[p]


def split(rng, frame, first, keypoints, extent, pieces=3):
    """Deal the rows of one frame (frame coordinates) out to up to `pieces` groups of consecutive rows, each with its own origin
    (subtracted from its rows' present joints, so that the map brings them back) and interior bits -> the groups; `keypoints` is
    changed in place.  The copies of a cluster land in different groups or in one as the permutation has it."""
    n = len(keypoints)
    cuts = sorted(rng.integers(0, n + 1, pieces - 1).tolist()) if n > pieces else [n] * (pieces - 1)
    groups, lo = [], 0
    for k, hi in enumerate(cuts + [n]):
        if hi - lo or k == 0:
            ox, oy = int(rng.integers(-50, 500)), int(rng.integers(-50, 500))
            there = keypoints[lo:hi, :, 2] != 0
            keypoints[lo:hi, :, 0][there] -= ox
            keypoints[lo:hi, :, 1][there] -= oy
            rect = (int(rng.integers(0, extent // 4)), int(rng.integers(0, extent // 4)), int(rng.integers(3 * extent // 4, extent)),
                    int(rng.integers(3 * extent // 4, extent)))
            groups.append(group(frame, first + lo, hi - lo, ox, oy, rect, int(rng.integers(0, 16))))
        lo = hi
    return groups


# ---- boundary cases with hand-derived answers (tests/test_pose_tiles_cpu.py: the model; tests/test_gpu_pose_tiles.py: the device) ----
def pose(joints):
    """{joint: (x, y)} -> (18, 3) int32 with present = 1 at those joints."""
    kp = np.zeros((18, 3), np.int32)
    for j, (x, y) in joints.items():
        kp[j] = (x, y, 1)
    return kp


def two_groups(poses, scores, params, source, same_group=False):
    """poses[0] in group 0, the others in group 1 (same_group: all in group 0) of one frame -> a case."""
    groups = [group(0, 0, len(poses))] if same_group else [group(0, 0, 1), group(0, 1, len(poses) - 1)]
    return groups, 1, np.stack(poses), np.array(scores, np.float64), params, source


def boundary_cases():
    """{name: (groups, n_frames, keypoints, scores, (radius, agree, min_shared, edge), the kept rows in output order)}"""
    cases = {}
    # radius 0.5, both extents 20 x 20: s2 = 400, r2 * S = 100.  One shared joint (2), agree 1: (dx, dy) = (6, 8) is 100, (6, 9) is 117
    a = pose({0: (0, 0), 1: (19, 19), 2: (5, 5)})
    for name, y, src in (('radius_on', 13, [0]), ('radius_off', 14, [0, 1])):
        b = pose({2: (11, y), 4: (20, 20), 5: (1, 1)})
        cases[name] = two_groups([a, b], [0.9, 0.8], (0.5, 1.0, 1, 0), src)
    # extents 101 x 101, radius 0.1: r2 * S = 102.01, a joint 50 pixels off does not match.  Four shared joints, agree 0.5
    a = pose({0: (0, 0), 1: (100, 0), 2: (0, 100), 3: (100, 100)})
    cases['agree_2_of_4'] = two_groups([a, pose({0: (0, 0), 1: (100, 0), 2: (50, 100), 3: (50, 100)})], [0.9, 0.8], (0.1, 0.5, 3, 0), [0])
    cases['agree_1_of_4'] = two_groups([a, pose({0: (0, 0), 1: (50, 0), 2: (50, 100), 3: (50, 100)})], [0.9, 0.8],
                                       (0.1, 0.5, 3, 0), [0, 1])
    # identical shared joints, one fewer than min_shared / exactly min_shared
    for ms in (1, 3, 18):
        full = {j: (10 * j, 7 * j) for j in range(18)}
        few = {j: full[j] for j in range(ms - 1)}
        if ms < 18:
            cases['min_shared_%d_meets' % ms] = two_groups([pose(full), pose({j: full[j] for j in range(ms)})], [0.5, 0.5], (0.1, 0.5, ms, 0), [0])
        if ms > 1:
            cases['min_shared_%d_short' % ms] = two_groups([pose(full), pose(few)], [0.5, 0.5], (0.1, 0.5, ms, 0), [0, 1])
    cases['min_shared_18_meets'] = two_groups([pose(full), pose(full)], [0.5, 0.5], (0.1, 0.5, 18, 0), [0])
    # two identical poses: one group keeps both, two groups keep the first
    cases['same_group'] = two_groups([a, a], [0.9, 0.8], (0.1, 0.5, 3, 0), [0, 1], same_group=True)
    cases['other_group'] = two_groups([a, a], [0.9, 0.8], (0.1, 0.5, 3, 0), [0])
    # np before score: row 1 has 17 joints and 0.1, row 0 five of them and 0.9
    full = {j: (10 * j, 7 * j) for j in range(17)}
    cases['order_np_first'] = two_groups([pose({j: full[j] for j in range(5)}), pose(full)], [0.9, 0.1], (0.1, 0.5, 3, 0), [1])
    # equal np, equal score (-0 == +0): the lower row
    cases['tie_lower_row'] = two_groups([a, a, a], [0.5, 0.5, 0.5], (0.1, 0.5, 3, 0), [0])
    cases['tie_signed_zero'] = two_groups([a, a], [-0.0, 0.0], (0.1, 0.5, 3, 0), [0])
    cases['score_before_row'] = two_groups([a, a], [0.25, 0.5], (0.1, 0.5, 3, 0), [1])
    # the edge rule, frame f = side f of the rectangle (100, 100, 200, 200), edge 10.  Rows 3 f, 3 f + 1: a pose on the limit and one a
    # pixel further in a group whose side f is interior; row 3 f + 2: the dropped one again in a group where only that side is not.
    # radius 0, agree 1: only a pose equal to a kept one would be its duplicate, and the one it equals was dropped
    rect, groups, poses, source = (100, 100, 200, 200), [], [], []
    for f, (axis, on, off, dropped) in enumerate(((0, 110, 109, 1), (1, 110, 109, 1), (0, 190, 189, 0), (1, 190, 189, 0))):
        inward = 1 if f < 2 else -1
        def at(v):
            pts = {0: (v, 150), 1: (v + 20 * inward, 160), 2: (v + 10 * inward, 140)}
            return pose(pts if axis == 0 else {j: (y, x) for j, (x, y) in pts.items()})
        groups += [group(f, 3 * f, 2, rect=rect, interior=1 << f), group(f, 3 * f + 2, 1, rect=rect, interior=15 - (1 << f))]
        poses += [at(on), at(off), at((on, off)[dropped])]
        source += [3 * f + 1 - dropped, 3 * f + 2]
    scores = np.linspace(0.9, 0.1, 12)
    cases['edge_per_side'] = (groups, 4, np.stack(poses), scores, (0.0, 1.0, 1, 10), source)
    cases['edge_zero_drops_nothing'] = (groups, 4, np.stack(poses), scores, (0.0, 1.0, 1, 0), [0, 1, 3, 4, 6, 7, 9, 10])
    return cases
