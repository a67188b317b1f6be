"""The contract of ta_poses_paint (include/terran_amd.h) restated on the host (no GPU): `paint` in numpy int64, and a second,
deliberately different formulation of the covered test for tiny frames -- Python ints pixel by pixel, the squared distance
from a pixel to a segment as the exact fraction (p.p L2 - t^2) / L2 compared as a `Fraction` -- plus the same test in floating
point, the wrong arithmetic a kernel could fall into."""
from fractions import Fraction

import numpy as np

HEAD, TORSO, LIMB = 0, 1, 2
JOINT_CLASS = (HEAD, TORSO, TORSO, LIMB, LIMB, TORSO, LIMB, LIMB, TORSO, LIMB, LIMB, TORSO, LIMB, LIMB, HEAD, HEAD, HEAD, HEAD)
# (a, b, class): the 17 connections of vis.POSE_CONNECTIONS in its order, then (8, 11)
SEGMENTS = ((0, 1, HEAD), (0, 14, HEAD), (14, 16, HEAD), (0, 15, HEAD), (15, 17, HEAD),
            (1, 2, TORSO), (2, 3, LIMB), (3, 4, LIMB), (1, 8, TORSO), (8, 9, LIMB), (9, 10, LIMB),
            (1, 5, TORSO), (5, 6, LIMB), (6, 7, LIMB), (1, 11, TORSO), (11, 12, LIMB), (12, 13, LIMB), (8, 11, TORSO))
DEFAULT_PERMILLE = (90, 90, 50)


def pose_row(joints):
    """{joint: (x, y)} -> (18, 3) int32, the joints named present."""
    row = np.zeros((18, 3), np.int32)
    for j, (x, y) in joints.items():
        row[j] = (x, y, 1)
    return row


def size_of(row):
    """M of a (18, 3) row, or None without a present joint."""
    at = np.asarray(row, np.int64)
    at = at[at[:, 2] != 0]
    if not len(at):
        return None
    return int(max(at[:, 0].max() - at[:, 0].min(), at[:, 1].max() - at[:, 1].min()))


def radii(row, radius_permille=DEFAULT_PERMILLE, min_radius=2):
    """(r_head, r_torso, r_limb) of a row, or None without a present joint: Python ints, a truncating division."""
    m = size_of(row)
    if m is None:
        return None
    return tuple(max(int(min_radius), m * int(p) // 1000) for p in radius_permille)      # m, p >= 0: // truncates


def shapes_of(row, radius_permille=DEFAULT_PERMILLE, min_radius=2):
    """[(ax, ay, bx, by, r)] of a row: a disc (A == B) per present joint, a capsule per segment with both ends present."""
    r = radii(row, radius_permille, min_radius)
    if r is None:
        return []
    q = [[int(v) for v in j] for j in np.asarray(row)]
    out = [(q[j][0], q[j][1], q[j][0], q[j][1], r[JOINT_CLASS[j]]) for j in range(18) if q[j][2] != 0]
    out += [(q[a][0], q[a][1], q[b][0], q[b][1], r[c]) for a, b, c in SEGMENTS if q[a][2] != 0 and q[b][2] != 0]
    return out


def covered(px, py, ax, ay, bx, by, r):
    """The header's test on int64 arrays px, py (broadcast) -> bool array."""
    px, py = np.asarray(px, np.int64), np.asarray(py, np.int64)
    dx, dy = np.int64(bx - ax), np.int64(by - ay)
    L2, r2 = dx * dx + dy * dy, np.int64(r) * np.int64(r)
    qx, qy = px - np.int64(ax), py - np.int64(ay)
    t = qx * dx + qy * dy
    ex, ey = px - np.int64(bx), py - np.int64(by)
    cross = qx * dy - qy * dx
    return np.where(t <= 0, qx * qx + qy * qy <= r2, np.where(t >= L2, ex * ex + ey * ey <= r2, cross * cross <= r2 * L2))


def covered_fraction(px, py, ax, ay, bx, by, r):
    """The other formulation, one pixel, Python ints: the squared distance to the segment, exactly, against r^2."""
    dx, dy, qx, qy = bx - ax, by - ay, px - ax, py - ay
    L2, t = dx * dx + dy * dy, qx * dx + qy * dy
    if L2 == 0 or t <= 0:
        d2 = Fraction(qx * qx + qy * qy)
    elif t >= L2:
        d2 = Fraction((px - bx) ** 2 + (py - by) ** 2)
    else:
        d2 = Fraction((qx * qx + qy * qy) * L2 - t * t, L2)      # |p|^2 - (p.d)^2 / |d|^2
    return d2 <= Fraction(r * r)


def covered_float(px, py, ax, ay, bx, by, r, dtype=np.float64):
    """The header's test with every value and product in `dtype`: the wrong one."""
    f = dtype
    px, py = np.asarray(px).astype(f), np.asarray(py).astype(f)
    dx, dy = f(bx) - f(ax), f(by) - f(ay)
    L2, r2 = dx * dx + dy * dy, f(r) * f(r)
    qx, qy = px - f(ax), py - f(ay)
    t = qx * dx + qy * dy
    ex, ey = px - f(bx), py - f(by)
    cross = qx * dy - qy * dx
    return np.where(t <= 0, qx * qx + qy * qy <= r2, np.where(t >= L2, ex * ex + ey * ey <= r2, cross * cross <= r2 * L2))


def shape_coverage(shape, h, w):
    """bool (h, w) of one shape, evaluated inside its box only."""
    ax, ay, bx, by, r = shape
    out = np.zeros((h, w), bool)
    x0, x1 = max(min(ax, bx) - r, 0), min(max(ax, bx) + r, w - 1)
    y0, y1 = max(min(ay, by) - r, 0), min(max(ay, by) + r, h - 1)
    if x0 <= x1 and y0 <= y1:
        out[y0:y1 + 1, x0:x1 + 1] = covered(np.arange(x0, x1 + 1)[None, :], np.arange(y0, y1 + 1)[:, None], ax, ay, bx, by, r)
    return out


def pose_coverage(row, h, w, radius_permille=DEFAULT_PERMILLE, min_radius=2):
    """bool (h, w): the pixels the pose covers, the OR of its shapes."""
    out = np.zeros((h, w), bool)
    for s in shapes_of(row, radius_permille, min_radius):
        out |= shape_coverage(s, h, w)
    return out


def blend(px, ink, a):
    """draw.hip's blend of uint8 samples (..., 3) with the ink (3,) under alpha a."""
    v = px.astype(np.int64) * (255 - int(a)) + np.asarray(ink, np.int64) * int(a) + 128
    return (((v >> 8) + v) >> 8).astype(np.uint8)


def paint(frames, pose_counts, keypoints, rgba, radius_permille=DEFAULT_PERMILLE, min_radius=2, clear=False):
    """ta_poses_paint on host frames (N, H, W, 3) uint8, in place; returns `frames`."""
    counts = np.asarray(pose_counts, np.int64).reshape(-1)
    kp = np.asarray(keypoints, np.int64).reshape(-1, 18, 3)
    rgba = np.asarray(rgba, np.int64).reshape(-1, 4)
    assert counts.sum() == len(kp) == len(rgba) and len(counts) <= len(frames)
    h, w = frames.shape[1:3]
    at = 0
    for f, n in enumerate(counts):
        if clear:
            frames[f] = 0
        for k in range(at, at + int(n)):
            cov = pose_coverage(kp[k], h, w, radius_permille, min_radius)
            frames[f][cov] = blend(frames[f][cov], rgba[k, :3], rgba[k, 3])
        at += int(n)
    return frames


def masks(shape, pose_counts, keypoints, radius_permille=DEFAULT_PERMILLE, min_radius=2):
    """vis.pose_masks: a new (N, H, W, 3) batch, 255 where a pose is."""
    out = np.zeros(tuple(shape[:3]) + (3,), np.uint8)
    kp = np.asarray(keypoints).reshape(-1, 18, 3)
    return paint(out, pose_counts, kp, np.full((len(kp), 4), 255, np.uint8), radius_permille, min_radius, True)


def boxes(pose_counts, keypoints, h, w, radius_permille=DEFAULT_PERMILLE, min_radius=2):
    """[(frame, pose in its frame, x0, y0, x1, y1)]: vis.pose_boxes' half-open boxes, from the header's words: the extent of
    the present joints widened by the largest of the three radii, clipped to the frame, empty ones left out."""
    out, at = [], 0
    kp = np.asarray(keypoints, np.int64).reshape(-1, 18, 3)
    for f, n in enumerate(np.asarray(pose_counts).reshape(-1)):
        for i in range(int(n)):
            r = radii(kp[at + i], radius_permille, min_radius)
            if r is None:
                continue
            q = kp[at + i][kp[at + i][:, 2] != 0]
            x0, y0 = max(int(q[:, 0].min()) - max(r), 0), max(int(q[:, 1].min()) - max(r), 0)
            x1, y1 = min(int(q[:, 0].max()) + max(r) + 1, w), min(int(q[:, 1].max()) + max(r) + 1, h)
            if x1 > x0 and y1 > y0:
                out.append((f, i, x0, y0, x1, y1))
        at += int(n)
    return out


def person(rng, cx, cy, size, absent=0.0):
    """A plausible standing skeleton about `size` tall around (cx, cy) -> (18, 3) int32; each joint absent with the given
    probability (an absent joint keeps garbage coordinates)."""
    s = size / 8.0
    proto = {0: (0, -3.3), 1: (0, -2.5), 2: (-0.9, -2.5), 3: (-1.2, -1.2), 4: (-1.3, 0), 5: (0.9, -2.5), 6: (1.2, -1.2), 7: (1.3, 0),
             8: (-0.5, 0), 9: (-0.6, 2), 10: (-0.6, 4), 11: (0.5, 0), 12: (0.6, 2), 13: (0.6, 4), 14: (-0.2, -3.5), 15: (0.2, -3.5),
             16: (-0.4, -3.4), 17: (0.4, -3.4)}
    row = np.zeros((18, 3), np.int32)
    for j, (x, y) in proto.items():
        row[j] = (int(cx + x * s + rng.integers(-2, 3)), int(cy + y * s + rng.integers(-2, 3)), 1)
    gone = rng.random(18) < absent
    row[gone, 2] = 0
    row[gone, :2] = rng.integers(-16000, 16000, (int(gone.sum()), 2))
    return row
