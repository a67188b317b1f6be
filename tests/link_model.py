"""The model of the face-to-skeleton link (no GPU import): what ta_faces_poses_link must answer, bit for bit.

`link_model` restates what include/terran_amd.h says of ta_faces_poses_link, literally and for clarity, not for speed: every
qualifying pair of a frame, sorted by (cost, f, p), walked once.  `link_rounds_model` is an independent second statement: the
mutual-best rounds the device runs, which also gives the round count the call reports.  Both work on Python ints, so no width
or rounding of any number format enters.  The generators below build the frames the CPU and the GPU tests share.
"""
import numpy as np

HEAD = (0, 14, 15, 16, 17)          # nose, right eye, left eye, right ear, left ear (terran_amd/vis.py)
COORD_LIMIT = 1 << 22
MAX_PER_FRAME = 16384


def _arrays(face_counts, boxes, pose_counts, keypoints):
    fc = np.asarray(face_counts, np.int64).reshape(-1)
    pc = np.asarray(pose_counts, np.int64).reshape(-1)
    boxes = np.asarray(boxes, np.int64).reshape(-1, 4)
    kp = np.asarray(keypoints, np.int64).reshape(-1, 18, 3)
    assert len(fc) == len(pc) and fc.sum() == len(boxes) and pc.sum() == len(kp)
    return fc, boxes, pc, kp


def head_joints(kp_row):
    """The present head joints of one (18, 3) row as a list of (x, y) Python ints."""
    return [(int(kp_row[j][0]), int(kp_row[j][1])) for j in HEAD if int(kp_row[j][2]) != 0]


def pair(box, joints, margin_permille, min_inside):
    """One face box against one pose's present head joints -> the pair's cost (a Python int), or None if it does not qualify."""
    x0, y0, x1, y1 = (int(v) for v in box)
    n = len(joints)
    w, h = x1 - x0, y1 - y0
    if n == 0 or w < 0 or h < 0:
        return None
    mx, my = (w * margin_permille) // 1000, (h * margin_permille) // 1000      # w, h >= 0: floor is truncation
    inside = sum(1 for x, y in joints if x0 - mx <= x <= x1 + mx and y0 - my <= y <= y1 + my)
    if inside < min_inside or 2 * inside < n:
        return None
    cx, cy = x0 + x1, y0 + y1
    s = sum((2 * x - cx) ** 2 + (2 * y - cy) ** 2 for x, y in joints)
    return s * (60 // n)


def frame_pairs(boxes, kp, margin_permille, min_inside):
    """Every qualifying pair of one frame as (cost, f, p)."""
    joints = [head_joints(r) for r in kp]
    out = []
    # a numpy prefilter on "some present head joint inside the widened box" keeps the explicit loop to the pairs that can qualify
    if len(boxes) == 0 or len(kp) == 0:
        return out
    b = np.asarray(boxes, np.int64)
    w, h = b[:, 2] - b[:, 0], b[:, 3] - b[:, 1]
    mx, my = np.where(w >= 0, w, 0) * margin_permille // 1000, np.where(h >= 0, h, 0) * margin_permille // 1000
    k = np.asarray(kp, np.int64)[:, HEAD, :]
    for f in range(len(b)):
        if w[f] < 0 or h[f] < 0:
            continue
        near = ((k[:, :, 2] != 0) & (k[:, :, 0] >= b[f, 0] - mx[f]) & (k[:, :, 0] <= b[f, 2] + mx[f]) &
                (k[:, :, 1] >= b[f, 1] - my[f]) & (k[:, :, 1] <= b[f, 3] + my[f])).any(1)
        for p in np.nonzero(near)[0]:
            c = pair(b[f], joints[p], margin_permille, min_inside)
            if c is not None:
                out.append((c, f, int(p)))
    return out


def _greedy(nf, npose, pairs):
    pof, fop = [-1] * nf, [-1] * npose
    for _, f, p in sorted(pairs):
        if pof[f] < 0 and fop[p] < 0:
            pof[f], fop[p] = p, f
    return pof, fop


def _rounds(nf, npose, pairs):
    """Mutual-best rounds -> (pose_of_face, face_of_pose, rounds run: the committing rounds and the silent one that ends them)."""
    pof, fop = [-1] * nf, [-1] * npose
    rounds = 0
    while True:
        rounds += 1
        best_p, best_f = {}, {}
        for c, f, p in pairs:
            if pof[f] >= 0 or fop[p] >= 0:
                continue
            if f not in best_p or (c, p) < best_p[f]:
                best_p[f] = (c, p)
            if p not in best_f or (c, f) < best_f[p]:
                best_f[p] = (c, f)
        commits = [(f, cp[1]) for f, cp in best_p.items() if best_f[cp[1]][1] == f]
        if not commits:
            return pof, fop, rounds
        for f, p in commits:
            pof[f], fop[p] = p, f


def _run(face_counts, boxes, pose_counts, keypoints, margin_permille, min_inside, by_rounds):
    fc, boxes, pc, kp = _arrays(face_counts, boxes, pose_counts, keypoints)
    pof, fop, links, rounds = [], [], [], 0
    f0 = p0 = 0
    for nf, npose in zip(fc, pc):
        nf, npose = int(nf), int(npose)
        pairs = frame_pairs(boxes[f0:f0 + nf], kp[p0:p0 + npose], margin_permille, min_inside)
        if by_rounds:
            a, b, r = _rounds(nf, npose, pairs)
            rounds = max(rounds, r)
        else:
            a, b = _greedy(nf, npose, pairs)
        pof += a
        fop += b
        links.append(sum(1 for v in a if v >= 0))
        f0, p0 = f0 + nf, p0 + npose
    out = (np.array(pof, np.int32).reshape(-1), np.array(fop, np.int32).reshape(-1), np.array(links, np.int32).reshape(-1))
    return out + (rounds,) if by_rounds else out


def link_model(face_counts, boxes, pose_counts, keypoints, margin_permille=250, min_inside=1):
    """The rule: -> (pose_of_face (F,), face_of_pose (P,), links (n_frames,)) int32."""
    return _run(face_counts, boxes, pose_counts, keypoints, margin_permille, min_inside, False)


def link_rounds_model(face_counts, boxes, pose_counts, keypoints, margin_permille=250, min_inside=1):
    """The same answer by mutual-best rounds -> (pose_of_face, face_of_pose, links, rounds): rounds is the largest number any
    frame ran, each frame running its committing rounds and the silent one after them; 0 for no frames."""
    return _run(face_counts, boxes, pose_counts, keypoints, margin_permille, min_inside, True)


def qualifying_per_face(face_counts, boxes, pose_counts, keypoints, margin_permille=250, min_inside=1):
    """How many poses each face qualifies with, (F,) int64."""
    fc, boxes, pc, kp = _arrays(face_counts, boxes, pose_counts, keypoints)
    out = np.zeros(len(boxes), np.int64)
    f0 = p0 = 0
    for nf, npose in zip(fc, pc):
        for _, f, _p in frame_pairs(boxes[f0:f0 + nf], kp[p0:p0 + npose], margin_permille, min_inside):
            out[f0 + f] += 1
        f0, p0 = f0 + int(nf), p0 + int(npose)
    return out


# ---- frames ------------------------------------------------------------------------------------------------------------
def pose_row(joints):
    """{joint index: (x, y)} -> one (18, 3) int32 row with those joints present."""
    r = np.zeros((18, 3), np.int32)
    for j, (x, y) in joints.items():
        r[j] = (x, y, 1)
    return r


def chain(length, x_at=0, y_at=0):
    """The worst case of the rounds -> (boxes (L, 4), keypoints (L, 18, 3)), to be linked with margin_permille = 0.

    Box centres C_i and single-nose skeletons N_i alternate on a horizontal line, C_0 N_0 C_1 N_1 ..., and the gaps between
    neighbours fall by one pixel a step: g_0 > g_1 > ...  Box i reaches exactly as far as its left neighbour N_(i-1) (box 0: as
    far as N_0), so it holds N_(i-1) and N_i and no other nose (the next ones are about three gaps away).  With one present joint
    the cost is 240 x the squared distance to the centre, so the costs fall along f0 p0 f1 p1 ...: every face but the last prefers
    the pose on its right, every pose the face on its right, and only the last pair is mutually best.  Committing it frees the
    pair before it: `length` committing rounds and one silent round, and f_i links p_i."""
    boxes, kp = np.zeros((length, 4), np.int32), np.zeros((length, 18, 3), np.int32)
    gap = lambda k: 2 * length + 50 - k                     # k = 0 .. 2 length - 2; the smallest is 52
    at = x_at
    for i in range(length):
        half = gap(2 * i - 1) if i else gap(0)
        boxes[i] = (at - half, y_at, at + half, y_at + 10)
        at += gap(2 * i)
        kp[i, 0] = (at, y_at + 5, 1)
        if i + 1 < length:
            at += gap(2 * i + 1)
    return boxes, kp


def crowd(rng, n_faces, n_poses, extent=256, box=(40, 80), spread=12):
    """One random frame on an extent x extent canvas -> (boxes (n_faces, 4), keypoints (n_poses, 18, 3)) int32.  Heads are five
    joints scattered `spread` pixels around a random centre, each present with probability 0.7 (a body joint or two are set as
    well and must not matter); absent joints hold random coordinates that must be ignored.  Boxes are `box` pixels on a side,
    large against the canvas so that most faces see several heads."""
    lo, hi = box
    x0, y0 = rng.integers(0, extent - lo, n_faces), rng.integers(0, extent - lo, n_faces)
    w, h = rng.integers(lo, hi + 1, n_faces), rng.integers(lo, hi + 1, n_faces)
    boxes = np.stack([x0, y0, x0 + w, y0 + h], 1).astype(np.int32).reshape(n_faces, 4)
    kp = np.zeros((n_poses, 18, 3), np.int32)
    c = rng.integers(0, extent, (n_poses, 1, 2))
    kp[:, :, :2] = c + rng.integers(-spread, spread + 1, (n_poses, 18, 2))
    kp[:, :, 2] = rng.random((n_poses, 18)) < 0.7
    kp[:, 1:14, :2] += rng.integers(20, 60, (n_poses, 13, 2))       # the body hangs below the head
    return boxes, kp


CROWD_FACES = (0, 1, 63, 64, 65, 127, 129, 300)
CROWD_SEED = 3


def crowd_call(seed=CROWD_SEED, faces=CROWD_FACES):
    """The crowd call of the tests: 8 frames, face counts `faces`, pose counts the same list reversed ->
    (face_counts, boxes, pose_counts, keypoints)."""
    rng = np.random.default_rng(seed)
    fc, pc = np.array(faces, np.int32), np.array(faces[::-1], np.int32)
    parts = [crowd(rng, int(a), int(b)) for a, b in zip(fc, pc)]
    return fc, np.concatenate([p[0] for p in parts]), pc, np.concatenate([p[1] for p in parts])


def reorder(face_counts, boxes, pose_counts, keypoints, order):
    """The same frames in another order."""
    fo, po = np.concatenate([[0], np.cumsum(face_counts)]), np.concatenate([[0], np.cumsum(pose_counts)])
    return (np.asarray(face_counts)[order], np.concatenate([boxes[fo[k]:fo[k + 1]] for k in order]),
            np.asarray(pose_counts)[order], np.concatenate([keypoints[po[k]:po[k + 1]] for k in order]))
