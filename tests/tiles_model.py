"""The numpy model of tiled detection (no GPU import): where the tiles lie, and what ta_detections_merge must answer.

`tile_grid_model` is written without looking at terran_amd.tiles.tile_grid.  `merge_model` restates section by section what
include/terran_amd.h says of ta_detections_merge, every step an explicit float32 operation; for the IoU metric the NMS is
oracle.retinaface_post.nms itself on each frame's ordered boxes, so the merge is tied to the detector's own NMS.
`merge_brute` says the same once more with Python loops over pairs (tests/test_tiles_cpu.py holds the two together).
"""
import numpy as np

from oracle import retinaface_post as orp

F32 = np.float32
GROUP_FIELDS = ('frame', 'first', 'count', 'ox', 'oy', 'zoom', 'x0', 'y0', 'x1', 'y1', 'interior')


def group(frame, first, count, ox=0.0, oy=0.0, zoom=1.0, rect=(0, 0, 0, 0), interior=0):
    """One group as a dict (what merge_model takes; a lib.MERGE_GROUP_DT record works as well)."""
    return dict(frame=frame, first=first, count=count, ox=ox, oy=oy, zoom=zoom, x0=rect[0], y0=rect[1], x1=rect[2], y1=rect[3],
                interior=interior)


def records(groups):
    """A list of such dicts -> the lib.MERGE_GROUP_DT array (imports the binding: only the GPU tests call this)."""
    from terran_amd import lib
    out = np.zeros(len(groups), lib.MERGE_GROUP_DT)
    for i, g in enumerate(groups):
        for k in GROUP_FIELDS:
            out[i][k] = g[k]
    return out


# ---- the grid ----------------------------------------------------------------------------------------------------------------------
def axis_model(L, t, overlap):
    """Origins along an axis of length L: tiles of min(t, L), a step of t - overlap apart, the last one flush with the end."""
    t = min(t, L)
    if t == L:
        return [0]
    last = L - t
    step = t - overlap
    origins = list(range(0, last, step))          # every origin with origin + t < L
    origins.append(last)
    return origins


def overlap_model(side, overlap):
    return int(round(overlap * side)) if isinstance(overlap, float) else int(overlap)


def tile_grid_model(height, width, tile, overlap):
    th, tw = (tile, tile) if np.isscalar(tile) else tile
    oy, ox = (overlap, overlap) if np.isscalar(overlap) else overlap
    ys = axis_model(height, th, overlap_model(th, oy))
    xs = axis_model(width, tw, overlap_model(tw, ox))
    return np.array([[y, x] for y in ys for x in xs], np.int32).reshape(-1, 2)


# ---- the merge ---------------------------------------------------------------------------------------------------------------------
def map_and_cut(groups, boxes, landmarks, edge):
    """-> (frame of every candidate or -1 for a row in no group, mapped boxes, mapped landmarks, bool: dropped by the edge rule)."""
    boxes = np.asarray(boxes, F32).reshape(-1, 4)
    landmarks = np.asarray(landmarks, F32).reshape(-1, 5, 2)
    C = len(boxes)
    frame = np.full(C, -1, np.int64)
    mb, ml = boxes.copy(), landmarks.copy()
    dropped = np.zeros(C, bool)
    edge = F32(edge)
    for g in groups:
        lo, hi = int(g['first']), int(g['first']) + int(g['count'])
        assert (frame[lo:hi] == -1).all(), 'a row in two groups'
        frame[lo:hi] = int(g['frame'])
        zoom, o = F32(g['zoom']), np.array([g['ox'], g['oy']], F32)
        mb[lo:hi] = (boxes[lo:hi].reshape(-1, 2, 2) / zoom + o).reshape(-1, 4)      # float32 / float32, then float32 + float32
        ml[lo:hi] = landmarks[lo:hi] / zoom + o
        assert mb.dtype == F32 and ml.dtype == F32
        if edge > 0:
            x0, y0, x1, y1 = (F32(g[k]) for k in ('x0', 'y0', 'x1', 'y1'))
            b, inner, cut = mb[lo:hi], int(g['interior']), np.zeros(hi - lo, bool)
            if inner & 1:
                cut |= b[:, 0] < x0 + edge
            if inner & 2:
                cut |= b[:, 1] < y0 + edge
            if inner & 4:
                cut |= b[:, 2] > x1 - edge
            if inner & 8:
                cut |= b[:, 3] > y1 - edge
            dropped[lo:hi] = cut
    return frame, mb, ml, dropped


def nms_ios(boxes, thr):
    """oracle.retinaface_post.nms with intersection over the smaller box."""
    boxes = np.asarray(boxes, F32)
    n, thr = len(boxes), F32(thr)
    x1, y1, x2, y2 = boxes[:, 0], boxes[:, 1], boxes[:, 2], boxes[:, 3]
    areas = (x2 - x1) * (y2 - y1)
    suppressed, keep = np.zeros(n, bool), []
    for i in range(n):
        if suppressed[i]:
            continue
        keep.append(i)
        w = np.maximum(F32(0), np.minimum(x2[i], x2[i + 1:]) - np.maximum(x1[i], x1[i + 1:]))
        h = np.maximum(F32(0), np.minimum(y2[i], y2[i + 1:]) - np.maximum(y1[i], y1[i + 1:]))
        inter = w * h
        with np.errstate(divide='ignore', invalid='ignore'):
            ovr = inter / np.minimum(areas[i], areas[i + 1:])
        suppressed[i + 1:] |= ovr > thr
    return np.asarray(keep, np.int64)


def merge_model(groups, n_frames, boxes, landmarks, scores, nms_thr, metric=0, edge=0.0, stats=None):
    """-> (counts (n_frames,) int32, boxes, landmarks, scores float32, source int32).  `stats`: a dict that receives
    'candidates' (rows in a group), 'cut' (dropped by the edge rule) and 'suppressed' (removed by the NMS)."""
    scores = np.asarray(scores, F32).reshape(-1)
    frame, mb, ml, dropped = map_and_cut(groups, boxes, landmarks, edge)
    counts, src = np.zeros(n_frames, np.int32), []
    for f in range(n_frames):
        rows = np.nonzero((frame == f) & ~dropped)[0]                    # ascending rows
        rows = rows[np.argsort(-scores[rows], kind='stable')]              # descending score, ties by ascending row
        keep = orp.nms(mb[rows], nms_thr) if metric == 0 else nms_ios(mb[rows], nms_thr)
        counts[f] = len(keep)
        src.append(rows[keep])
    src = np.concatenate(src).astype(np.int32) if src else np.zeros(0, np.int32)
    if stats is not None:
        stats.update(candidates=int((frame >= 0).sum()), cut=int(dropped.sum()), suppressed=int((frame >= 0).sum() - dropped.sum() - len(src)))
    return counts, mb[src], ml[src], scores[src], src


def merge_brute(groups, n_frames, boxes, landmarks, scores, nms_thr, metric=0, edge=0.0):
    """The same answer by scalar loops: one candidate, one pair at a time."""
    boxes = np.asarray(boxes, F32).reshape(-1, 4)
    landmarks = np.asarray(landmarks, F32).reshape(-1, 5, 2)
    scores = np.asarray(scores, F32).reshape(-1)
    edge, thr = F32(edge), F32(nms_thr)
    cand = {f: [] for f in range(n_frames)}
    mb, ml = {}, {}
    for g in groups:
        zoom, ox, oy = F32(g['zoom']), F32(g['ox']), F32(g['oy'])
        for c in range(int(g['first']), int(g['first']) + int(g['count'])):
            b = boxes[c]
            m = [F32(b[0] / zoom) + ox, F32(b[1] / zoom) + oy, F32(b[2] / zoom) + ox, F32(b[3] / zoom) + oy]
            mb[c] = np.array(m, F32)
            ml[c] = np.array([[F32(p[0] / zoom) + ox, F32(p[1] / zoom) + oy] for p in landmarks[c]], F32)
            inner = int(g['interior'])
            if edge > 0 and ((inner & 1 and m[0] < F32(g['x0']) + edge) or (inner & 2 and m[1] < F32(g['y0']) + edge) or
                             (inner & 4 and m[2] > F32(g['x1']) - edge) or (inner & 8 and m[3] > F32(g['y1']) - edge)):
                continue
            cand[int(g['frame'])].append(c)
    counts, src = np.zeros(n_frames, np.int32), []
    for f in range(n_frames):
        order = sorted(cand[f], key=lambda c: (-float(scores[c]), c))
        gone = set()
        for k, i in enumerate(order):
            if i in gone:
                continue
            src.append(i)
            counts[f] += 1
            a = mb[i]
            area_a = F32(a[2] - a[0]) * F32(a[3] - a[1])
            for j in order[k + 1:]:
                b = mb[j]
                area_b = F32(b[2] - b[0]) * F32(b[3] - b[1])
                w = max(F32(0), F32(min(a[2], b[2]) - max(a[0], b[0])))
                h = max(F32(0), F32(min(a[3], b[3]) - max(a[1], b[1])))
                inter = F32(w * h)
                with np.errstate(divide='ignore', invalid='ignore'):
                    ovr = inter / F32(F32(area_a + area_b) - inter) if metric == 0 else inter / min(area_a, area_b)
                if ovr > thr:
                    gone.add(j)
    src = np.array(src, np.int32)
    if len(src) == 0:
        return counts, np.zeros((0, 4), F32), np.zeros((0, 5, 2), F32), np.zeros(0, F32), src
    return counts, np.stack([mb[c] for c in src]), np.stack([ml[c] for c in src]), scores[src], src


# ---- synthetic candidates ----------------------------------------------------------------------------------------------------------
def clustered_candidates(rng, n, extent=2000.0, exact=False):
    """n candidates in clusters of 1 to 4 near-duplicates (exact: exact duplicates with equal scores), as overlapping tiles
    produce them -> (boxes (n, 4), landmarks (n, 5, 2), scores (n,)) float32, in random order."""
    boxes, scores = [], []
    while len(boxes) < n:
        k = min(int(rng.integers(1, 5)), n - len(boxes))
        c, wh, s = rng.uniform(0, extent, 2), rng.uniform(12, 60, 2), rng.uniform(0.5, 1.0)
        for _ in range(k):
            j = np.zeros(4) if exact else rng.normal(0, 1.0, 4)
            boxes.append([c[0] - wh[0] / 2 + j[0], c[1] - wh[1] / 2 + j[1], c[0] + wh[0] / 2 + j[2], c[1] + wh[1] / 2 + j[3]])
            scores.append(s if exact else rng.uniform(0.5, 1.0))
    boxes, scores = np.array(boxes, F32).reshape(-1, 4), np.array(scores, F32)
    p = rng.permutation(len(boxes))
    boxes, scores = boxes[p], scores[p]
    lm = (boxes[:, None, :2] + rng.uniform(0, 1, (len(boxes), 5, 2)) * (boxes[:, None, 2:] - boxes[:, None, :2])).astype(F32)
    return boxes, lm, scores
