"""SORT face tracking over `Detection` output (the reference's terran/tracking/face.py), host side.

Tracking is sequential per stream and tiny next to the networks (a 7-state constant-velocity Kalman filter per face,
one Hungarian assignment per frame), so it stays on the host like the reference's -- but laid out as struct-of-arrays
over all live tracks (states (T,7), covariances (T,7,7)) with the filter written for this model's F and H instead of
one `filterpy.KalmanFilter` object per face:

  F = I + shift(4)   : x <- x F',  P <- F P F' + Q   (every sum has at most two non-zero terms: order-independent)
  H = [I4 | 0]       : S = P[:4,:4] + R,  K = P[:, :4] S^-1,  Joseph-form covariance update

Contract kept from the reference (file:line = terran/tracking/face.py):
  * `Sort(max_age, min_hits, return_unmatched).update(faces)` returns the same face dicts with a 'track' key, matched
    tracks first (in track order), then new tracks; id policy of :389-404; pruning by `max_age` :409-411.
  * IoU matrix in float32 from float64 arithmetic, assignment on its negation, matches below 0.3 IoU split back into
    unmatched face + unmatched track (:229-266).  `scipy.optimize.linear_sum_assignment`, as the reference (:4).
  * track ids ascend across ALL Sort instances of the process (`KalmanTracker.count`, :114,149-150).
  * a track whose predicted box is not finite is dropped before association (:372-381).
Deviations (the reference code cannot run these paths): `FaceTracking.__call__` on a single image wraps it into a
batch (the reference indexes `frames[0]`, :459-461, which drops the image); `face_tracking()` builds `Sort` from the
resolved `max_age` / `min_hits` (the reference reads `video.framerate` unconditionally, :548-551, and so raises
without a video).
"""
import itertools

import numpy as np

_ids = itertools.count()

_R = np.diag([1.0, 1.0, 10.0, 10.0])                                  # :139
_P0 = np.diag([10.0] * 4 + [10000.0] * 3)                             # :140-141
_Q = np.diag([1.0, 1.0, 1.0, 1.0, 0.01, 0.01, 0.0001])                # :142-143
_I7 = np.eye(7)
_H = np.eye(4, 7)
_F = np.eye(7)
_F[0, 4] = _F[1, 5] = _F[2, 6] = 1.0                                  # :126-134
_FT = _F.T.copy()


def reset_track_ids(start=0):
    """Restart the process-wide id counter (tests / new video)."""
    global _ids
    _ids = itertools.count(start)


def boxes_to_state(bbox):
    """(n,4) corner boxes -> (n,4) [cx, cy, area, ratio] (:47-71); integer inputs divide as floats."""
    b = np.asarray(bbox)
    w, h = b[:, 2] - b[:, 0], b[:, 3] - b[:, 1]
    with np.errstate(all='ignore'):
        return np.stack([b[:, 0] + w / 2.0, b[:, 1] + h / 2.0, (w * h).astype(np.float64), w / h], axis=1)


def state_to_boxes(x):
    """(T,>=4) states -> (T,4) corner boxes (:74-95)."""
    with np.errstate(all='ignore'):
        w = np.sqrt(x[:, 2] * x[:, 3])
        h = x[:, 2] / w
    return np.stack([x[:, 0] - w / 2.0, x[:, 1] - h / 2.0, x[:, 0] + w / 2.0, x[:, 1] + h / 2.0], axis=1)


def iou_matrix(face_boxes, track_boxes):
    """float32 (n_faces, n_tracks) IoU, computed like :14-44 (face area in the faces' own dtype)."""
    f = np.asarray(face_boxes)
    t = np.asarray(track_boxes, dtype=np.float64)
    with np.errstate(all='ignore'):
        iw = np.maximum(0.0, np.minimum(f[:, None, 2], t[None, :, 2]) - np.maximum(f[:, None, 0], t[None, :, 0]))
        ih = np.maximum(0.0, np.minimum(f[:, None, 3], t[None, :, 3]) - np.maximum(f[:, None, 1], t[None, :, 1]))
        inter = iw * ih
        fa = (f[:, 2] - f[:, 0]) * (f[:, 3] - f[:, 1])
        ta = (t[:, 2] - t[:, 0]) * (t[:, 3] - t[:, 1])
        return (inter / (fa[:, None] + ta[None, :] - inter)).astype(np.float32)


def associate(face_boxes, track_boxes, iou_threshold=0.3):
    """-> matches (K,2) [face, track], unmatched face indices (reference order), unmatched track indices (:206-272)."""
    from scipy.optimize import linear_sum_assignment
    n_f, n_t = len(face_boxes), len(track_boxes)
    if n_t == 0:
        return np.empty((0, 2), dtype=int), list(range(n_f)), []
    m = iou_matrix(face_boxes, track_boxes) if n_f else np.zeros((0, n_t), np.float32)
    rows, cols = linear_sum_assignment(-m)
    unmatched_f = sorted(set(range(n_f)) - set(rows.tolist()))
    unmatched_t = sorted(set(range(n_t)) - set(cols.tolist()))
    matches = []
    for fi, ti in zip(rows.tolist(), cols.tolist()):
        if m[fi, ti] < iou_threshold:
            unmatched_f.append(fi)
            unmatched_t.append(ti)
        else:
            matches.append((fi, ti))
    return np.array(matches, dtype=int).reshape(-1, 2), unmatched_f, unmatched_t


class Sort:
    """Appearance-agnostic tracking-by-detection (:275-411): attaches an identity to each detection or filters it."""

    def __init__(self, max_age=1, min_hits=3, return_unmatched=False):
        self.max_age, self.min_hits, self.return_unmatched = max_age, min_hits, return_unmatched
        self.frame_count = 0
        self.x = np.zeros((0, 7))
        self.P = np.zeros((0, 7, 7))
        self.hits = np.zeros(0, np.int64)
        self.time_since_update = np.zeros(0, np.int64)
        self.ids = np.zeros(0, np.int64)

    def __len__(self):
        return len(self.ids)

    def _keep(self, mask):
        self.x, self.P = self.x[mask], self.P[mask]
        self.hits, self.time_since_update, self.ids = self.hits[mask], self.time_since_update[mask], self.ids[mask]

    def _predict(self):
        x, P = self.x, self.P
        with np.errstate(all='ignore'):
            x[(x[:, 6] + x[:, 2]) <= 0, 6] = 0.0                                      # :196-197
            x = x @ _FT                                                                # keeps 0*inf -> nan of F.x
            P = _F @ P @ _FT + _Q
        self.x, self.P = x, P
        self.time_since_update += 1
        return state_to_boxes(x)

    def _correct(self, rows, z):
        """Kalman update of tracks `rows` with measurements z (k,4)."""
        x, P = self.x[rows], self.P[rows]
        y = z - x[:, :4]
        PHT = P[:, :, :4]
        S = P[:, :4, :4] + _R
        K = PHT @ np.linalg.inv(S)
        x = x + (K @ y[:, :, None])[:, :, 0]
        I_KH = _I7 - K @ _H
        P = I_KH @ P @ np.swapaxes(I_KH, 1, 2) + K @ _R @ np.swapaxes(K, 1, 2)
        self.x[rows], self.P[rows] = x, P
        self.time_since_update[rows] = 0
        self.hits[rows] += 1

    def update(self, faces):
        """Call once per frame (also with no faces).  Returns the face dicts with 'track' (:333-411)."""
        self.frame_count += 1
        boxes = self._predict() if len(self) else np.zeros((0, 4))
        ok = np.isfinite(boxes).all(axis=1)
        if not ok.all():
            self._keep(ok)
            boxes = boxes[ok]
        face_boxes = np.stack([np.asarray(f['bbox']) for f in faces]) if len(faces) else np.zeros((0, 4))
        matches, unmatched_f, _ = associate(face_boxes, boxes)
        out = []
        if len(matches):
            order = np.argsort(matches[:, 1], kind='stable')                           # matched tracks in track order
            matches = matches[order]
            with np.errstate(all='ignore'):
                self._correct(matches[:, 1], boxes_to_state(face_boxes[matches[:, 0]]))
            for fi, ti in matches.tolist():
                confirmed = self.hits[ti] >= self.min_hits or self.frame_count <= self.min_hits
                out.append({'track': int(self.ids[ti]) if confirmed else None, **faces[fi]})
        if unmatched_f:
            n = len(unmatched_f)
            x0 = np.zeros((n, 7))
            x0[:, :4] = boxes_to_state(face_boxes[unmatched_f])
            new_ids = np.array([next(_ids) for _ in range(n)], np.int64)
            self.x = np.concatenate([self.x, x0])
            self.P = np.concatenate([self.P, np.broadcast_to(_P0, (n, 7, 7))])
            self.hits = np.concatenate([self.hits, np.zeros(n, np.int64)])
            self.time_since_update = np.concatenate([self.time_since_update, np.zeros(n, np.int64)])
            self.ids = np.concatenate([self.ids, new_ids])
            for fi, tid in zip(unmatched_f, new_ids.tolist()):
                out.append({'track': tid if self.min_hits == 0 else None, **faces[fi]})
        if not self.return_unmatched:
            out = [f for f in out if f['track'] is not None]
        self._keep(self.time_since_update <= self.max_age)
        return out


class FaceTracking:
    """Drop-in for a `Detection` object that adds a 'track' field to every face (:414-473)."""

    def __init__(self, detector=None, tracker=None):
        self.detector = detector
        self.tracker = tracker

    def __call__(self, frames):
        single = not isinstance(frames, (list, tuple)) and getattr(frames, 'ndim', 4) == 3
        batch = [frames] if single else frames
        per_frame = [self.tracker.update(d) for d in self.detector(batch)]
        return per_frame[0] if single else per_frame


def face_tracking(*, video=None, max_age=None, min_hits=None, detector=None, return_unmatched=False):
    """Factory with the reference's defaults (:476-554): one second of frames for `max_age`, a fifth of a second for
    `min_hits` when a video (anything with `.framerate`) is given, else 30 / 6."""
    import terran_amd
    from . import facade
    max_age_, min_hits_ = 30, 6
    if video is not None:
        max_age_, min_hits_ = video.framerate, video.framerate // 5
    max_age = max_age_ if max_age is None else max_age
    min_hits = min_hits_ if min_hits is None else min_hits
    if detector is None:
        detector = terran_amd.face_detection
    elif not isinstance(detector, facade.Detection):
        raise ValueError('`detector` must be an instance of `terran.face.Detection`.')
    return FaceTracking(detector=detector, tracker=Sort(max_age=max_age, min_hits=min_hits,
                                                        return_unmatched=return_unmatched))


# ---- skeletons ---------------------------------------------------------------------------------------------------------------
# Not the reference's (it has no pose tracker): the rule of ta_poses_track (include/terran_amd.h), in integers and on the
# device; what stays on the host is the bookkeeping between calls.
_pose_ids = itertools.count()


def reset_pose_track_ids(start=0):
    """Restart the process-wide counter of skeleton track ids (tests / new video); the faces' counter is a separate one."""
    global _pose_ids
    _pose_ids = itertools.count(start)


class PoseTracker:
    """Follows the skeletons of one stream: `update(poses)` takes the next consecutive frames and writes pose['pose_track'].

    A skeleton continues the cheapest open skeleton of the `max_gap + 1` frames before it whose shared joints moved, in the
    mean square, at most (`radius` x the larger skeleton's size)^2 per frame of gap, with at least `min_shared` joints in common
    (ta_poses_track states the rule to the bit); one that continues nothing starts a track, ids ascending in row order over all
    trackers of the process.  The last `max_gap + 1` frames' keypoints, ids and successor flags are kept and prepended to the
    next call as history, so a clip tracked in one call and in batches of any size gets the same ids.  `carry`: a tracked
    skeleton that lacks one of these keys receives the value its track last carried -- the name that `identify` and
    `link_faces_poses` gave a body stays when the person turns away."""

    def __init__(self, max_gap=5, radius=0.1, min_shared=3, carry=('text', 'track', 'cluster'), ctx=None, device=None):
        if isinstance(device, (list, tuple)):
            raise ValueError('`device`: PoseTracker does not offer fan-out over a device list yet; pass one device')
        self.max_gap, self.min_shared, self.carry = int(max_gap), int(min_shared), tuple(carry)
        self.radius_permille = int(round(float(radius) * 1000))
        self.ctx, self.device = ctx, device
        self._history = []              # per kept frame: (keypoints (n, 18, 3) int32, ids (n,) int64, closed (n,) uint8)
        self._carried = {}              # id -> {key: the value the track last carried}

    def _context(self):
        if self.ctx is None:
            from . import runtime
            self.ctx = runtime.get_context(self.device)
        return self.ctx

    def update(self, poses):
        """poses: a list of lists of dicts, one per frame, or one frame's list of dicts -> the per-frame int64 id arrays (that
        one array for the single-frame form)."""
        poses = list(poses)
        nested = [isinstance(v, (list, tuple)) for v in poses]
        if any(nested) and not all(nested):
            raise ValueError('poses must be one list of dicts, or one list of dicts per frame')
        single = not any(nested)
        frames = [poses] if single else [list(v) for v in poses]
        hist = self._history
        new_kp = [np.array([np.asarray(p['keypoints']).reshape(18, 3) for p in v], np.int32).reshape(-1, 18, 3) for v in frames]
        kp = np.concatenate([h[0] for h in hist] + new_kp) if hist or new_kp else np.zeros((0, 18, 3), np.int32)
        counts = np.array([len(h[0]) for h in hist] + [len(v) for v in frames], np.int32)
        n_hist = int(counts[:len(hist)].sum())
        closed = np.concatenate([h[2] for h in hist] + [np.zeros(len(kp) - n_hist, np.uint8)])
        prev, root, _ = self._context().poses_track([len(counts)], [len(hist)], counts, kp, closed, self.radius_permille, self.min_shared,
                                                    self.max_gap)
        ids = np.concatenate([h[1] for h in hist] + [np.full(len(kp) - n_hist, -1, np.int64)])
        for row in range(n_hist, len(kp)):              # a root lies in an earlier row, or is the row itself
            r = int(root[row])
            ids[row] = next(_pose_ids) if r == row else ids[r]
        closed[prev[prev >= 0]] = 1
        out, at = [], n_hist
        for v in frames:
            mine = ids[at:at + len(v)].copy()
            for pose, k in zip(v, mine.tolist()):
                pose['pose_track'] = k
                kept = self._carried.setdefault(k, {})
                for key in self.carry:
                    if key in pose:
                        kept[key] = pose[key]
                    elif key in kept:
                        pose[key] = kept[key]
            out.append(mine)
            at += len(v)
        # what the next call can still link to: the last max_gap + 1 frames
        starts = np.concatenate([[0], np.cumsum(counts)])
        keep = range(max(0, len(counts) - (self.max_gap + 1)), len(counts))
        self._history = [(kp[starts[f]:starts[f + 1]].copy(), ids[starts[f]:starts[f + 1]].copy(), closed[starts[f]:starts[f + 1]].copy()) for f in keep]
        live = set(int(k) for h in self._history for k in h[1])
        self._carried = {k: v for k, v in self._carried.items() if k in live}     # an id that left the window never returns
        return out[0] if single else out


class PoseTracking:
    """Drop-in for an `Estimation` / `TiledEstimation` object that adds a 'pose_track' field to every skeleton."""

    def __init__(self, estimator=None, tracker=None):
        self.estimator = estimator
        self.tracker = tracker

    def __call__(self, frames):
        single = not isinstance(frames, (list, tuple)) and getattr(frames, 'ndim', 4) == 3
        batch = [frames] if single else frames
        per_frame = [list(v) for v in self.estimator(batch)]
        self.tracker.update(per_frame)
        return per_frame[0] if single else per_frame


def pose_tracking(*, video=None, max_gap=None, estimator=None, **rule):
    """Factory: a fifth of a second of frames for `max_gap` when a video (anything with `.framerate`) is given, else 5;
    `rule` goes to `PoseTracker` (radius, min_shared, carry, ctx, device)."""
    import terran_amd
    from . import facade
    if max_gap is None:
        max_gap = video.framerate // 5 if video is not None else 5
    if estimator is None:
        estimator = terran_amd.pose_estimation
    elif not isinstance(estimator, (facade.Estimation, facade.TiledEstimation)):
        raise ValueError('`estimator` must be an instance of `Estimation` or `TiledEstimation`.')
    return PoseTracking(estimator=estimator, tracker=PoseTracker(max_gap=max_gap, **rule))


# ---- tracks filled across missed frames and joints ----------------------------------------------------------------------------
# Not the reference's (its tracker "will not interpolate a face whenever there's a missing observation in between"): the rule of
# ta_tracks_fill (include/terran_amd.h), in integers and on the device; the host builds the links from the ids and the dicts
# from the answer.
def prev_of_ids(ids_per_frame):
    """Per frame a sequence of track ids -> prev (rows,) int32: for every row, frames concatenated, the global row that carried
    its id last, in whichever earlier frame, or -1.  An id that is None or negative joins no chain; the same id twice in one
    frame is a ValueError."""
    last, prev = {}, []
    for t, ids in enumerate(ids_per_frame):
        seen = set()
        for k in ids:
            k = None if k is None else int(k)
            if k is None or k < 0:
                prev.append(-1)
                continue
            if k in seen:
                raise ValueError('frame %d carries id %d twice: a track has one row a frame' % (t, k))
            seen.add(k)
            prev.append(last.get(k, -1))
            last[k] = len(prev) - 1                 # the row just appended
    return np.array(prev, np.int32).reshape(-1)


def _own(d):
    """A shallow copy of a result dict with its own arrays."""
    return {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in d.items()}


def _fill_tracks(who, per_frame, pack, n_points, unpack, max_gap, mark, key, carry, ctx, device):
    if isinstance(device, (list, tuple)):
        raise ValueError('`device`: %s does not offer fan-out over a device list yet; pass one device' % who)
    frames = [list(v) for v in per_frame]
    if any(not isinstance(d, dict) for v in frames for d in v):
        raise ValueError('%s takes one list of dicts per frame' % who)
    prev = prev_of_ids([[d.get(key) for d in v] for v in frames])
    rows = [d for v in frames for d in v]
    points = np.array([pack(d) for d in rows], np.int32).reshape(-1, n_points, 3)
    counts = np.array([len(v) for v in frames], np.int32)
    if ctx is None:
        from . import runtime
        ctx = runtime.get_context(device)
    out_counts, out_points, out_source = ctx.tracks_fill(counts, points, prev, int(max_gap), int(mark))
    out, at = [], 0
    for c in out_counts.tolist():
        mine = []
        for (a, b), p in zip(out_source[at:at + c].tolist(), out_points[at:at + c]):
            if a == b:
                d = _own(rows[a])
                unpack(d, p, True)
            else:
                d = {'filled': True, key: rows[b][key]}
                unpack(d, p, False)
                scores = [rows[r]['score'] for r in (a, b) if 'score' in rows[r]]
                if scores:
                    d['score'] = min(scores)
                for k in carry:
                    if k in rows[a]:
                        d[k] = rows[a][k]
            mine.append(d)
        out.append(mine)
        at += c
    return out


def fill_pose_tracks(poses_per_frame, max_gap=5, mark=2, key='pose_track', carry=('text', 'track', 'cluster'), ctx=None, device=None):
    """The skeletons of one clip, one list of dicts per consecutive frame with the track ids `PoseTracker` wrote under `key`, ->
    new per-frame lists in which a track that missed up to `max_gap` frames has a synthesized skeleton in each of them, behind
    the frame's own skeletons, and a joint that a track lost for up to `max_gap` frames is interpolated between the nearest
    frames that have it (ta_tracks_fill states the rule to the bit).  A filled joint carries `mark` as its third value, which
    `vis`, `link`, `paint` and the tracker take as present.  A synthesized dict carries 'filled': True, the id under `key`,
    the smaller 'score' of its two neighbours and the `carry` keys of its predecessor.  The input and its arrays are not
    modified: every returned dict is a shallow copy with its own arrays.  An id that is missing, None or negative joins no chain."""
    def pack(d):
        return np.asarray(d['keypoints']).reshape(18, 3)

    def unpack(d, p, real):
        d['keypoints'] = p.copy()

    return _fill_tracks('fill_pose_tracks', poses_per_frame, pack, 18, unpack, max_gap, mark, key, carry, ctx, device)


def pack_face(face):
    """A face dict -> its 7 points (7, 3) int32, all present: the two corners of 'bbox', then the five 'landmarks'; fractions
    are cut off as blur_faces cuts them."""
    p = np.ones((7, 3), np.int32)
    p[:2, :2] = np.asarray(face['bbox']).reshape(2, 2).astype(np.int32)
    p[2:, :2] = np.asarray(face['landmarks']).reshape(5, 2).astype(np.int32)
    return p


def unpack_face(points):
    """(7, 3) points -> ('bbox' int32 (4,), 'landmarks' int32 (5, 2))."""
    points = np.asarray(points, np.int32).reshape(7, 3)
    return points[:2, :2].reshape(4).copy(), points[2:, :2].copy()


def fill_face_tracks(faces_per_frame, max_gap=5, key='track', carry=('text', 'cluster', 'pose'), ctx=None, device=None):
    """`fill_pose_tracks` for faces with the ids `face_tracking` wrote under `key`: a face is its box's two corners and its five
    landmarks, 7 points that are all present, so only whole missed frames are filled; a synthesized face carries 'bbox' int32
    (4,) and 'landmarks' int32 (5, 2).  The faces a frame had are returned as they were."""
    def unpack(d, p, real):
        if not real:
            d['bbox'], d['landmarks'] = unpack_face(p)

    return _fill_tracks('fill_face_tracks', faces_per_frame, pack_face, 7, unpack, max_gap, 1, key, carry, ctx, device)
