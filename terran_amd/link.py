"""Whose face is this body's?  Faces and skeletons of the same frames, linked one to one on the GPU.

    faces, poses = face_detection(frames), pose_estimation(frames)
    gallery.identify(faces, extract_features(frames, faces))
    link_faces_poses(faces, poses)          # face['pose'] = k, pose['face'] = k; the skeleton inherits 'text', 'track', 'cluster'

The detector, `FaceGallery.identify`, `face_tracking` and `cluster_faces` all write into face dicts; the skeletons of
`Estimation` / `TiledEstimation` carry none of it.  `link_faces_poses` joins the two sides with one `ta_faces_poses_link` call
(include/terran_amd.h states the rule: head joints inside the widened face box, cheapest pairs first, all in integers), so
"what is Ada doing?" is a lookup.  `head_boxes` turns skeletons into face-like boxes on the host: the people whose face the
detector missed can still be blurred, cropped or measured.
"""
from math import isqrt

import numpy as np

HEAD = (0, 14, 15, 16, 17)              # nose, right eye, left eye, right ear, left ear (vis.py)
NOSE, NECK = 0, 1


def _per_frame(faces, poses):
    """-> (faces per frame, poses per frame) as lists of lists; the single-image form (one list of dicts each) is one frame."""
    faces, poses = list(faces), list(poses)
    nested = lambda seq: any(isinstance(v, (list, tuple)) for v in seq)
    if nested(faces) or nested(poses):
        if not (all(isinstance(v, (list, tuple)) for v in faces) and all(isinstance(v, (list, tuple)) for v in poses)):
            raise ValueError('faces and poses must both be one list of dicts, or both one list of dicts per frame')
        if len(faces) != len(poses):
            raise ValueError('%d frames of faces for %d frames of poses' % (len(faces), len(poses)))
        return [list(v) for v in faces], [list(v) for v in poses]
    return [faces], [poses]


def _permille(margin):
    return int(round(float(margin) * 1000))


def link_faces_poses(faces, poses, margin=0.25, min_inside=1, inherit=('text', 'track', 'cluster'), ctx=None, device=None):
    """Link every face to the skeleton it belongs to.  faces / poses: what `face_detection` and `pose_estimation` (or the tiled
    classes, `face_tracking`, the triples of `StreamPipeline.run`) return for the same frames -- a list of lists of dicts per
    frame, or one image's list of dicts each.

    A skeleton qualifies for a face when at least `min_inside` of its present head joints (nose, eyes, ears), and at least
    half of them, lie in the face's bbox widened by `margin` of its size on every side; pairs link cheapest first by the mean
    squared distance of the head joints to the box centre, each face and each skeleton at most once (ta_faces_poses_link).
    A linked face gets face['pose'] = k, the index into its frame's pose list, and that skeleton pose['face'] = k'; the others
    keep no such key (one left by an earlier call is removed).  For every key of `inherit` that the linked face carries and
    the skeleton does not, the skeleton receives the face's value: names from `identify`, ids from `face_tracking`, clusters.
    Returns the per-frame int32 pose_of_face arrays (-1: not linked); for the single-image form, that one array."""
    if isinstance(device, (list, tuple)):
        raise ValueError('`device`: link_faces_poses does not offer fan-out over a device list yet; pass one device')
    single = not any(isinstance(v, (list, tuple)) for v in list(faces) + list(poses))
    fpf, ppf = _per_frame(faces, poses)
    fc = np.array([len(v) for v in fpf], np.int32)
    pc = np.array([len(v) for v in ppf], np.int32)
    boxes = np.array([np.asarray(f['bbox']).reshape(4) for v in fpf for f in v], np.int32).reshape(-1, 4)
    kp = np.array([np.asarray(p['keypoints']).reshape(18, 3) for v in ppf for p in v], np.int32).reshape(-1, 18, 3)
    if ctx is None:
        from . import runtime
        ctx = runtime.get_context(device)
    pof, fop, _, _ = ctx.faces_poses_link(fc, boxes, pc, kp, _permille(margin), int(min_inside))
    out, f0, p0 = [], 0, 0
    for fl, pl in zip(fpf, ppf):
        mine = np.array(pof[f0:f0 + len(fl)], np.int32)
        for face, p in zip(fl, mine):
            if p >= 0:
                face['pose'] = int(p)
            else:
                face.pop('pose', None)
        for pose, f in zip(pl, fop[p0:p0 + len(pl)]):
            if f >= 0:
                pose['face'] = int(f)
                for key in inherit:
                    if key in fl[f] and key not in pose:
                        pose[key] = fl[f][key]
            else:
                pose.pop('face', None)
        out.append(mine)
        f0, p0 = f0 + len(fl), p0 + len(pl)
    return out[0] if single else out


def head_box(keypoints, margin_permille=250):
    """One skeleton's head as a box, in integers: int32 (x0, y0, x1, y1), or None.  bx0 .. by1 are the extent of the present
    head joints; q = isqrt(dx^2 + dy^2) between nose and neck when both are present (a head seen from behind or in profile has
    joints close together, the neck gives its size), else 0; side = max(bx1 - bx0, by1 - by0, q); no present head joint, or
    side == 0, gives no box; m = side * margin_permille // 1000; x0 = (bx0 + bx1 - side) // 2 - m,
    x1 = (bx0 + bx1 + side + 1) // 2 + m, the same for y; // is floor division."""
    k = np.asarray(keypoints).reshape(18, 3)
    pts = [(int(k[j][0]), int(k[j][1])) for j in HEAD if int(k[j][2]) != 0]
    if not pts:
        return None
    bx0, bx1 = min(p[0] for p in pts), max(p[0] for p in pts)
    by0, by1 = min(p[1] for p in pts), max(p[1] for p in pts)
    q = 0
    if int(k[NOSE][2]) != 0 and int(k[NECK][2]) != 0:
        dx, dy = int(k[NOSE][0]) - int(k[NECK][0]), int(k[NOSE][1]) - int(k[NECK][1])
        q = isqrt(dx * dx + dy * dy)
    side = max(bx1 - bx0, by1 - by0, q)
    if side == 0:
        return None
    m = side * int(margin_permille) // 1000
    return np.array([(bx0 + bx1 - side) // 2 - m, (by0 + by1 - side) // 2 - m,
                     (bx0 + bx1 + side + 1) // 2 + m, (by0 + by1 + side + 1) // 2 + m], np.int32)


def head_boxes(poses, margin=0.25, only_unlinked=False):
    """Skeletons -> face-like dicts, host only: per frame a list of {'bbox': int32 (4,), 'pose': k} that `blur_faces`,
    `crop_faces` and `face_stats` accept as faces (`head_box` states the rule).  `only_unlinked` skips the skeletons that carry
    a 'face' key: after `link_faces_poses`, what is left are the people whose face the detector missed.  poses: a list of
    lists of dicts per frame, or one image's list of dicts (which gives one list)."""
    poses = list(poses)
    single = not any(isinstance(v, (list, tuple)) for v in poses)
    permille = _permille(margin)
    out = []
    for pl in ([poses] if single else poses):
        boxes = []
        for k, pose in enumerate(pl):
            if only_unlinked and 'face' in pose:
                continue
            b = head_box(pose['keypoints'], permille)
            if b is not None:
                boxes.append({'bbox': b, 'pose': k})
        out.append(boxes)
    return out[0] if single else out
