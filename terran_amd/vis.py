"""Drawing results into frames on the GPU: the reference's `terran.vis` (vis_faces / vis_poses, its Pillow path).

`vis_faces(image, faces, scale)` / `vis_poses(image, poses, scale)` keep the reference's signatures and return values: a
host uint8 (H, W, 3) image in, a new array with the markers drawn out.  `draw_faces` / `draw_poses` draw in place into a
resident `lib.Frames` batch (what `video.RawVideoReader` yields and `StreamPipeline.run(..., free_resident=False)` hands
back), one list of results per frame, so a video job never downloads a frame to draw on it.

The pixels are the reference's bit for bit (Pillow's ImageDraw.Draw(img, 'RGBA') rectangle outlines, lines and ellipses,
restated in csrc/draw.hip).  The colours follow the reference's tables; FACE_COLORMAP is, as there, module-global and
stateful: a label gets the next palette colour the first time it is seen, and a face without a label (no `name`, and
`track` absent or 0) a random one from Python's `random`.

Known difference: faces that carry `text` or `track` get their marker in the label's colour, but the label text itself is
not rendered (the reference's `draw_label` raises AttributeError on Pillow >= 10, so it renders none either).

Host glue only: the packing of results into primitives is vectorised numpy; the drawing is one ta_frames_draw launch.
Importing this module needs no GPU.
"""
import random

import numpy as np

from . import lib

# the default 10-colour categorical d3 palette
PALETTE = [tuple(int(h[i:i + 2], 16) for i in (0, 2, 4)) for h in
           ('1f77b4', 'ff7f0e', '2ca02c', 'd62728', '9467bd', '8c564b', 'e377c2', '7f7f7f', 'bcbd22', '17becf')]


def build_colormap():
    """label -> (r, g, b): a label takes the next palette colour the first time it is seen; None -> a random colour."""
    seen = {}

    def colormap(label=None):
        if label is None:
            return random.choice(PALETTE)
        if label not in seen:
            seen[label] = PALETTE[len(seen) % len(PALETTE)]
        return seen[label]

    return colormap


FACE_COLORMAP = build_colormap()


def _rgb(hexes):
    return np.array([[int(h[i:i + 2], 16) for i in (0, 2, 4)] for h in hexes.split()], np.uint8)


# OpenPose body parts (terran.pose.Keypoint): 0 nose, 1 neck, 2-4 right shoulder / elbow / hand, 5-7 left ...,
# 8-10 right hip / knee / foot, 11-13 left ..., 14 / 15 right / left eye, 16 / 17 right / left ear
POSE_CONNECTIONS = np.array([(0, 1), (0, 14), (14, 16), (0, 15), (15, 17),
                             (1, 2), (2, 3), (3, 4), (1, 8), (8, 9), (9, 10),
                             (1, 5), (5, 6), (6, 7), (1, 11), (11, 12), (12, 13)], np.int64)
POSE_CONNECTION_COLORS = _rgb('e6550d fd8d3c fdae6b 843c39 ad494a 637939 8ca252 b5cf6b 843c39 ad494a d6616b '
                              '3182bd 6baed6 9ecae1 8c6d31 bd9e39 e7ba52')
POSE_KEYPOINT_COLORS = _rgb('e6550d fd8d3c 637939 8ca252 b5cf6b 3182bd 6baed6 9ecae1 843c39 ad494a d6616b '
                            '8c6d31 bd9e39 e7ba52 fdae6b 843c39 ad494a d6616b')     # by keypoint index
MARKER_ALPHA, LIMB_ALPHA, KEYPOINT_ALPHA = 255, 180, 225
COORD_LIMIT = 1 << 24                                   # what ta_frames_draw accepts


def _as_list(x):
    return x if isinstance(x, (list, tuple)) else [x]


def _prims(n):
    return np.zeros(n, lib.PRIM_DT)


def _check_coords(a, what):
    if not np.all(np.abs(a) <= COORD_LIMIT):
        raise ValueError('%s coordinates must be finite and within +-2^24' % what)


def pack_faces(faces_per_frame, scale=1.0):
    """-> PRIM_DT array: each face's rectangle outline (Pillow draw.rectangle(bbox, outline=rgb + (255,), width=int(3 *
    scale))) as up to four opaque bars, faces in order, frame by frame.  Every box is checked first: an inverted one
    raises ValueError (as Pillow does) before anything is drawn."""
    boxes, colors, frame = [], [], []
    for f, faces in enumerate(faces_per_frame):
        for face in _as_list(faces):
            colors.append(FACE_COLORMAP(face.get('name') or face.get('track')))
            boxes.append(np.asarray(face['bbox'], np.float64).reshape(4))
            frame.append(f)
    if not boxes:
        return _prims(0)
    b = np.stack(boxes)
    if np.any(b[:, 2] < b[:, 0]):
        raise ValueError('x1 must be greater than or equal to x0')
    if np.any(b[:, 3] < b[:, 1]):
        raise ValueError('y1 must be greater than or equal to y0')
    _check_coords(b, 'box')
    w = int(3 * scale)
    if w <= 0:                                          # Pillow: rectangle(width=0) draws nothing
        return _prims(0)
    x0, y0, x1, y1 = np.trunc(b).astype(np.int64).T     # Pillow's (int) of the float coordinates
    # outline of width w: rows y0 .. y0+w-1 and y1-w+1 .. y1 across x0..x1, and the columns x0 .. x0+w-1, x1-w+1 .. x1
    # over the rows of Pillow's side lines from y0+w towards y1-w+1 (its end point excluded)
    ya, yb = y0 + w, y1 - w + 1
    s_lo = np.where(ya <= yb, ya, yb + 1)
    s_hi = np.where(ya <= yb, yb - 1, ya)
    m = len(b)
    out = _prims(4 * m)
    out['frame'] = np.repeat(frame, 4)
    out['kind'] = lib.DRAW_BAR
    out['x0'] = np.stack([x0, x0, x1 - w + 1, x0], 1).ravel()
    out['x1'] = np.stack([x1, x1, x1, x0 + w - 1], 1).ravel()
    out['y0'] = np.stack([y0, y1 - w + 1, s_lo, s_lo], 1).ravel()
    out['y1'] = np.stack([y0 + w - 1, y1, s_hi, s_hi], 1).ravel()
    out['rgba'][:, :3] = np.repeat(np.array(colors, np.uint8), 4, 0)
    out['rgba'][:, 3] = MARKER_ALPHA
    return out[(out['y1'] >= out['y0']) & (out['x1'] >= out['x0'])]


def _keypoints(poses_per_frame):
    """-> (P, 18, 3) float64 keypoints of every person, (P,) frame index."""
    kps, frame = [], []
    for f, poses in enumerate(poses_per_frame):
        for pose in _as_list(poses):
            kps.append(np.asarray(pose['keypoints'], np.float64).reshape(18, 3))
            frame.append(f)
    if not kps:
        return np.zeros((0, 18, 3)), np.zeros(0, np.int64)
    return np.stack(kps), np.asarray(frame, np.int64)


def pack_poses(poses_per_frame, scale=1.0):
    """-> PRIM_DT array: first every limb of every person (Pillow draw.line(..., fill=rgb + (180,), width=int(scale * 8)),
    the 17 connections in order, skipped when an end is missing), then every present keypoint (draw.ellipse of radius
    int(3 * int(scale * 4) / 2), fill=rgb + (225,)), frame by frame."""
    k, frame = _keypoints(poses_per_frame)
    if not len(k):
        return _prims(0)
    _check_coords(k[..., :2], 'keypoint')
    xy = np.trunc(k[..., :2]).astype(np.int64)
    present = k[..., 2] != 0
    src, dst = POSE_CONNECTIONS[:, 0], POSE_CONNECTIONS[:, 1]
    lm = present[:, src] & present[:, dst]                                   # (P, 17), person-major: the reference's order
    p_idx, l_idx = np.nonzero(lm)
    limbs = _prims(len(p_idx))
    limbs['frame'] = frame[p_idx]
    limbs['kind'] = lib.DRAW_LINE
    limbs['x0'], limbs['y0'] = xy[p_idx, src[l_idx], 0], xy[p_idx, src[l_idx], 1]
    limbs['x1'], limbs['y1'] = xy[p_idx, dst[l_idx], 0], xy[p_idx, dst[l_idx], 1]
    limbs['width'] = int(scale * 8)
    limbs['rgba'][:, :3] = POSE_CONNECTION_COLORS[l_idx]
    limbs['rgba'][:, 3] = LIMB_ALPHA

    r = int(3 * int(scale * 4) / 2)
    p_idx, k_idx = np.nonzero(present)
    x, y = k[p_idx, k_idx, 0], k[p_idx, k_idx, 1]
    dots = _prims(len(p_idx))
    dots['frame'] = frame[p_idx]
    dots['kind'] = lib.DRAW_DISC
    dots['x0'], dots['y0'] = np.trunc(x - r), np.trunc(y - r)               # Pillow truncates each corner
    dots['x1'], dots['y1'] = np.trunc(x + r), np.trunc(y + r)
    dots['rgba'][:, :3] = POSE_KEYPOINT_COLORS[k_idx]
    dots['rgba'][:, 3] = KEYPOINT_ALPHA
    return np.concatenate([limbs, dots])


def _check_batch(frames, per_frame):
    if len(per_frame) > len(frames):
        raise ValueError('%d result lists for a batch of %d frames' % (len(per_frame), len(frames)))


def draw_faces(frames, faces_per_frame, scale=1.0, ctx=None):
    """Draw face markers into the resident batch `frames` (lib.Frames) in place: faces_per_frame[i] (a dict, or a list of
    dicts as face_detection / face_tracking return) goes into frame i.  `ctx`: the caller's context (default: the
    batch's own)."""
    _check_batch(frames, faces_per_frame)
    frames.draw(pack_faces(faces_per_frame, scale), ctx=ctx)
    return frames


def draw_poses(frames, poses_per_frame, scale=1.0, ctx=None):
    """Draw poses (as pose_estimation returns them) into the resident batch `frames` in place, one list per frame."""
    _check_batch(frames, poses_per_frame)
    frames.draw(pack_poses(poses_per_frame, scale), ctx=ctx)
    return frames


def _on_host_image(image, prims, device=None):
    from . import runtime
    image = np.asarray(image)
    if image.dtype != np.uint8 or image.ndim != 3 or image.shape[2] != 3:
        raise ValueError('expected a uint8 (H, W, 3) RGB image, got %s %s' % (image.dtype, image.shape))
    ctx = runtime.get_context(device)
    frames = ctx.upload(image[None])
    try:
        frames.draw(prims)
        return frames.download()[0]
    finally:
        frames.free()


def vis_faces(image, faces, scale=1.0):
    """terran.vis.vis_faces: a copy of `image` with a box drawn over every face (dict or list of dicts)."""
    return _on_host_image(image, pack_faces([faces], scale))


def vis_poses(image, poses, scale=1.0):
    """terran.vis.vis_poses: a copy of `image` with the limbs and keypoints of every pose (dict or list of dicts)."""
    return _on_host_image(image, pack_poses([poses], scale))
