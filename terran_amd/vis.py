"""Drawing results into frames on the GPU: the reference's `terran.vis` (vis_faces / vis_poses, its Pillow path).

`vis_faces(image, faces, scale)` / `vis_poses(image, poses, scale)` keep the reference's signatures and return values: a
host uint8 (H, W, 3) image in, a new array with the markers drawn out.  `draw_faces` / `draw_poses` draw in place into a
resident `lib.Frames` batch (what `video.RawVideoReader` yields and `StreamPipeline.run(..., free_resident=False)` hands
back), one list of results per frame, so a video job never downloads a frame to draw on it.

The pixels are the reference's bit for bit (Pillow's ImageDraw.Draw(img, 'RGBA') rectangle outlines, lines and ellipses,
restated in csrc/draw.hip).  The colours follow the reference's tables; FACE_COLORMAP is, as there, module-global and
stateful: a label gets the next palette colour the first time it is seen, and a face without a label (no `name`, and
`track` absent or 0) a random one from Python's `random`.

Labels (`labels=True` on vis_faces / draw_faces / pack_faces; off by default): a face that carries `text`, or else
`track` (label '#<track>'), gets the reference's `draw_label` after its marker -- a filled tab in the face's colour at the
box's top-left corner and the text on it in white -- with `FreeTypeFont.getsize(t)`, which Pillow 10 removed and the
reference still calls, read as `getbbox(t)[2:4]` (what it returned).  The glyphs are rasterised on the host by Pillow's
font (FreeType), once per distinct (font, size, text, fractional start): an LRU keeps the coverage bitmaps, and a call
uploads each distinct one once, however many frames show it.  The tab is a bar, the text a DRAW_MASK primitive.

Blurring (`blur_faces` in place on a resident batch, `anonymize_faces` on a host image; not in the reference): every
face's box, int()-truncated and clipped to the frame, is replaced by Pillow's
`im.crop(box).filter(ImageFilter.GaussianBlur(radius))` bit for bit (csrc/blur.hip), optionally only under the ellipse
`ImageDraw.ellipse` draws into that box, so a video job makes its faces unrecognisable without downloading a frame.

With method='pixelate' the box becomes a mosaic instead (Pillow's resize to 1 / block with BOX and back with NEAREST;
csrc/resample.hip).  `crop_faces` cuts the same boxes out of a resident batch as chips of one size, Pillow's
`resize(size, resample, box=box)` bit for bit, into one new resident batch that `image.encode_jpeg` / `save_images`
take as it is.

Host glue only: the packing of results into primitives is numpy; the drawing is one ta_frames_draw(_masks) launch, the
blurring one ta_frames_blur or ta_frames_pixelate call, the cropping one ta_frames_resample call, the aligned chips of
`align_faces` (the embedder's five-point similarity, Pillow's Image.transform; csrc/transform.hip) one ta_frames_transform
call, the upright chips `quad_chips` cuts out of quadrilaterals (Pillow's Image.QUAD) one ta_frames_transform_mesh call.
Importing this module needs no GPU and no Pillow.
"""
import collections
import math
import random

import numpy as np

from . import image, lib

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


# ---- labels: the reference's draw_label --------------------------------------------------------------------------------
LABEL_FONT_NAMES = ('DejaVuSans-Bold', 'DroidSans-Bold')        # the reference's choice on Linux, in its order
LABEL_CACHE_SIZE = 1024
LABEL_INK = (255, 255, 255, 255)                                # draw.text's default ink


class PillowFont:
    """What label packing needs of a font: `key` (hashable: which font, which size), `measure(text)` -> (width, height),
    the reference's `getsize`, and `mask(text, start)` -> (uint8 (h, w) coverage bitmap, (x, y) offset from the integer
    pen position), what draw.text places.  This one wraps a Pillow font, FreeType or bitmap."""

    def __init__(self, font, key):
        self.font, self.key = font, key

    def measure(self, text):
        return tuple(self.font.getbbox(text)[2:4])

    def mask(self, text, start):
        try:
            core, offset = self.font.getmask2(text, 'L', anchor='la', start=start)
        except AttributeError:                          # a bitmap font: no bearings, no fractional start
            core, offset = self.font.getmask(text, 'L'), (0, 0)
        w, h = core.size
        bitmap = np.frombuffer(bytes(core), np.uint8).reshape(h, w) if w and h else np.zeros((0, 0), np.uint8)
        return bitmap, (int(offset[0]), int(offset[1]))


_system_font = []                                       # [font or None], resolved on first use
_fonts = {}                                             # size -> PillowFont
_masks = collections.OrderedDict()    # (font key, text, start) -> (bitmap, offset), (font key, text, None) -> metrics: an LRU


def label_font(size):
    """The reference's label font at `size` (its round(16 * scale)): DejaVuSans-Bold as ImageFont.truetype finds it,
    else Pillow's default font as it is."""
    if size not in _fonts:
        from PIL import ImageFont
        if not _system_font:
            font = None
            for name in LABEL_FONT_NAMES:
                try:
                    font = ImageFont.truetype(name)
                    break
                except IOError:
                    continue
            _system_font.append(font)
        base = _system_font[0]
        if base is not None:
            _fonts[size] = PillowFont(base.font_variant(size=size), (base.path, size))
        else:
            _fonts[size] = PillowFont(ImageFont.load_default(), ('default', 0))
    return _fonts[size]


def _cached(key, make):
    hit = _masks.get(key)
    if hit is None:
        hit = _masks[key] = make()
        while len(_masks) > LABEL_CACHE_SIZE:
            _masks.popitem(last=False)
    else:
        _masks.move_to_end(key)
    return hit


def _label_measure(font, text):
    return _cached((font.key, text, None), lambda: font.measure(text))


def _label_mask(font, text, start):
    def make():
        bitmap, offset = font.mask(text, start)
        return bitmap if bitmap.any() else bitmap[:0], offset      # no coverage (spaces): nothing to place
    key = (font.key, text, start)
    return key, _cached(key, make)


def _face_text(face):
    if face.get('text') is not None:
        return str(face['text'])
    if face.get('track') is not None:
        return '#%s' % (face['track'],)
    return None


def _pack_labels(labelled, colors, frame, scale):
    """draw_label for the faces `labelled` [(face index, bbox as the caller gave it, text)] -> (PRIM_DT array of a tab and
    a mask per label, face index of each, atlas).  The corner arithmetic runs on the caller's own scalars, as the
    reference's does (a float32 box stays float32 under NumPy 2), and is then converted as Pillow converts it: float(),
    C's (int) for the rectangle, int() and math.modf for the text."""
    size = round(16 * scale)
    if size < 1:
        raise ValueError('font size must be greater than 0, not %d (scale %r)' % (size, scale))
    for _, _, text in labelled:
        if '\n' in text:
            raise ValueError('multiline labels are not supported: %r' % text)
    font = label_font(size)
    margin_w = 0.2 * _label_measure(font, 'M')[0]
    line_h = _label_measure(font, 'Mq')[1]
    atlas, where, total = [], {}, 0
    rows = []                                           # (face, frame, kind, x0, y0, x1, y1, width, r, g, b)
    for i, bbox, text in labelled:
        x, y = bbox[0], bbox[1]
        x1, y1 = int(float(x + _label_measure(font, text)[0] + 3 * margin_w)), int(float(y + line_h * 1.15))
        rows.append((i, frame[i], lib.DRAW_BAR, int(float(x)), int(float(y)), min(x1, COORD_LIMIT), min(y1, COORD_LIMIT), 0)
                    + tuple(colors[i]))
        tx, ty = float(x + margin_w), float(y)
        key, (bitmap, offset) = _label_mask(font, text, (math.modf(tx)[0], math.modf(ty)[0]))
        h, w = bitmap.shape
        x0, y0 = int(tx) + offset[0], int(ty) + offset[1]
        if not bitmap.size or max(abs(x0), abs(y0), abs(x0 + w - 1), abs(y0 + h - 1)) > COORD_LIMIT:
            continue                                    # a label of spaces: the tab only; beyond any frame: nothing to see
        if key not in where:
            where[key] = total
            atlas.append(bitmap.ravel())
            total += bitmap.size
        rows.append((i, frame[i], lib.DRAW_MASK, x0, y0, x0 + w - 1, y0 + h - 1, where[key]) + LABEL_INK[:3])
    r = np.array(rows, np.int64)
    out = _prims(len(r))
    for c, name in enumerate(('frame', 'kind', 'x0', 'y0', 'x1', 'y1', 'width'), 1):
        out[name] = r[:, c]
    out['rgba'][:, :3] = r[:, 8:]
    out['rgba'][:, 3] = MARKER_ALPHA
    return out, r[:, 0], np.concatenate(atlas) if atlas else np.zeros(0, np.uint8)


def pack_faces(faces_per_frame, scale=1.0, labels=False):
    """-> PRIM_DT array: each face's rectangle outline (Pillow draw.rectangle(bbox, outline=rgb + (255,), width=int(3 *
    scale))) as up to four opaque bars, faces in order, frame by frame.  Every box is checked first: an inverted one
    raises ValueError (as Pillow does) before anything is drawn.

    labels=True -> (PRIM_DT array, uint8 atlas): after its marker every face with `text` or `track` gets its label, a
    bar (the tab) and a DRAW_MASK primitive (the text) whose `width` is the offset of its bitmap in the atlas; equal
    bitmaps share one place there.  `Frames.draw(prims, masks=atlas)` draws them."""
    boxes, colors, frame, labelled = [], [], [], []
    for f, faces in enumerate(faces_per_frame):
        for face in _as_list(faces):
            colors.append(FACE_COLORMAP(face.get('name') or face.get('track')))
            boxes.append(np.asarray(face['bbox'], np.float64).reshape(4))
            frame.append(f)
            if labels and _face_text(face) is not None:
                labelled.append((len(boxes) - 1, face['bbox'], _face_text(face)))
    prims, face_of = _pack_markers(boxes, colors, frame, scale)
    if not labels:
        return prims
    if not labelled:
        return prims, np.zeros(0, np.uint8)
    tabs, tab_face, atlas = _pack_labels(labelled, colors, frame, scale)
    both, face_of = np.concatenate([prims, tabs]), np.concatenate([face_of, tab_face])
    return both[np.argsort(face_of, kind='stable')], atlas     # face by face: marker, tab, text


def _pack_markers(boxes, colors, frame, scale):
    """-> (PRIM_DT array of the faces' outlines, face index of each bar)."""
    if not boxes:
        return _prims(0), np.zeros(0, np.int64)
    b = np.stack(boxes)
    if np.any(b[:, 2] < b[:, 0]):
        raise ValueError('x1 must be greater than or equal to x0')
    if np.any(b[:, 3] < b[:, 1]):
        raise ValueError('y1 must be greater than or equal to y0')
    _check_coords(b, 'box')
    w = int(3 * scale)
    if w <= 0:                                          # Pillow: rectangle(width=0) draws nothing
        return _prims(0), np.zeros(0, np.int64)
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
    keep = (out['y1'] >= out['y0']) & (out['x1'] >= out['x0'])
    return out[keep], np.repeat(np.arange(m), 4)[keep]


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


def draw_faces(frames, faces_per_frame, scale=1.0, ctx=None, labels=False):
    """Draw face markers into the resident batch `frames` (lib.Frames) in place: faces_per_frame[i] (a dict, or a list of
    dicts as face_detection / face_tracking return) goes into frame i.  `ctx`: the caller's context (default: the
    batch's own).  `labels`: write each face's `text`, or '#<track>', on a tab at its box's corner."""
    _check_batch(frames, faces_per_frame)
    if labels:
        frames.draw(*pack_faces(faces_per_frame, scale, labels=True), ctx=ctx)
    else:
        frames.draw(pack_faces(faces_per_frame, scale), ctx=ctx)
    return frames


def draw_poses(frames, poses_per_frame, scale=1.0, ctx=None):
    """Draw poses (as pose_estimation returns them) into the resident batch `frames` in place, one list per frame."""
    _check_batch(frames, poses_per_frame)
    frames.draw(pack_poses(poses_per_frame, scale), ctx=ctx)
    return frames


# ---- blurring faces ----------------------------------------------------------------------------------------------------
BLUR_SHAPES = {'box': lib.BLUR_BOX, 'ellipse': lib.BLUR_ELLIPSE}
BLUR_RADIUS_LIMIT = 1024.0                              # what ta_frames_blur accepts


def _frame_sizes(shapes, n):
    """`shapes` of pack_blur -> (n, 2) int array of (H, W)."""
    s = np.asarray(shapes, np.int64)
    if s.ndim == 1 and s.size in (2, 3):                # (H, W) or (H, W, 3): every frame
        s = np.broadcast_to(s[:2], (n, 2))
    elif s.ndim == 1 and s.size == 4:                   # a batch's (N, H, W, 3)
        s = np.broadcast_to(s[1:3], (n, 2))
    elif s.ndim == 2 and s.shape[1] >= 2 and len(s) >= n:
        s = s[:, :2]
    else:
        raise ValueError('shapes must be (H, W), a batch shape (N, H, W, 3) or one (H, W) per frame, got %r' % (shapes,))
    return s


def pack_blur(faces_per_frame, shapes, radius=None, margin=0.0, shape='box'):
    """-> lib.BLUR_DT array, faces in order, frame by frame: each face's bbox, widened by `margin` x its width left and
    right and `margin` x its height top and bottom (Python floats), int()-truncated and clipped to its frame, as the
    half-open region [x0, x1) x [y0, y1); a face whose region is empty is left out.  `shapes`: the frames' (H, W) --
    one pair for all, a batch's shape (N, H, W, 3), or a pair per frame.  `radius`: GaussianBlur's, 0 .. 1024; None:
    max(w, h) / 8 of the clipped region (at most 1024).  `shape`: 'box', or 'ellipse' (only the ellipse Pillow draws into the region is replaced).
    Bad values raise ValueError before anything is blurred."""
    if shape not in BLUR_SHAPES:
        raise ValueError("shape must be 'box' or 'ellipse', got %r" % (shape,))
    if radius is not None and not 0 <= float(radius) <= BLUR_RADIUS_LIMIT:
        raise ValueError('radius must be within 0 .. %g, got %r' % (BLUR_RADIUS_LIMIT, radius))
    rows = []
    for f, _, x0, y0, x1, y1 in _clipped_boxes(faces_per_frame, shapes, margin):
        r = max(x1 - x0, y1 - y0) / 8 if radius is None else float(radius)
        rows.append((f, x0, y0, x1, y1, BLUR_SHAPES[shape], min(r, BLUR_RADIUS_LIMIT)))
    return np.array(rows, lib.BLUR_DT)


def pack_pixelate(faces_per_frame, shapes, block=None, margin=0.0, shape='box'):
    """-> lib.PIXELATE_DT array: pack_blur's regions (the same margin, truncation, clipping and order) with the side of a
    mosaic cell in place of the radius.  `block`: an int 1 .. 16384; None: max(1, max(w, h) // 8) of the clipped region."""
    if shape not in BLUR_SHAPES:
        raise ValueError("shape must be 'box' or 'ellipse', got %r" % (shape,))
    if block is not None and (isinstance(block, bool) or not isinstance(block, (int, np.integer))
                              or not 1 <= block <= lib.RESAMPLE_SIDE_LIMIT):
        raise ValueError('block must be an int within 1 .. %d, got %r' % (lib.RESAMPLE_SIDE_LIMIT, block))
    rows = []
    for f, _, x0, y0, x1, y1 in _clipped_boxes(faces_per_frame, shapes, margin):
        b = max(1, max(x1 - x0, y1 - y0) // 8) if block is None else int(block)
        rows.append((f, x0, y0, x1, y1, BLUR_SHAPES[shape], min(b, lib.RESAMPLE_SIDE_LIMIT)))
    return np.array(rows, lib.PIXELATE_DT)


def pack_crops(faces_per_frame, shapes, margin=0.0):
    """-> (lib.RESAMPLE_DT array, int32 (n, 2) index of (frame, face) pairs): pack_blur's regions (the same margin,
    truncation, clipping and order) as the source boxes of Frames.resample; a face whose region is empty is left out of
    both.  Host only."""
    rows, index = [], []
    for f, k, x0, y0, x1, y1 in _clipped_boxes(faces_per_frame, shapes, margin):
        rows.append((f, x0, y0, x1, y1))
        index.append((f, k))
    return np.array(rows, lib.RESAMPLE_DT), np.array(index, np.int32).reshape(-1, 2)


def pack_stats(faces_per_frame, shapes, margin=0.0, shape='box'):
    """-> (lib.HIST_DT array, int32 (n, 2) index of (frame, face) pairs): pack_blur's regions (the same margin, truncation,
    clipping and order) for Frames.histogram; a face whose region is empty is left out of both.  Host only."""
    if shape not in BLUR_SHAPES:
        raise ValueError("shape must be 'box' or 'ellipse', got %r" % (shape,))
    rows, index = [], []
    for f, k, x0, y0, x1, y1 in _clipped_boxes(faces_per_frame, shapes, margin):
        rows.append((f, x0, y0, x1, y1, BLUR_SHAPES[shape]))
        index.append((f, k))
    return np.array(rows, lib.HIST_DT), np.array(index, np.int32).reshape(-1, 2)


def face_stats(frames, faces_per_frame, margin=0.0, shape='box', mode='RGB', ctx=None):
    """Exposure statistics of the faces of the resident batch `frames` (lib.Frames) -> (stats, index): `stats` is
    `image.histogram_stats` of one `ta_frames_histogram` call over the faces' boxes as pack_blur clips them -- Pillow's
    `ImageStat.Stat(frame.crop(box))` (mode 'L': of its `convert('L')`), under `shape` 'ellipse' with the ellipse Pillow
    draws into the box as Stat's mask -- a dict of arrays (n_faces, 3) or (n_faces, 1), plus 'histogram', the uint32 counts
    they come from; `index` the int32 (n_faces, 2) (frame, face) pairs, as `crop_faces` returns them.  (None, []) when
    there is no face.  Choosing the best-exposed chip of a track is an argmax over these."""
    _check_batch(frames, faces_per_frame)
    if mode not in lib.HIST_MODES:
        raise ValueError("mode must be 'RGB' or 'L', got %r" % (mode,))
    regions, index = pack_stats(faces_per_frame, frames.shape, margin, shape)
    if not len(regions):
        return None, []
    hist = frames.histogram(regions, lib.HIST_MODES[mode], ctx=ctx)
    stats = image.histogram_stats(hist if hist.ndim == 3 else hist[:, None])
    stats['histogram'] = hist
    return stats, index


def _clipped_boxes(faces_per_frame, shapes, margin):
    """[(frame, face, x0, y0, x1, y1)]: every face's bbox widened by `margin`, int()-truncated and clipped to its frame,
    faces in order, frame by frame; empty ones left out."""
    margin = float(margin)
    if not math.isfinite(margin):
        raise ValueError('margin must be finite, got %r' % (margin,))
    sizes = _frame_sizes(shapes, len(faces_per_frame))
    out = []
    for f, faces in enumerate(faces_per_frame):
        h, w = int(sizes[f][0]), int(sizes[f][1])
        for k, face in enumerate(_as_list(faces)):
            x0, y0, x1, y1 = (float(v) for v in np.asarray(face['bbox']).reshape(4))
            if margin:
                dx, dy = margin * (x1 - x0), margin * (y1 - y0)
                x0, y0, x1, y1 = x0 - dx, y0 - dy, x1 + dx, y1 + dy
            if not all(abs(v) <= COORD_LIMIT for v in (x0, y0, x1, y1)):
                raise ValueError('box coordinates must be finite and within +-2^24')
            x0, y0, x1, y1 = max(int(x0), 0), max(int(y0), 0), min(int(x1), w), min(int(y1), h)
            if x1 <= x0 or y1 <= y0:
                continue
            out.append((f, k, x0, y0, x1, y1))
    return out


def crop_faces(frames, faces_per_frame, size=(112, 112), margin=0.0, resample='bicubic', ctx=None):
    """Cut the faces of the resident batch `frames` (lib.Frames) out as chips of one size -> (chips, index): `chips` one
    resident (n_faces, height, width, 3) lib.Frames, faces in order, frame by frame (None when there is no face), each
    Pillow's `Image.fromarray(frame).resize(size, resample, box=box)` of the face's box as pack_blur clips it; `index`
    the int32 (n_faces, 2) (frame, face) pairs of the chips.  `size`: (width, height); `resample`: a filter's name or
    Pillow's code.  `encode_jpeg` / `save_images` take `chips` as they are.  `ctx`: the caller's context."""
    _check_batch(frames, faces_per_frame)
    width, height = _chip_size(size)
    code = lib.resample_filter(resample)
    regions, index = pack_crops(faces_per_frame, frames.shape, margin)
    if not len(regions):
        return None, index
    return frames.resample(regions, height, width, code, ctx=ctx), index


def pack_align(faces_per_frame, side=112):
    """-> (lib.TRANSFORM_DT array, int32 (n, 2) index of (frame, face) pairs): for every face, in order, frame by frame, the
    AFFINE map of its landmark-aligned side x side chip -- the five-point similarity the embedder cuts its crops with
    (arcface.align_matrices; the template scaled by side / 112).  A face without 'landmarks' raises ValueError.  Host only."""
    from . import arcface
    lms, index = [], []
    for f, faces in enumerate(faces_per_frame):
        for k, face in enumerate(_as_list(faces)):
            lm = face.get('landmarks') if hasattr(face, 'get') else None
            if lm is None or np.asarray(lm).shape != (5, 2) or not np.isfinite(np.asarray(lm, np.float64)).all():
                raise ValueError('align_faces: face %d of frame %d has no (5, 2) finite landmarks' % (k, f))
            lms.append(np.asarray(lm))
            index.append((f, k))
    regions = np.zeros(len(lms), lib.TRANSFORM_DT)
    if lms:
        regions['frame'] = [f for f, _ in index]
        regions['method'] = lib.AFFINE
        regions['a'][:, :6] = arcface.align_matrices(np.stack(lms), side)
    return regions, np.array(index, np.int32).reshape(-1, 2)


def align_faces(frames, faces_per_frame, size=(112, 112), resample='bilinear', ctx=None):
    """Cut the landmark-aligned chips of the faces of the resident batch `frames` (lib.Frames) -> (chips, index) as
    `crop_faces` returns them: `chips` one resident (n_faces, side, side, 3) RGB lib.Frames (None when there is no face),
    each Pillow's `Image.fromarray(frame).transform(size, AFFINE, matrix, resample)` with the embedder's five-point
    similarity (at (112, 112) bilinear: the very crops the embedder sees, bit for bit); `index` the int32 (n_faces, 2)
    (frame, face) pairs.  `size`: (side, side), square; `resample`: 'nearest', 'bilinear', 'bicubic' or Pillow's code."""
    _check_batch(frames, faces_per_frame)
    width, height = _chip_size(size)
    if width != height:
        raise ValueError('align_faces: size must be square (the template is), got %r' % (size,))
    code = lib.resample_filter(resample)
    if code not in lib.TRANSFORM_FILTERS:
        raise ValueError("align_faces: resample must be 'nearest', 'bilinear' or 'bicubic', got %r" % (resample,))
    regions, index = pack_align(faces_per_frame, width)
    if not len(regions):
        return None, []
    return frames.transform(regions, height, width, code, ctx=ctx), index


def pack_quads(quads_per_frame, size):
    """-> (lib.MESH_CELL_DT array, lib.MESH_IMAGE_DT array, int32 (n, 2) index of (frame, quad) pairs): for every quad, in
    order, frame by frame, the one-cell mesh ((0, 0) + size, quad) of its chip and the frame it is cut from; mesh k is cell
    k.  A quad is 8 finite numbers, the corners nw, sw, se, ne as (x, y) in its frame.  Host only."""
    width, height = _chip_size(size)
    quads, index = [], []
    for f, per in enumerate(quads_per_frame):
        try:
            per = np.asarray(per, np.float64)
        except (TypeError, ValueError):
            per = np.zeros(1)
        if per.size == 0:
            per = np.zeros((0, 8))
        elif per.shape == (8,):                             # a single quad for this frame
            per = per[None]
        if per.ndim != 2 or per.shape[1] != 8 or not np.isfinite(per).all():
            raise ValueError('quad_chips: the quads of frame %d must be 8 finite numbers each' % f)
        quads.extend(per)
        index.extend((f, k) for k in range(len(per)))
    cells = np.zeros(len(quads), lib.MESH_CELL_DT)
    images = np.zeros(len(quads), lib.MESH_IMAGE_DT)
    if quads:
        cells['x1'], cells['y1'], cells['quad'] = width, height, np.stack(quads)
        images['frame'], images['mesh'] = [f for f, _ in index], np.arange(len(quads))
    return cells, images, np.array(index, np.int32).reshape(-1, 2)


def quad_chips(frames, quads_per_frame, size, resample='bilinear', ctx=None):
    """Cut quadrilaterals -- screens, whiteboards, plates, given by their four corners -- out of the resident batch `frames`
    (lib.Frames) as upright chips of one size -> (chips, index) as `crop_faces` returns them: `chips` one resident
    (n_quads, height, width, 3) lib.Frames (None when there is no quad), each Pillow's
    `Image.fromarray(frame).transform(size, Image.QUAD, quad, resample)`; `index` the int32 (n_quads, 2) (frame, quad) pairs.
    quads_per_frame[i]: the quads of frame i, 8 numbers each (nw, sw, se, ne; x, y).  One ta_frames_transform_mesh call
    for all quads of all frames, one single-cell mesh per chip.  `size`: (width, height); `resample`: 'nearest',
    'bilinear', 'bicubic' or Pillow's code."""
    _check_batch(frames, quads_per_frame)
    width, height = _chip_size(size)
    code = lib.resample_filter(resample)
    if code not in lib.TRANSFORM_FILTERS:
        raise ValueError("quad_chips: resample must be 'nearest', 'bilinear' or 'bicubic', got %r" % (resample,))
    cells, images, index = pack_quads(quads_per_frame, size)
    if not len(cells):
        return None, []
    if len(cells) > lib.MESH_MAX_CELLS:
        raise ValueError('quad_chips: more than %d quads' % lib.MESH_MAX_CELLS)
    return frames.transform_mesh(cells, np.arange(len(cells) + 1), images, height, width, code, ctx=ctx), index


def _chip_size(size):
    try:
        width, height = (int(v) for v in size)
    except (TypeError, ValueError):
        raise ValueError('size must be (width, height), got %r' % (size,)) from None
    if not (1 <= width <= lib.RESAMPLE_SIDE_LIMIT and 1 <= height <= lib.RESAMPLE_SIDE_LIMIT):
        raise ValueError('size must be within 1 .. %d a side, got %r' % (lib.RESAMPLE_SIDE_LIMIT, size))
    return width, height


BLUR_METHODS = ('gaussian', 'pixelate')


def _pack_anonymize(faces_per_frame, shapes, radius, margin, shape, method, block):
    """-> (regions, pixelate?) for blur_faces / anonymize_faces; every argument is checked before anything is launched."""
    if method not in BLUR_METHODS:
        raise ValueError("method must be 'gaussian' or 'pixelate', got %r" % (method,))
    if method == 'pixelate':
        if radius is not None:
            raise ValueError("radius belongs to method='gaussian'; method='pixelate' takes block")
        return pack_pixelate(faces_per_frame, shapes, block, margin, shape), True
    if block is not None:
        raise ValueError("block belongs to method='pixelate'; method='gaussian' takes radius")
    return pack_blur(faces_per_frame, shapes, radius, margin, shape), False


def blur_faces(frames, faces_per_frame, radius=None, margin=0.0, shape='box', ctx=None, method='gaussian', block=None):
    """Blur the faces of the resident batch `frames` (lib.Frames) in place: faces_per_frame[i] (a dict, or a list of dicts
    as face_detection / face_tracking return) goes into frame i, in list order (a later face blurs what an earlier one it
    overlaps left).  `radius`, `margin`, `shape`: pack_blur's.  `ctx`: the caller's context (default: the batch's own).
    `method`: 'gaussian', or 'pixelate' (a mosaic: Pillow's `region.resize(small, BOX).resize(region.size, NEAREST)` with
    cells of `block` pixels, None: max(1, max(w, h) // 8) of each box; it takes no `radius`)."""
    _check_batch(frames, faces_per_frame)
    regions, pixelate = _pack_anonymize(faces_per_frame, frames.shape, radius, margin, shape, method, block)
    if pixelate:
        frames.pixelate(regions, ctx=ctx)
    else:
        frames.blur(regions, ctx=ctx)
    return frames


def pack_color(faces_per_frame, shapes, margin=0.0, shape='box'):
    """-> lib.COLOR_REGION_DT array with op 0: pack_blur's regions (the same margin, truncation, clipping and order).
    Host only."""
    if shape not in BLUR_SHAPES:
        raise ValueError("shape must be 'box' or 'ellipse', got %r" % (shape,))
    boxes = _clipped_boxes(faces_per_frame, shapes, margin)
    q = np.zeros(len(boxes), lib.COLOR_REGION_DT)
    for r, (f, _, x0, y0, x1, y1) in zip(q, boxes):
        r['frame'], r['x0'], r['y0'], r['x1'], r['y1'], r['shape'] = f, x0, y0, x1, y1, BLUR_SHAPES[shape]
    return q


def color_faces(frames, faces_per_frame, op, margin=0.0, shape='box', ctx=None):
    """Convert the colours of the faces of the resident batch `frames` in place (ta_frames_color): `op` is what
    terran_amd.image.color_spec takes -- a 12-tuple matrix, 'ycbcr' / 'hsv' and back, a Color3DLUT or (size, table) --, so a
    grade, a tint or a desaturating matrix shows only in the faces.  The boxes, their clipping and their order are
    blur_faces'."""
    _check_batch(frames, faces_per_frame)
    rec, table = image.color_spec(op)
    frames.color(pack_color(faces_per_frame, frames.shape, margin, shape), rec, table, ctx=ctx)
    return frames


# ---- two batches: a processed copy inside the face boxes, chips back into the frame ------------------------------------
def pack_composite(faces_per_frame, shapes, other_frames=None, margin=0.0, shape='box', alpha=None):
    """-> lib.COMBINE_DT array: pack_blur's regions (the same margin, truncation, clipping and order) as PASTE records that
    read the same box of the other batch -- frame i of it, or frame 0 when it has `other_frames` = 1 frame; `alpha`: None,
    or 0 .. 1: a constant mask round(255 alpha).  Host only."""
    if shape not in BLUR_SHAPES:
        raise ValueError("shape must be 'box' or 'ellipse', got %r" % (shape,))
    if alpha is not None and not 0 <= float(alpha) <= 1:
        raise ValueError('alpha must be None or within 0 .. 1, got %r' % (alpha,))
    boxes = _clipped_boxes(faces_per_frame, shapes, margin)
    q = np.zeros(len(boxes), lib.COMBINE_DT)
    for r, (f, _, x0, y0, x1, y1) in zip(q, boxes):
        r['frame'], r['x0'], r['y0'], r['x1'], r['y1'], r['shape'] = f, x0, y0, x1, y1, BLUR_SHAPES[shape]
        r['src_frame'], r['src_x'], r['src_y'], r['op'] = 0 if other_frames == 1 else f, x0, y0, lib.COMBINE_PASTE
        if alpha is not None:
            r['mask_kind'], r['mask_value'] = lib.MASK_CONSTANT, int(round(255 * float(alpha)))
    return q


def composite_faces(frames, other, faces_per_frame, margin=0.0, shape='box', alpha=None, ctx=None):
    """Give every face box of the resident batch `frames` the pixels of `other`, in place: `other` a batch of the frames'
    size, with as many frames or one -- a denoised, blurred or equalised copy that is to show only in the faces.  The
    boxes, their clipping and their order are blur_faces'; `alpha`: None pastes, a float 0 .. 1 blends under the constant
    mask round(255 alpha), as Pillow's paste does."""
    _check_batch(frames, faces_per_frame)
    if other.shape[1:3] != frames.shape[1:3] or other.shape[0] not in (1, frames.shape[0]):
        raise ValueError('composite_faces: other must be %s frames, one or %d, got %s' % (frames.shape[1:3], frames.shape[0], other.shape))
    frames.combine(other, pack_composite(faces_per_frame, frames.shape, other.shape[0], margin, shape, alpha), ctx=ctx)
    return frames


def pack_insets(index, chips_shape, shapes, origin=(8, 8), gap=4):
    """-> lib.COMBINE_DT array: chip k of a (n, h, w, 3) chip batch, which belongs to frame index[k][0], pasted into that
    frame: each frame's chips in a row from `origin` = (x, y), `gap` pixels apart, a new row below at the frame's right
    edge; a chip that no longer fits into the frame is left out.  Host only."""
    n, ch, cw = (int(v) for v in chips_shape[:3])
    index = np.asarray(index, np.int64).reshape(-1, 2)
    if len(index) != n:
        raise ValueError('%d index pairs for %d chips' % (len(index), n))
    ox, oy, gap = int(origin[0]), int(origin[1]), int(gap)
    if ox < 0 or oy < 0 or gap < 0:
        raise ValueError('origin and gap must not be negative, got %r, %r' % (origin, gap))
    frames = int(index[:, 0].max()) + 1 if n else 0
    sizes = _frame_sizes(shapes, frames)
    rows, at = [], {}
    for k, f in enumerate(int(v) for v in index[:, 0]):
        if f < 0:
            raise ValueError('frame %d in the index' % f)
        h, w = int(sizes[f][0]), int(sizes[f][1])
        x, y = at.get(f, (ox, oy))
        if x + cw > w and x != ox:
            x, y = ox, y + ch + gap
        at[f] = (x, y)
        if x + cw > w or y + ch > h:
            continue
        rows.append((f, x, y, x + cw, y + ch, lib.BLUR_BOX, k, 0, 0, lib.COMBINE_PASTE, 0.0, 0, lib.MASK_NONE, 0, 0, 0, 0, 0))
        at[f] = (x + cw + gap, y)
    return np.array(rows, lib.COMBINE_DT)


def inset_chips(frames, chips, index, origin=(8, 8), gap=4, ctx=None):
    """Paste the chips that `crop_faces` / `align_faces` cut (`chips`, `index` as they return them) back into their frames
    of the resident batch `frames` as thumbnails, in place; the layout is pack_insets'."""
    if chips is None or not len(index):
        return frames
    frames.combine(chips, pack_insets(index, chips.shape, frames.shape, origin, gap), ctx=ctx)
    return frames


def pack_filter(faces_per_frame, shapes, margin=0.0, shape='box'):
    """-> lib.FILTER_REGION_DT array: pack_blur's regions (the same margin, truncation, clipping and order) for
    Frames.filter, every one with spec 0.  Host only."""
    if shape not in BLUR_SHAPES:
        raise ValueError("shape must be 'box' or 'ellipse', got %r" % (shape,))
    rows = [(f, x0, y0, x1, y1, BLUR_SHAPES[shape], 0) for f, _, x0, y0, x1, y1 in _clipped_boxes(faces_per_frame, shapes, margin)]
    return np.array(rows, lib.FILTER_REGION_DT)


def filter_faces(frames, faces_per_frame, flt, margin=0.0, shape='box', ctx=None):
    """Filter the faces of the resident batch `frames` (lib.Frames) in place, Pillow's `crop(box).filter(flt)` pasted back
    under `shape`: sharpen soft faces before they are cropped, denoise them, take their edges.  The boxes, their clipping
    and their order are blur_faces'; `flt`: what `image.filter_spec` takes (a GaussianBlur goes the way of blur_faces)."""
    _check_batch(frames, faces_per_frame)
    spec = image.filter_spec(flt)
    if spec['kind'] == image.FILTER_GAUSSIAN:
        frames.blur(pack_blur(faces_per_frame, frames.shape, float(spec['radius']), margin, shape), ctx=ctx)
    else:
        frames.filter(pack_filter(faces_per_frame, frames.shape, margin, shape), spec, ctx=ctx)
    return frames


# ---- whole people: silhouettes from skeletons --------------------------------------------------------------------------
# ta_poses_paint (include/terran_amd.h states the rule to the bit): every present joint a disc, every connection a capsule,
# their radii a share of the skeleton's size by class.  Not the reference's: it draws stick figures only.
HEAD, TORSO, LIMB = 0, 1, 2
SILHOUETTE_JOINT_CLASS = np.array([HEAD, TORSO, TORSO, LIMB, LIMB, TORSO, LIMB, LIMB, TORSO, LIMB, LIMB, TORSO, LIMB, LIMB,
                                   HEAD, HEAD, HEAD, HEAD], np.int64)
SILHOUETTE_SEGMENTS = np.concatenate([POSE_CONNECTIONS, [(8, 11)]])           # the 17 connections and the hip line
SILHOUETTE_SEGMENT_CLASS = np.array([HEAD] * 5 + [TORSO, LIMB, LIMB, TORSO, LIMB, LIMB, TORSO, LIMB, LIMB, TORSO, LIMB, LIMB, TORSO], np.int64)
SILHOUETTE_COORD_LIMIT = 1 << 14                        # what ta_poses_paint accepts
POSE_COLORMAP = build_colormap()                        # module-global and stateful like FACE_COLORMAP: a track keeps its colour over calls


def _one_device(device, who):
    if isinstance(device, (list, tuple)):
        raise ValueError('`device`: %s does not offer fan-out over a device list yet; pass one device' % who)


def _permilles(head, torso, limb, min_radius):
    p = [int(round(float(v) * 1000)) for v in (head, torso, limb)]
    if not all(0 <= v <= 1000 for v in p):
        raise ValueError('head, torso and limb must be within 0 .. 1, got %r' % ((head, torso, limb),))
    if isinstance(min_radius, bool) or not isinstance(min_radius, (int, np.integer)) or not 0 <= min_radius <= 4096:
        raise ValueError('min_radius must be an int within 0 .. 4096, got %r' % (min_radius,))
    return p, int(min_radius)


def pack_silhouettes(poses_per_frame, colors=None, alpha=255):
    """-> (pose_counts (n_frames,) int32, keypoints (P, 18, 3) int32, rgba (P, 4) uint8), what `Context.poses_paint` takes:
    the skeletons frame by frame in list order, coordinates truncated as pack_poses truncates them, an absent joint as
    (0, 0, 0).  `colors`: None (white), one (r, g, b), one per pose ((P, 3)), or 'track': POSE_COLORMAP (a build_colormap()) of
    pose['pose_track'], else of pose['track'], else of the pose's index in its frame -- the same id gets the same colour in
    every frame and every later call.  `alpha`: 0 .. 255, one for all or one per pose.  Host only, no device."""
    per_frame = [_as_list(poses) for poses in poses_per_frame]
    k, _ = _keypoints(per_frame)
    present = k[..., 2] != 0
    xy = np.where(present[..., None], k[..., :2], 0.0)
    if not np.all(np.abs(xy) < SILHOUETTE_COORD_LIMIT):
        raise ValueError('keypoint coordinates must be finite and below 2^14 in size')
    kp = np.concatenate([np.trunc(xy).astype(np.int32), present[..., None].astype(np.int32)], -1)
    counts = np.array([len(poses) for poses in per_frame], np.int32)
    n = len(kp)
    rgba = np.empty((n, 4), np.uint8)
    if colors is None:
        rgba[:, :3] = 255
    elif isinstance(colors, str):
        if colors != 'track':
            raise ValueError("colors must be None, one (r, g, b), one per pose or 'track', got %r" % (colors,))
        at = 0
        for poses in per_frame:
            for i, pose in enumerate(poses):
                key = pose.get('pose_track')
                if key is None:
                    key = pose.get('track')
                rgba[at, :3] = POSE_COLORMAP(i if key is None else key)
                at += 1
    else:
        c = np.asarray(colors)
        if c.shape not in ((3,), (n, 3)) or c.dtype.kind not in 'iu' or c.size and (c.min() < 0 or c.max() > 255):
            raise ValueError("colors must be None, one (r, g, b), one per pose or 'track', got %r" % (colors,))
        rgba[:, :3] = c
    a = np.asarray(alpha)
    if a.shape not in ((), (n,)) or a.dtype.kind not in 'iu' or a.size and (a.min() < 0 or a.max() > 255):
        raise ValueError('alpha must be an int 0 .. 255, one for all or one per pose, got %r' % (alpha,))
    rgba[:, 3] = a
    return counts, kp, rgba


def pose_boxes(poses_per_frame, shapes, head=0.09, torso=0.09, limb=0.05, min_radius=2):
    """[(frame, pose, x0, y0, x1, y1)]: for every skeleton with a present joint the extent of its present joints widened by
    its largest radius (max(min_radius, size x share) per class, ta_poses_paint's) and clipped to its frame, as the
    half-open box [x0, x1) x [y0, y1) -- everything its silhouette can cover; empty ones left out.  `shapes`: pack_blur's.
    Host only."""
    permille, min_radius = _permilles(head, torso, limb, min_radius)
    counts, kp, _ = pack_silhouettes(poses_per_frame)
    sizes = _frame_sizes(shapes, len(counts))
    out, at = [], 0
    for f, n in enumerate(counts):
        h, w = int(sizes[f][0]), int(sizes[f][1])
        for i in range(int(n)):
            q = kp[at + i].astype(np.int64)
            at_joint = q[q[:, 2] != 0]
            if not len(at_joint):
                continue
            lo, hi = at_joint[:, :2].min(0), at_joint[:, :2].max(0)
            m = int((hi - lo).max())
            r = max(max(min_radius, m * p // 1000) for p in permille)
            x0, y0, x1, y1 = max(int(lo[0]) - r, 0), max(int(lo[1]) - r, 0), min(int(hi[0]) + r + 1, w), min(int(hi[1]) + r + 1, h)
            if x1 > x0 and y1 > y0:
                out.append((f, i, x0, y0, x1, y1))
        at += int(n)
    return out


def _per_batch(batches, poses_per_frame, who):
    """The result lists of each batch of a list of batches (frames counted through, as the tone callers count them)."""
    total = sum(b.shape[0] for b in batches)
    per_frame = list(poses_per_frame)
    if len(per_frame) > total:
        raise ValueError('%s: %d result lists for %d frames' % (who, len(per_frame), total))
    out, at = [], 0
    for b in batches:
        out.append(per_frame[at:at + b.shape[0]])
        at += b.shape[0]
    return out


def pose_masks(frames_or_shape, poses_per_frame, head=0.09, torso=0.09, limb=0.05, min_radius=2, ctx=None, device=None):
    """Mattes of the people: a NEW resident batch (a list of them for a list of batches) of the frames' size with 255 in all
    three bands where a skeleton's silhouette is and 0 elsewhere -- one allocation and one ta_poses_paint with clear=1.
    `image.composite_frames` and `image.paste_frames` take it as `mask`.  `frames_or_shape`: a lib.Frames batch, a list of
    them, or a shape (N, H, W[, 3]) (then `ctx`, or the context of `device`, owns the result).

    A silhouette is a disc at every present joint and a capsule along every connection (the 17 of POSE_CONNECTIONS and the
    hip line), of radius max(min_radius, share x size) with size the larger side of the present joints' extent.  The
    default shares come from geometry, not from tuning on data: a standing person is about eight heads tall, so a head's
    radius is about size / 16 and 0.09 x size covers it from the nose or an ear; the hip joints lie about size / 6 apart,
    so 0.09 x size closes the torso between the two neck-hip capsules; a thigh is about 0.05 x size in half-width."""
    who = 'pose_masks'
    _one_device(device, who)
    permille, min_radius = _permilles(head, torso, limb, min_radius)
    if isinstance(frames_or_shape, lib.Frames) or (isinstance(frames_or_shape, (list, tuple)) and frames_or_shape
                                                   and isinstance(frames_or_shape[0], lib.Frames)):
        batches, listed = image._batches(frames_or_shape, who)
        plans = [(ctx if ctx is not None else b.ctx, b.shape[:3]) for b in batches]
    else:
        try:
            n, h, w = (int(v) for v in tuple(frames_or_shape)[:3])
        except (TypeError, ValueError):
            raise ValueError('%s: a lib.Frames batch, a list of them or a shape (N, H, W[, 3]), got %r' % (who, frames_or_shape)) from None
        if ctx is None:
            from . import runtime
            ctx = runtime.get_context(device)
        plans, listed = [(ctx, (n, h, w))], False
    total = sum(s[0] for _, s in plans)
    per_frame = list(poses_per_frame)
    if len(per_frame) > total:
        raise ValueError('%s: %d result lists for %d frames' % (who, len(per_frame), total))
    packed, at = [], 0
    for _, (n, h, w) in plans:                              # everything is packed and checked before anything is allocated
        mine = per_frame[at:at + n]
        packed.append(pack_silhouettes(mine + [[]] * (n - len(mine))))
        at += n
    outs = []
    for (c, (n, h, w)), (counts, kp, rgba) in zip(plans, packed):
        out = lib.Frames.zeros(c, n, h, w)
        if n:
            c.poses_paint(out, counts, kp, rgba, permille, min_radius, clear=True)
        outs.append(out)
    return outs if listed else outs[0]


def paint_poses(frames, poses_per_frame, colors='track', alpha=128, head=0.09, torso=0.09, limb=0.05, min_radius=2, ctx=None,
                device=None):
    """Paint every skeleton's silhouette into the resident batch `frames` (a lib.Frames, or a list of them) in place, one
    list of poses per frame: translucent people, by default coloured by track (pose['pose_track'] as `PoseTracker` writes
    it; pack_silhouettes' `colors` and `alpha`).  A pixel is blended once per person that covers it, however many of that
    person's limbs do; people of one frame in list order.  The shape: pose_masks'."""
    who = 'paint_poses'
    _one_device(device, who)
    permille, min_radius = _permilles(head, torso, limb, min_radius)
    batches, _ = image._batches(frames, who)
    per_batch = _per_batch(batches, poses_per_frame, who)
    if not isinstance(colors, str) and colors is not None and np.ndim(colors) == 2:
        colors, at, each = np.asarray(colors), 0, []       # one per pose: cut as the poses are
        for mine in per_batch:
            n = sum(len(_as_list(p)) for p in mine)
            each.append(colors[at:at + n])
            at += n
        packed = [pack_silhouettes(mine, c, alpha) for mine, c in zip(per_batch, each)]
    else:
        packed = [pack_silhouettes(mine, colors, alpha) for mine in per_batch]
    for b, (counts, kp, rgba) in zip(batches, packed):
        if len(kp):
            (ctx if ctx is not None else b.ctx).poses_paint(b, counts, kp, rgba, permille, min_radius)
    return frames


def pack_pose_blur(poses_per_frame, shapes, radius=None, method='gaussian', block=None, head=0.09, torso=0.09, limb=0.05,
                   min_radius=2):
    """-> (regions, pixelate?) for blur_poses: pose_boxes' boxes as lib.BLUR_DT records (`radius`: GaussianBlur's, None:
    max(w, h) / 8 of the box, blur_faces' rule) or lib.PIXELATE_DT records (`block`: None: max(1, max(w, h) // 8)), shape
    'box'.  Every argument is checked here.  Host only."""
    if method not in BLUR_METHODS:
        raise ValueError("method must be 'gaussian' or 'pixelate', got %r" % (method,))
    pixelate = method == 'pixelate'
    if pixelate:
        if radius is not None:
            raise ValueError("radius belongs to method='gaussian'; method='pixelate' takes block")
        if block is not None and (isinstance(block, bool) or not isinstance(block, (int, np.integer))
                                  or not 1 <= block <= lib.RESAMPLE_SIDE_LIMIT):
            raise ValueError('block must be an int within 1 .. %d, got %r' % (lib.RESAMPLE_SIDE_LIMIT, block))
    else:
        if block is not None:
            raise ValueError("block belongs to method='pixelate'; method='gaussian' takes radius")
        if radius is not None and not 0 <= float(radius) <= BLUR_RADIUS_LIMIT:
            raise ValueError('radius must be within 0 .. %g, got %r' % (BLUR_RADIUS_LIMIT, radius))
    rows = []
    for f, _, x0, y0, x1, y1 in pose_boxes(poses_per_frame, shapes, head, torso, limb, min_radius):
        if pixelate:
            v = max(1, max(x1 - x0, y1 - y0) // 8) if block is None else int(block)
            rows.append((f, x0, y0, x1, y1, lib.BLUR_BOX, min(v, lib.RESAMPLE_SIDE_LIMIT)))
        else:
            v = max(x1 - x0, y1 - y0) / 8 if radius is None else float(radius)
            rows.append((f, x0, y0, x1, y1, lib.BLUR_BOX, min(v, BLUR_RADIUS_LIMIT)))
    return np.array(rows, lib.PIXELATE_DT if pixelate else lib.BLUR_DT), pixelate


def _free(batches):
    for b in batches:
        b.free()


def blur_poses(frames, poses_per_frame, radius=None, method='gaussian', block=None, head=0.09, torso=0.09, limb=0.05,
               min_radius=2, ctx=None, device=None):
    """Make whole people unrecognisable in the resident batch `frames` (a lib.Frames, or a list of them) in place: clothes,
    tattoos and build go with the face.  A copy of the frames (`image.copy_frames`) is blurred -- or with
    method='pixelate' turned into a mosaic -- over every skeleton's box (pose_boxes; in list order, `radius` / `block` as
    blur_faces takes them), and the copy is pasted back under the people's matte (`pose_masks`) in one whole-frame
    `image.composite_frames`: outside the silhouettes no pixel changes.  The shape: pose_masks'."""
    who = 'blur_poses'
    _one_device(device, who)
    batches, _ = image._batches(frames, who)
    per_batch = _per_batch(batches, poses_per_frame, who)
    plans = [pack_pose_blur(mine, b.shape, radius, method, block, head, torso, limb, min_radius) for b, mine in zip(batches, per_batch)]
    for b, mine, (regions, pixelate) in zip(batches, per_batch, plans):
        if not len(regions):
            continue
        c = ctx if ctx is not None else b.ctx
        copy = image.copy_frames(b, ctx=c)
        matte = None
        try:
            if pixelate:
                copy.pixelate(regions, ctx=c)
            else:
                copy.blur(regions, ctx=c)
            matte = pose_masks(b, mine, head, torso, limb, min_radius, ctx=c)
            image.composite_frames(b, copy, matte, ctx=c)
        finally:
            _free([copy] + ([matte] if matte is not None else []))
    return frames


def spotlight_poses(frames, poses_per_frame, dim=0.4, head=0.09, torso=0.09, limb=0.05, min_radius=2, ctx=None, device=None):
    """Darken everything but the people of the resident batch `frames` (a lib.Frames, or a list of them) in place:
    `image.brightness_frames(frames, dim)`, then the original pixels pasted back under the people's matte (`pose_masks`)."""
    who = 'spotlight_poses'
    _one_device(device, who)
    _permilles(head, torso, limb, min_radius)
    lut = image.brightness_lut(dim)
    batches, _ = image._batches(frames, who)
    per_batch = _per_batch(batches, poses_per_frame, who)
    for mine in per_batch:
        pack_silhouettes(mine)                              # checked before anything is launched
    for b, mine in zip(batches, per_batch):
        c = ctx if ctx is not None else b.ctx
        copy = image.copy_frames(b, ctx=c)
        matte = None
        try:
            image.point_frames(b, lut, ctx=c)
            matte = pose_masks(b, mine, head, torso, limb, min_radius, ctx=c)
            image.composite_frames(b, copy, matte, ctx=c)
        finally:
            _free([copy] + ([matte] if matte is not None else []))
    return frames


def anonymize_poses(image, poses, radius=None, method='gaussian', block=None, head=0.09, torso=0.09, limb=0.05, min_radius=2,
                    device=None):
    """A copy of the host image (uint8 (H, W, 3)) with every person (dict or list of dicts, as pose_estimation returns them)
    blurred: `blur_poses` of the uploaded image, as anonymize_faces is to blur_faces."""
    from . import runtime
    _one_device(device, 'anonymize_poses')
    image = np.asarray(image)
    if image.dtype != np.uint8 or image.ndim != 3 or image.shape[2] != 3:
        raise ValueError('expected a uint8 (H, W, 3) RGB image, got %s %s' % (image.dtype, image.shape))
    pack_pose_blur([poses], image.shape[:2], radius, method, block, head, torso, limb, min_radius)
    frames = runtime.get_context(device).upload(image[None])
    try:
        return blur_poses(frames, [poses], radius, method, block, head, torso, limb, min_radius).download()[0]
    finally:
        frames.free()


def anonymize_faces(image, faces, radius=None, margin=0.0, shape='box', method='gaussian', block=None):
    """A copy of the host image (uint8 (H, W, 3)) with every face (dict or list of dicts, face_tracking's included)
    blurred: Pillow's crop / GaussianBlur(radius) / paste of each box, or with method='pixelate' its crop / resize(BOX) /
    resize(NEAREST) / paste (`block`: blur_faces')."""
    image = np.asarray(image)
    regions, pixelate = _pack_anonymize([faces], image.shape[:2], radius, margin, shape, method, block)
    return _on_host_image(image, regions, blur='pixelate' if pixelate else True)


def _on_host_image(image, prims, masks=None, device=None, blur=False):
    from . import runtime
    image = np.asarray(image)
    if image.dtype != np.uint8 or image.ndim != 3 or image.shape[2] != 3:
        raise ValueError('expected a uint8 (H, W, 3) RGB image, got %s %s' % (image.dtype, image.shape))
    ctx = runtime.get_context(device)
    frames = ctx.upload(image[None])
    try:
        if blur == 'pixelate':
            frames.pixelate(prims)
        elif blur:
            frames.blur(prims)
        else:
            frames.draw(prims, masks)
        return frames.download()[0]
    finally:
        frames.free()


def vis_faces(image, faces, scale=1.0, labels=False):
    """terran.vis.vis_faces: a copy of `image` with a box drawn over every face (dict or list of dicts), and with
    `labels` the face's `text`, or '#<track>', on a tab at the box's corner."""
    if labels:
        return _on_host_image(image, *pack_faces([faces], scale, labels=True))
    return _on_host_image(image, pack_faces([faces], scale))


def vis_poses(image, poses, scale=1.0):
    """terran.vis.vis_poses: a copy of `image` with the limbs and keypoints of every pose (dict or list of dicts)."""
    return _on_host_image(image, pack_poses([poses], scale))
