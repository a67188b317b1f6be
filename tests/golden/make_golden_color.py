"""Generate tests/golden/color.npz with Pillow alone: the contract of ta_frames_color and of the colour callers of
terran_amd.image and terran_amd.vis.color_faces.

Stored: noise sources (frames of every width 1, 3, 5, 53, 64, 257 and height 1, 2, 37, a batch of three 37 x 53 frames, one
20 x 31 frame), the case lists (regions as rows (frame, x0, y0, x1, y1, shape, op), ops as rows (kind, s0, s1, s2, first
float of its table), the float32 tables -- but not those of 3-D table ops, which are color_model.formula_lut of the op's
size one after the other --) and what Pillow returns for them:

    matrix            im.paste(im.crop(box).convert('RGB', m), box[, mask])
    ycbcr, hsv        ... crop.convert('YCbCr' | 'HSV'), its three bands kept as the frame's three bytes
    rgb_from_*        ... Image.frombytes('YCbCr' | 'HSV', size, the crop's bytes).convert('RGB')
    lut               ... crop.filter(ImageFilter.Color3DLUT(size, table))
    mask              ImageDraw.Draw(Image.new('L', (w, h))).ellipse([0, 0, w - 1, h - 1], fill=255)

For the exhaustive cases only the SHA-256 of Pillow's output bytes over the frame of all 2^24 colours (pixel k = y * 4096 +
x is (k & 255, k >> 8 & 255, k >> 16)): per conversion, for the two matrices and for the 17^3 and 33^3 formula tables.
Only tests/color_model.py's constants, its all-colours frame and its table formula are imported here, none of its
arithmetic.

    python tests/golden/make_golden_color.py
"""
import hashlib
import os
import sys

import numpy as np
import PIL
from PIL import Image, ImageDraw, ImageFilter

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
from tests import color_model as M      # noqa: E402  (constants, all_colours and formula_lut only)

WIDTHS, HEIGHTS = [1, 3, 5, 53, 64, 257], [1, 2, 37]
BOX, ELLIPSE = 0, 1
LUT_SIZES = [(2, 2, 2), (3, 5, 7), (17, 17, 17), (33, 33, 33), (65, 65, 65)]


def mask_image(w, h):
    m = Image.new('L', (w, h))
    ImageDraw.Draw(m).ellipse([0, 0, w - 1, h - 1], fill=255)
    return m


def as_rgb(im):
    """The three bands of a 'YCbCr' or 'HSV' image as the bytes of an 'RGB' one: what a mode-less batch holds."""
    return Image.frombytes('RGB', im.size, im.tobytes())


def pil_op(crop, op, tables):
    kind, s0, s1, s2, at = (int(v) for v in op)
    if kind == M.MATRIX:
        return crop.convert('RGB', tuple(float(v) for v in tables[at:at + 12]))
    if kind == M.RGB2YCBCR:
        return as_rgb(crop.convert('YCbCr'))
    if kind == M.RGB2HSV:
        return as_rgb(crop.convert('HSV'))
    if kind == M.YCBCR2RGB:
        return Image.frombytes('YCbCr', crop.size, crop.tobytes()).convert('RGB')
    if kind == M.HSV2RGB:
        return Image.frombytes('HSV', crop.size, crop.tobytes()).convert('RGB')
    return crop.filter(ImageFilter.Color3DLUT((s0, s1, s2), [float(v) for v in tables[at:at + 3 * s0 * s1 * s2]]))


def pil_apply(frames, regions, ops, tables):
    """regions: rows (frame, x0, y0, x1, y1, shape, op), in list order, in place."""
    ims = [Image.fromarray(f) for f in frames]
    for row in regions:
        f, x0, y0, x1, y1, shape, op = (int(v) for v in row)
        box = (x0, y0, x1, y1)
        out = pil_op(ims[f].crop(box), ops[op], tables)
        if shape == ELLIPSE:
            ims[f].paste(out, box, mask_image(x1 - x0, y1 - y0))
        else:
            ims[f].paste(out, box)
    return np.stack([np.asarray(im) for im in ims])


def std_regions(h, w):
    """tone.npz's: the whole frame, single pixels, rows and columns, boxes at even and odd x0, both shapes."""
    rows = [(0, 0, 0, w, h, BOX), (0, w - 1, h - 1, w, h, BOX), (0, 0, h // 2, w, h // 2 + 1, BOX),
            (0, w // 2, 0, w // 2 + 1, h, BOX), (0, w // 3, h // 3, w, h, BOX), (0, 0, 0, w, h, ELLIPSE)]
    if w > 1:
        rows += [(0, 1, 0, w, h, BOX), (0, 1, 0, w, h, ELLIPSE)]
    if w > 6 and h > 2:
        rows += [(0, 3, 1, w - 2, h - 1, BOX), (0, 3, 1, w - 2, h - 1, ELLIPSE)]
    return rows


def op_list(entries):
    """entries: kind, or (kind, 12 floats), or (LUT3D, size) -> (int32 (n, 5) ops, float32 tables)."""
    ops, tables = [], []
    for e in entries:
        at = sum(len(t) for t in tables)
        if isinstance(e, int):
            ops.append((e, 0, 0, 0, 0))
        elif e[0] == M.MATRIX:
            ops.append((M.MATRIX, 0, 0, 0, at))
            tables.append(np.asarray(e[1], np.float32))
        else:
            ops.append((M.LUT3D,) + tuple(e[1]) + (at,))
            tables.append(M.formula_lut(e[1]))
    return np.array(ops, np.int32), np.concatenate(tables) if tables else np.zeros(0, np.float32)


def digest(a):
    return hashlib.sha256(np.ascontiguousarray(a, np.uint8).tobytes()).hexdigest()


def main():
    rng = np.random.default_rng(20261020)
    out = {'pillow_version': np.array(PIL.__version__)}
    batch = rng.integers(0, 256, (3, 37, 53, 3), dtype=np.uint8)
    small = rng.integers(0, 256, (20, 31, 3), dtype=np.uint8)
    out['batch'], out['small'] = batch, small
    H, W = 37, 53

    def case(name, frames, rows, ops, tables, source=None):
        rows = np.array(rows, np.int32)
        out[source or '%s_source' % name] = frames
        out['%s_regions' % name], out['%s_ops' % name] = rows, ops
        if not (ops[:, 0] == M.LUT3D).any():                  # the tables of 3-D ops are formula_lut's: color_model.case_tables
            out['%s_tables' % name] = tables
        out['%s_expected' % name] = pil_apply(frames, rows, ops, tables)

    # ---- the walk: every op kind over every width and height, std_regions of each ----
    kinds = [('matrix', (M.MATRIX, M.WILD)), ('ycbcr', M.RGB2YCBCR), ('rgb_from_ycbcr', M.YCBCR2RGB), ('hsv', M.RGB2HSV),
             ('rgb_from_hsv', M.HSV2RGB), ('lut', (M.LUT3D, (3, 5, 7)))]
    out['walk_kinds'] = np.array([k[0] for k in kinds])
    out['walk_sizes'] = np.array([(h, w) for h in HEIGHTS for w in WIDTHS], np.int32)
    for h, w in out['walk_sizes']:
        noise = rng.integers(0, 256, (1, h, w, 3), dtype=np.uint8)
        for name, entry in kinds:
            ops, tables = op_list([entry])
            case('walk_%s_%dx%d' % (name, h, w), noise, [r + (0,) for r in std_regions(int(h), int(w))], ops, tables, 'walk_source_%dx%d' % (h, w))

    # ---- 3-D tables of every size: whole frames, a box at odd x0, an ellipse; the five tables in one call ----
    ops, tables = op_list([(M.LUT3D, s) for s in LUT_SIZES])
    rows = [(k % 3, 0, 0, W, H, BOX, k) for k in range(5)] + [(1, 7, 3, 50, 30, BOX, 3), (2, 2, 1, 53, 36, ELLIPSE, 4), (0, 5, 5, 21, 30, ELLIPSE, 2)]
    case('lut_sizes', batch, rows, ops, tables)

    # ---- order: overlapping regions of one frame with ops that do not commute, frames out of order, a box twice ----
    ops, tables = op_list([M.RGB2YCBCR, (M.MATRIX, M.SEPIA), M.RGB2HSV])
    a, b = (4, 3, 36, 28, BOX), (21, 15, 53, 37, BOX)
    case('order_ycbcr_then_matrix', batch, [(2,) + a + (0,), (0,) + a + (0,), (2,) + b + (1,), (0,) + b + (1,), (1, 0, 0, W, H, ELLIPSE, 2),
                                            (0,) + a + (0,)], ops, tables)
    case('order_matrix_then_ycbcr', batch, [(2,) + a + (1,), (0,) + a + (1,), (2,) + b + (0,), (0,) + b + (0,), (1, 0, 0, W, H, ELLIPSE, 2),
                                            (0,) + a + (1,)], ops, tables)
    assert not np.array_equal(out['order_ycbcr_then_matrix_expected'], out['order_matrix_then_ycbcr_expected'])
    out['order_names'] = np.array(['order_ycbcr_then_matrix', 'order_matrix_then_ycbcr'])

    # ---- callers: a mixed-size list, two 37 x 53 frames and one 20 x 31 frame ----
    parts = {'a': batch[:2], 'b': small[None]}
    shift = 77
    hue_table = [(i + shift) % 256 for i in range(256)] + list(range(256)) * 2
    lut17 = ImageFilter.Color3DLUT(17, [float(v) for v in M.formula_lut((17, 17, 17))])

    def hue(im):
        hsv = im.convert('HSV').point(hue_table)
        return hsv.convert('RGB')
    calls = [('hue', hue), ('ycbcr', lambda im: as_rgb(im.convert('YCbCr'))), ('hsv', lambda im: as_rgb(im.convert('HSV'))),
             ('matrix', lambda im: im.convert('RGB', M.SEPIA)), ('lut', lambda im: im.filter(lut17)),
             ('round_trip', lambda im: im.convert('YCbCr').convert('RGB'))]
    out['call_names'], out['call_hue_shift'] = np.array([c[0] for c in calls]), np.array(shift)
    for name, fn in calls:
        for key, frames in parts.items():
            out['call_%s_%s' % (name, key)] = np.stack([np.asarray(fn(Image.fromarray(f))) for f in frames])
    boxes = [(3, 2, 41, 30), (0, 0, 53, 1), (30, 19, 31, 20)]
    out['call_boxes'] = np.array(boxes, np.int32)
    listed = [f for frames in parts.values() for f in frames]
    boxed = []
    for f, box in zip(listed, boxes):
        im = Image.fromarray(f)
        im.paste(im.crop(box).convert('RGB', M.WILD), box, mask_image(box[2] - box[0], box[3] - box[1]))
        boxed.append(np.asarray(im))
    out['call_boxed_matrix_a'], out['call_boxed_matrix_b'] = np.stack(boxed[:2]), boxed[2][None]

    # ---- faces: blur_faces' boxes with a margin that leaves the frame ----
    faces = [[[10.2, 5.5, 30.9, 28.1], [40.0, 20.0, 52.0, 36.5]], [], [[-4.0, -3.0, 9.5, 8.0], [20.0, 30.0, 21.0, 31.0], [60.0, 5.0, 70.0, 9.0]]]
    margin = 0.25
    out['face_bboxes'] = np.array([b for f in faces for b in f], np.float64)
    out['face_frames'] = np.array([i for i, f in enumerate(faces) for _ in f], np.int32)
    out['face_margin'] = np.array(margin)
    for shape in ('box', 'ellipse'):
        rows = []
        for i, per in enumerate(faces):
            for x0, y0, x1, y1 in per:
                dx, dy = margin * (x1 - x0), margin * (y1 - y0)
                x0, y0, x1, y1 = max(int(x0 - dx), 0), max(int(y0 - dy), 0), min(int(x1 + dx), W), min(int(y1 + dy), H)
                if x1 > x0 and y1 > y0:
                    rows.append((i, x0, y0, x1, y1, ELLIPSE if shape == 'ellipse' else BOX, 0))
        ops, tables = op_list([(M.MATRIX, M.SEPIA)])
        out['face_%s_expected' % shape] = pil_apply(batch, rows, ops, tables)

    # ---- every colour: digests of Pillow's bytes ----
    allc = M.all_colours()
    im = Image.fromarray(allc)
    raw = lambda mode: Image.frombytes(mode, im.size, allc.tobytes())      # noqa: E731
    digests = {'ycbcr': im.convert('YCbCr'), 'rgb_from_ycbcr': raw('YCbCr').convert('RGB'), 'hsv': im.convert('HSV'),
               'rgb_from_hsv': raw('HSV').convert('RGB'), 'matrix_sepia': im.convert('RGB', M.SEPIA), 'matrix_wild': im.convert('RGB', M.WILD)}
    for s in (17, 33):
        digests['lut_%d' % s] = im.filter(ImageFilter.Color3DLUT(s, [float(v) for v in M.formula_lut((s, s, s))]))
    out['digest_names'] = np.array(sorted(digests))
    for name, res in digests.items():
        out['digest_' + name] = np.array(digest(np.asarray(res)))
        print('%-16s %s' % (name, out['digest_' + name]))
    wild = np.asarray(digests['matrix_wild'])
    assert (wild == 0).any() and (wild == 255).any()                      # clips at both ends
    for s in (17, 33):
        t = M.formula_lut((s, s, s))
        assert t.min() < 0 and t.max() > 32767 / 16320.0                  # below 0, above 1 and into int16 saturation

    path = os.path.join(HERE, 'color.npz')
    np.savez_compressed(path, **out)
    print('%s: %d arrays, %d bytes, Pillow %s' % (path, len(out), os.path.getsize(path), PIL.__version__))


if __name__ == '__main__':
    main()
