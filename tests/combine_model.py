"""The contract of ta_frames_combine and of the two-image callers of terran_amd.image / terran_amd.vis restated in numpy
(no Pillow, no GPU), sample by sample as Pillow 12 computes them (libImaging/Paste.c, Blend.c, Chops.c):

    paste under an 'L' mask m   t = a (255 - m) + b m + 128; ((t >> 8) + t) >> 8         (one division by 255, not two)
    Image.blend(a, b, f)        tests/tone_model.blend: float32 a + f (b - a), a multiply and an add
    lighter, darker, difference max, min, |a - b|
    multiply, screen            a b / 255,  255 - (255 - a) (255 - b) / 255
    add, subtract               float32 (a +- b) / scale + offset, a correctly rounded division and an addition; the float
                                is truncated to int, then clipped to 0 .. 255
    add_modulo, subtract_modulo (a +- b) mod 256
    soft_light                  (255 - a) (a b) / 65536 + a (255 - (255 - a) (255 - b) / 255) / 255, mod 256
    hard_light                  b < 128 ? a b / 127 : 255 - (255 - b) (255 - a) / 127, mod 256;  overlay: a < 128 decides

Regions are lib.COMBINE_DT arrays: per region a = dst.crop(box), b = the equally sized box of `src`, the result pasted
back in list order under ImageDraw.ellipse's coverage of the box for shape 1.  Also the wrong arithmetic a kernel could
fall into (two divisions in paste, a reciprocal multiply in add, a fused multiply-add in blend), the walk of a row as
csrc/pixel_walk.h cuts it, the sources the golden does not store and the loader of tests/golden/combine.npz."""
import os

import numpy as np

from tests import tone_model as T

f32 = np.float32
BOX, ELLIPSE = 0, 1
(PASTE, BLEND, LIGHTER, DARKER, DIFFERENCE, MULTIPLY, SCREEN, ADD, SUBTRACT, ADD_MODULO, SUBTRACT_MODULO, SOFT_LIGHT, HARD_LIGHT,
 OVERLAY) = range(14)
OP_NAMES = ['paste', 'blend', 'lighter', 'darker', 'difference', 'multiply', 'screen', 'add', 'subtract', 'add_modulo',
            'subtract_modulo', 'soft_light', 'hard_light', 'overlay']
MASK_NONE, MASK_CONSTANT, MASK_BITMAP, MASK_FRAMES = range(4)
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'combine.npz')
# the columns of a golden's int32 region rows; `alpha` travels beside them as float32
COLUMNS = ('frame', 'x0', 'y0', 'x1', 'y1', 'shape', 'src_frame', 'src_x', 'src_y', 'op', 'offset', 'mask_kind', 'mask_value',
           'mask_frame', 'mask_x', 'mask_y', 'mask_band')


# ---- samples -----------------------------------------------------------------------------------------------------------
def paste_mask(a, b, m):
    t = a.astype(np.int64) * (255 - m) + b.astype(np.int64) * m + 128
    return (((t >> 8) + t) >> 8).astype(np.uint8)


def paste_two_divisions(a, b, m):
    """The wrong one: MULDIV255(a, 255 - m) + MULDIV255(b, m)."""
    def muldiv(x, y):
        t = x.astype(np.int64) * y + 128
        return ((t >> 8) + t) >> 8
    return (muldiv(a, 255 - m) + muldiv(b, m)).astype(np.uint8)


def _clip_trunc(t):
    """A float32 array as C's (int), then CHOP's clip; a quotient beyond int's range saturates (Pillow: undefined)."""
    return np.clip(np.trunc(t.astype(np.float64)), 0, 255).astype(np.uint8)


def add(a, b, scale=1.0, offset=0, sign=1, reciprocal=False):
    """ImageChops.add (sign 1) / subtract (sign -1); `reciprocal`: the wrong one, a multiply by float32 1 / scale."""
    s = a.astype(np.int32) + sign * b.astype(np.int32)
    if reciprocal:
        q = s.astype(f32) * (f32(1) / f32(scale))
    else:
        q = s.astype(f32) / f32(scale)
    t = q + f32(offset)
    assert q.dtype == f32 and t.dtype == f32
    return _clip_trunc(t)


def chop(op, a, b, alpha=0.0, offset=0):
    """R of a region without a mask: uint8 arrays of one shape."""
    if op == PASTE:
        return b.copy()
    if op == BLEND:
        return T.blend(a, b, alpha)
    if op == ADD:
        return add(a, b, alpha, offset)
    if op == SUBTRACT:
        return add(a, b, alpha, offset, sign=-1)
    x, y = a.astype(np.int64), b.astype(np.int64)
    if op == LIGHTER:
        r = np.maximum(x, y)
    elif op == DARKER:
        r = np.minimum(x, y)
    elif op == DIFFERENCE:
        r = np.abs(x - y)
    elif op == MULTIPLY:
        r = x * y // 255
    elif op == SCREEN:
        r = 255 - (255 - x) * (255 - y) // 255
    elif op == ADD_MODULO:
        r = x + y
    elif op == SUBTRACT_MODULO:
        r = x - y
    elif op == SOFT_LIGHT:
        r = ((255 - x) * (x * y)) // 65536 + (x * (255 - ((255 - x) * (255 - y) // 255))) // 255
    elif op == HARD_LIGHT:
        r = np.where(y < 128, x * y // 127, 255 - (255 - y) * (255 - x) // 127)
    elif op == OVERLAY:
        r = np.where(x < 128, x * y // 127, 255 - (255 - x) * (255 - y) // 127)
    else:
        raise ValueError(op)
    return (r & 255).astype(np.uint8)


# ---- regions -----------------------------------------------------------------------------------------------------------
def region_mask(q, masks, mask_frames):
    """The 'L' mask of a PASTE region as an (h, w) uint8 array, or None."""
    w, h = int(q['x1'] - q['x0']), int(q['y1'] - q['y0'])
    kind = int(q['mask_kind'])
    if kind == MASK_NONE:
        return None
    if kind == MASK_CONSTANT:
        return np.full((h, w), int(q['mask_value']), np.uint8)
    if kind == MASK_BITMAP:
        at = int(q['mask_value'])
        return np.asarray(masks, np.uint8).reshape(-1)[at:at + w * h].reshape(h, w)
    mx, my = int(q['mask_x']), int(q['mask_y'])
    return mask_frames[q['mask_frame']][my:my + h, mx:mx + w, int(q['mask_band'])]


def combine_regions(dst, src, regions, masks=None, mask_frames=None, paste=paste_mask, blend=None, add_reciprocal=False, seen=None):
    """Apply a lib.COMBINE_DT array to the host frames `dst` (N, H, W, 3) in place, in list order; `src`, `mask_frames`:
    host batches of any size.  `paste`, `blend`, `add_reciprocal` swap in the wrong arithmetic; `seen` collects (a, b,
    region) as every region meets them."""
    for q in regions:
        w, h = int(q['x1'] - q['x0']), int(q['y1'] - q['y0'])
        crop = dst[q['frame']][q['y0']:q['y1'], q['x0']:q['x1']]
        b = src[q['src_frame']][q['src_y']:q['src_y'] + h, q['src_x']:q['src_x'] + w]
        assert crop.shape == b.shape == (h, w, 3), (crop.shape, b.shape)
        op, m = int(q['op']), region_mask(q, masks, mask_frames)
        if seen is not None:
            seen.append((crop.copy(), b.copy(), q))
        if m is not None:
            assert op == PASTE and m.shape == (h, w)
            out = paste(crop, b, m[..., None].astype(np.int64))
        elif op == BLEND and blend is not None:
            out = blend(crop, b, q['alpha'])
        elif op in (ADD, SUBTRACT) and add_reciprocal:
            out = add(crop, b, q['alpha'], int(q['offset']), 1 if op == ADD else -1, reciprocal=True)
        else:
            out = chop(op, crop, b, q['alpha'], int(q['offset']))
        cover = T.mask_of(h, w, int(q['shape']))
        crop[cover] = out[cover]
    return dst


def records(dt, rows, alpha):
    """The golden's int32 rows (COLUMNS) and float32 alphas as a record array of dtype `dt` (lib.COMBINE_DT)."""
    q = np.zeros(len(rows), dt)
    for k, name in enumerate(COLUMNS):
        q[name] = rows[:, k] if len(rows) else 0
    q['alpha'] = alpha
    return q


def wrong_counts(seen):
    """Pixels of the regions in `seen` that the wrong arithmetic would change -> (paste under a constant mask as two
    divisions, add / subtract with a reciprocal multiply, blend with a fused multiply-add)."""
    two = recip = fma = 0
    for a, b, q in seen:
        op = int(q['op'])
        if op == PASTE and q['mask_kind'] == MASK_CONSTANT:
            m = np.int64(q['mask_value'])
            two += int((paste_mask(a, b, m) != paste_two_divisions(a, b, m)).any(-1).sum())
        elif op in (ADD, SUBTRACT):
            sign = 1 if op == ADD else -1
            wrong = add(a, b, q['alpha'], int(q['offset']), sign, reciprocal=True)
            recip += int((add(a, b, q['alpha'], int(q['offset']), sign) != wrong).any(-1).sum())
        elif op == BLEND:
            fma += int((T.blend(a, b, q['alpha']) != T.blend_fused(a, b, q['alpha'])).any(-1).sum())
    return two, recip, fma


MODEL_DT = np.dtype([(name, '<i4') for name in COLUMNS] + [('alpha', '<f4')])


# ---- the walk of a destination row (csrc/pixel_walk.h) -------------------------------------------------------------------
def row_units(address, npx):
    """(head, groups, tail): single pixels up to the first one on a 4-byte boundary, groups of four, single pixels."""
    head = min(npx, address & 3)
    groups = (npx - head) >> 2
    return head, groups, npx - head - 4 * groups


def grouped_rows(q, dst_shape, src_shape, mask_shape=None):
    """For every row of a BOX region whose walk has a group: (dst address mod 4, src address mod 4, mask address mod 4 or
    None, the last unit is a group, the byte behind the row's last source pixel).  The bitmaps start on a 16-byte boundary."""
    _, H, W, _ = dst_shape
    _, sh, sw, _ = src_shape
    out = []
    w = int(q['x1'] - q['x0'])
    for r in range(int(q['y1'] - q['y0'])):
        d = ((int(q['frame']) * H + int(q['y0']) + r) * W + int(q['x0'])) * 3
        s = ((int(q['src_frame']) * sh + int(q['src_y']) + r) * sw + int(q['src_x'])) * 3
        head, groups, tail = row_units(d, w)
        if not groups:
            continue
        m = None
        if q['mask_kind'] == MASK_BITMAP:
            m = (int(q['mask_value']) + r * w + head) & 3
        elif q['mask_kind'] == MASK_FRAMES:
            _, mh, mw, _ = mask_shape
            m = (((int(q['mask_frame']) * mh + int(q['mask_y']) + r) * mw + int(q['mask_x']) + head) * 3) & 3
        out.append((d & 3, (s + 3 * head) & 3, m, tail == 0, s + 3 * w))
    return out


# ---- sources the golden does not store ---------------------------------------------------------------------------------
def ramp_pair():
    """Two (1, 4, 511, 3) frames: row 0 holds every sum 0 .. 510 of a sample of the first and one of the second, row 1 every
    difference -255 .. 255, rows 2 and 3 mixed values."""
    k = np.arange(511)
    a, b = np.zeros((4, 511, 3), np.int64), np.zeros((4, 511, 3), np.int64)
    a[0], b[0] = np.minimum(k, 255)[:, None], (k - np.minimum(k, 255))[:, None]
    a[1], b[1] = np.maximum(k - 255, 0)[:, None], np.maximum(255 - k, 0)[:, None]
    for y in (2, 3):
        for c in range(3):
            a[y, :, c], b[y, :, c] = (k * 7 + 31 * c + 5 * y) % 256, (k * 13 + 17 * c + 101 * y) % 256
    return a.astype(np.uint8)[None], b.astype(np.uint8)[None]


def matte(n, h, w):
    """A soft matte as an RGB batch: band c of frame f ramps across the frame, with true 0 and 255 stretches."""
    y, x = np.mgrid[:h, :w]
    bands = [np.clip((x * 9 + y * 5 + 40 * c) % 384 - 64, 0, 255) for c in range(3)]
    one = np.stack(bands, -1)
    return np.stack([np.roll(one, 7 * f, 1) for f in range(n)]).astype(np.uint8)


# ---- the layout of vis.inset_chips --------------------------------------------------------------------------------------
def inset_layout(index, chip_h, chip_w, frame_h, frame_w, origin=(8, 8), gap=4):
    """[(chip, frame, x, y)]: each frame's chips in a row from `origin`, `gap` apart, a new row at the frame's right edge;
    a chip that no longer fits is left out."""
    out, at = [], {}
    for k, (f, _) in enumerate(np.asarray(index).reshape(-1, 2)):
        x, y = at.get(int(f), (int(origin[0]), int(origin[1])))
        if x + chip_w > frame_w and x != origin[0]:
            x, y = int(origin[0]), y + chip_h + gap
        if x + chip_w > frame_w or y + chip_h > frame_h:
            at[int(f)] = (x, y)
            continue
        out.append((k, int(f), x, y))
        at[int(f)] = (x + chip_w + gap, y)
    return out


# ---- tests/golden/combine.npz -------------------------------------------------------------------------------------------
_golden = None


def golden():
    """The recorded Pillow results, loaded once and shared (read-only arrays): a dict of everything in the file."""
    global _golden
    if _golden is None:
        with np.load(GOLDEN) as z:
            _golden = {k: z[k] for k in z.files}
        for v in _golden.values():
            v.setflags(write=False)
    return _golden


def case(g, name):
    """A combine case of the golden -> dict(dst, src, mask_frames or None, rows, alpha, masks or None, expected).  A batch
    is stored under the case's own key or named in '<case>_<role>_name': another stored array, 'ramp_a' / 'ramp_b', or
    'dst' (the source is the destination batch itself)."""
    def batch(role):
        key = 'case_%s_%s' % (name, role)
        if key in g:
            return g[key]
        if key + '_name' not in g:
            return None
        ref = str(g[key + '_name'])
        if ref in ('ramp_a', 'ramp_b'):
            return ramp_pair()[ref == 'ramp_b']
        if ref.startswith('matte_'):
            return matte(*(int(v) for v in ref.split('_')[1].split('x')))
        return ref if ref == 'dst' else g[ref]
    out = {role: batch(role) for role in ('dst', 'src', 'mask_frames')}
    out['rows'], out['alpha'] = g['case_%s_rows' % name], g['case_%s_alpha' % name]
    out['masks'] = g.get('case_%s_masks' % name)
    out['expected'] = g['case_%s_expected' % name]
    return out


def coverage(g):
    """What the golden's cases reach, derived from their regions and batch shapes: the (destination, source) addresses mod 4
    of rows with a group, the mask addresses mod 4 per kind, the alignments of a last group that ends at the last byte of
    its source batch, widths, heights, (op, shape) and (mask kind, shape) pairs, the most regions in a call, and whether a
    source of another size and batch length occurs."""
    out = dict(pairs=set(), bitmap=set(), mask_frames=set(), tails=set(), widths=set(), heights=set(), ops=set(), kinds=set(),
               most_regions=0, other_size=False)
    for name in (str(n) for n in g['case_names']):
        c = case(g, name)
        dst = c['dst']
        src = dst if isinstance(c['src'], str) else c['src']
        mf = dst if isinstance(c['mask_frames'], str) else c['mask_frames']
        q = records(MODEL_DT, c['rows'], c['alpha'])
        out['most_regions'] = max(out['most_regions'], len(q))
        out['widths'].add(dst.shape[2]), out['heights'].add(dst.shape[1])
        out['other_size'] |= src.shape[0] != dst.shape[0] and src.shape[1] != dst.shape[1] and src.shape[2] != dst.shape[2]
        for r in q:
            out['ops'].add((int(r['op']), int(r['shape']))), out['kinds'].add((int(r['mask_kind']), int(r['shape'])))
            if r['shape'] != BOX:
                continue
            for d, s, m, last_is_group, end in grouped_rows(r, dst.shape, src.shape, None if mf is None else mf.shape):
                out['pairs'].add((d, s))
                if r['mask_kind'] == MASK_BITMAP:
                    out['bitmap'].add(m)
                if r['mask_kind'] == MASK_FRAMES:
                    out['mask_frames'].add(m)
                if last_is_group and end == src.size:
                    out['tails'].add((end - 12) & 3)
    return out
