"""Generate tests/golden/combine.npz with Pillow alone: the contract of ta_frames_combine and of the two-image callers of
terran_amd.image and terran_amd.vis.

Stored: the noise sources, the cases (region rows in tests/combine_model.COLUMNS order, alphas, packed bitmaps) and what
Pillow returns for them.  Only that module's source generators (ramp pair, matte), its column list and its description of
the kernel's row walk (to aim the boxes at every alignment) are imported here, none of its arithmetic.  Every expected
value comes from Pillow; per region, with a = dst.crop(box), b = src.crop(source box):

    PASTE      R = a.copy(); R.paste(b, (0, 0), mask)   mask: None | Image.new('L', size, v) | a bitmap | getchannel(band)
    BLEND      R = Image.blend(a, b, alpha)
    the rest   R = ImageChops.<op>(a, b[, scale, offset])
    then       dst.paste(R, box[, ellipse mask])        ImageDraw.Draw(Image.new('L', (w, h))).ellipse([0, 0, w - 1, h - 1], fill=255)

The file also records how many expected pixels the wrong arithmetic would change (float emulation, no model code): paste
as the sum of two MULDIV255s, add / subtract with a multiply by the reciprocal, blend with a fused multiply-add.  Each
count must be at least 1, or a kernel that takes the shortcut could pass.

    python tests/golden/make_golden_combine.py
"""
import os
import sys

import numpy as np
import PIL
from PIL import Image, ImageChops, ImageDraw

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
from tests import combine_model as M   # noqa: E402  (sources, COLUMNS, row walk only)
from tests import tone_model as T      # noqa: E402  (clipped_box only)

WIDTHS, HEIGHTS = [1, 3, 5, 53, 64, 257], [1, 2, 37]
BOX, ELLIPSE = 0, 1
CHOPS = {M.LIGHTER: ImageChops.lighter, M.DARKER: ImageChops.darker, M.DIFFERENCE: ImageChops.difference,
         M.MULTIPLY: ImageChops.multiply, M.SCREEN: ImageChops.screen, M.ADD_MODULO: ImageChops.add_modulo,
         M.SUBTRACT_MODULO: ImageChops.subtract_modulo, M.SOFT_LIGHT: ImageChops.soft_light, M.HARD_LIGHT: ImageChops.hard_light,
         M.OVERLAY: ImageChops.overlay}


def ellipse_image(w, h):
    m = Image.new('L', (w, h))
    ImageDraw.Draw(m).ellipse([0, 0, w - 1, h - 1], fill=255)
    return m


def row(frame, x0, y0, x1, y1, shape=BOX, src=(0, 0, 0), op=M.PASTE, alpha=0.0, offset=0, mask=(M.MASK_NONE, 0), mask_at=(0, 0, 0), band=0):
    """-> (the int32 columns, alpha); src, mask_at: (frame, x, y)."""
    return (frame, x0, y0, x1, y1, shape) + tuple(src) + (op, offset) + tuple(mask) + tuple(mask_at) + (band,), alpha


def pil_region(a, b, q, alpha, masks, mask_ims):
    op, w, h = q['op'], a.size[0], a.size[1]
    if op == M.PASTE:
        kind = q['mask_kind']
        mask = None
        if kind == M.MASK_CONSTANT:
            mask = Image.new('L', (w, h), q['mask_value'])
        elif kind == M.MASK_BITMAP:
            mask = Image.frombytes('L', (w, h), bytes(masks[q['mask_value']:q['mask_value'] + w * h]))
        elif kind == M.MASK_FRAMES:
            mx, my = q['mask_x'], q['mask_y']
            mask = mask_ims[q['mask_frame']].crop((mx, my, mx + w, my + h)).getchannel(q['mask_band'])
        out = a.copy()
        out.paste(b, (0, 0), mask)
        return out
    if op == M.BLEND:
        return Image.blend(a, b, alpha)
    if op == M.ADD:
        return ImageChops.add(a, b, alpha, q['offset'])
    if op == M.SUBTRACT:
        return ImageChops.subtract(a, b, alpha, q['offset'])
    return CHOPS[op](a, b)


def pil_combine(dst, src, rows, masks=None, mask_frames=None, seen=None):
    """rows: [(columns, alpha)]; `src` may be `dst` itself (then the frames read are never written).  -> expected frames."""
    ims = [Image.fromarray(f) for f in dst]
    src_ims = ims if src is dst else [Image.fromarray(f) for f in src]
    mask_ims = None if mask_frames is None else ims if mask_frames is dst else [Image.fromarray(f) for f in mask_frames]
    for cols, alpha in rows:
        q = dict(zip(M.COLUMNS, (int(v) for v in cols)))
        box = (q['x0'], q['y0'], q['x1'], q['y1'])
        w, h = box[2] - box[0], box[3] - box[1]
        a = ims[q['frame']].crop(box)
        b = src_ims[q['src_frame']].crop((q['src_x'], q['src_y'], q['src_x'] + w, q['src_y'] + h))
        if seen is not None:
            seen.append((np.asarray(a).copy(), np.asarray(b).copy(), q, alpha))
        out = pil_region(a, b, q, float(alpha), masks, mask_ims)
        if q['shape'] == ELLIPSE:
            ims[q['frame']].paste(out, box, ellipse_image(w, h))
        else:
            ims[q['frame']].paste(out, box)
    return np.stack([np.asarray(im) for im in ims])


def std_regions(h, w):
    rows = [(0, 0, w, h, BOX), (w - 1, h - 1, w, h, BOX), (0, h // 2, w, h // 2 + 1, BOX), (w // 2, 0, w // 2 + 1, h, BOX),
            (w // 3, h // 3, w, h, BOX), (0, 0, w, h, ELLIPSE)]
    if w > 1:
        rows += [(1, 0, w, h, BOX), (1, 0, w, h, ELLIPSE)]
    if w > 6 and h > 2:
        rows += [(3, 1, w - 2, h - 1, BOX), (3, 1, w - 2, h - 1, ELLIPSE)]
    return rows


# ---- the wrong arithmetic, emulated here (no model code) ----------------------------------------------------------------
def wrong_counts(seen):
    two = recip = fma = 0
    for a, b, q, alpha in seen:
        a, b = a.astype(np.int64), b.astype(np.int64)
        f = np.float32(alpha)
        if q['op'] == M.PASTE and q['mask_kind'] == M.MASK_CONSTANT:
            m = q['mask_value']
            t = a * (255 - m) + b * m + 128
            t1, t2 = a * (255 - m) + 128, b * m + 128
            two += int(((((t >> 8) + t) >> 8) != (((t1 >> 8) + t1) >> 8) + (((t2 >> 8) + t2) >> 8)).any(-1).sum())
        elif q['op'] in (M.ADD, M.SUBTRACT):
            s = (a + b if q['op'] == M.ADD else a - b).astype(np.float32)
            off = np.float32(q['offset'])
            clip = lambda t: np.clip(np.trunc(t.astype(np.float64)), 0, 255)      # noqa: E731
            recip += int((clip(s / f + off) != clip(s * (np.float32(1) / f) + off)).any(-1).sum())
        elif q['op'] == M.BLEND and f not in (0, 1):
            d = (b - a)
            plain = a.astype(np.float32) + f * d.astype(np.float32)
            fused = (a.astype(np.float64) + np.float64(f) * d.astype(np.float64)).astype(np.float32)
            if 0 <= f <= 1:
                fma += int((plain.astype(np.int32) != fused.astype(np.int32)).any(-1).sum())
            else:
                clip = lambda t: np.where(t <= 0, 0, np.where(t >= 255, 255, np.clip(t, 0, 255).astype(np.int32)))    # noqa: E731
                fma += int((clip(plain) != clip(fused)).any(-1).sum())
    return two, recip, fma


def main():
    rng = np.random.default_rng(20261019)
    out = {'pillow_version': np.array(PIL.__version__)}
    noise = lambda *shape: rng.integers(0, 256, shape + (3,), dtype=np.uint8)      # noqa: E731
    for h in HEIGHTS:
        for w in WIDTHS:
            out['noise_a_%dx%d' % (h, w)], out['noise_b_%dx%d' % (h, w)] = noise(1, h, w), noise(1, h, w)
    out['one'], out['pair'], out['batch'] = noise(1, 37, 53), noise(2, 37, 53), noise(3, 37, 53)
    out['src_big'], out['src_odd'], out['small'], out['small_b'] = noise(2, 41, 59), noise(3, 20, 31), noise(1, 20, 31), noise(1, 20, 31)
    names, seen = [], []

    def get(ref, dst=None):
        if isinstance(ref, np.ndarray):
            return ref
        if ref == 'dst':
            return dst
        if ref in ('ramp_a', 'ramp_b'):
            return M.ramp_pair()[ref == 'ramp_b']
        if ref.startswith('matte_'):
            return M.matte(*(int(v) for v in ref.split('_')[1].split('x')))
        return out[ref]

    def add_case(name, dst, src, rows, masks=None, mask_frames=None):
        """dst, src, mask_frames: the name of a stored or regenerated batch, or an array that the case stores itself."""
        names.append(name)
        for role, ref in (('dst', dst), ('src', src), ('mask_frames', mask_frames)):
            if isinstance(ref, str):
                out['case_%s_%s_name' % (name, role)] = np.array(ref)
            elif ref is not None:
                out['case_%s_%s' % (name, role)] = ref
        d = get(dst).copy()
        s = get(src, d)
        mf = None if mask_frames is None else get(mask_frames, d)
        out['case_%s_rows' % name] = np.array([r[0] for r in rows], np.int32).reshape(len(rows), len(M.COLUMNS))
        out['case_%s_alpha' % name] = np.array([r[1] for r in rows], np.float32)
        if masks is not None:
            out['case_%s_masks' % name] = np.asarray(masks, np.uint8)
        out['case_%s_expected' % name] = pil_combine(d, s, rows, masks, mf, seen)
        return out['case_%s_expected' % name]

    # ---- every width and height: overlapping regions in list order, the ops by turns ----
    turns = [dict(op=M.PASTE), dict(op=M.DIFFERENCE), dict(op=M.BLEND, alpha=0.3), dict(op=M.PASTE, mask=(M.MASK_CONSTANT, 100)),
             dict(op=M.MULTIPLY), dict(op=M.ADD, alpha=1.7, offset=-3), dict(op=M.SCREEN), dict(op=M.PASTE, mask='bitmap'),
             dict(op=M.OVERLAY), dict(op=M.SUBTRACT, alpha=0.75, offset=9)]
    for h in HEIGHTS:
        for w in WIDTHS:
            rows, masks = [], np.zeros(0, np.uint8)
            for k, (x0, y0, x1, y1, shape) in enumerate(std_regions(h, w)):
                kw = dict(turns[(k + h + w) % len(turns)])
                if kw.get('mask') == 'bitmap':
                    kw['mask'] = (M.MASK_BITMAP, len(masks))
                    masks = np.concatenate([masks, rng.integers(0, 256, (x1 - x0) * (y1 - y0), dtype=np.uint8)])
                rows.append(row(0, x0, y0, x1, y1, shape, src=(0, x0, y0), **kw))
            add_case('size_%dx%d' % (h, w), 'noise_a_%dx%d' % (h, w), 'noise_b_%dx%d' % (h, w), rows, masks if len(masks) else None)

    # ---- every op and every mask kind under both shapes; the source has another size and batch length ----
    W, H = 53, 37
    params = {M.BLEND: dict(alpha=0.3), M.ADD: dict(alpha=1.7, offset=-20), M.SUBTRACT: dict(alpha=0.5, offset=30)}
    bitmap = rng.integers(0, 256, 51 * 19 + 8, dtype=np.uint8)
    bitmap[::7], bitmap[3::11] = 0, 255

    def shapes(**kw):
        k1 = dict(kw)
        if kw.get('mask', (0,))[0] == M.MASK_BITMAP:
            k1['mask'] = (M.MASK_BITMAP, 4)                         # another part of the buffer for the second size
        return [row(0, 2, 0, 53, 18, BOX, src=(1, 5, 3), mask_at=(1, 4, 9), **kw),
                row(0, 0, 18, 51, 37, ELLIPSE, src=(0, 1, 2), mask_at=(0, 7, 0), **k1),
                row(0, 52, 36, 53, 37, ELLIPSE, src=(0, 0, 0), **k1)]
    for op, name in enumerate(M.OP_NAMES):
        add_case('op_' + name, 'one', 'src_big', shapes(op=op, **params.get(op, {})))
    add_case('mask_constant', 'one', 'src_big', shapes(mask=(M.MASK_CONSTANT, 77)))
    add_case('mask_bitmap', 'one', 'src_big', shapes(mask=(M.MASK_BITMAP, 1)), masks=bitmap)
    add_case('mask_frames', 'one', 'src_big', shapes(mask=(M.MASK_FRAMES, 0), band=1), mask_frames='matte_2x41x59')
    assert np.array_equal(out['case_op_paste_expected'][0, 36, 52], out['one'][0, 36, 52])     # the 1 x 1 ellipse changes nothing

    # ---- all 16 pairs of (destination, source) address mod 4; bitmap and frames masks at every offset mod 4 ----
    cyc = [dict(op=M.PASTE), dict(op=M.DIFFERENCE), dict(op=M.PASTE, mask=(M.MASK_CONSTANT, 200)), dict(op=M.BLEND, alpha=0.7)]
    rows = [row(k % 2, 3 + 11 * k, 2 + k, 12 + 11 * k, 10 + k, BOX, src=((2, 0, 1, 2)[k], k, k + 1), **cyc[k]) for k in range(4)]
    add_case('align', 'pair', 'src_odd', rows)
    masks = rng.integers(0, 256, 4 * 72 + 6, dtype=np.uint8)
    rows = [row(k % 2, 3 + 11 * k, 2 + k, 12 + 11 * k, 10 + k, BOX, src=(k % 3, k, k + 1), mask=(M.MASK_BITMAP, 73 * k)) for k in range(4)]
    add_case('align_bitmap', 'pair', 'src_odd', rows, masks=masks)
    rows = [row(k % 2, 3 + 11 * k, 2 + k, 12 + 11 * k, 10 + k, BOX, src=(k % 2, k, k + 1), mask=(M.MASK_FRAMES, 0),
                mask_at=(2 - k % 3, 3 - k, k), band=k % 3) for k in range(4)]
    add_case('align_mask_frames', 'pair', 'src_big', rows, mask_frames='src_odd')

    # ---- a source box that ends at the last pixel of the last frame of src, its last group at every alignment ----
    tails = [((1, 4, 7), dict(op=M.PASTE)), ((1, 5, 7), dict(op=M.DIFFERENCE)), ((2, 3, 7), dict(op=M.PASTE, mask=(M.MASK_CONSTANT, 130))),
             ((1, 3, 7), dict(op=M.ADD, alpha=1.7, offset=-2))]
    for k, ((n, h, w), kw) in enumerate(tails):
        total = n * h * w * 3
        found = None
        for x0 in range(0, 31 - 7):
            q = dict(frame=0, x0=x0, y0=5, x1=x0 + 7, y1=7, src_frame=n - 1, src_x=0, src_y=h - 2, mask_kind=0)
            last = M.grouped_rows(q, (1, 20, 31, 3), (n, h, w, 3))
            if len(last) == 2 and last[-1][3] and last[-1][4] == total:
                found = x0
                break
        assert found is not None and (total - 12) % 4 == k, (k, total)
        out['tail_src_%d' % k] = noise(n, h, w)
        add_case('tail_%d' % k, 'small', 'tail_src_%d' % k, [row(0, found, 5, found + 7, 7, BOX, src=(n - 1, 0, h - 2), **kw)])

    # ---- add / subtract on the ramp pair: every sum and every difference, three scales, a negative offset ----
    for op in (M.ADD, M.SUBTRACT):
        for scale, offset in ((1.0, 0), (1.7, -7), (3.0, -40)):
            add_case('ramp_%s_%g' % (M.OP_NAMES[op], scale), 'ramp_a', 'ramp_b', [row(0, 0, 0, 511, 4, op=op, alpha=scale, offset=offset)])
    ra, rb = (x.astype(int) for x in M.ramp_pair())
    assert set(range(511)) <= set((ra + rb).ravel().tolist()) and set(range(-255, 256)) <= set((ra - rb).ravel().tolist())

    # ---- blend inside 0 .. 1 and outside ----
    for alpha in (0.0, 0.3, 0.5, 1.0, 1.7, -0.5):
        add_case('blend_%g' % alpha, 'one', 'src_big', [row(0, 0, 0, W, H, op=M.BLEND, alpha=alpha, src=(1, 3, 2))])
    assert np.array_equal(out['case_blend_0_expected'], out['one'])

    # ---- 40 regions in one call: frames out of order, overlaps in list order, three bitmaps shared by regions ----
    pool = [(9, 8), (16, 5), (7, 7)]
    offs, masks = [], np.zeros(0, np.uint8)
    for w, h in pool:
        offs.append(len(masks) + 1)
        masks = np.concatenate([masks, rng.integers(0, 256, w * h + 1, dtype=np.uint8)])
    rows = []
    for k in range(40):
        f = (2, 0, 1)[k] if k < 3 else int(rng.integers(0, 3))
        pick = int(rng.integers(0, 20))
        if pick < 6:
            w, h = pool[pick % 3]
        else:
            w, h = int(rng.integers(1, 30)), int(rng.integers(1, 20))
        x0, y0 = int(rng.integers(0, W - w + 1)), int(rng.integers(0, H - h + 1))
        src = (int(rng.integers(0, 2)), int(rng.integers(0, 59 - w + 1)), int(rng.integers(0, 41 - h + 1)))
        shape = int(rng.integers(0, 2))
        if pick < 6:
            kw = dict(mask=(M.MASK_BITMAP, offs[pick % 3]))
        elif pick < 9:
            kw = dict(mask=(M.MASK_FRAMES, 0), band=pick % 3,
                      mask_at=(int(rng.integers(0, 2)), int(rng.integers(0, 59 - w + 1)), int(rng.integers(0, 41 - h + 1))))
        elif pick < 11:
            kw = dict(mask=(M.MASK_CONSTANT, int(rng.integers(0, 256))))
        else:
            op = int(rng.integers(0, 14))
            kw = dict(op=op, alpha=float(rng.choice([0.25, 0.6, 1.3, 2.0])), offset=int(rng.integers(-30, 30)))
        rows.append(row(f, x0, y0, x0 + w, y0 + h, shape, src=src, **kw))
    add_case('many', 'batch', 'src_big', rows, masks=masks, mask_frames='matte_2x41x59')
    cols = np.array([r[0] for r in rows])
    assert cols[:3, 0].tolist() == [2, 0, 1]
    assert any(a[0] == b[0] and a[1] < b[3] and b[1] < a[3] and a[2] < b[4] and b[2] < a[4] for i, a in enumerate(cols) for b in cols[:i])
    assert all(sum(1 for c in cols if c[11] == M.MASK_BITMAP and c[12] == o) >= 2 for o in offs)

    # ---- the destination batch as its own source and mask batch: frames 0 and 2 written, frame 1 read ----
    rows = [row(0, 0, 0, W, H, src=(1, 0, 0), op=M.DIFFERENCE), row(2, 5, 4, 45, 30, ELLIPSE, src=(1, 8, 7), op=M.BLEND, alpha=0.5),
            row(2, 20, 10, 53, 37, src=(1, 0, 0), mask=(M.MASK_FRAMES, 0), mask_at=(1, 3, 2), band=2)]
    add_case('self', 'batch', 'dst', rows, mask_frames='dst')
    assert np.array_equal(out['case_self_expected'][1], out['batch'][1])

    two, recip, fma = wrong_counts(seen)
    out['count_paste_two_divisions'], out['count_add_reciprocal'], out['count_blend_fma'] = np.array(two), np.array(recip), np.array(fma)
    print('wrong arithmetic would change: paste %d, add %d, blend %d pixels' % (two, recip, fma))
    assert two >= 1 and recip >= 1 and fma >= 1
    out['case_names'] = np.array(names)

    # ---- the callers ----
    im = Image.fromarray
    batch, one, pair, small, small_b = out['batch'], out['one'], out['pair'], out['small'], out['small_b']
    # a one-frame `other` applied to every frame of a batch
    out['call_blend_one'] = np.stack([np.asarray(Image.blend(im(f), im(one[0]), 0.25)) for f in batch])
    out['call_difference_one'] = np.stack([np.asarray(ImageChops.difference(im(f), im(one[0]))) for f in batch])
    # a mixed-size list: two 37 x 53 frames with a one-frame other, one 20 x 31 frame with its own
    parts = [(pair, one, M.matte(1, 37, 53)), (small, small_b, M.matte(1, 20, 31))]
    bitmap = rng.integers(0, 256, (12, 17), dtype=np.uint8)
    out['call_bitmap'] = bitmap

    def each(fn):
        return [np.stack([np.asarray(fn(im(f), im(o[0]), im(m[0]))) for f in frames]) for frames, o, m in parts]

    def pasted(box, mask):
        def fn(a, b, m):
            a = a.copy()
            a.paste(b, box, mask)
            return a
        return fn
    calls = {'difference': lambda a, b, m: ImageChops.difference(a, b), 'composite': lambda a, b, m: Image.composite(b, a, m.getchannel(0)),
             'screen': lambda a, b, m: ImageChops.screen(a, b), 'add': lambda a, b, m: ImageChops.add(a, b, 1.7, -5),
             'blend': lambda a, b, m: Image.blend(a, b, 1.7),
             'paste_corner': pasted((-5, 11), None), 'paste_constant': pasted((40, -3), Image.new('L', (53, 37), 90))}
    for name, fn in calls.items():
        if name.startswith('paste'):                     # the one 37 x 53 frame pasted into every frame, clipped by Pillow
            res = [np.stack([np.asarray(fn(im(f), im(one[0]), None)) for f in frames]) for frames, _, _ in parts]
        else:
            res = each(fn)
        out['call_%s_a' % name], out['call_%s_b' % name] = res
    # a 17 x 12 piece of `other` from (3, 2), under a host bitmap, at a box that leaves the frame on the right
    piece = im(one[0]).crop((3, 2, 20, 14))
    res = [np.stack([np.asarray(pasted((45, 30), Image.fromarray(bitmap))(im(f), piece, None)) for f in frames]) for frames, _, _ in parts]
    out['call_paste_bitmap_a'], out['call_paste_bitmap_b'] = res
    out['call_names'] = np.array(sorted(calls) + ['paste_bitmap'])

    # composite_faces: the boxes of blur_faces (margin, truncation, clipping), other = the batch in reverse order
    faces = [[[10.2, 5.5, 30.9, 28.1], [40.0, 20.0, 52.0, 36.5]], [], [[-4.0, -3.0, 9.5, 8.0], [20.0, 30.0, 21.0, 31.0], [60.0, 5.0, 70.0, 9.0]]]
    margin = 0.25
    out['face_bboxes'] = np.array([b for f in faces for b in f], np.float64)
    out['face_frames'] = np.array([i for i, f in enumerate(faces) for _ in f], np.int32)
    out['face_margin'] = np.array(margin)
    other = batch[::-1]
    for shape in ('box', 'ellipse'):
        for alpha in (None, 0.4):
            ims = [im(f) for f in batch]
            for i, per in enumerate(faces):
                for bbox in per:
                    x0, y0, x1, y1 = T.clipped_box(bbox, H, W, margin)
                    if x1 <= x0 or y1 <= y0:
                        continue
                    box, size = (x0, y0, x1, y1), (x1 - x0, y1 - y0)
                    r = ims[i].crop(box)
                    r.paste(im(other[i]).crop(box), (0, 0), None if alpha is None else Image.new('L', size, round(255 * alpha)))
                    ims[i].paste(r, box, ellipse_image(*size) if shape == 'ellipse' else None)
            out['faces_%s_%s' % (shape, 'paste' if alpha is None else 'alpha')] = np.stack([np.asarray(x) for x in ims])

    # inset_chips: eight 14 x 12 chips, seven of frame 0 (three a row; the third row no longer fits) and one of frame 2
    chips = noise(8, 14, 12)
    index = np.array([(0, k) for k in range(7)] + [(2, 0)], np.int32)
    ims = [im(f) for f in batch]
    places = [(3, 2), (17, 2), (31, 2), (3, 18), (17, 18), (31, 18), None, (3, 2)]
    for chip, (f, _), at in zip(chips, index, places):
        if at is not None:
            ims[f].paste(im(chip), at)
    out['inset_chips'], out['inset_index'], out['inset_expected'] = chips, index, np.stack([np.asarray(x) for x in ims])
    out['inset_places'] = np.array([(-1, -1) if p is None else p for p in places], np.int32)

    path = os.path.join(HERE, 'combine.npz')
    np.savez_compressed(path, **out)
    print('%s: %d arrays, %d bytes, Pillow %s' % (path, len(out), os.path.getsize(path), PIL.__version__))
    assert os.path.getsize(path) < (1 << 20)


if __name__ == '__main__':
    main()
