"""Generate tests/golden/tone.npz with Pillow alone: the contracts of ta_frames_histogram / ta_frames_point /
ta_frames_saturate and of the pixel-value callers of terran_amd.image and terran_amd.vis.face_stats.

Stored: the noise sources (frames of every width 1, 3, 5, 53, 64, 257 and height 1, 2, 37, a batch of three 37 x 53
frames, one 20 x 31 frame), the case lists (regions, tables, factors) and what Pillow returns for them.  Flat, ramp,
two-valued and dim sources are regenerated from tests/tone_model.py by whoever reads the file; only that module's source
generators and box clipping are imported here, none of its arithmetic.  Every expected value comes from Pillow:

    histogram   im.crop(box).histogram(mask), im.crop(box).convert('L').histogram(mask)
    point       im.paste(im.crop(box).point(lut), box[, mask])
    saturate    im.paste(ImageEnhance.Color(im.crop(box)).enhance(factor), box[, mask])
    callers     ImageOps.equalize / autocontrast, ImageEnhance.Brightness / Contrast / Color, convert('L').convert('RGB'),
                ImageStat.Stat; the tables ImageOps hands to point() are recorded too
    mask        ImageDraw.Draw(Image.new('L', (w, h))).ellipse([0, 0, w - 1, h - 1], fill=255)

For every saturate case the file also records how many of its expected pixels a fused multiply-add in Image.blend's
expression would change (the product and the sum evaluated exactly in float64 and rounded to float32 once): the 1.2 and
1.7 cases must have at least one, or a contracted build could pass them.

    python tests/golden/make_golden_tone.py
"""
import os
import sys

import numpy as np
import PIL
from PIL import Image, ImageDraw, ImageEnhance, ImageOps, ImageStat

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
from tests import tone_model as T      # noqa: E402  (sources and clipped_box only)

WIDTHS, HEIGHTS = [1, 3, 5, 53, 64, 257], [1, 2, 37]
BOX, ELLIPSE = 0, 1


def mask_image(w, h):
    m = Image.new('L', (w, h))
    ImageDraw.Draw(m).ellipse([0, 0, w - 1, h - 1], fill=255)
    return m


def pil_hist(frames, regions):
    rgb, lum = [], []
    for f, x0, y0, x1, y1, shape in regions:
        crop = Image.fromarray(frames[f]).crop((x0, y0, x1, y1))
        mask = mask_image(x1 - x0, y1 - y0) if shape == ELLIPSE else None
        rgb.append(np.array(crop.histogram(mask), np.uint32).reshape(3, 256))
        lum.append(np.array(crop.convert('L').histogram(mask), np.uint32))
    return np.stack(rgb), np.stack(lum)


def pil_apply(frames, regions, fn):
    """regions: rows (frame, x0, y0, x1, y1, shape, ...); fn(crop image, row) -> image; in list order, in place."""
    ims = [Image.fromarray(f) for f in frames]
    for row in regions:
        f, x0, y0, x1, y1, shape = (int(v) for v in row[:6])
        box = (x0, y0, x1, y1)
        out = fn(ims[f].crop(box), row)
        if shape == ELLIPSE:
            ims[f].paste(out, box, mask_image(x1 - x0, y1 - y0))
        else:
            ims[f].paste(out, box)
    return np.stack([np.asarray(im) for im in ims])


def std_regions(h, w):
    rows = [(0, 0, 0, w, h, BOX), (0, w - 1, h - 1, w, h, BOX), (0, 0, h // 2, w, h // 2 + 1, BOX),
            (0, w // 2, 0, w // 2 + 1, h, BOX), (0, w // 3, h // 3, w, h, BOX), (0, 0, 0, w, h, ELLIPSE)]
    if w > 1:
        rows += [(0, 1, 0, w, h, BOX), (0, 1, 0, w, h, ELLIPSE)]
    if w > 6 and h > 2:
        rows += [(0, 3, 1, w - 2, h - 1, BOX), (0, 3, 1, w - 2, h - 1, ELLIPSE)]
    return rows


def fma_count(expected_regions):
    """Pixels of the saturate case's regions that a fused multiply-add would change: float64 emulation, no model code."""
    def color(img, f, fused):
        a = img.astype(np.int64)
        l = (19595 * a[..., 0] + 38470 * a[..., 1] + 7471 * a[..., 2] + 0x8000) >> 16
        d = a - l[..., None]
        f = np.float32(f)
        if fused:
            t = (l[..., None].astype(np.float64) + np.float64(f) * d.astype(np.float64)).astype(np.float32)
        else:
            t = l[..., None].astype(np.float32) + f * d.astype(np.float32)
        if 0 <= f <= 1:
            return t.astype(np.int32)
        return np.where(t <= 0, 0, np.where(t >= 255, 255, np.clip(t, 0, 255).astype(np.int32)))
    n = 0
    for img, f in expected_regions:
        if np.float32(f) in (0, 1):
            continue
        n += int((color(img, f, False) != color(img, f, True)).any(-1).sum())
    return n


def main():
    rng = np.random.default_rng(20261019)
    out = {'pillow_version': np.array(PIL.__version__)}
    for h in HEIGHTS:
        for w in WIDTHS:
            out['noise_%dx%d' % (h, w)] = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
    batch = rng.integers(0, 256, (3, 37, 53, 3), dtype=np.uint8)
    small = rng.integers(0, 256, (20, 31, 3), dtype=np.uint8)
    out['batch'], out['small'] = batch, small

    # ---- histogram ----
    cases = [('noise_%dx%d' % (h, w), std_regions(h, w)) for h in HEIGHTS for w in WIDTHS]
    H, W = 37, 53
    order = [(2, 0, 0, W, H, BOX), (0, 5, 3, 40, 30, BOX), (1, 7, 0, 53, 37, ELLIPSE), (2, 11, 9, 12, 10, ELLIPSE),
             (0, 5, 3, 40, 30, BOX), (1, 20, 20, 22, 22, ELLIPSE), (0, 13, 4, 22, 10, ELLIPSE), (2, 11, 9, 12, 10, BOX)]
    cases.append(('batch', order))
    many = []
    for _ in range(40):
        x0, y0 = int(rng.integers(0, W - 1)), int(rng.integers(0, H - 1))
        many.append((int(rng.integers(0, 3)), x0, y0, int(rng.integers(x0 + 1, W + 1)), int(rng.integers(y0 + 1, H + 1)),
                     int(rng.integers(0, 2))))
    cases.append(('batch', many))
    cases.append(('two_37x64', std_regions(37, 64)))
    cases.append(('ramp_37x257', std_regions(37, 257)))
    cases.append(('flat_517x300', [(0, 0, 0, 300, 517, BOX), (0, 0, 0, 300, 517, ELLIPSE), (0, 7, 1, 299, 500, BOX)]))
    out['hist_sources'] = np.array([c[0] for c in cases])
    for i, (name, rows) in enumerate(cases):
        frames = T.source(name, out)
        rgb, lum = pil_hist(frames, rows)
        out['hist_%d_regions' % i], out['hist_%d_rgb' % i], out['hist_%d_l' % i] = np.array(rows, np.int32), rgb, lum
    assert out['hist_%d_rgb' % (len(cases) - 1)].max() == 517 * 300 > 65535
    assert not out['hist_%d_rgb' % (len(cases) - 5)][3].any()            # the 1 x 1 ellipse covers nothing

    # ---- point ----
    ident = np.tile(np.arange(256), 3)
    three = np.concatenate([rng.permutation(256) for _ in range(3)])
    per_frame = np.stack([np.concatenate([rng.integers(0, 256, 256) for _ in range(3)]) for _ in range(3)])
    inv = np.tile(np.arange(255, -1, -1), 3)
    post = np.tile(np.arange(256) & ~(2 ** 6 - 1), 3)
    a, b = (0, 4, 3, 36, 28, BOX), (0, 21, 15, 53, 37, BOX)
    pcases = [('identity', batch, [(f, 0, 0, W, H, BOX, 0) for f in range(3)], [ident]),
              ('three_bands', batch[:1], [(0, 0, 0, W, H, BOX, 0)], [three]),
              ('per_frame', batch, [(f, 0, 0, W, H, BOX, f) for f in (1, 2, 0)], per_frame),
              ('invert_then_posterize', batch[:1], [a + (0,), b + (1,)], [inv, post]),
              ('posterize_then_invert', batch[:1], [a + (1,), b + (0,)], [inv, post]),
              ('ellipse', batch[1:2], [(0, 3, 2, 50, 35, ELLIPSE, 0), (0, 0, 0, 1, 1, ELLIPSE, 1), (0, 51, 35, 53, 37, ELLIPSE, 1)],
               [three, inv])]
    out['point_names'] = np.array([c[0] for c in pcases])
    for name, frames, rows, luts in pcases:
        luts = np.array(luts, np.uint8)
        exp = pil_apply(frames, rows, lambda crop, row: crop.point([int(v) for v in luts[row[6]]]))
        out['point_%s_source' % name], out['point_%s_regions' % name] = frames, np.array(rows, np.int32)
        out['point_%s_luts' % name], out['point_%s_expected' % name] = luts, exp
    assert not np.array_equal(out['point_invert_then_posterize_expected'], out['point_posterize_then_invert_expected'])

    # ---- saturate ----
    two = batch[:2]
    scases = [('factor_%g' % f, [(k, 0, 0, W, H, BOX) for k in range(2)], [f, f]) for f in T.FACTORS]
    scases.append(('overlap', [(0,) + a[1:], (0,) + b[1:], (1,) + b[1:], (1,) + a[1:]], [1.7, 0.3, 1.7, 0.3]))
    scases.append(('ellipse', [(0, 3, 2, 50, 35, ELLIPSE), (1, 0, 0, 1, 1, ELLIPSE), (1, 10, 10, 19, 16, ELLIPSE)], [0.0, 0.0, 2.5]))
    out['saturate_names'] = np.array([c[0] for c in scases])
    for name, rows, factors in scases:
        rows = [r + (k,) for k, r in enumerate(rows)]
        seen = []

        def enhance(crop, row):
            seen.append((np.asarray(crop).copy(), factors[row[6]]))
            return ImageEnhance.Color(crop).enhance(factors[row[6]])
        exp = pil_apply(two, rows, enhance)
        out['saturate_%s_regions' % name] = np.array([r[:6] for r in rows], np.int32)
        out['saturate_%s_factors' % name] = np.array(factors, np.float32)
        out['saturate_%s_expected' % name] = exp
        out['saturate_%s_fma' % name] = np.array(fma_count(seen))
        print('saturate %-12s fused multiply-add would change %d pixels' % (name, out['saturate_%s_fma' % name]))
    assert out['saturate_factor_1.2_fma'] >= 1 and out['saturate_factor_1.7_fma'] >= 1
    assert np.array_equal(out['saturate_factor_1_expected'], two)

    # ---- callers: a mixed-size list, two dim 37 x 53 frames and one dim 20 x 31 frame ----
    parts = {'a': T.dim(batch)[:2], 'b': T.dim(small)[None]}
    tables = []
    real_lut = ImageOps._lut

    def spy(image, lut):
        tables.append(np.clip(lut if len(lut) == 768 else lut * 3, 0, 255).astype(np.uint8))      # point() clips the entries
        return real_lut(image, lut)
    ImageOps._lut = spy
    grey = lambda im: im.convert('L').convert('RGB')                                 # noqa: E731
    calls = [('equalize', ImageOps.equalize), ('autocontrast', ImageOps.autocontrast),
             ('autocontrast_cutoff', lambda im: ImageOps.autocontrast(im, cutoff=(2, 5))),
             ('autocontrast_ignore', lambda im: ImageOps.autocontrast(im, ignore=0)),
             ('autocontrast_tone', lambda im: ImageOps.autocontrast(im, cutoff=1, preserve_tone=True)),
             ('brightness', lambda im: ImageEnhance.Brightness(im).enhance(1.2)),
             ('contrast', lambda im: ImageEnhance.Contrast(im).enhance(1.7)),
             ('color', lambda im: ImageEnhance.Color(im).enhance(1.2)), ('grayscale', grey)]
    out['call_names'] = np.array([c[0] for c in calls])
    for name, fn in calls:
        del tables[:]
        for key, frames in parts.items():
            out['call_%s_%s' % (name, key)] = np.stack([np.asarray(fn(Image.fromarray(f))) for f in frames])
        if tables:
            out['call_%s_luts' % name] = np.stack(tables)                        # per frame, in list order
    ImageOps._lut = real_lut
    assert not np.array_equal(out['call_autocontrast_a'], out['call_autocontrast_ignore_a'])

    # Image.blend with a constant first image, as a table: Brightness (in1 = 0) and Contrast (in1 = the mean grey)
    blends = [(in1, f) for in1 in (0, 1, 77, 128, 254, 255) for f in (0.0, 0.3, 0.5, 0.999, 1.0, 1.2, 1.7, 2.5, -0.5, 3.3333)]
    identity = Image.frombytes('L', (256, 1), bytes(range(256)))
    out['blend_in1'], out['blend_factor'] = np.array([b[0] for b in blends]), np.array([b[1] for b in blends], np.float64)
    out['blend_table'] = np.stack([np.asarray(Image.blend(Image.new('L', (256, 1), in1), identity, f))[0] for in1, f in blends])

    # ImageStat.Stat: whole frames, one box per frame, faces (box and ellipse) with a margin that leaves the frame
    def stat_arrays(items):
        """items: (crop image, mask or None) -> dict of arrays over (item, band) for 'RGB' and 'L'."""
        res = {}
        for mode in ('RGB', 'L'):
            st = [ImageStat.Stat(im if mode == 'RGB' else im.convert('L'), m) for im, m in items]
            for k in T.STAT_KEYS:
                res['%s_%s' % (mode, k)] = np.array([getattr(s, k) for s in st])
            res['%s_hist' % mode] = np.array([s.h for s in st], np.uint32).reshape(len(st), -1, 256)
        return res
    listed = [f for frames in parts.values() for f in frames]
    for k, v in stat_arrays([(Image.fromarray(f), None) for f in listed]).items():
        out['stat_frames_' + k] = v
    boxes = [(3, 2, 41, 30), (0, 0, 53, 1), (30, 19, 31, 20)]
    out['stat_boxes'] = np.array(boxes, np.int32)
    for k, v in stat_arrays([(Image.fromarray(f).crop(b), None) for f, b in zip(listed, boxes)]).items():
        out['stat_boxes_' + k] = v
    faces = [[[10.2, 5.5, 30.9, 28.1], [40.0, 20.0, 52.0, 36.5]], [], [[-4.0, -3.0, 9.5, 8.0], [20.0, 30.0, 21.0, 31.0], [60.0, 5.0, 70.0, 9.0]]]
    margin = 0.25
    out['face_bboxes'] = np.array([b for f in faces for b in f], np.float64)
    out['face_frames'] = np.array([i for i, f in enumerate(faces) for _ in f], np.int32)
    out['face_margin'] = np.array(margin)
    dim3 = T.dim(batch)
    for shape in ('box', 'ellipse'):
        items, index = [], []
        for i, per in enumerate(faces):
            for k, bbox in enumerate(per):
                x0, y0, x1, y1 = T.clipped_box(bbox, H, W, margin)
                if x1 <= x0 or y1 <= y0:
                    continue
                items.append((Image.fromarray(dim3[i]).crop((x0, y0, x1, y1)), mask_image(x1 - x0, y1 - y0) if shape == 'ellipse' else None))
                index.append((i, k))
        for k, v in stat_arrays(items).items():
            out['face_%s_%s' % (shape, k)] = v
        out['face_index'] = np.array(index, np.int32)

    path = os.path.join(HERE, 'tone.npz')
    np.savez_compressed(path, **out)
    print('%s: %d arrays, %d bytes, Pillow %s' % (path, len(out), os.path.getsize(path), PIL.__version__))


if __name__ == '__main__':
    main()
