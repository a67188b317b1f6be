"""Generate tests/golden/filter.npz with Pillow alone: the contract of ta_frames_filter and of the filter callers of
terran_amd.image and terran_amd.vis.

Stored: the noise sources (a frame of every width 1, 2, 3, 4, 5, 6, 53, 64, 257 and height 1, 2, 3, 5, 6, 37; two frames
just beyond csrc/filter.hip's 128 x 32 tile; a batch of three 37 x 53 frames; one 24 x 31 frame), the specs (a
lib.FILTER_SPEC_DT array built here from Pillow's own filter objects), the case list (source, regions) and what Pillow
returns for every case.  Flat and two-valued sources are regenerated from tests/tone_model.py by whoever reads the file;
only source generators and box clipping are imported here, no filter arithmetic.  Every expected value comes from Pillow:

    im.paste(im.crop(box).filter(F), box[, mask])         F: Kernel, the ten built-ins, RankFilter, UnsharpMask
    im.paste(ImageEnhance.Sharpness(im.crop(box)).enhance(factor), box[, mask])
    mask        ImageDraw.Draw(Image.new('L', (w, h))).ellipse([0, 0, w - 1, h - 1], fill=255)

For every case with a kernel the file also records how many of its expected pixels a build that contracts a multiply and
the add behind it into a fused multiply-add would change (the product and the sum evaluated exactly in float64 and
rounded to float32 once; the same for Image.blend's expression).  Fusing can only change a result where a product is not
exact in float32 AND the exact sum lies on an integer, so that the rounding decides the truncation:
  * DETAIL (/ 6) and SMOOTH_MORE (/ 100) have such sums (n / 6 + 0.5 and n / 100 + 0.5 are integers for some n) and must
    change at least one pixel; BLUR, SHARPEN and EDGE_ENHANCE divide by powers of two, the other built-ins by 1: their
    products are exact and fusing changes nothing; SMOOTH's sums n / 13 + 0.5 are never within rounding of an integer;
  * the random kernels are drawn as tenths over the scales 1.5 and 3.0 with offsets -3.3 and 7.6, so that entries are
    fifteenths and thirtieths (not exact in float32) and the sums meet integers often; they must change at least one pixel;
  * the sharpness factor 1.7 is not exact in float32 and must change at least one pixel; 0.5, 2 and -0.5 give exact
    products on top of SMOOTH, so no input can tell a fused build from Pillow there, and with 3.3 the two roundings agree
    on every 24 x 31 frame tried: their counts are recorded, not required.
The seed is advanced until these and the unsharp conditions (pixels on both sides of the threshold, clipped at both ends)
hold.

    python tests/golden/make_golden_filter.py
"""
import os
import sys

import numpy as np
import PIL
from PIL import Image, ImageDraw, ImageEnhance, ImageFilter

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
from terran_amd.lib import FILTER_SPEC_DT      # noqa: E402  (the record's layout only)
from tests import filter_model as M            # noqa: E402  (constants, sources)
from tests import tone_model as T              # noqa: E402  (clipped_box)

BOX, ELLIPSE = 0, 1
BUILTINS = ['BLUR', 'CONTOUR', 'DETAIL', 'EDGE_ENHANCE', 'EDGE_ENHANCE_MORE', 'EMBOSS', 'FIND_EDGES', 'SHARPEN', 'SMOOTH', 'SMOOTH_MORE']


def mask_image(w, h):
    m = Image.new('L', (w, h))
    ImageDraw.Draw(m).ellipse([0, 0, w - 1, h - 1], fill=255)
    return m


def spec_of(flt):
    """A Pillow filter object, or ('sharpness', factor) -> a FILTER_SPEC_DT record, from the object's own attributes."""
    s = np.zeros((), FILTER_SPEC_DT)
    if isinstance(flt, tuple):
        s = spec_of(ImageFilter.SMOOTH())
        s['has_factor'], s['factor'] = 1, flt[1]
    elif isinstance(flt, ImageFilter.BuiltinFilter):
        (w, h), scale, offset, kernel = flt.filterargs
        assert w == h
        s['kind'], s['size'], s['scale'], s['offset'] = 0, w, scale, offset
        s['kernel'][:w * h] = kernel
    elif isinstance(flt, ImageFilter.RankFilter):
        s['kind'], s['size'], s['rank'] = 1, flt.size, flt.rank
    else:
        assert isinstance(flt, ImageFilter.UnsharpMask)
        s['kind'], s['radius'], s['percent'], s['threshold'] = 2, flt.radius, flt.percent, flt.threshold
    return s


def pil_filter(crop, flt):
    return ImageEnhance.Sharpness(crop).enhance(flt[1]) if isinstance(flt, tuple) else crop.filter(flt)


def pil_apply(frames, rows, filters, seen=None):
    """rows: (frame, x0, y0, x1, y1, shape, spec); in list order."""
    ims = [Image.fromarray(f) for f in frames]
    for f, x0, y0, x1, y1, shape, s in rows:
        box = (x0, y0, x1, y1)
        crop = ims[f].crop(box)
        if seen is not None:
            seen.append((np.asarray(crop).copy(), s))
        out = pil_filter(crop, filters[s])
        if shape == ELLIPSE:
            ims[f].paste(out, box, mask_image(x1 - x0, y1 - y0))
        else:
            ims[f].paste(out, box)
    return np.stack([np.asarray(im) for im in ims])


def emulate(img, spec, fused):
    """The kernel (and blend) of `spec` on a crop in float64 emulation, no model code: every float32 operation is its exact
    float64 value rounded once; fused: a multiply and the add behind it are rounded once together."""
    f32, f64 = np.float32, np.float64
    size = int(spec['size'])
    r, (h, w) = size // 2, img.shape[:2]
    out = img.copy()
    if spec['has_factor'] and spec['factor'] == 1:            # Image.blend returns the image
        return out
    if w >= size and h >= size:
        k = (spec['kernel'][:size * size].astype(f64) / f64(spec['scale'])).astype(f32)
        ss = np.full((h - 2 * r, w - 2 * r, 3), f32(f64(spec['offset']) + 0.5), f32)
        p = img.astype(f64)
        for j in range(size):
            rows = p[2 * r - j:h - j]
            acc = (rows[:, 0:w - 2 * r] * f64(k[j * size])).astype(f32)
            for i in range(1, size):
                prod = rows[:, i:w - 2 * r + i] * f64(k[j * size + i])
                acc = (acc.astype(f64) + (prod if fused else prod.astype(f32).astype(f64))).astype(f32)
            ss = (ss.astype(f64) + acc.astype(f64)).astype(f32)
        out[r:h - r, r:w - r] = np.where(ss <= 0, 0, np.where(ss >= 255, 255, np.clip(ss, 0, 255).astype(np.int32)))
    if spec['has_factor']:
        f = f32(spec['factor'])
        a, d = out.astype(f64), img.astype(f64) - out.astype(f64)
        prod = f64(f) * d
        t = (a + (prod if fused else prod.astype(f32).astype(f64))).astype(f32)
        out = t.astype(np.int32) if 0 <= f <= 1 else np.where(t <= 0, 0, np.where(t >= 255, 255, np.clip(t, 0, 255).astype(np.int32)))
    return out.astype(np.uint8)


def random_kernel(rng, size, scale, offset):
    tenths = rng.integers(-5, 6, size * size)
    tenths[size * size // 2] += round(10 * scale) - tenths.sum()    # the sum over the scale is 1: results stay inside 0 .. 255 mostly
    return ImageFilter.Kernel((size, size), [float(v) / 10 for v in tenths], scale=scale, offset=offset)


def whole(h, w, spec, shape=BOX):
    return [(0, 0, 0, w, h, shape, spec)]


def build(seed):
    rng = np.random.default_rng(seed)
    out = {'pillow_version': np.array(PIL.__version__), 'seed': np.array(seed)}
    for h in M.HEIGHTS:
        for w in M.WIDTHS:
            out['noise_%dx%d' % (h, w)] = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
    tiles = [(M.TILE_H + 1, M.TILE_W + 1), (M.TILE_H + M.HALO - 1, M.TILE_W + M.HALO - 1)]
    for h, w in tiles:
        out['tile_%dx%d' % (h, w)] = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
    batch = rng.integers(0, 256, (3, 37, 53, 3), dtype=np.uint8)
    inner = (20, 10, 35, 25)                                # frame 1: a dark box in bright surroundings
    dark = batch[1, inner[1]:inner[3], inner[0]:inner[2]] % 30
    batch[1] = 200 + batch[1] % 56
    batch[1, inner[1]:inner[3], inner[0]:inner[2]] = dark
    small = rng.integers(0, 256, (24, 31, 3), dtype=np.uint8)
    out['batch'], out['small'] = batch, small

    # ---- the filters and their specs ----
    filters = [getattr(ImageFilter, n)() for n in BUILTINS]
    names = ['builtin_' + n.lower() for n in BUILTINS]
    filters += [random_kernel(rng, 3, 1.5, -3.3), random_kernel(rng, 5, 3.0, 7.6)]
    names += ['k3', 'k5']
    filters += [ImageFilter.RankFilter(s, r) for s, r in M.RANKS]
    names += ['rank_%d_%d' % sr for sr in M.RANKS]
    filters += [ImageFilter.UnsharpMask(*u) for u in M.UNSHARPS]
    names += ['unsharp_%g_%d_%d' % u for u in M.UNSHARPS]
    filters += [('sharpness', f) for f in M.SHARPNESS]
    names += ['sharpness_%g' % f for f in M.SHARPNESS]
    specs = np.stack([spec_of(f) for f in filters])
    out['specs'], out['spec_names'] = specs, np.array(names)
    S = {n: i for i, n in enumerate(names)}

    cases = []                                              # (name, source name, rows)
    for h in M.HEIGHTS:                                     # every shape: both kernel sizes, a rank window, an unsharp mask
        for w in M.WIDTHS:
            for n in ('k3', 'k5', 'rank_5_12', 'unsharp_1.3_73_0'):
                cases.append(('%s_%dx%d' % (n, h, w), 'noise_%dx%d' % (h, w), whole(h, w, S[n])))
    for h, w in tiles:
        for n in ('k5', 'rank_7_24', 'sharpness_1.7'):
            cases.append(('%s_tile_%dx%d' % (n, h, w), 'tile_%dx%d' % (h, w), whole(h, w, S[n])))
        cases.append(('ellipse_tile_%dx%d' % (h, w), 'tile_%dx%d' % (h, w), whole(h, w, S['rank_3_4'], ELLIPSE)))
    for n in names:                                         # every filter on the 24 x 31 frame
        if n not in ('k3', 'k5'):
            cases.append((n, 'small', whole(24, 31, S[n])))
    for kind in ('flat', 'two'):                            # ranks on a flat and on a two-valued frame (ties)
        for s, r in M.RANKS:
            cases.append(('rank_%d_%d_%s' % (s, r, kind), '%s_24x31' % kind, whole(24, 31, S['rank_%d_%d' % (s, r)])))
    cases.append(('builtin_sharpen_batch', 'batch', [(f, 0, 0, 53, 37, BOX, S['builtin_sharpen']) for f in range(3)]))

    # one call of many regions
    H, W = 37, 53
    x0, y0, x1, y1 = inner
    rows = [(2, 0, 0, W, H, BOX, S['builtin_emboss']), (0, 5, 3, 40, 30, BOX, S['k5']), (1, 7, 0, 53, 37, ELLIPSE, S['rank_3_4']),
            (0, 5, 3, 40, 30, BOX, S['k5']),                                     # a box twice
            (0, 20, 10, 53, 37, BOX, S['rank_5_12']), (0, 0, 0, 21, 11, BOX, S['unsharp_2_150_3']),      # overlaps, other filters
            (1, x0, y0, x1, y1, BOX, S['k5']), (1, x0, y0, x1, y1, BOX, S['rank_7_48']),     # the dark box: nothing from outside
            (1, x0, y0, x1, y1, BOX, S['unsharp_5_500_10']), (1, x0 + 1, y0, x1, y1 - 1, BOX, S['builtin_contour']),
            (2, 11, 9, 12, 10, ELLIPSE, S['rank_3_8']), (2, 20, 20, 22, 22, ELLIPSE, S['rank_3_0']),     # 1 x 1, 2 x 2
            (2, 13, 4, 22, 10, ELLIPSE, S['builtin_find_edges']), (0, 13, 4, 22, 10, ELLIPSE, S['sharpness_3.3']),   # 9 x 6
            (2, 0, 0, 7, H, BOX, S['k3']), (2, W - 6, 0, W, H, BOX, S['sharpness_-0.5']),    # the left and right edges
            (0, 3, 0, 50, 5, BOX, S['builtin_smooth_more']), (0, 4, H - 5, 49, H, BOX, S['unsharp_0.4_33_1']),   # top, bottom
            (1, 0, 30, 4, 37, BOX, S['k3']), (1, 1, 0, 3, 2, BOX, S['rank_5_3'])]            # narrower than the kernel; tiny
    while len(rows) < 44:
        a, b = int(rng.integers(0, W - 1)), int(rng.integers(0, H - 1))
        rows.append((int(rng.integers(0, 3)), a, b, int(rng.integers(a + 1, W + 1)), int(rng.integers(b + 1, H + 1)),
                     int(rng.integers(0, 2)), int(rng.integers(0, len(names)))))
    assert {r[1] % 2 for r in rows} == {0, 1} and [r[0] for r in rows[:3]] == [2, 0, 1] and rows[1] == rows[3]
    cases.append(('many', 'batch', rows))

    # faces, as vis.filter_faces clips them
    faces = [[[10.2, 5.5, 30.9, 28.1], [40.0, 20.0, 52.0, 36.5]], [], [[-4.0, -3.0, 9.5, 8.0], [20.0, 30.0, 21.0, 31.0], [60.0, 5.0, 70.0, 9.0]]]
    margin = 0.25
    out['face_bboxes'] = np.array([b for f in faces for b in f], np.float64)
    out['face_frames'] = np.array([i for i, f in enumerate(faces) for _ in f], np.int32)
    out['face_margin'] = np.array(margin)
    rows = []
    for i, per in enumerate(faces):
        for bbox in per:
            a, b, c, d = T.clipped_box(bbox, H, W, margin)
            if c > a and d > b:
                rows.append((i, a, b, c, d, ELLIPSE, S['builtin_sharpen']))
    assert len(rows) == 4
    cases.append(('faces', 'batch', rows))

    out['case_names'], out['case_sources'] = np.array([c[0] for c in cases]), np.array([c[1] for c in cases])
    fma = np.full(len(cases), -1, np.int64)
    ok = True
    for i, (name, src, rows) in enumerate(cases):
        frames = M.source(src, out)
        seen = []
        exp = pil_apply(frames, rows, filters, seen)
        out['case_%d_regions' % i] = np.array(rows, np.int32)
        if name == 'sharpness_1':
            assert np.array_equal(exp, frames)             # Image.blend returns the image: nothing to store
        else:
            out['case_%d_expected' % i] = exp
        kernels = [(crop, specs[s]) for crop, s in seen if specs[s]['kind'] == 0]
        if kernels and len(rows) == 1:
            crop, spec = kernels[0]
            plain = emulate(crop, spec, False)
            assert np.array_equal(plain, exp[0]), name      # the emulation is Pillow's arithmetic
            fma[i] = int((plain != emulate(crop, spec, True)).any(-1).sum())
            must = name.split('_')[0] in ('k3', 'k5') or name in ('builtin_detail', 'builtin_smooth_more', 'sharpness_1.7')
            if must and src in ('small', 'noise_37x53', 'tile_33x129', 'tile_34x130') and fma[i] < 1:
                print('seed %d: %s: a fused multiply-add changes nothing' % (seed, name))
                ok = False
        if name.startswith('unsharp') and src == 'small':
            r, p, t = specs[rows[0][6]]['radius'], int(specs[rows[0][6]]['percent']), int(specs[rows[0][6]]['threshold'])
            a = frames[0].astype(np.int64)
            b = np.asarray(Image.fromarray(frames[0]).filter(ImageFilter.GaussianBlur(float(r)))).astype(np.int64)
            d = a - b
            raw = a + np.sign(d) * (np.abs(d) * p // 100)
            moved = np.abs(d) > t
            if not (moved.any() and (~moved).any() and (raw[moved] < 0).any() and (raw[moved] > 255).any()):
                print('seed %d: %s: not on both sides of the threshold and clipped at both ends' % (seed, name))
                ok = False
    out['case_fma'] = fma
    assert np.array_equal(out['case_%d_expected' % [c[0] for c in cases].index('sharpness_0')],
                          out['case_%d_expected' % [c[0] for c in cases].index('builtin_smooth')])
    return out if ok else None


def main():
    seed = 20261019
    out = build(seed)
    while out is None:
        seed += 1
        out = build(seed)
    names = [str(n) for n in out['case_names']]
    for n, c in zip(names, out['case_fma']):
        if c >= 0 and not n[0] == 'k' or n in ('k3_37x53', 'k5_37x53'):
            print('%-28s a fused multiply-add would change %d pixels' % (n, c))
    # the conditions the file must keep
    assert len(out['case_%d_regions' % names.index('many')]) >= 40
    for n in ['builtin_detail', 'builtin_smooth_more', 'k5_tile_33x129', 'k5_tile_34x130', 'k3_37x53', 'k5_37x53', 'sharpness_1.7']:
        assert out['case_fma'][names.index(n)] >= 1, n
    for n, lo, hi in (('builtin_emboss', 0, 255), ('builtin_contour', 0, 255)):
        e = out['case_%d_expected' % names.index(n)][0, 1:-1, 1:-1]
        assert (e == lo).any() and (e == hi).any(), n
    path = os.path.join(HERE, 'filter.npz')
    np.savez_compressed(path, **out)
    print('%s: %d arrays, %d cases, %d bytes, seed %d, Pillow %s' % (path, len(out), len(names), os.path.getsize(path), seed, PIL.__version__))


if __name__ == '__main__':
    main()
