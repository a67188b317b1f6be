"""The contracts of ta_frames_histogram / ta_frames_point / ta_frames_saturate and of the terran_amd.image pixel-value
callers restated in numpy and plain Python (no Pillow, no GPU), operation by operation as Pillow 12 does them:

    convert('L')            (19595 R + 38470 G + 7471 B + 0x8000) >> 16
    histogram(mask)         counts of the pixels whose mask is non-zero, band after band
    point(lut)              band c of the result is lut[256 c + v]
    Image.blend(a, b, f)    float32 a + f * (b - a), a multiply and an add; truncated for 0 <= f <= 1, clipped to 0 .. 255
                            first otherwise; f == 0 copies a, f == 1 copies b
    ImageEnhance.Color      blend(convert('L') as RGB, im, f);  Brightness: blend(black, im, f);
    ImageEnhance.Contrast   blend(grey int(Stat(L).mean + 0.5), im, f)
    ImageOps.equalize / autocontrast / invert / posterize / solarize: integer tables from the histogram, then point()
    ImageStat.Stat          float64 sums over the histogram

Regions are lib.HIST_DT / POINT_DT / SATURATE_DT arrays: half-open boxes, applied in list order, under ImageDraw.ellipse's
coverage of the box for shape 1.  Also the sources the golden does not store (flat, ramp, two-valued and dim frames) and
the loader of tests/golden/tone.npz."""
import math
import os

import numpy as np

from tests.vis_blur_model import ellipse_mask

f32 = np.float32
BOX, ELLIPSE = 0, 1
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'tone.npz')
FACTORS = [0.0, 0.3, 1.0, 1.2, 1.7, -0.5, 3.3333]       # the saturate cases; 1.2 and 1.7 are the ones a fused multiply-add changes


# ---- sources the golden does not store ---------------------------------------------------------------------------------
def flat(h, w, rgb=(200, 17, 255)):
    return np.broadcast_to(np.array(rgb, np.uint8), (h, w, 3)).copy()


def ramp(h, w):
    y, x = np.mgrid[:h, :w]
    return np.stack([x % 256, (x + 3 * y) % 256, 255 - (x * 7 + y) % 256], -1).astype(np.uint8)


def two_valued(h, w):
    y, x = np.mgrid[:h, :w]
    on = ((x * x + 3 * y) % 5 < 2)[..., None]
    return np.where(on, np.array([250, 3, 128], np.uint8), np.array([4, 3, 129], np.uint8)).astype(np.uint8)


def dim(noise):
    """Under-exposed footage out of noise frames: band c within 30 + 10 c .. 30 + 10 c + 90 + 30 c, so autocontrast,
    equalize and contrast have something to do and the bands differ; a sprinkle of black pixels (about 3 %) gives
    autocontrast's ignore=0 something to ignore."""
    c = np.arange(3)
    out = 30 + 10 * c + noise.astype(np.int64) * (90 + 30 * c) // 255
    out[noise[..., 0] < 8] = 0
    return out.astype(np.uint8)


# ---- pixels ------------------------------------------------------------------------------------------------------------
def luma(img):
    a = img.astype(np.int64)
    return ((19595 * a[..., 0] + 38470 * a[..., 1] + 7471 * a[..., 2] + 0x8000) >> 16).astype(np.uint8)


def mask_of(h, w, shape):
    return ellipse_mask(h, w) if shape == ELLIPSE else np.ones((h, w), bool)


def histogram(img, mode='RGB', mask=None):
    """im.histogram(mask) of a uint8 (h, w, 3) array ('L': of its convert('L')) -> uint32 (3, 256) or (256,)."""
    sel = img[mask] if mask is not None else img.reshape(-1, 3)
    if mode == 'L':
        return np.bincount(luma(sel), minlength=256).astype(np.uint32)
    return np.stack([np.bincount(sel[:, c], minlength=256) for c in range(3)]).astype(np.uint32)


def hist_regions(frames, regions, mode='RGB'):
    out = [histogram(frames[q['frame']][q['y0']:q['y1'], q['x0']:q['x1']], mode,
                     mask_of(q['y1'] - q['y0'], q['x1'] - q['x0'], q['shape'])) for q in regions]
    return np.stack(out) if out else np.zeros((0, 3, 256) if mode == 'RGB' else (0, 256), np.uint32)


def point(img, lut):
    """im.point(lut): lut of 768 entries."""
    lut = np.asarray(lut).reshape(3, 256)
    return np.stack([lut[c][img[..., c]] for c in range(3)], -1).astype(np.uint8)


def blend(in1, in2, factor):
    """Image.blend on uint8 arrays of one shape."""
    f = f32(factor)
    if f == 0:
        return in1.copy()
    if f == 1:
        return in2.copy()
    a, b = in1.astype(np.int32), in2.astype(np.int32)
    prod = f * (b - a).astype(f32)
    t = a.astype(f32) + prod
    assert prod.dtype == f32 and t.dtype == f32
    if 0 <= f <= 1:
        return t.astype(np.int32).astype(np.uint8)
    return np.where(t <= 0, 0, np.where(t >= 255, 255, np.clip(t, 0, 255).astype(np.int32))).astype(np.uint8)


def blend_fused(in1, in2, factor):
    """The same with the multiply and the add fused (what a contracted build computes): the product and the sum are exact
    in float64 (24 + 9 bits), rounded to float32 once."""
    f = f32(factor)
    if f == 0 or f == 1:
        return blend(in1, in2, factor)
    a, b = in1.astype(np.int32), in2.astype(np.int32)
    t = (a.astype(np.float64) + np.float64(f) * (b - a).astype(np.float64)).astype(f32)
    if 0 <= f <= 1:
        return t.astype(np.int32).astype(np.uint8)
    return np.where(t <= 0, 0, np.where(t >= 255, 255, np.clip(t, 0, 255).astype(np.int32))).astype(np.uint8)


def color(img, factor, fused=False):
    """ImageEnhance.Color(im).enhance(factor)."""
    grey = np.repeat(luma(img)[..., None], 3, -1)
    return (blend_fused if fused else blend)(grey, img, factor)


def fma_changes(img, factor):
    """Pixels of color(img, factor) that a fused multiply-add would change."""
    return int((color(img, factor) != color(img, factor, fused=True)).any(-1).sum())


def _apply(frames, regions, fn):
    for q in regions:
        crop = frames[q['frame']][q['y0']:q['y1'], q['x0']:q['x1']]
        m = mask_of(crop.shape[0], crop.shape[1], q['shape'])
        crop[m] = fn(crop, q)[m]
    return frames


def point_regions(frames, regions, luts):
    """Apply a lib.POINT_DT array to host frames (N, H, W, 3) in place, in list order."""
    return _apply(frames, regions, lambda crop, q: point(crop, luts[q['lut']]))


def saturate_regions(frames, regions):
    return _apply(frames, regions, lambda crop, q: color(crop, q['factor']))


# ---- tables (Pillow's ImageOps, statement by statement) -----------------------------------------------------------------
def equalize_lut(h):
    h = [int(v) for v in np.asarray(h).reshape(-1)]
    lut = []
    for b in range(0, len(h), 256):
        histo = [_f for _f in h[b:b + 256] if _f]
        if len(histo) <= 1:
            lut.extend(list(range(256)))
        else:
            step = (sum(histo) - histo[-1]) // 255
            if not step:
                lut.extend(list(range(256)))
            else:
                n = step // 2
                for i in range(256):
                    lut.append(n // step)
                    n = n + h[i + b]
    return np.clip(lut, 0, 255).astype(np.uint8)        # point() clips its table's entries (an entry can reach 257 here)


def autocontrast_lut(histogram, cutoff=0, ignore=None):
    histogram = [int(v) for v in np.asarray(histogram).reshape(-1)]
    lut = []
    for layer in range(0, len(histogram), 256):
        h = histogram[layer:layer + 256]
        if ignore is not None:
            if isinstance(ignore, int):
                h[ignore] = 0
            else:
                for ix in ignore:
                    h[ix] = 0
        if cutoff:
            if not isinstance(cutoff, tuple):
                cutoff = (cutoff, cutoff)
            n = 0
            for ix in range(256):
                n = n + h[ix]
            cut = int(n * cutoff[0] // 100)
            for lo in range(256):
                if cut > h[lo]:
                    cut = cut - h[lo]
                    h[lo] = 0
                else:
                    h[lo] -= cut
                    cut = 0
                if cut <= 0:
                    break
            cut = int(n * cutoff[1] // 100)
            for hi in range(255, -1, -1):
                if cut > h[hi]:
                    cut = cut - h[hi]
                    h[hi] = 0
                else:
                    h[hi] -= cut
                    cut = 0
                if cut <= 0:
                    break
        for lo in range(256):
            if h[lo]:
                break
        for hi in range(255, -1, -1):
            if h[hi]:
                break
        if hi <= lo:
            lut.extend(list(range(256)))
        else:
            scale = 255.0 / (hi - lo)
            offset = -lo * scale
            for ix in range(256):
                ix = int(ix * scale + offset)
                if ix < 0:
                    ix = 0
                elif ix > 255:
                    ix = 255
                lut.append(ix)
    return np.array(lut, np.uint8)


def blend_lut(in1, factor):
    return blend(np.full(256, in1, np.uint8), np.arange(256).astype(np.uint8), factor)


def stats(h):
    """ImageStat.Stat(list) of a histogram of 256 x bands counts -> dict of lists, one entry per band."""
    h = [int(v) for v in np.asarray(h).reshape(-1)]
    bands = range(len(h) // 256)
    count = [sum(h[i:i + 256]) for i in range(0, len(h), 256)]
    total, total2, median, extrema = [], [], [], []
    for i in range(0, len(h), 256):
        s = s2 = 0.0
        for j in range(256):
            s += j * h[i + j]
            s2 += (j ** 2) * float(h[i + j])
        total.append(s)
        total2.append(s2)
        used = [j for j in range(256) if h[i + j]]
        extrema.append((used[0], used[-1]) if used else (255, 0))
    for i in bands:
        s, half = 0, count[i] // 2
        for j in range(256):
            s = s + h[i * 256 + j]
            if s > half:
                break
        median.append(j)
    var = [(total2[i] - (total[i] ** 2.0) / count[i]) / count[i] if count[i] else 0 for i in bands]
    return dict(count=count, sum=total, sum2=total2, median=median, extrema=extrema, var=var,
                mean=[total[i] / count[i] if count[i] else 0 for i in bands],
                rms=[math.sqrt(total2[i] / count[i]) if count[i] else 0 for i in bands],
                stddev=[math.sqrt(v) for v in var])


STAT_KEYS = ('count', 'sum', 'sum2', 'mean', 'median', 'rms', 'var', 'stddev', 'extrema')


def stats_stack(hists):
    """stats() of each of a stack of (bands, 256) histograms -> dict of arrays (n, bands) (extrema: (n, bands, 2))."""
    each = [stats(h) for h in hists]
    return {k: np.array([s[k] for s in each]) for k in STAT_KEYS}


# ---- the callers of terran_amd.image, per frame ------------------------------------------------------------------------
def equalize(img):
    return point(img, equalize_lut(histogram(img)))


def autocontrast(img, cutoff=0, ignore=None, preserve_tone=False):
    if preserve_tone:
        return point(img, np.tile(autocontrast_lut(histogram(img, 'L'), cutoff, ignore), 3))
    return point(img, autocontrast_lut(histogram(img), cutoff, ignore))


def brightness(img, factor):
    return blend(np.zeros_like(img), img, factor)


def contrast(img, factor):
    mean = int(stats(histogram(img, 'L'))['mean'][0] + 0.5)
    return blend(np.full_like(img, mean), img, factor)


def clipped_box(bbox, h, w, margin):
    x0, y0, x1, y1 = (float(v) for v in bbox)
    if margin:
        dx, dy = margin * (x1 - x0), margin * (y1 - y0)
        x0, y0, x1, y1 = x0 - dx, y0 - dy, x1 + dx, y1 + dy
    return max(int(x0), 0), max(int(y0), 0), min(int(x1), w), min(int(y1), h)


# ---- tests/golden/tone.npz ---------------------------------------------------------------------------------------------
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


def source(name, g=None):
    """A frame batch (N, H, W, 3) by its name in the golden's case lists: 'noise_HxW' and 'batch' are stored, the rest is
    regenerated: 'flat_HxW', 'ramp_HxW', 'two_HxW', 'dim' (of 'batch'), 'dim_small' (of 'small')."""
    g = g if g is not None else golden()
    if name in g:
        a = g[name]
        return a if a.ndim == 4 else a[None]
    if name == 'dim':
        return dim(g['batch'])
    if name == 'dim_small':
        return dim(g['small'])[None]
    kind, size = name.split('_')
    h, w = (int(v) for v in size.split('x'))
    return {'flat': flat, 'ramp': ramp, 'two': two_valued}[kind](h, w)[None]
