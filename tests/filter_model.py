"""The contract of ta_frames_filter and of the terran_amd.image / terran_amd.vis filter callers restated in numpy (no
Pillow, no GPU), operation by operation as Pillow 12 does them (libImaging Filter.c, RankFilter.c, UnsharpMask.c):

    Kernel((s, s), kernel, scale, offset)   k = float32 kernel / float32 scale, ss = float32 offset + 0.5; kernel row j goes
                            with image row y + s // 2 - j; a row's products are summed left to right, then added to ss, every
                            multiply and add rounded to float32; 0 if ss <= 0, 255 if ss >= 255, else truncated.  The outer
                            s // 2 pixels keep their values; an image narrower or shorter than s is copied.
    ImageEnhance.Sharpness  Image.blend(im.filter(SMOOTH), im, factor)   (tone_model.blend)
    RankFilter(s, rank)     per band the rank-th smallest of the s x s window over the edge-replicated image
    UnsharpMask(r, p, t)    b = GaussianBlur(r) (vis_blur_model); d = in - b; in where |d| <= t, else clip(in + d * p / 100) with
                            C's integer division

Regions are lib.FILTER_REGION_DT arrays with lib.FILTER_SPEC_DT specs: half-open boxes, applied in list order, the filter
seeing the box's own pixels only, pasted under ImageDraw.ellipse's coverage of the box for shape 1.  Also the loader of
tests/golden/filter.npz and the sources it does not store (flat, ramp and two-valued frames, from tone_model)."""
import os

import numpy as np

from tests import tone_model as T
from tests.vis_blur_model import gaussian_blur

f32 = np.float32
BOX, ELLIPSE = 0, 1
KERNEL, RANK, UNSHARP = 0, 1, 2
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'filter.npz')
TILE_W, TILE_H, HALO = 128, 32, 3                   # csrc/filter.hip's tile and its widest halo (rank size 7)
WIDTHS, HEIGHTS = [1, 2, 3, 4, 5, 6, 53, 64, 257], [1, 2, 3, 5, 6, 37]
SHARPNESS = [0.0, 0.5, 1.0, 1.7, 2.0, -0.5, 3.3]
RANKS = [(3, 0), (3, 4), (3, 8), (5, 3), (5, 12), (7, 24), (7, 48), (1, 0)]
UNSHARPS = [(2, 150, 3), (1.3, 73, 0), (5, 500, 10), (0.4, 33, 1)]


def normalise(spec):
    """-> (float32 (size * size,) kernel / scale, float32 offset + 0.5): what the host hands to the device."""
    n = int(spec['size']) ** 2
    k = spec['kernel'][:n].astype(f32) / f32(spec['scale'])
    off = f32(spec['offset']) + f32(0.5)
    assert k.dtype == f32 and off.dtype == f32
    return k, off


def clip8(ss):
    return np.where(ss <= 0, 0, np.where(ss >= 255, 255, np.clip(ss, 0, 255).astype(np.int32))).astype(np.uint8)


def convolve(img, size, k, ss0):
    """im.filter(Kernel) of a uint8 (h, w, 3) array with the normalised kernel k and ss0 = offset + 0.5."""
    h, w = img.shape[:2]
    r = size // 2
    out = img.copy()
    if w < size or h < size:
        return out
    p = img.astype(f32)
    ss = np.full((h - 2 * r, w - 2 * r, 3), ss0, f32)
    for j in range(size):
        rows = p[2 * r - j:h - j]
        acc = rows[:, 0:w - 2 * r] * k[j * size]
        for i in range(1, size):
            acc = acc + rows[:, i:w - 2 * r + i] * k[j * size + i]
        ss = ss + acc
        assert acc.dtype == f32 and ss.dtype == f32
    out[r:h - r, r:w - r] = clip8(ss)
    return out


def rank_filter(img, size, rank):
    h, w = img.shape[:2]
    r = size // 2
    ys, xs = np.clip(np.arange(-r, h + r), 0, h - 1), np.clip(np.arange(-r, w + r), 0, w - 1)
    pad = img[ys][:, xs]
    win = np.stack([pad[j:j + h, i:i + w] for j in range(size) for i in range(size)])
    return np.sort(win, 0)[rank]


def unsharp(img, radius, percent, threshold):
    a, b = img.astype(np.int64), gaussian_blur(img, radius).astype(np.int64)
    d = a - b
    moved = d * int(percent)
    moved = a + np.sign(moved) * (np.abs(moved) // 100)            # C's division truncates towards zero
    return np.where(np.abs(d) <= threshold, a, np.clip(moved, 0, 255)).astype(np.uint8)


def apply_spec(img, spec):
    """im.filter(F) (has_factor: ImageEnhance.Sharpness' blend) of a uint8 (h, w, 3) array for one FILTER_SPEC_DT record."""
    kind = int(spec['kind'])
    if kind == KERNEL:
        k, off = normalise(spec)
        out = convolve(img, int(spec['size']), k, off)
        return T.blend(out, img, spec['factor']) if spec['has_factor'] else out
    if kind == RANK:
        return rank_filter(img, int(spec['size']), int(spec['rank']))
    assert kind == UNSHARP
    return unsharp(img, spec['radius'], spec['percent'], spec['threshold'])


def filter_regions(frames, regions, specs):
    """Apply a lib.FILTER_REGION_DT array to host frames (N, H, W, 3) in place, in list order."""
    for q in regions:
        crop = frames[q['frame']][q['y0']:q['y1'], q['x0']:q['x1']]
        m = T.mask_of(crop.shape[0], crop.shape[1], q['shape'])
        crop[m] = apply_spec(crop.copy(), specs[q['spec']])[m]
    return frames


# ---- tests/golden/filter.npz -------------------------------------------------------------------------------------------
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
    """A frame batch (N, H, W, 3) by its name in the golden's case list: 'noise_HxW', 'tile_HxW', 'batch' and 'small' are
    stored, 'flat_HxW', 'ramp_HxW' and 'two_HxW' are regenerated."""
    g = g if g is not None else golden()
    if name in g:
        a = g[name]
        return a if a.ndim == 4 else a[None]
    kind, size = name.split('_')
    h, w = (int(v) for v in size.split('x'))
    return {'flat': T.flat, 'ramp': T.ramp, 'two': T.two_valued}[kind](h, w)[None]


def regions_of(rows, dt):
    """int (n, 7) rows (frame, x0, y0, x1, y1, shape, spec) -> a lib.FILTER_REGION_DT array."""
    q = np.zeros(len(rows), dt)
    for k, name in enumerate(('frame', 'x0', 'y0', 'x1', 'y1', 'shape', 'spec')):
        q[name] = rows[:, k] if len(rows) else 0
    return q


def cases(g=None):
    """[(name, source name, int (n, 7) region rows, expected (N, H, W, 3))] in the file's order; a case without a stored
    result expects its source (a blend factor of 1)."""
    g = g if g is not None else golden()
    out = []
    for i, (name, src) in enumerate(zip(g['case_names'], g['case_sources'])):
        key = 'case_%d_expected' % i
        out.append((str(name), str(src), g['case_%d_regions' % i], g[key] if key in g else source(str(src), g)))
    return out
