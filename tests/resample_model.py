"""numpy restatement of the device arithmetic of csrc/resample.hip (ta_frames_resample, ta_frames_pixelate) on the tables
ta_resample_plan gives: integers only.  What the kernels do, pass by pass, so the CPU suite can hold the tables and the
arithmetic against Pillow without a GPU, and the GPU suite can hold the kernels against this."""
import numpy as np

from terran_amd import lib

PRECISION_BITS = 22


def convolve(src, bounds, coefs, axis):
    """One pass along `axis` (0: vertical, 1: horizontal) of a uint8 (H, W, 3) image: out sample i is
    clip8((2^21 + sum_t src[first_i + t] * coef[i, t]) >> 22) in int32."""
    src = np.moveaxis(np.asarray(src, np.uint8), axis, 0).astype(np.int32)
    out = np.zeros((len(bounds),) + src.shape[1:], np.uint8)
    for i, (first, count) in enumerate(bounds):
        acc = np.full(src.shape[1:], 1 << (PRECISION_BITS - 1), np.int32)
        for t in range(int(count)):
            acc = acc + src[first + t] * np.int32(coefs[i, t])          # int32, wrapping like the device's
        out[i] = np.clip(acc >> PRECISION_BITS, 0, 255)
    return np.moveaxis(out, 0, axis)


def resize(image, size, filter, box=None):
    """Image.fromarray(image).resize(size, filter, box=box) as ta_frames_resample computes it: the horizontal pass over the
    rows the vertical tables reference, then the vertical one; a pass is skipped when its size is unchanged and the box
    spans the whole axis; both skipped: a copy."""
    image = np.asarray(image, np.uint8)
    h, w = image.shape[:2]
    ow, oh = size
    x0, y0, x1, y1 = (np.float32(v) for v in (box if box is not None else (0, 0, w, h)))
    need_x = ow != w or x0 != 0 or x1 != w
    need_y = oh != h or y0 != 0 or y1 != h
    out = image
    yb = yc = None
    first = 0
    if need_y:
        yb, yc = lib.resample_plan(h, y0, y1, oh, filter)
        first, last = int(yb[:, 0].min()), int((yb[:, 0] + yb[:, 1]).max())
        out = out[first:last]
    if need_x:
        xb, xc = lib.resample_plan(w, x0, x1, ow, filter)
        out = convolve(out, xb, xc, 1)
    if need_y:
        yb = yb.copy()
        yb[:, 0] -= first
        out = convolve(out, yb, yc, 0)
    return out.copy()


def ellipse_mask(w, h):
    """ImageDraw.ellipse([0, 0, w - 1, h - 1], fill=) coverage as tests/vis_blur_model.py restates it."""
    from tests import vis_blur_model as B
    return B.ellipse_mask(h, w)


def pixelate_regions(frames, regions):
    """ta_frames_pixelate on host frames (N, H, W, 3), in place, regions (lib.PIXELATE_DT) in list order."""
    for q in regions:
        f, x0, y0, x1, y1 = (int(q[k]) for k in ('frame', 'x0', 'y0', 'x1', 'y1'))
        block = int(q['block'])
        if block == 1:
            continue
        w, h = x1 - x0, y1 - y0
        sw, sh = max(1, w // block), max(1, h // block)
        crop = frames[f, y0:y1, x0:x1].copy()
        big = resize(resize(crop, (sw, sh), lib.BOX), (w, h), lib.NEAREST)
        if int(q['shape']) == lib.BLUR_ELLIPSE:
            m = ellipse_mask(w, h)
            big = np.where(m[..., None], big, crop)
        frames[f, y0:y1, x0:x1] = big
    return frames


def big_image(h=300, w=517):
    """The deterministic texture of tests/golden/make_golden_resample.py (its strong-downscale source; not stored)."""
    y, x, c = np.meshgrid(np.arange(h), np.arange(w), np.arange(3), indexing='ij')
    return ((x * x * 3 + y * 7 + c * 85 + (x * y) % 251 + (y * y) % 97 * 2) % 256).astype(np.uint8)


def golden(path):
    """tests/golden/resample.npz -> (the npz, [resize case: dict(source (N, H, W, 3), filter, size (w, h), regions
    (lib.RESAMPLE_DT), expected (n, h, w, 3))], [pixelate scene: dict(name, base, faces, block, margin, shape, expected)])."""
    z = np.load(path)
    sources = [z['frames'], z['tiny'], big_image()[None]]
    cases, at = [], 0
    for k, n in enumerate(z['rs_count']):
        rows = z['rs_regions'][at:at + n]
        at += n
        regions = np.zeros(n, lib.RESAMPLE_DT)
        regions['frame'] = rows[:, 0]
        for c, name in enumerate(('x0', 'y0', 'x1', 'y1'), 1):
            regions[name] = rows[:, c]
        cases.append(dict(source=sources[int(z['rs_source'][k])], filter=int(z['rs_filter'][k]),
                          size=tuple(int(v) for v in z['rs_size'][k]), regions=regions, expected=z['rs_%d' % k]))
    scenes = []
    for s, name in enumerate(z['px_names']):
        block = int(z['px_blocks'][s])
        scenes.append(dict(name=str(name), base=z['px_%d_base' % s], faces=[{'bbox': b} for b in z['px_%d_bbox' % s]],
                           block=None if block < 0 else block, margin=float(z['px_margins'][s]),
                           shape=str(z['px_shapes'][s]), expected=z['px_%d_expected' % s]))
    return z, cases, scenes


def resample_regions(source, regions, size, filter):
    """ta_frames_resample on host frames: (n, h, w, 3)."""
    return np.stack([resize(source[int(q['frame'])], size, filter, (q['x0'], q['y0'], q['x1'], q['y1'])) for q in regions])
