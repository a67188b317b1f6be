"""numpy restatement of csrc/transform.hip (ta_frames_transform, ta_frames_transpose): Pillow's `Image.transform` for the
AFFINE and PERSPECTIVE methods with the NEAREST, BILINEAR and BICUBIC filters, and `Image.transpose`, on uint8 RGB.  What
the kernels do, route by route (libImaging/Geometry.c), so the CPU suite can hold the arithmetic against Pillow without a
GPU and the GPU suite can hold the kernels against the recorded golden.  Needs numpy only.

All coordinate arithmetic is float64 without fused multiply-adds, as in Pillow's C:
    xin = x + 0.5, yin = y + 0.5
    affine       xs = a0 xin + a1 yin + a2,  ys = a3 xin + a4 yin + a5
    perspective  both divided by a6 xin + a7 yin + 1
A pixel whose source point fails 0 <= xs < W and 0 <= ys < H keeps the fill colour.  BILINEAR / BICUBIC: subtract 0.5,
floor, 2 x 2 / 4 x 4 taps clipped to the image.  NEAREST takes one of four routes:
    scale        affine with a1 == a3 == 0: ImagingScaleAffine, per-axis coordinates ACCUMULATED from a2 + a0 / 2 by a0
    fixed        other affine maps whose four output corners stay below 32768: 16.16 fixed point
    accumulate   the remaining affine maps: the double coordinate accumulated along x by a0, a3 and along y by a1, a4
    generic      perspective: (int) of the double coordinate
"""
import numpy as np

AFFINE, PERSPECTIVE = 0, 2
NEAREST, BILINEAR, BICUBIC = 0, 2, 3
FLIP_LEFT_RIGHT, FLIP_TOP_BOTTOM, ROTATE_90, ROTATE_180, ROTATE_270, TRANSPOSE, TRANSVERSE = range(7)


# ---- sources: formulas, so the golden's maker and the tests share them without storing them -------------------------------
def noise(h, w, seed):
    """Deterministic integer hash noise, uint8 (h, w, 3)."""
    y, x, c = np.meshgrid(np.arange(h, dtype=np.uint64), np.arange(w, dtype=np.uint64), np.arange(3, dtype=np.uint64), indexing='ij')
    m = np.uint64(0xFFFFFFFF)
    v = (x * np.uint64(73856093) + y * np.uint64(19349663) + c * np.uint64(83492791) + np.uint64(seed) * np.uint64(2654435761)) & m
    v ^= v >> np.uint64(15)
    v = (v * np.uint64(2246822519)) & m
    v ^= v >> np.uint64(13)
    v = (v * np.uint64(3266489917)) & m
    v ^= v >> np.uint64(16)
    return (v & np.uint64(255)).astype(np.uint8)


def blocks(h, w, seed):
    """Few grey levels in 5 x 4 blocks, no symmetry: compresses well and still tells every flip and rotation apart."""
    y, x, c = np.meshgrid(np.arange(h), np.arange(w), np.arange(3), indexing='ij')
    return (((x // 5) * 3 + (y // 4) * 5 + c * 2 + seed + (x // 5) * (y // 4)) % 8 * 36).astype(np.uint8)


def checkerboard(h=16, w=16):
    y, x = np.meshgrid(np.arange(h), np.arange(w), indexing='ij')
    return np.repeat((((x + y) % 2) * 255).astype(np.uint8)[..., None], 3, 2)


def sources():
    """[uint8 (N, H, W, 3)]: 0: 1 x 1 noise, 1: 2 x 3 (h x w), 2: three 37 x 53 frames, 3: 300 x 517, 4: the 16 x 16
    checkerboard of 0 and 255, 5: three 48 x 64 frames in blocks, 6: 37 x 53 in blocks, 7: 48 x 48 in blocks."""
    return [noise(1, 1, 1)[None], noise(2, 3, 2)[None], np.stack([noise(37, 53, 3 + k) for k in range(3)]),
            noise(300, 517, 6)[None], checkerboard()[None], np.stack([blocks(48, 64, 7 + k) for k in range(3)]),
            blocks(37, 53, 10)[None], blocks(48, 48, 11)[None]]


# ---- Image.transform ---------------------------------------------------------------------------------------------------
def coordinates(method, a, ow, oh):
    """The double source point of every output pixel centre: (xs, ys), each (oh, ow)."""
    a = [float(v) for v in a]
    xin = (np.arange(ow, dtype=np.float64) + 0.5)[None, :]
    yin = (np.arange(oh, dtype=np.float64) + 0.5)[:, None]
    xs = a[0] * xin + a[1] * yin + a[2]
    ys = a[3] * xin + a[4] * yin + a[5]
    if method == PERSPECTIVE:
        with np.errstate(divide='ignore', invalid='ignore'):
            d = a[6] * xin + a[7] * yin + 1
            xs, ys = xs / d, ys / d
    return xs, ys


def nearest_route(method, a, ow, oh):
    if method == PERSPECTIVE:
        return 'generic'
    if a[1] == 0 and a[3] == 0:
        return 'scale'

    def ok(x, y):
        return abs(x * a[0] + y * a[1] + a[2]) < 32768.0 and abs(x * a[3] + y * a[4] + a[5]) < 32768.0
    return 'fixed' if ok(0, 0) and ok(ow, oh) and ok(0, oh) and ok(ow, 0) else 'accumulate'


def _accumulated(start, step, n):
    """start, start + step, (start + step) + step, ...: n values, each sum rounded as a C loop rounds it."""
    return np.cumsum(np.concatenate([[start], np.full(max(n - 1, 0), step)]))[:n]


def _fix(v):
    v = v * 65536.0 + 0.5
    return int(np.floor(v)) if v < 0 else int(v)


def _nearest_indices(method, a, ow, oh, w, h):
    """-> (sy, sx, inside), each (oh, ow): the source pixel of every output pixel and whether it has one."""
    a = [float(v) for v in a]
    route = nearest_route(method, a, ow, oh)
    if route == 'generic':
        xs, ys = coordinates(method, a, ow, oh)
        inside = (xs >= 0) & (xs < w) & (ys >= 0) & (ys < h)
        return np.where(inside, ys, 0).astype(np.int64), np.where(inside, xs, 0).astype(np.int64), inside
    if route == 'scale':
        xs = _accumulated(a[2] + a[0] * 0.5, a[0], ow)[None, :] + np.zeros((oh, 1))
        ys = _accumulated(a[5] + a[4] * 0.5, a[4], oh)[:, None] + np.zeros((1, ow))
    elif route == 'fixed':
        f0, f1, f3, f4 = _fix(a[0]), _fix(a[1]), _fix(a[3]), _fix(a[4])
        f2, f5 = _fix(a[2] + a[0] * 0.5 + a[1] * 0.5), _fix(a[5] + a[3] * 0.5 + a[4] * 0.5)
        x, y = np.arange(ow, dtype=np.int64)[None, :], np.arange(oh, dtype=np.int64)[:, None]

        def wrap(v):                                    # int32 arithmetic
            return ((v + 2 ** 31) % 2 ** 32 - 2 ** 31) >> 16
        sx, sy = wrap(f2 + y * f1 + x * f0), wrap(f5 + y * f4 + x * f3)
        inside = (sx >= 0) & (sx < w) & (sy >= 0) & (sy < h)
        return np.where(inside, sy, 0), np.where(inside, sx, 0), inside
    else:
        x0 = _accumulated(a[2] + a[1] * 0.5 + a[0] * 0.5, a[1], oh)
        y0 = _accumulated(a[5] + a[4] * 0.5 + a[3] * 0.5, a[4], oh)
        xs = np.stack([_accumulated(x0[y], a[0], ow) for y in range(oh)])
        ys = np.stack([_accumulated(y0[y], a[3], ow) for y in range(oh)])
    inside = (xs >= 0) & (xs < w) & (ys >= 0) & (ys < h)
    return np.where(inside, ys, 0).astype(np.int64), np.where(inside, xs, 0).astype(np.int64), inside


def _cubic(v1, v2, v3, v4, d):
    p1 = v2
    p2 = -v1 + v3
    p3 = 2 * (v1 - v2) + v3 - v4
    p4 = -v1 + v2 - v3 + v4
    return p1 + d * (p2 + d * (p3 + d * p4))


def transform(image, size, method, data, resample=NEAREST, fill=None):
    """Image.fromarray(image).transform(size, method, data, resample, fillcolor=fill) as ta_frames_transform computes it."""
    image = np.asarray(image, np.uint8)
    h, w = image.shape[:2]
    ow, oh = size
    out = np.zeros((oh, ow, 3), np.uint8)
    if fill is not None:
        out[:] = np.asarray(fill, np.uint8)
    if resample == NEAREST:
        sy, sx, inside = _nearest_indices(method, data, ow, oh, w, h)
        out[inside] = image[sy[inside], sx[inside]]
        return out
    xs, ys = coordinates(method, data, ow, oh)
    inside = (xs >= 0) & (xs < w) & (ys >= 0) & (ys < h)                  # False for NaN
    xs, ys = xs[inside] - 0.5, ys[inside] - 0.5
    x, y = np.floor(xs), np.floor(ys)
    dx, dy = (xs - x)[:, None], (ys - y)[:, None]
    x, y = x.astype(np.int64), y.astype(np.int64)
    src = image.astype(np.float64)
    if resample == BILINEAR:
        x0, x1 = np.clip(x, 0, w - 1), np.clip(x + 1, 0, w - 1)
        y0, y1 = np.clip(y, 0, h - 1), np.clip(y + 1, 0, h - 1)
        v1 = src[y0, x0] + (src[y0, x1] - src[y0, x0]) * dx
        v2 = src[y1, x0] + (src[y1, x1] - src[y1, x0]) * dx
        out[inside] = (v1 + (v2 - v1) * dy).astype(np.uint8)                # in 0 .. 255: truncation
        return out
    if resample != BICUBIC:
        raise ValueError(resample)
    cols = [np.clip(x - 1 + k, 0, w - 1) for k in range(4)]
    rows = [_cubic(*[src[np.clip(y - 1 + r, 0, h - 1), c] for c in cols], dx) for r in range(4)]
    v = _cubic(*rows, dy)
    out[inside] = np.where(v <= 0.0, 0, np.where(v >= 255.0, 255, v)).astype(np.uint8)
    return out


def transpose(image, op):
    """Image.transpose(op) of a uint8 (H, W, 3) image (or of every image of a batch, the two axes before the last)."""
    a = np.asarray(image)
    if op == FLIP_LEFT_RIGHT:
        a = a[..., :, ::-1, :]
    elif op == FLIP_TOP_BOTTOM:
        a = a[..., ::-1, :, :]
    elif op == ROTATE_180:
        a = a[..., ::-1, ::-1, :]
    elif op in (ROTATE_90, ROTATE_270, TRANSPOSE, TRANSVERSE):
        t = np.swapaxes(a, -3, -2)
        a = {ROTATE_90: t[..., ::-1, :, :], ROTATE_270: t[..., :, ::-1, :], TRANSPOSE: t, TRANSVERSE: t[..., ::-1, ::-1, :]}[op]
    else:
        raise ValueError(op)
    return np.ascontiguousarray(a)


# ---- the golden ------------------------------------------------------------------------------------------------------------
def golden(path):
    """tests/golden/transform.npz -> (the npz, sources(), [transform case: dict(source (index), filter, size (w, h), fill
    (None or 3 ints), regions [(frame, method, 8 doubles)], expected (n, h, w, 3))], [transpose case: dict(source, op,
    expected)], [rotate case: dict(source, angle, expand, center, translate, filter, expected (h, w, 3))])."""
    z = np.load(path)
    cases, at = [], 0
    for k, n in enumerate(z['tf_count']):
        rows = z['tf_regions'][at:at + n]
        at += n
        fill = z['tf_fill'][k]
        cases.append(dict(source=int(z['tf_source'][k]), filter=int(z['tf_filter'][k]), size=tuple(int(v) for v in z['tf_size'][k]),
                          fill=None if fill[0] < 0 else tuple(int(v) for v in fill),
                          regions=[(int(r[0]), int(r[1]), tuple(float(v) for v in r[2:10])) for r in rows], expected=z['tf_%d' % k]))
    transposes = [dict(source=int(s), op=int(op), expected=z['tp_%d' % k]) for k, (s, op) in enumerate(z['tp_cases'])]
    rotates = []
    for k, r in enumerate(z['rot_cases']):
        moved = bool(r[3])
        rotates.append(dict(source=int(r[0]), angle=float(r[1]), expand=bool(r[2]), center=(10, 7) if moved else None,
                            translate=(3, -2) if moved else None, filter=int(r[4]), expected=z['rot_%d' % k]))
    return z, sources(), cases, transposes, rotates
