"""The raw YUV conversions of include/terran_amd.h (ta_frames_from_yuv, ta_frames_to_yuv) restated in numpy: the standards'
affine maps with exact rational coefficients, rounded once, half up.  Exact integer arithmetic: every map is brought over
its reduced common denominator and evaluated in int64 with numpy's floor division, and an assertion bounds every
numerator.  It reads no Pillow and no reference; ffmpeg's swscale computes something else (tables at fewer bits)."""
from fractions import Fraction as F
from math import lcm

import numpy as np

FORMATS = ('yuv420p', 'nv12', 'yuv444p')
MATRICES = {'bt601': (F(299, 1000), F(114, 1000)), 'bt709': (F(2126, 10000), F(722, 10000))}
RANGES = {'tv': (16, 219, 224), 'pc': (0, 255, 255)}           # luma offset, luma span, chroma span


def rgb_rows(matrix, range):
    """255 X' + 1/2 for X = R, G, B as ((coefficient of Y, of Cb, of Cr), constant), Fractions."""
    kr, kb = MATRICES[matrix]
    kg = 1 - kr - kb
    y0, ys, cs = RANGES[range]
    ay = F(255, ys)
    rows = [(ay, F(0), 255 * 2 * (1 - kr) / cs),
            (ay, -255 * 2 * kb * (1 - kb) / kg / cs, -255 * 2 * kr * (1 - kr) / kg / cs),
            (ay, 255 * 2 * (1 - kb) / cs, F(0))]
    return [(c, -c[0] * y0 - 128 * (c[1] + c[2]) + F(1, 2)) for c in rows]


def yuv_rows(matrix, range):
    """v + 1/2 for v = Y, Cb, Cr as ((coefficient of R, of G, of B), constant), Fractions."""
    kr, kb = MATRICES[matrix]
    kg = 1 - kr - kb
    y0, ys, cs = RANGES[range]
    sy, sb, sr = F(ys, 255), F(cs, 255) / (2 * (1 - kb)), F(cs, 255) / (2 * (1 - kr))
    return [((sy * kr, sy * kg, sy * kb), y0 + F(1, 2)),
            ((-sb * kr, -sb * kg, sb * (1 - kb)), 128 + F(1, 2)),
            ((sr * (1 - kr), -sr * kg, -sr * kb), 128 + F(1, 2))]


def _affine(row, a, b, c, k=None):
    """clip(floor(c0 + (c[0] a + c[1] b + c[2] c) / k), 0, 255) as uint8; a, b, c integer arrays, k an integer array or None (1)."""
    coef, c0 = row
    q = lcm(c0.denominator, *[x.denominator for x in coef])
    n = [int(x * q) for x in coef]
    n0 = int(c0 * q)
    a, b, c = (np.asarray(v).astype(np.int64) for v in (a, b, c))
    k = np.int64(1) if k is None else np.asarray(k).astype(np.int64)
    top = max(int(np.max(v, initial=0)) for v in (a, b, c))
    assert (sum(abs(x) for x in n) * top + abs(n0) * int(np.max(k))) < 2 ** 62 and q * int(np.max(k)) < 2 ** 62, 'int64 overflow'
    num = n0 * k + n[0] * a + n[1] * b + n[2] * c
    return np.clip(num // (q * k), 0, 255).astype(np.uint8)


def yuv_to_rgb(y, cb, cr, matrix='bt709', range='tv'):
    """(..., 3) uint8 RGB of 8-bit Y, Cb, Cr arrays of one shape."""
    return np.stack([_affine(r, y, cb, cr) for r in rgb_rows(matrix, range)], axis=-1)


def rgb_to_yuv(r, g, b, matrix='bt709', range='tv', k=None):
    """(..., 3) uint8 Y, Cb, Cr of R, G, B -- or of the SUMS r, g, b of k pixels each: the exact mean, rounded once."""
    return np.stack([_affine(row, r, g, b, k) for row in yuv_rows(matrix, range)], axis=-1)


def chroma_size(h, w):
    return (h + 1) >> 1, (w + 1) >> 1


def frame_bytes(fmt, h, w):
    ch, cw = chroma_size(h, w)
    return {'yuv420p': w * h + 2 * cw * ch, 'nv12': w * h + 2 * cw * ch, 'yuv444p': 3 * w * h}[fmt]


def join_planes(fmt, y, u, v):
    """One frame's bytes from its planes: y (h, w); u, v (ch, cw) for the 4:2:0 formats, (h, w) for yuv444p."""
    if fmt == 'nv12':
        return np.concatenate([y.reshape(-1), np.stack([u, v], axis=-1).reshape(-1)]).astype(np.uint8)
    return np.concatenate([y.reshape(-1), u.reshape(-1), v.reshape(-1)]).astype(np.uint8)


def split_planes(fmt, frame, h, w):
    """The planes y, u, v of one frame's bytes."""
    frame = np.asarray(frame, np.uint8).reshape(-1)
    assert frame.size == frame_bytes(fmt, h, w)
    y = frame[:h * w].reshape(h, w)
    if fmt == 'yuv444p':
        return y, frame[h * w:2 * h * w].reshape(h, w), frame[2 * h * w:].reshape(h, w)
    ch, cw = chroma_size(h, w)
    if fmt == 'nv12':
        uv = frame[h * w:].reshape(ch, cw, 2)
        return y, uv[..., 0], uv[..., 1]
    return y, frame[h * w:h * w + ch * cw].reshape(ch, cw), frame[h * w + ch * cw:].reshape(ch, cw)


def upsample_chroma(c, h, w, chroma='bilinear', siting='left'):
    """The 8-bit chroma of every pixel of an h x w frame from its (ch, cw) plane; every index clamped to the plane."""
    c = np.asarray(c).astype(np.int64)
    ch, cw = c.shape
    ys, xs = np.arange(h), np.arange(w)
    if chroma == 'nearest':
        return c[(ys >> 1)[:, None], (xs >> 1)[None, :]].astype(np.uint8)
    assert chroma == 'bilinear'
    j = ys >> 1
    v = 3 * c[j] + c[np.clip(np.where(ys % 2 == 0, j - 1, j + 1), 0, ch - 1)]          # (h, cw), in quarters
    i = xs >> 1
    if siting == 'left':
        s = np.where(xs % 2 == 0, 2 * v[:, i], v[:, i] + v[:, np.clip(i + 1, 0, cw - 1)])
        return ((s + 4) >> 3).astype(np.uint8)
    assert siting == 'center'
    s = 3 * v[:, i] + v[:, np.clip(np.where(xs % 2 == 0, i - 1, i + 1), 0, cw - 1)]
    return ((s + 8) >> 4).astype(np.uint8)


def from_yuv(data, n, h, w, fmt='yuv420p', matrix='bt709', range='tv', chroma='bilinear', siting='left'):
    """(n, h, w, 3) uint8 RGB of n raw frames."""
    data = np.asarray(data, np.uint8).reshape(n, frame_bytes(fmt, h, w))
    out = np.empty((n, h, w, 3), np.uint8)
    for f in np.arange(n):
        y, u, v = split_planes(fmt, data[f], h, w)
        if fmt != 'yuv444p':
            u, v = upsample_chroma(u, h, w, chroma, siting), upsample_chroma(v, h, w, chroma, siting)
        out[f] = yuv_to_rgb(y, u, v, matrix, range)
    return out


def to_yuv(frames, fmt='yuv420p', matrix='bt709', range='tv'):
    """(n, frame_bytes) uint8 raw frames of (n, h, w, 3) uint8 RGB."""
    frames = np.asarray(frames, np.uint8)
    n, h, w = frames.shape[:3]
    out = np.empty((n, frame_bytes(fmt, h, w)), np.uint8)
    ch, cw = chroma_size(h, w)
    pad = np.zeros((n, 2 * ch, 2 * cw, 4), np.int64)                   # R, G, B and a one per pixel inside the frame
    pad[:, :h, :w, :3] = frames
    pad[:, :h, :w, 3] = 1
    sums = pad.reshape(n, ch, 2, cw, 2, 4).sum(axis=(2, 4))
    for f in np.arange(n):
        full = rgb_to_yuv(frames[f, ..., 0], frames[f, ..., 1], frames[f, ..., 2], matrix, range)
        if fmt == 'yuv444p':
            out[f] = join_planes(fmt, full[..., 0], full[..., 1], full[..., 2])
        else:
            sub = rgb_to_yuv(sums[f, ..., 0], sums[f, ..., 1], sums[f, ..., 2], matrix, range, k=sums[f, ..., 3])
            out[f] = join_planes(fmt, full[..., 0], sub[..., 1], sub[..., 2])
    return out
