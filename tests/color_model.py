"""The contract of ta_frames_color / ta_color_plan and of the terran_amd.image colour callers restated in numpy (no Pillow,
no GPU), operation by operation as Pillow 12 does them on 'RGB' bytes:

    convert('RGB', m)       per output band float32 m0 r + m1 g + m2 b + m3, left to right, every product and sum rounded on
                            its own, then + 0.5; 0 at or below 0, 255 at or above 255, truncated between (libImaging/Matrix.c).
                            C adds the 0.5 as a double and rounds the sum to float32.  That equals the float32 addition: the
                            double sum of a float32 s and 0.5 is exact for 2^-30 <= |s| < 2^29 (the two fit 53 bits), so it
                            is rounded once; a smaller |s| gives 0.5 either way (it is far from the nearest float32
                            midpoint 0.5 +- 2^-25), and a larger one is at or beyond 255 in size either way.
    convert('YCbCr')        int16 tables at 6 fractional bits, entry (int)(c * 64 * i + 0.5): C's cast, which truncates
                            towards zero, so a negative entry is rounded UP; (T_R[r] + T_G[g] + T_B[b]) >> 6, + 128 for
                            chroma; c = 0.299, 0.587, 0.114 / -0.16874, -0.33126, 0.5 / 0.5, -0.41869, -0.08131
    'YCbCr' -> 'RGB'        entries (int)(c * 64 * (i - 128) + 0.5): R = Y + (T[Cr] >> 6) with 1.402, G = Y + ((T[Cb] + T[Cr])
                            >> 6) with -0.34414 and -0.71414, B = Y + (T[Cb] >> 6) with 1.772; clipped
    convert('HSV')          V = max, S = (int)((float32)(max - min) / max * 255.0), H from float32 rc, gc, bc:
                            h = bc - gc in float32, or 2.0 + rc - bc / 4.0 + gc - rc in double rounded to float32;
                            h = (float32)fmod(h / 6.0 + 1.0, 1.0) in double; H = (int)(h * 255.0)
    'HSV' -> 'RGB'          s == 0: grey; h6 = (double)(float32)h * 6.0 / 255.0, i = floor, f = (float32)(h6 - i),
                            fs = (float32)(s / 255.0); p, q, t = round-half-away((float32)(v * (1 - fs [* f | * (1 - f)])))
                            with the factor in double (float32 operands), clipped; selected on i % 6
    filter(Color3DLUT)      the table quantised to int16 at 6 fractional bits, trilinear in integers (see lut3d)

Both open points of the issue are settled by test_color_cpu against live Pillow over all 2^24 colours: the YCbCr entries
are truncated after adding 0.5 (not rounded to nearest), with the four-digit JFIF coefficients; the hue's 2.0 + rc - bc is
a double expression rounded to float32 before the division.

Regions are lib.COLOR_REGION_DT arrays: half-open boxes, applied in list order, under ImageDraw.ellipse's coverage of the
box for shape 1; ops are lib.COLOR_OP_DT arrays into one float32 table array.  Also the LUT formula of the exhaustive
cases and the loader of tests/golden/color.npz."""
import hashlib
import os

import numpy as np

from tests.vis_blur_model import ellipse_mask

f32, f64 = np.float32, np.float64
BOX, ELLIPSE = 0, 1
MATRIX, RGB2YCBCR, YCBCR2RGB, RGB2HSV, HSV2RGB, LUT3D = range(6)
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'color.npz')

# the matrices of the exhaustive cases: a sepia (all inside 0 .. 255 for most colours), and one with negative entries and
# offsets that clips at both ends
SEPIA = (0.393, 0.769, 0.189, 0.0, 0.349, 0.686, 0.168, 0.0, 0.272, 0.534, 0.131, 0.0)
WILD = (1.7, -0.9, 0.3, -40.25, -0.45, 1.31, 0.52, 12.5, 0.11, -1.6, 2.2, 90.0)
CONVERSIONS = {'ycbcr': RGB2YCBCR, 'rgb_from_ycbcr': YCBCR2RGB, 'hsv': RGB2HSV, 'rgb_from_hsv': HSV2RGB}


def all_colours():
    """The 4096 x 4096 frame of every colour: pixel k = y * 4096 + x is (k & 255, k >> 8 & 255, k >> 16)."""
    k = np.arange(1 << 24, dtype=np.uint32)
    return np.stack([k & 255, k >> 8 & 255, k >> 16], -1).astype(np.uint8).reshape(4096, 4096, 3)


def digest(a):
    return hashlib.sha256(np.ascontiguousarray(a, np.uint8).tobytes()).hexdigest()


# ---- matrix ------------------------------------------------------------------------------------------------------------
def matrix(img, m):
    m = np.asarray(m, f32).reshape(3, 4)
    r, g, b = (img[..., c].astype(f32) for c in range(3))
    out = []
    for k in range(3):
        v = m[k, 0] * r
        v = v + m[k, 1] * g
        v = v + m[k, 2] * b
        v = v + m[k, 3]
        v = v + f32(0.5)
        assert v.dtype == f32
        out.append(np.where(v <= 0, 0, np.where(v >= 255, 255, np.clip(v, 0, 255).astype(np.int32))))
    return np.stack(out, -1).astype(np.uint8)


# ---- YCbCr -------------------------------------------------------------------------------------------------------------
def _entries(c, i):
    return np.trunc(f64(c) * 64 * i + 0.5).astype(np.int32)


def ycbcr_tables():
    """int16 (13, 256): Y_R Y_G Y_B Cb_R Cb_G Cb_B Cr_R Cr_G Cr_B, then R_Cr G_Cb G_Cr B_Cb."""
    i = np.arange(256)
    fwd = [_entries(c, i) for c in (0.299, 0.587, 0.114, -0.16874, -0.33126, 0.5, 0.5, -0.41869, -0.08131)]
    inv = [_entries(c, i - 128) for c in (1.402, -0.34414, -0.71414, 1.772)]
    t = np.stack(fwd + inv)
    assert np.abs(t).max() < 32768
    return t.astype(np.int16)


def rgb_to_ycbcr(img):
    t = ycbcr_tables().astype(np.int32)
    r, g, b = (img[..., c] for c in range(3))
    y = (t[0][r] + t[1][g] + t[2][b]) >> 6
    cb = ((t[3][r] + t[4][g] + t[5][b]) >> 6) + 128
    cr = ((t[6][r] + t[7][g] + t[8][b]) >> 6) + 128
    return np.stack([y, cb, cr], -1).astype(np.uint8)       # Pillow casts; all three are inside 0 .. 255


def ycbcr_to_rgb(img):
    t = ycbcr_tables().astype(np.int32)
    y, cb, cr = img[..., 0].astype(np.int32), img[..., 1], img[..., 2]
    r = y + (t[9][cr] >> 6)
    g = y + ((t[10][cb] + t[11][cr]) >> 6)
    b = y + (t[12][cb] >> 6)
    return np.clip(np.stack([r, g, b], -1), 0, 255).astype(np.uint8)


# ---- HSV ---------------------------------------------------------------------------------------------------------------
def rgb_to_hsv(img):
    a = img.astype(np.int32)
    r, g, b = a[..., 0], a[..., 1], a[..., 2]
    mx, mn = a.max(-1), a.min(-1)
    grey = mx == mn
    cr = np.where(grey, 1, mx - mn).astype(f32)
    s = cr / np.where(grey, 1, mx).astype(f32)
    rc, gc, bc = ((mx - c).astype(f32) / cr for c in (r, g, b))
    assert s.dtype == f32 and rc.dtype == f32
    h_r = (bc - gc).astype(f32)
    h_g = ((2.0 + rc.astype(f64)) - bc.astype(f64)).astype(f32)
    h_b = ((4.0 + gc.astype(f64)) - rc.astype(f64)).astype(f32)
    h = np.where(r == mx, h_r, np.where(g == mx, h_g, h_b))
    h = np.fmod(h.astype(f64) / 6.0 + 1.0, 1.0).astype(f32)
    uh = np.clip((h.astype(f64) * 255.0).astype(np.int32), 0, 255)
    us = np.clip((s.astype(f64) * 255.0).astype(np.int32), 0, 255)
    return np.stack([np.where(grey, 0, uh), np.where(grey, 0, us), mx], -1).astype(np.uint8)


def _round_half_away(x):
    return np.where(x >= 0, np.floor(x + 0.5), np.ceil(x - 0.5)).astype(np.int32)


def hsv_to_rgb(img):
    h, s, v = (img[..., c].astype(np.int32) for c in range(3))
    h6 = h.astype(f32).astype(f64) * 6.0 / 255.0
    i = np.floor(h6)
    f = (h6 - i).astype(f32).astype(f64)
    fs = (s.astype(f64) / 255.0).astype(f32).astype(f64)
    vf = v.astype(f64)

    def level(x):
        return np.clip(_round_half_away((vf * x).astype(f32).astype(f64)), 0, 255)
    p, q, t = level(1.0 - fs), level(1.0 - fs * f), level(1.0 - fs * (1.0 - f))
    k = i.astype(np.int32) % 6
    pick = lambda six: np.choose(k, six)       # noqa: E731
    r, g, b = pick([v, q, p, p, t, v]), pick([t, v, v, q, p, p]), pick([p, p, t, v, v, q])
    grey = (s == 0)[..., None]
    return np.where(grey, v[..., None], np.stack([r, g, b], -1)).astype(np.uint8)


# ---- 3-D LUT -----------------------------------------------------------------------------------------------------------
def quantise(table):
    """The int16 entries libImaging interpolates (_prepare_lut_table): item = t * (255 << 6), a float32 product (in
    double 506 of 2^24 / 119 sampled colours of the 17^3 formula table come out one off); +-0x7fff at the ends, else
    rounded half away from zero."""
    item = (np.asarray(table, f32) * f32(255 << 6)).astype(f64)
    q = np.where(item < 0, np.ceil(item - 0.5), np.floor(item + 0.5))
    q = np.where(item >= 0x7fff - 0.5, 0x7fff, np.where(item <= -0x7fff + 0.5, -0x7fff, q))
    return q.astype(np.int16)


def lut3d(img, size, table):
    """filter(Color3DLUT(size, table)): size (s0, s1, s2), table float32 (s2, s1, s0, 3) flattened, R fastest."""
    s0, s1, s2 = (int(v) for v in size)
    t = quantise(table).astype(np.int64).reshape(s2, s1, s0, 3)
    idx, sh = [], []
    for c, s in enumerate((s0, s1, s2)):
        scale = int((s - 1) / 255.0 * (1 << 18))
        i = img[..., c].astype(np.int64) * scale
        idx.append(i >> 18)
        sh.append(((i & ((1 << 18) - 1)) >> 3)[..., None])
    assert all(int(i.max()) + 1 <= s - 1 for i, s in zip(idx, (s0, s1, s2)))      # no read leaves the table
    lerp = lambda a, b, w: (a * ((1 << 15) - w) + b * w) >> 15      # noqa: E731  (arithmetic shift of signed values)
    at = lambda dz, dy, dx: t[idx[2] + dz, idx[1] + dy, idx[0] + dx]      # noqa: E731
    ll, lr = lerp(at(0, 0, 0), at(0, 0, 1), sh[0]), lerp(at(0, 1, 0), at(0, 1, 1), sh[0])
    rl, rr = lerp(at(1, 0, 0), at(1, 0, 1), sh[0]), lerp(at(1, 1, 0), at(1, 1, 1), sh[0])
    x = lerp(lerp(ll, lr, sh[1]), lerp(rl, rr, sh[1]), sh[2])
    return np.clip((x + 32) >> 6, 0, 255).astype(np.uint8)


def formula_lut(size):
    """The table of the exhaustive and walk cases, + - x only in float64 and rounded to float32, so that every machine
    builds the same one: a channel rotation with cross terms; its values go below 0 (to -0.9), above 1 and, in the
    corner where r and b are large and g small, above 2.0 (int16 saturation at 32767 / 16320 = 2.0078)."""
    s0, s1, s2 = (int(v) for v in size)
    b, g, r = np.meshgrid(np.arange(s2) * (1.0 / (s2 - 1)), np.arange(s1) * (1.0 / (s1 - 1)), np.arange(s0) * (1.0 / (s0 - 1)), indexing='ij')
    out = np.stack([1.5 * g - 0.35 + 0.25 * r * b, 1.1 * b * b + 0.1 * r - 0.05, 2.6 * r * b - 0.9 * g * r + 0.2 * (1.0 - g)], -1)
    return out.astype(f32).reshape(-1)


# ---- ops, regions ------------------------------------------------------------------------------------------------------
def apply_op(img, op, tables):
    kind = int(op['kind'])
    if kind == MATRIX:
        return matrix(img, tables[op['table']:op['table'] + 12])
    if kind == LUT3D:
        size = [int(v) for v in op['size']]
        return lut3d(img, size, tables[op['table']:op['table'] + 3 * size[0] * size[1] * size[2]])
    return {RGB2YCBCR: rgb_to_ycbcr, YCBCR2RGB: ycbcr_to_rgb, RGB2HSV: rgb_to_hsv, HSV2RGB: hsv_to_rgb}[kind](img)


def color_regions(frames, regions, ops, tables):
    """Apply a lib.COLOR_REGION_DT array to host frames (N, H, W, 3) in place, in list order."""
    tables = np.asarray(tables, f32)
    for q in regions:
        crop = frames[q['frame']][q['y0']:q['y1'], q['x0']:q['x1']]
        h, w = crop.shape[:2]
        m = ellipse_mask(h, w) if q['shape'] == ELLIPSE else np.ones((h, w), bool)
        crop[m] = apply_op(crop, ops[q['op']], tables)[m]
    return frames


def plan_rounds(regions):
    """ta_color_plan's rounds: a region runs one round after the latest earlier region of its frame that it intersects."""
    rounds = []
    for i, q in enumerate(regions):
        r = 0
        for j in range(i):
            e = regions[j]
            if e['frame'] == q['frame'] and q['x0'] < e['x1'] and e['x0'] < q['x1'] and q['y0'] < e['y1'] and e['y0'] < q['y1']:
                r = max(r, rounds[j] + 1)
        rounds.append(r)
    return np.array(rounds, np.int32)


def hue_lut(shift):
    """point()'s table of hue_frames: (h + shift) mod 256 on band 0, identity on S and V."""
    i = np.arange(256)
    return np.concatenate([(i + int(shift)) % 256, i, i]).astype(np.uint8)


# ---- tests/golden/color.npz --------------------------------------------------------------------------------------------
_golden = None


def golden():
    """The recorded Pillow results, loaded once and shared (read-only arrays)."""
    global _golden
    if _golden is None:
        with np.load(GOLDEN) as z:
            _golden = {k: z[k] for k in z.files}
        for v in _golden.values():
            v.setflags(write=False)
    return _golden


def case_tables(g, name):
    """The float32 tables of a recorded case: stored, or (a case of 3-D table ops only) formula_lut of every op's size."""
    if name + '_tables' in g:
        return g[name + '_tables']
    return np.concatenate([formula_lut(op[1:4]) for op in g[name + '_ops']])


def case_ops(g, name, dtype):
    """The case's ops, rows (kind, s0, s1, s2, table), as a lib.COLOR_OP_DT array."""
    rows = g[name + '_ops']
    ops = np.zeros(len(rows), dtype)
    ops['kind'], ops['size'], ops['table'] = rows[:, 0], rows[:, 1:4], rows[:, 4]
    return ops


def case_regions(rows, dtype):
    q = np.zeros(len(rows), dtype)
    for k, name in enumerate(('frame', 'x0', 'y0', 'x1', 'y1', 'shape', 'op')):
        q[name] = rows[:, k] if len(rows) else 0
    return q
