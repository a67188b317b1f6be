"""numpy restatement of ta_frames_transform_mesh (csrc/transform.hip): Pillow's `Image.transform(size, MESH, [(box, quad),
...], resample, fillcolor=)` -- and QUAD, the mesh of the one cell ((0, 0) + size, quad) -- on uint8 RGB, so the CPU suite
can hold the arithmetic against Pillow without a GPU and the GPU suite the kernel against the recorded golden
(tests/golden/mesh.npz).  Needs numpy only.

The output starts as the fill colour (zeros without one).  The cells apply in list order.  A cell with box (x0, y0, x1, y1)
and quad (nw, sw, se, ne; x, y each) has, in float64 without fused multiply-adds and left to right,
    w = x1 - x0, h = y1 - y0, As = 1.0 / w, At = 1.0 / h
    a0 = nw.x, a1 = (ne.x - nw.x) As, a2 = (sw.x - nw.x) At, a3 = (se.x - sw.x - ne.x + nw.x) As At       (a4 .. a7: the y's)
and writes the pixels of its box CLAMPED to the output, with xin = (x - cx0) + 0.5, yin = (y - cy0) + 0.5 relative to the
clamped origin:  xs = a0 + a1 xin + a2 yin + a3 xin yin,  ys = a4 + a5 xin + a6 yin + a7 xin yin.  A point with
0 <= xs < W and 0 <= ys < H gives the pixel the filter's sample (the taps of tests/transform_model.py); a point outside
makes it 0 without a fill colour and leaves it as it is with one.
"""
import numpy as np

from tests import transform_model as T

NEAREST, BILINEAR, BICUBIC = T.NEAREST, T.BILINEAR, T.BICUBIC
FILTERS = (NEAREST, BILINEAR, BICUBIC)
TILE_W, TILE_H = 64, 16                                 # TA_MESH_TILE_W, TA_MESH_TILE_H


def coefficients(box, quad):
    """a0 .. a7 of a cell, as Image.__transformer derives them for QUAD."""
    x0, y0, x1, y1 = (int(v) for v in box)
    q = [float(v) for v in quad]
    nw, sw, se, ne = q[0:2], q[2:4], q[4:6], q[6:8]
    As, At = 1.0 / (x1 - x0), 1.0 / (y1 - y0)
    return (nw[0], (ne[0] - nw[0]) * As, (sw[0] - nw[0]) * At, (se[0] - sw[0] - ne[0] + nw[0]) * As * At,
            nw[1], (ne[1] - nw[1]) * As, (sw[1] - nw[1]) * At, (se[1] - sw[1] - ne[1] + nw[1]) * As * At)


def clamped(box, ow, oh):
    x0, y0, x1, y1 = (int(v) for v in box)
    return max(x0, 0), max(y0, 0), min(x1, ow), min(y1, oh)


def points(box, quad, ow, oh):
    """(xs, ys), each (cy1 - cy0, cx1 - cx0): the source point of every pixel of the clamped box (which must not be empty)."""
    a = coefficients(box, quad)
    cx0, cy0, cx1, cy1 = clamped(box, ow, oh)
    xin = (np.arange(cx0, cx1) - cx0 + 0.5)[None, :] + np.zeros((cy1 - cy0, 1))
    yin = (np.arange(cy0, cy1) - cy0 + 0.5)[:, None] + np.zeros((1, cx1 - cx0))
    return a[0] + a[1] * xin + a[2] * yin + a[3] * xin * yin, a[4] + a[5] * xin + a[6] * yin + a[7] * xin * yin


def sample(image, xs, ys, resample):
    """The filter's samples (n, 3) uint8 at points that passed the inside test: transform_model.transform's taps."""
    h, w = image.shape[:2]
    if resample == NEAREST:
        return image[ys.astype(np.int64), xs.astype(np.int64)]
    xs, ys = xs - 0.5, ys - 0.5
    x, y = np.floor(xs), np.floor(ys)
    dx, dy = (xs - x)[:, None], (ys - y)[:, None]
    x, y = x.astype(np.int64), y.astype(np.int64)
    src = image.astype(np.float64)
    if resample == BILINEAR:
        x0, x1 = np.clip(x, 0, w - 1), np.clip(x + 1, 0, w - 1)
        y0, y1 = np.clip(y, 0, h - 1), np.clip(y + 1, 0, h - 1)
        v1 = src[y0, x0] + (src[y0, x1] - src[y0, x0]) * dx
        v2 = src[y1, x0] + (src[y1, x1] - src[y1, x0]) * dx
        return (v1 + (v2 - v1) * dy).astype(np.uint8)
    if resample != BICUBIC:
        raise ValueError(resample)
    cols = [np.clip(x - 1 + k, 0, w - 1) for k in range(4)]
    rows = [T._cubic(*[src[np.clip(y - 1 + r, 0, h - 1), c] for c in cols], dx) for r in range(4)]
    v = T._cubic(*rows, dy)
    return np.where(v <= 0.0, 0, np.where(v >= 255.0, 255, v)).astype(np.uint8)


def mesh(image, size, cells, resample=NEAREST, fill=None):
    """Image.fromarray(image).transform(size, Image.MESH, cells, resample, fillcolor=fill)."""
    image = np.asarray(image, np.uint8)
    h, w = image.shape[:2]
    ow, oh = size
    out = np.zeros((oh, ow, 3), np.uint8)
    if fill is not None:
        out[:] = np.asarray(fill, np.uint8)
    for box, quad in cells:
        cx0, cy0, cx1, cy1 = clamped(box, ow, oh)
        if cx1 <= cx0 or cy1 <= cy0:
            continue
        xs, ys = points(box, quad, ow, oh)
        inside = (xs >= 0) & (xs < w) & (ys >= 0) & (ys < h)              # False for NaN
        region = out[cy0:cy1, cx0:cx1]
        if fill is None:
            region[~inside] = 0
        region[inside] = sample(image, xs[inside], ys[inside], resample)
    return out


def quad(image, size, q, resample=NEAREST, fill=None):
    """Image.transform(size, Image.QUAD, q, resample, fillcolor=fill)."""
    return mesh(image, size, [((0, 0, size[0], size[1]), q)], resample, fill)


def tile_lists(cells, ow, oh):
    """[the indices of the cells whose clamped box touches tile t, in list order] for the row-major TILE_W x TILE_H tiles."""
    tx_n, ty_n = -(-ow // TILE_W), -(-oh // TILE_H)
    lists = [[] for _ in range(tx_n * ty_n)]
    for k, (box, _) in enumerate(cells):
        cx0, cy0, cx1, cy1 = clamped(box, ow, oh)
        for t in range(tx_n * ty_n):
            ty, tx = divmod(t, tx_n)
            if cx0 < min((tx + 1) * TILE_W, ow) and tx * TILE_W < cx1 and cy0 < min((ty + 1) * TILE_H, oh) and ty * TILE_H < cy1:
                lists[t].append(k)
    return lists


def undistort_points(u, v, camera, dist, new_camera=None):
    """Brown-Conrady, float64: the source point (Pillow's corner coordinates) of the output point (u, v), scalars or arrays."""
    k = np.asarray(camera, np.float64)
    kn = k if new_camera is None else np.asarray(new_camera, np.float64)
    d = list(np.asarray(dist, np.float64)) + [0.0]
    k1, k2, p1, p2, k3 = d[:5]
    y = (np.asarray(v, np.float64) - 0.5 - kn[1, 2]) / kn[1, 1]
    x = (np.asarray(u, np.float64) - 0.5 - kn[0, 2] - kn[0, 1] * y) / kn[0, 0]
    r2 = x * x + y * y
    radial = 1 + k1 * r2 + k2 * r2 * r2 + k3 * r2 * r2 * r2
    xd = x * radial + 2 * p1 * x * y + p2 * (r2 + 2 * x * x)
    yd = y * radial + p1 * (r2 + 2 * y * y) + 2 * p2 * x * y
    return k[0, 0] * xd + k[0, 1] * yd + k[0, 2] + 0.5, k[1, 1] * yd + k[1, 2] + 0.5


# ---- the cases of the golden: formulas, so its maker and the tests share them without storing them ----------------------------
FILL = (7, 8, 9)


def sources():
    """[uint8 (N, H, W, 3)]: 0: 45 x 70 (h x w) noise, 1: 1 x 1, 2: one row of 23, 3: three 37 x 53 frames, 4: 33 x 48 in
    blocks."""
    return [T.noise(45, 70, 41)[None], T.noise(1, 1, 42)[None], T.noise(1, 23, 43)[None],
            np.stack([T.noise(37, 53, 44 + k) for k in range(3)]), T.blocks(33, 48, 5)[None]]


def lattice(ow, oh, step, w, h, wobble=0.18, reach=1.0):
    """A regular lattice of `step`-pixel cells over ow x oh (the last column and row narrower) whose vertices map into a
    w x h source through a smooth wobbling map; reach > 1 pushes the rim of the map outside the source."""
    xv = list(range(0, ow, step)) + [ow]
    yv = list(range(0, oh, step)) + [oh]

    def at(x, y):
        u, v = x / ow - 0.5, y / oh - 0.5
        return ((0.5 + reach * u * (1 + wobble * np.sin(5 * v + 1))) * w, (0.5 + reach * v * (1 + wobble * np.cos(4 * u + 2))) * h)
    cells = []
    for j in range(len(yv) - 1):
        for i in range(len(xv) - 1):
            nw, sw, se, ne = at(xv[i], yv[j]), at(xv[i], yv[j + 1]), at(xv[i + 1], yv[j + 1]), at(xv[i + 1], yv[j])
            cells.append(((xv[i], yv[j], xv[i + 1], yv[j + 1]), tuple(float(c) for c in nw + sw + se + ne)))
    return cells


def cases():
    """name -> (source index, (ow, oh), [mesh, ...], [(frame, mesh), ...]): what one ta_frames_transform_mesh call gets.  Each
    is recorded for the three filters and for fillcolor None and FILL."""
    W, H = 70, 45                                       # source 0
    inside_q = (5.5, 3.25, 2.0, 40.5, 66.0, 43.0, 61.5, 6.0)
    c = {}
    c['lattice'] = (0, (67, 35), [lattice(67, 35, 16, W, H)], [(0, 0)])                  # 16 does not divide 67 or 35
    c['ones'] = (0, (9, 5), [lattice(9, 5, 1, W, H)], [(0, 0)])                          # 1 x 1 cells
    c['quad'] = (0, (40, 30), [[((0, 0, 40, 30), inside_q)]], [(0, 0)])
    # the later cell's points fall outside the source on its left half: with a fill colour the earlier cell shows through
    c['overlap'] = (0, (40, 30), [[((0, 0, 40, 30), inside_q), ((10, 5, 30, 25), (-25.0, 4.0, -22.0, 39.0, 30.0, 41.0, 33.0, 2.0)),
                                   ((22, 0, 40, 12), (60.0, 1.0, 58.0, 20.0, 75.0, 22.0, 78.0, -4.0))]], [(0, 0)])
    c['gap'] = (0, (40, 30), [[((0, 0, 17, 22), (1.0, 1.0, 3.0, 30.0, 30.0, 33.0, 28.0, 2.0)),
                               ((23, 4, 40, 30), (35.0, 5.0, 33.0, 44.0, 69.0, 40.0, 66.0, 3.0))]], [(0, 0)])
    c['negative'] = (0, (40, 30), [[((-7, -5, 20, 18), (2.0, 2.0, 4.0, 40.0, 50.0, 42.0, 47.0, 3.0)),
                                    ((20, -9, 45, 30), (30.0, 1.0, 31.0, 44.0, 68.0, 41.0, 69.0, 0.5))]], [(0, 0)])
    c['past_edge'] = (0, (40, 30), [[((0, 0, 40, 30), inside_q), ((25, 20, 50, 43), (10.0, 10.0, 12.0, 35.0, 60.0, 33.0, 58.0, 8.0))]], [(0, 0)])
    c['outside'] = (0, (40, 30), [[((45, 0, 60, 10), inside_q), ((3, 2, 30, 28), inside_q), ((-20, -20, -1, -1), inside_q),
                                   ((0, 30, 40, 35), inside_q), ((40, 0, 41, 30), inside_q)]], [(0, 0)])
    c['mirror'] = (0, (40, 30), [[((0, 0, 40, 30), (61.5, 6.0, 66.0, 43.0, 2.0, 40.5, 5.5, 3.25))]], [(0, 0)])
    c['all_sides'] = (0, (40, 30), [[((0, 0, 40, 30), (-10.0, -8.0, -12.0, 54.0, 81.0, 52.0, 78.0, -9.0))]], [(0, 0)])
    for ow, oh in ((63, 15), (64, 16), (65, 17), (129, 33)):                             # around one tile, and 3 x 3 tiles
        c['tile_%d_%d' % (ow, oh)] = (0, (ow, oh), [lattice(ow, oh, 20, W, H, reach=1.15)], [(0, 0)])
    # 5 x 7 x 3 = 105 bytes an image: images 1 and 2 start off a dword, every row but each fourth does, and rows are ragged
    c['bytes'] = (3, (5, 7), [[((0, 0, 5, 4), (3.0, 2.0, 1.0, 30.0, 50.0, 35.0, 48.0, 1.0)), ((1, 3, 7, 9), (60.0, 10.0, -4.0, 12.0, -2.0, 30.0, 50.0, 33.0))]],
                  [(0, 0), (2, 0), (1, 0)])
    c['two_meshes'] = (3, (24, 16), [lattice(24, 16, 7, 53, 37, reach=1.1), [((2, 1, 20, 15), (50.0, 35.0, 48.0, 2.0, 3.0, 1.0, 5.0, 33.0)),
                                                                             ((12, 8, 30, 20), (0.0, 0.0, 0.0, 37.0, 53.0, 37.0, 53.0, 0.0))]],
                       [(2, 1), (0, 0), (1, 1), (0, 1), (2, 0), (2, 1)])
    c['empty_mesh'] = (3, (24, 16), [[], lattice(24, 16, 9, 53, 37)], [(1, 0), (1, 1)])
    c['source_1x1'] = (1, (9, 6), [[((0, 0, 9, 6), (-0.5, -0.5, -0.5, 1.5, 1.5, 1.5, 1.5, -0.5)), ((2, 2, 5, 4), (0.0, 0.0, 0.0, 1.0, 1.0, 1.0, 1.0, 0.0))]], [(0, 0)])
    c['source_row'] = (2, (20, 6), [lattice(20, 6, 4, 23, 1, reach=1.2)], [(0, 0)])
    return c


def expected(S, case, resample, fill):
    """The model's result of one case: (n_images, oh, ow, 3)."""
    src, size, meshes, images = case
    return np.stack([mesh(S[src][f], size, meshes[m], resample, fill) for f, m in images])


def pack(meshes):
    """[mesh, ...] -> (rows (x0, y0, x1, y1, 8 quad values) of all cells, mesh_first)."""
    rows = [tuple(box) + tuple(q) for m in meshes for box, q in m]
    first = np.concatenate([[0], np.cumsum([len(m) for m in meshes])]).astype(np.int32)
    return rows, first


# the public functions' cases
CAMERA = ((60.0, 0.0, 26.0), (0.0, 58.0, 18.5), (0.0, 0.0, 1.0))             # for the 37 x 53 frames of source 3
NEW_CAMERA = ((52.0, 0.0, 26.5), (0.0, 51.0, 18.0), (0.0, 0.0, 1.0))
DIST = (-0.28, 0.09, 0.002, -0.003, -0.01)
API_QUADS = [(5.5, 3.25, 2.0, 30.5, 46.0, 33.0, 41.5, 6.0), (51.0, 2.0, 50.0, 36.0, 1.0, 35.0, 3.0, 1.0), (-5.0, -4.0, 10.0, 41.0, 58.0, 30.0, 40.0, 3.0)]
API_EXTENTS = [(3.5, 2.25, 40.0, 30.0), (-4.0, -3.0, 60.0, 40.0), (10.0, 5.0, 12.0, 6.5)]
CHIP_QUADS = [[(5.0, 4.0, 6.0, 30.0, 40.0, 28.0, 38.0, 2.0), (50.0, 2.0, 20.0, 3.0, 22.0, 35.0, 49.0, 30.0)], [],
              [(0.0, 0.0, 0.0, 37.0, 53.0, 37.0, 53.0, 0.0)]]


class Deformer:
    """As ImageOps.deform takes it: the mesh depends on the size of the image it is asked about."""

    def getmesh(self, image):
        w, h = image.size
        assert (image.width, image.height) == (w, h)
        return lattice(w, h, 11, w, h, wobble=0.3)


def golden(path):
    """tests/golden/mesh.npz -> (the npz, sources(), cases(), {(name, filter, fill is None): expected})."""
    z = np.load(path)
    C = cases()
    want = {}
    for name in C:
        for f in FILTERS:
            for nofill in (True, False):
                want[name, f, nofill] = z['%s_%d_%d' % (name, f, int(nofill))]
    return z, sources(), C, want
