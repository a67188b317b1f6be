"""numpy restatement of the three drawing primitives of terran/vis/pillow.py and of Pillow's alpha blend.

Test infrastructure (the yardstick of tests/test_vis_cpu.py and tests/test_gpu_vis.py), written from Pillow's documented
behaviour and pinned black-box against the installed Pillow (test_vis_cpu.py's fuzz) -- not a copy of Pillow's C:

  rectangle(xy, rgba, width)  draw.rectangle(xy, outline=rgba, width=width)
  line(xy, rgba, width)       draw.line(xy, fill=rgba, width=width)
  ellipse(xy, rgba)           draw.ellipse(xy, fill=rgba)

on an RGB image drawn through ImageDraw.Draw(img, 'RGBA').  Each primitive becomes a list of horizontal runs
(y, x_lo, x_hi), unclipped, exactly as Pillow's rasteriser issues them (a pixel may be blended more than once within a
rectangle outline; never within a line or an ellipse); `apply` clips and blends them in order.  Everything that rounds
runs in the precision Pillow's C uses (float32 polygon scan, double wide-line geometry through libm's hypot).
"""
import math

import numpy as np

f32 = np.float32


def div255_blend(base, ink, a):
    """Pillow's BLEND: DIV255(in * (255 - a) + ink * a), DIV255(v) = ((v + 128) + ((v + 128) >> 8)) >> 8."""
    v = base.astype(np.int32) * (255 - a) + np.asarray(ink, np.int32) * a + 128
    return (((v >> 8) + v) >> 8).astype(np.uint8)


def apply(img, runs, rgba):
    """Blend `runs` [(y, x_lo, x_hi)] of one primitive into img (H, W, 3) uint8 in place, clipped to the image."""
    H, W = img.shape[:2]
    ink, a = np.asarray(rgba[:3], np.int32), int(rgba[3])
    for y, xa, xb in runs:
        if not 0 <= y < H:
            continue
        xa, xb = max(xa, 0), min(xb, W - 1)
        if xa <= xb:
            img[y, xa:xb + 1] = div255_blend(img[y, xa:xb + 1], ink, a)
    return img


def _coords(xy):
    xy = [float(v) for v in np.asarray(xy, np.float64).ravel()]
    return xy, [int(v) for v in xy]                       # C's (int): truncation toward zero


# ---- rectangle outline ------------------------------------------------------------------------------------------------
def thin_points(x0, y0, x1, y1):
    """Pillow's Bresenham line WITHOUT its end point: [(x, y)]."""
    pts = []
    dx, xs = (x1 - x0, 1) if x1 >= x0 else (x0 - x1, -1)
    dy, ys = (y1 - y0, 1) if y1 >= y0 else (y0 - y1, -1)
    if dx == 0:
        for _ in range(dy):
            pts.append((x0, y0))
            y0 += ys
    elif dy == 0:
        for _ in range(dx):
            pts.append((x0, y0))
            x0 += xs
    elif dx > dy:
        e = 2 * dy - dx
        for _ in range(dx):
            pts.append((x0, y0))
            if e >= 0:
                y0 += ys
                e -= 2 * dx
            e += 2 * dy
            x0 += xs
    else:
        e = 2 * dx - dy
        for _ in range(dy):
            pts.append((x0, y0))
            if e >= 0:
                x0 += xs
                e -= 2 * dy
            e += 2 * dx
            y0 += ys
    return pts


def rectangle_runs(xy, width):
    (fx0, fy0, fx1, fy1), (x0, y0, x1, y1) = _coords(xy)
    if fx1 < fx0:
        raise ValueError('x1 must be greater than or equal to x0')
    if fy1 < fy0:
        raise ValueError('y1 must be greater than or equal to y0')
    runs = []
    if width == 0:
        return runs
    for i in range(width):
        runs += [(y0 + i, x0, x1), (y1 - i, x0, x1)]
        for x in (x1 - i, x0 + i):
            runs += [(y, px, px) for px, y in thin_points(x, y0 + width, x, y1 - width + 1)]
    return runs


# ---- lines ------------------------------------------------------------------------------------------------------------
def _round_up_f(f):      # ROUND_UP on a float32: floor(f + 0.5F) away from zero, the sum in float32
    f = f32(f)
    return int(math.floor(f32(f + f32(0.5)))) if f >= 0 else -int(math.floor(f32(abs(f) + f32(0.5))))


def _round_down_f(f):
    f = f32(f)
    return int(math.ceil(f32(f - f32(0.5)))) if f >= 0 else -int(math.ceil(f32(abs(f) - f32(0.5))))


def _round_up_d(f):
    return int(math.floor(f + 0.5)) if f >= 0 else -int(math.floor(abs(f) + 0.5))


def _round_down_d(f):
    return int(math.ceil(f - 0.5)) if f >= 0 else -int(math.ceil(abs(f) - 0.5))


def _roundf(v):          # C roundf: halves away from zero
    return f32(math.floor(abs(v) + 0.5) * (1 if v >= 0 else -1))


def wide_line_quad(x0, y0, x1, y1, width):
    """The four integer vertices Pillow puts around a segment of `width` > 1 (double arithmetic, libm hypot)."""
    dx, dy = x1 - x0, y1 - y0
    big = float(np.hypot(float(dx), float(dy)))
    small = (width - 1) / 2.0
    rmax, rmin = _round_up_d(small) / big, _round_down_d(small) / big
    dxmin, dxmax = _round_down_d(rmin * dy), _round_down_d(rmax * dy)
    dymin, dymax = _round_down_d(rmin * dx), _round_down_d(rmax * dx)
    return [(x0 - dxmin, y0 + dymax), (x1 - dxmin, y1 + dymax), (x1 + dxmax, y1 - dymin), (x0 + dxmax, y0 - dymin)]


class _Edge:
    def __init__(self, a, b):
        (x0, y0), (x1, y1) = a, b
        self.x0, self.y0 = x0, y0
        self.xmin, self.xmax, self.ymin, self.ymax = min(x0, x1), max(x0, x1), min(y0, y1), max(y0, y1)
        self.dx = f32(0) if y0 == y1 else f32(f32(x1 - x0) / f32(y1 - y0))

    def x_at(self, y):
        return f32(f32(f32(y - self.y0) * self.dx) + f32(self.x0))


def polygon_runs(H, vertices):
    """Pillow's scanline fill of a polygon drawn with alpha: per row the sorted edge crossings, paired, rounded inwards,
    with a running x position so that no pixel of the row is blended twice, horizontal edges merged in."""
    n = len(vertices)
    es = [_Edge(vertices[i], vertices[(i + 1) % n]) for i in range(n)]
    ymin, ymax = H - 1, 0
    table = []
    for e in es:
        ymin, ymax = min(ymin, e.ymin), max(ymax, e.ymax)
        if e.ymin != e.ymax:
            table.append(e)
    ymin, ymax = max(ymin, 0), min(ymax, H)
    runs = []

    def horizontal(xpos, y):
        for e in es:
            if e.ymin == y == e.ymax:
                xmin = e.xmin
                if xpos != -1 and xpos < xmin:
                    continue
                if xpos > xmin:
                    xmin = xpos
                    if e.xmax < xmin:
                        continue
                runs.append((y, xmin, e.xmax))
                xpos = e.xmax + 1
        return xpos

    for y in range(ymin, ymax + 1):
        xx = []
        for i, cur in enumerate(table):
            if not cur.ymin <= y <= cur.ymax:
                continue
            xx.append(cur.x_at(y))
            if y == cur.ymax and y < ymax:
                xx.append(xx[-1])
            elif cur.dx != 0 and len(xx) % 2 == 1 and _roundf(xx[-1]) == xx[-1]:
                for oth in table[:i]:          # a corner of two edges running the same way: reach the next row's pixels
                    if (cur.dx > 0 and oth.dx <= 0) or (cur.dx < 0 and oth.dx >= 0):
                        continue
                    if xx[-1] == oth.x_at(y):
                        off = -1 if y == ymax else 1
                        a1 = cur.x_at(y + off)
                        if oth.ymin <= y + off <= oth.ymax:
                            a2 = oth.x_at(y + off)
                            if xx[-1] > f32(a1 + 1) and xx[-1] > f32(a2 + 1):
                                xx[-1] = f32(_roundf(max(a1, a2)) + 1)
                            elif xx[-1] < f32(a1 - 1) and xx[-1] < f32(a2 - 1):
                                xx[-1] = f32(_roundf(min(a1, a2)) - 1)
                            break
        xx.sort()
        xpos = -1 if not xx else 0
        for i in range(1, len(xx), 2):
            xe = _round_down_f(xx[i])
            if xe < xpos:
                continue
            xpos = horizontal(xpos, y)
            if xe < xpos:
                continue
            xs = _round_up_f(xx[i - 1])
            if xpos > xs:
                xs = xpos
                if xe < xs:
                    continue
            runs.append((y, xs, xe))
            xpos = xe + 1
        horizontal(xpos, y)
    return runs


def line_runs(H, xy, width):
    _, (x0, y0, x1, y1) = _coords(xy)
    if width <= 1:                                      # thin: Bresenham, then the end point
        return [(y, x, x) for x, y in thin_points(x0, y0, x1, y1) + [(x1, y1)]]
    if x0 == x1 and y0 == y1:
        return [(y0, x0, x0)]
    return polygon_runs(H, wide_line_quad(x0, y0, x1, y1, width))


# ---- ellipse ----------------------------------------------------------------------------------------------------------
class _Quarter:
    """Pillow's integer walk along a quarter of the ellipse with diameters (a, b), in doubled coordinates."""

    def __init__(self, a, b):
        self.fin = a < 0 or b < 0
        if not self.fin:
            self.cx, self.cy, self.ex, self.ey = a, b % 2, a % 2, b
            self.a2, self.b2 = a * a, b * b
            self.a2b2 = self.a2 * self.b2

    def _delta(self, x, y):
        return abs(self.a2 * y * y + self.b2 * x * x - self.a2b2)

    def next(self):
        if self.fin:
            return None
        out = (self.cx, self.cy)
        if self.cx == self.ex and self.cy == self.ey:
            self.fin = True
        else:
            nx, ny = self.cx, self.cy + 2
            nd = self._delta(nx, ny)
            if nx > 1:
                d = self._delta(self.cx - 2, self.cy + 2)
                if nd > d:
                    nx, ny, nd = self.cx - 2, self.cy + 2, d
                d = self._delta(self.cx - 2, self.cy)
                if nd > d:
                    nx, ny = self.cx - 2, self.cy
            self.cx, self.cy = nx, ny
        return out


def ellipse_runs(xy):
    (fx0, fy0, fx1, fy1), (x0, y0, x1, y1) = _coords(xy)
    if fx1 < fx0:
        raise ValueError('x1 must be greater than or equal to x0')
    if fy1 < fy0:
        raise ValueError('y1 must be greater than or equal to y0')
    a, b = x1 - x0, y1 - y0
    runs = []
    if a < 0 or b < 0 or a + b < 1:
        return runs
    q = _Quarter(a, b)
    pr, py = q.next()
    l = a % 2                                             # filled: no inner rim, the left end stays at the centre
    done = False
    while not done:
        y, r = py, pr
        while True:
            nxt = q.next()
            if nxt is None or nxt[1] > y:
                break
        if nxt is None:
            done = True
        else:
            pr, py = nxt
        parts = []
        if (l > 0 or r > 0) and y > 0:
            parts.append((2 if l == 0 else l, y, r))
        if y > 0:
            parts.append((-r, y, -l))
        if l > 0 or r > 0:
            parts.append((2 if l == 0 else l, -y, r))
        parts.append((-r, -y, -l))
        runs += [(y0 + (Y + b) // 2, x0 + (X0 + a) // 2, x0 + (X1 + a) // 2) for X0, Y, X1 in parts]
    return runs


# ---- drawing calls ----------------------------------------------------------------------------------------------------
def rectangle(img, xy, rgba, width):
    return apply(img, rectangle_runs(xy, width), rgba)


def line(img, xy, rgba, width):
    return apply(img, line_runs(img.shape[0], xy, width), rgba)


def ellipse(img, xy, rgba):
    return apply(img, ellipse_runs(xy), rgba)


# ---- the reference's vis_faces / vis_poses over these primitives -----------------------------------------------------
def render_faces(img, faces, scale, colormap):
    """terran/vis/pillow.py vis_faces' drawing (markers only) on a copy of img; `colormap` plays FACE_COLORMAP."""
    img = np.array(img, np.uint8, copy=True)
    for face in faces if isinstance(faces, (list, tuple)) else [faces]:
        rgb = tuple(colormap(face.get('name') or face.get('track')))
        rectangle(img, list(face['bbox']), rgb + (255,), int(3 * scale))
    return img


def render_poses(img, poses, scale, connections, connection_colors, keypoint_colors):
    img = np.array(img, np.uint8, copy=True)
    poses = poses if isinstance(poses, (list, tuple)) else [poses]
    for pose in poses:
        kps = pose['keypoints']
        for idx, (s, d) in enumerate(connections):
            xs, ys, ps = kps[s]
            xd, yd, pd = kps[d]
            if ps and pd:
                line(img, [xs, ys, xd, yd], tuple(connection_colors[idx]) + (180,), int(scale * 8))
    r = int(3 * int(scale * 4) / 2)
    for pose in poses:
        for idx, (x, y, p) in enumerate(pose['keypoints']):
            if p:
                ellipse(img, [x - r, y - r, x + r, y + r], tuple(keypoint_colors[idx]) + (225,))
    return img


# ---- the drawing primitives of ta_frames_draw (terran_amd.lib.PRIM_DT), restated -----------------------------------
def draw_prims(frames, prims):
    """Apply a PRIM_DT array to host frames (N, H, W, 3) in place, in order: BAR fills x0..x1 x y0..y1, LINE is
    draw.line([x0, y0, x1, y1], width=width), DISC is draw.ellipse([x0, y0, x1, y1])."""
    H = frames.shape[1]
    for p in prims:
        img, rgba, k = frames[int(p['frame'])], tuple(int(c) for c in p['rgba']), int(p['kind'])
        x0, y0, x1, y1 = int(p['x0']), int(p['y0']), int(p['x1']), int(p['y1'])
        if k == 0:
            runs = [(y, x0, x1) for y in range(max(y0, 0), min(y1, H - 1) + 1)]
        elif k == 1:
            runs = line_runs(H, [x0, y0, x1, y1], int(p['width']))
        else:
            runs = ellipse_runs([x0, y0, x1, y1])
        apply(img, runs, rgba)
    return frames


# ---- tests/golden/vis.npz ---------------------------------------------------------------------------------------------
def golden_scenes(path):
    """-> (npz, [scene dict]): kind, seed, scale, base, expected, and the inputs (faces or poses) of every scene."""
    from terran_amd import synth
    z = np.load(path)
    out = []
    for s, kind in enumerate(z['kinds']):
        kind = str(kind)
        h, w = (int(v) for v in z['shapes'][s])
        seed = int(z['seeds'][s])
        base = synth.frames(seed, 1, h, w)[0]
        exp = base.copy().reshape(-1, 3)
        idx = np.cumsum(z['%d_didx' % s].astype(np.int64))
        exp[idx] = (exp[idx] + z['%d_dval' % s]).astype(np.uint8)
        sc = dict(kind=kind, seed=seed, scale=float(z['scales'][s]), base=base, expected=exp.reshape(h, w, 3))
        if kind.startswith('faces'):
            faces = []
            for b, k, n, t in zip(z['%d_bbox' % s], z['%d_label_kind' % s], z['%d_name' % s], z['%d_track' % s]):
                d = {'bbox': b, 'score': np.float32(0.9)}
                if k == 1:
                    d['name'] = str(n)
                elif k == 2:
                    d['track'] = int(t)
                faces.append(d)
            sc['input'] = faces[0] if kind == 'faces_single' else faces
            sc['colors'] = z['%d_colors' % s]
        else:
            poses = [{'keypoints': k, 'score': 1.0} for k in z['%d_keypoints' % s]]
            sc['input'] = poses[0] if kind == 'poses_single' else poses
        out.append(sc)
    return z, out
