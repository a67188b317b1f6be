"""The contract of terran_amd.vis.blur_faces / anonymize_faces / ta_frames_blur restated in numpy (no Pillow, no GPU):

    region = im.crop(box).filter(ImageFilter.GaussianBlur(radius)); im.paste(region, box)

for the clipped int() box of every face, in list order, optionally under ImageDraw.ellipse's coverage of the box.
Pillow's Gaussian blur (libImaging/BoxBlur.c) is three box passes along the rows and three along the columns, each rounded
to uint8; its set-up is float32 arithmetic with double literals, restated here operation by operation."""
import math

import numpy as np

from tests import vis_raster as V

f32 = np.float32
BOX, ELLIPSE = 0, 1
SHAPES = {'box': BOX, 'ellipse': ELLIPSE}


def box_radius(radius):
    """_gaussian_blur_radius(radius, passes=3): float variables, double literals -> float32."""
    radius = f32(radius)
    s2 = f32(f32(radius * radius) / f32(3))
    L = f32(math.sqrt(12.0 * float(s2) + 1.0))
    l = f32(math.floor((float(L) - 1.0) / 2.0))
    a = f32(f32(f32(2) * l + f32(1)) * f32(f32(l * f32(l + f32(1))) - f32(f32(3) * s2)))
    a = f32(a / f32(f32(6) * f32(s2 - f32(f32(l + f32(1)) * f32(l + f32(1))))))
    return f32(l + a)


def weights(fr):
    """-> (r, ww, fw): the window's whole radius, the weight of a window pixel (a float32 division, truncated) and of the
    two pixels beside the window (uint32 arithmetic), 2^24 = 1."""
    fr = f32(fr)
    r = int(fr)
    ww = int(f32(1 << 24) / f32(f32(fr * f32(2)) + f32(1)))
    fw = (((1 << 24) - (2 * r + 1) * ww) & 0xffffffff) // 2
    return r, ww, fw


def box_pass(a, fr):
    """One pass along axis 1 of a (lines, n, C) uint8 array, indices clamped to [0, n - 1]."""
    r, ww, fw = weights(fr)
    n = a.shape[1]
    pad = a[:, np.clip(np.arange(-r - 1, n + r + 1), 0, n - 1)].astype(np.uint64)     # pad[i] = p[i - r - 1]
    cs = np.concatenate([np.zeros_like(pad[:, :1]), np.cumsum(pad, 1)], 1)           # cs[i] = sum pad[:i]
    x = np.arange(n)
    acc = cs[:, x + 2 * r + 2] - cs[:, x + 1]                                          # p[x - r .. x + r]
    far = pad[:, x] + pad[:, x + 2 * r + 2]
    return ((((acc * ww + far * fw) & 0xffffffff) + (1 << 23) & 0xffffffff) >> 24).astype(np.uint8)


def gaussian_blur(img, radius):
    """Image.fromarray(img).filter(ImageFilter.GaussianBlur(radius)) of a uint8 (h, w, 3) array."""
    if f32(radius) == 0:
        return img.copy()
    fr = box_radius(radius)
    a = img
    for _ in range(3):
        a = box_pass(a, fr)
    a = a.transpose(1, 0, 2)
    for _ in range(3):
        a = box_pass(a, fr)
    return np.ascontiguousarray(a.transpose(1, 0, 2))


def ellipse_mask(h, w):
    """ImageDraw.Draw(Image.new('L', (w, h))).ellipse([0, 0, w - 1, h - 1], fill=255) == 255."""
    m = np.zeros((h, w), bool)
    for y, x0, x1 in V.ellipse_runs([0, 0, w - 1, h - 1]):
        m[y, x0:x1 + 1] = True
    return m


def face_regions(faces, h, w, radius=None, margin=0.0, shape='box'):
    """The contract's steps 1-4 for the faces of one h x w frame -> [(x0, y0, x1, y1, radius, shape code)], empty
    regions skipped."""
    out = []
    for face in faces if isinstance(faces, (list, tuple)) else [faces]:
        x0, y0, x1, y1 = (float(v) for v in face['bbox'])
        if margin:
            dx, dy = margin * (x1 - x0), margin * (y1 - y0)
            x0, y0, x1, y1 = x0 - dx, y0 - dy, x1 + dx, y1 + dy
        x0, y0, x1, y1 = max(int(x0), 0), max(int(y0), 0), min(int(x1), w), min(int(y1), h)
        if x1 <= x0 or y1 <= y0:
            continue
        out.append((x0, y0, x1, y1, max(x1 - x0, y1 - y0) / 8 if radius is None else radius, SHAPES[shape]))
    return out


def blur_region(img, x0, y0, x1, y1, radius, shape):
    """One region of one frame, in place."""
    crop = img[y0:y1, x0:x1]
    blurred = gaussian_blur(crop, radius)
    if shape == ELLIPSE:
        m = ellipse_mask(y1 - y0, x1 - x0)
        crop[m] = blurred[m]
    else:
        crop[...] = blurred
    return img


def blur_regions(frames, regions):
    """Apply a lib.BLUR_DT array to host frames (N, H, W, 3) in place, in list order."""
    for q in regions:
        blur_region(frames[int(q['frame'])], int(q['x0']), int(q['y0']), int(q['x1']), int(q['y1']), float(q['radius']),
                    int(q['shape']))
    return frames


def anonymize(img, faces, radius=None, margin=0.0, shape='box'):
    """A blurred copy of img: what vis.anonymize_faces returns."""
    img = np.array(img, np.uint8, copy=True)
    for q in face_regions(faces, img.shape[0], img.shape[1], radius, margin, shape):
        blur_region(img, *q)
    return img


def rounds(regions):
    """Round of every region of a BLUR_DT array: one after the latest round of an earlier region of its frame that it
    intersects (rounds run in order; the regions of one round are disjoint within their frame)."""
    out = []
    for i, q in enumerate(regions):
        k = 0
        for j in range(i):
            e = regions[j]
            if e['frame'] == q['frame'] and q['x0'] < e['x1'] and e['x0'] < q['x1'] and q['y0'] < e['y1'] and e['y0'] < q['y1']:
                k = max(k, out[j] + 1)
        out.append(k)
    return out


# ---- tests/golden/vis_blur.npz ----------------------------------------------------------------------------------------
def golden_scenes(path):
    """-> (Pillow version, [scene dict]): name, base, faces (list of dicts, or one dict), radius (None: the default),
    margin, shape, expected."""
    z = np.load(path)
    out = []
    for s, name in enumerate(z['names']):
        faces = [{'bbox': b} for b in z['%d_bbox' % s]]
        radius = float(z['radii'][s])
        out.append(dict(name=str(name), base=z['%d_base' % s], expected=z['%d_expected' % s],
                        faces=faces[0] if z['single'][s] else faces, radius=None if radius < 0 else radius,
                        margin=float(z['margins'][s]), shape=str(z['shapes'][s])))
    return str(z['pillow_version']), out
