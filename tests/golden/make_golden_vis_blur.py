"""Generate tests/golden/vis_blur.npz with Pillow alone: the contract of terran_amd.vis.blur_faces / anonymize_faces.

Every scene holds a base frame (at most 96 x 128), faces, a radius (-1: the default, max(w, h) / 8 of the clipped region),
a margin, a shape, and the frame this loop leaves:

    for each face, in order:  box = int() of the bbox (widened by the margin), clipped to the frame; skipped when empty
        region = im.crop(box).filter(ImageFilter.GaussianBlur(radius))
        'box':      im.paste(region, box)
        'ellipse':  only where ImageDraw.Draw(Image.new('L', (w, h))).ellipse([0, 0, w - 1, h - 1], fill=255) is 255

Reads neither the reference nor this package.  The Pillow version is recorded in the file.

    python tests/golden/make_golden_vis_blur.py
"""
import os

import numpy as np
import PIL
from PIL import Image, ImageDraw, ImageFilter

HERE = os.path.dirname(os.path.abspath(__file__))


def base_frame(rng, h, w, kind):
    if kind == 0:                                       # noise: every rounding step matters
        return rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
    if kind == 1:                                       # black and white blocks: the extremes of the window sum
        cells = rng.integers(0, 2, ((h + 3) // 4, (w + 3) // 4, 3)) * 255
        return np.repeat(np.repeat(cells, 4, 0), 4, 1)[:h, :w].astype(np.uint8)
    walk = np.cumsum(rng.integers(-9, 10, (h, w, 3)), 1) + np.cumsum(rng.integers(-9, 10, (h, 1, 3)), 0) + 128
    return np.clip(walk, 0, 255).astype(np.uint8)       # smooth, clipped at both ends


def clipped_box(bbox, h, w, margin):
    x0, y0, x1, y1 = (float(v) for v in bbox)
    if margin:
        dx, dy = margin * (x1 - x0), margin * (y1 - y0)
        x0, y0, x1, y1 = x0 - dx, y0 - dy, x1 + dx, y1 + dy
    return max(int(x0), 0), max(int(y0), 0), min(int(x1), w), min(int(y1), h)


def expected(base, boxes, radius, margin, shape):
    im = Image.fromarray(base)
    h, w = base.shape[:2]
    done = 0
    for bbox in boxes:
        box = clipped_box(bbox, h, w, margin)
        bw, bh = box[2] - box[0], box[3] - box[1]
        if bw <= 0 or bh <= 0:
            continue
        crop = im.crop(box)
        region = crop.filter(ImageFilter.GaussianBlur(max(bw, bh) / 8 if radius < 0 else radius))
        if shape == 'ellipse':
            mask = Image.new('L', (bw, bh))
            ImageDraw.Draw(mask).ellipse([0, 0, bw - 1, bh - 1], fill=255)
            keep = (np.asarray(mask) != 255)[..., None]
            region = Image.fromarray(np.where(keep, np.asarray(crop), np.asarray(region)))
        im.paste(region, box)
        done += 1
    return np.asarray(im), done


def main():
    rng = np.random.default_rng(20261018)
    H, W = 96, 128
    scenes = []                                         # (name, (h, w), base kind, boxes, radius, margin, shape, single)

    def some_boxes(h, w, m):
        b = []
        for _ in range(m):
            x0, y0 = rng.uniform(0, w - 12), rng.uniform(0, h - 12)
            b.append([x0, y0, x0 + rng.uniform(5, w / 2), y0 + rng.uniform(5, h / 2)])
        return b
    for i, radius in enumerate([0.0, 0.25, 0.3, 1.0, 2.5, 12.3]):
        h, w = [(61, 83), (48, 64), (50, 71), (64, 64), (77, 101), (96, 128)][i]
        scenes.append(('radius_%g' % radius, (h, w), i % 3, some_boxes(h, w, 3), radius, 0.0, 'box', False))
    scenes.append(('radius_beyond_region', (40, 56), 0, [[3, 4, 13, 11], [20, 20, 23, 39], [30, 2, 55, 6]], 30.0, 0.0, 'box', False))
    thin = [[2, 2, 3, 30], [6, 2, 8, 30], [11, 2, 14, 30], [20, 3, 50, 4], [20, 7, 50, 9], [20, 12, 50, 15],
            [20, 20, 21, 21], [24, 20, 26, 22], [29, 20, 32, 23]]
    scenes.append(('thin_1_2_3', (36, 56), 0, thin, 2.5, 0.0, 'box', False))
    scenes.append(('thin_1_2_3_default', (36, 56), 2, thin, -1.0, 0.0, 'box', False))
    edges = [[-9.5, 20, 14.2, 44], [70, -12, 97.7, 9.9], [W - 21.5, 30, W + 15, 61], [40, H - 17.3, 66, H + 30],
             [-5, -5, 9, 9], [W - 8, H - 8, W + 8, H + 8], [-40, 50, -3, 70], [30, H + 1, 50, H + 9]]
    scenes.append(('off_every_edge', (H, W), 0, edges, -1.0, 0.0, 'box', False))
    scenes.append(('off_every_edge_ellipse', (H, W), 1, edges, 3.0, 0.1, 'ellipse', False))
    scenes.append(('whole_frame', (53, 67), 0, [[-3.2, -1, 80, 60]], -1.0, 0.0, 'box', False))
    scenes.append(('whole_frame_exact', (53, 67), 2, [[0, 0, 67, 53]], 5.0, 0.0, 'ellipse', False))
    over = [[10, 10, 50, 45], [30, 25, 75, 60]]
    scenes.append(('two_overlapping', (70, 90), 0, over, -1.0, 0.0, 'box', False))
    scenes.append(('two_overlapping_ellipse', (70, 90), 0, over + [[40, 5, 60, 66]], 4.0, 0.0, 'ellipse', False))
    ell = [[2, 2, 3, 31], [6, 2, 30, 3], [6, 6, 7, 7], [10, 6, 12, 8], [15, 6, 18, 9], [22, 6, 26, 10], [30, 4, 61, 27],
           [5, 33, 40, 47.9], [44, 30, 62, 48]]
    scenes.append(('ellipses_1xn', (50, 64), 0, ell, 2.0, 0.0, 'ellipse', False))
    scenes.append(('ellipses_default', (50, 64), 1, ell, -1.0, 0.0, 'ellipse', False))
    scenes.append(('margin', (80, 100), 0, [[30.6, 20.2, 60.1, 55.5], [70, 5, 95, 30]], -1.0, 0.25, 'box', False))
    scenes.append(('single_dict', (44, 60), 0, [[8.9, 5.5, 41.2, 39.99]], -1.0, 0.0, 'ellipse', True))

    out = {'pillow_version': np.array(PIL.__version__)}
    for s, (name, (h, w), kind, boxes, radius, margin, shape, single) in enumerate(scenes):
        base = base_frame(rng, h, w, kind)
        exp, done = expected(base, boxes, radius, margin, shape)
        out['%d_base' % s], out['%d_expected' % s] = base, exp
        out['%d_bbox' % s] = np.array(boxes, np.float64).reshape(-1, 4)
        print('%-26s %3d x %-3d  %d faces (%d blurred), %d pixels changed' % (name, h, w, len(boxes), done, (exp != base).any(-1).sum()))
    out.update({'names': np.array([s[0] for s in scenes]), 'radii': np.array([s[4] for s in scenes], np.float64),
                'margins': np.array([s[5] for s in scenes], np.float64), 'shapes': np.array([s[6] for s in scenes]),
                'single': np.array([s[7] for s in scenes], bool)})
    path = os.path.join(HERE, 'vis_blur.npz')
    np.savez_compressed(path, **out)
    print('%s: %d scenes, %d bytes, Pillow %s' % (path, len(scenes), os.path.getsize(path), PIL.__version__))


if __name__ == '__main__':
    main()
