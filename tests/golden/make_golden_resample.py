"""Generate tests/golden/resample.npz with Pillow alone: the contract of ta_frames_resample / ta_frames_pixelate and of
terran_amd.image.resize_frames, vis.crop_faces and vis.blur_faces(method='pixelate').

    resize cases    Image.fromarray(src[frame]).resize((w, h), filter, box=box) for lists of (frame, box) over a 3-frame
                    37 x 53 batch (whole frame, every border, fractional, narrower than a pixel, frames out of order),
                    every filter, outputs 1 x 1, 5 x 3, 64 x 48, one size kept per axis, both kept; a 1 x 1 source; a
                    300 x 517 source (`big_image`, a formula: not stored) shrunk to 7 x 5
    mixed           three images of different sizes resized to one size
    chips           the faces of a 2-frame batch cut out: box = int() of the bbox widened by the margin, clipped
    pixelate        for each face, in order: box as above; sw, sh = max(1, w // block), max(1, h // block);
                    region = im.crop(box).resize((sw, sh), BOX).resize((w, h), NEAREST); pasted whole ('box') or where
                    ImageDraw.ellipse([0, 0, w - 1, h - 1], fill=255) covers ('ellipse'); block -1: max(1, max(w, h) // 8)

Reads neither the reference nor this package.  The Pillow version is recorded in the file.

    python tests/golden/make_golden_resample.py
"""
import os

import numpy as np
import PIL
from PIL import Image, ImageDraw

HERE = os.path.dirname(os.path.abspath(__file__))
NEAREST, LANCZOS, BILINEAR, BICUBIC, BOX, HAMMING = range(6)

REGIONS = [(2, 0, 0, 53, 37), (0, 0, 0, 20.5, 37), (1, 30.25, 0, 53, 18.75), (2, 10.5, 20.25, 53, 37),
           (0, 7.3, 5.9, 41.2, 30.1), (1, 12.2, 9.4, 12.9, 9.9), (1, 0, 0, 53, 37), (0, 3, 4, 19, 25)]


def big_image(h=300, w=517):
    """Deterministic integer texture, the same in the tests."""
    y, x, c = np.meshgrid(np.arange(h), np.arange(w), np.arange(3), indexing='ij')
    return ((x * x * 3 + y * 7 + c * 85 + (x * y) % 251 + (y * y) % 97 * 2) % 256).astype(np.uint8)


def resize(img, size, filt, box):
    box = None if box is None else tuple(float(np.float32(v)) for v in box)
    return np.asarray(Image.fromarray(img).resize(size, filt, box=box))


def clipped_box(bbox, h, w, margin):
    x0, y0, x1, y1 = (float(v) for v in bbox)
    if margin:
        dx, dy = margin * (x1 - x0), margin * (y1 - y0)
        x0, y0, x1, y1 = x0 - dx, y0 - dy, x1 + dx, y1 + dy
    return max(int(x0), 0), max(int(y0), 0), min(int(x1), w), min(int(y1), h)


def pixelate(base, boxes, block, margin, shape):
    im = Image.fromarray(base)
    h, w = base.shape[:2]
    for bbox in boxes:
        box = clipped_box(bbox, h, w, margin)
        bw, bh = box[2] - box[0], box[3] - box[1]
        if bw <= 0 or bh <= 0:
            continue
        b = max(1, max(bw, bh) // 8) if block < 0 else block
        crop = im.crop(box)
        region = crop.resize((max(1, bw // b), max(1, bh // b)), BOX).resize((bw, bh), NEAREST)
        if shape == 'ellipse':
            mask = Image.new('L', (bw, bh))
            ImageDraw.Draw(mask).ellipse([0, 0, bw - 1, bh - 1], fill=255)
            keep = (np.asarray(mask) != 255)[..., None]
            region = Image.fromarray(np.where(keep, np.asarray(crop), np.asarray(region)))
        im.paste(region, box)
    return np.asarray(im)


def main():
    rng = np.random.default_rng(20261018)
    frames = rng.integers(0, 256, (3, 37, 53, 3), dtype=np.uint8)
    frames[1] = np.clip(np.cumsum(rng.integers(-9, 10, (37, 53, 3)), 1) + 128, 0, 255)      # smooth, clipped at both ends
    frames[2, ::2, ::3] = 255
    frames[2, 1::4, 1::2] = 0                                                               # extremes: the filters' overshoot
    tiny = rng.integers(0, 256, (1, 1, 1, 3), dtype=np.uint8)
    sources = [frames, tiny, big_image()[None]]
    out = {'pillow_version': np.array(PIL.__version__), 'frames': frames, 'tiny': tiny}
    cases = []                                          # (source, filter, (w, h), regions)
    for filt in range(6):
        cases.append((0, filt, (1, 1), REGIONS))
        cases.append((0, filt, (5, 3), REGIONS))
        cases.append((0, filt, (64, 48), REGIONS[:5]))
        cases.append((1, filt, (5, 3), [(0, 0, 0, 1, 1), (0, 0.25, 0.5, 0.75, 1)]))
    cases.append((2, LANCZOS, (7, 5), [(0, 0, 0, 517, 300)]))
    cases.append((2, BICUBIC, (3, 2), [(0, 100.5, 0, 517, 299.5)]))
    for filt in (BICUBIC, BOX, NEAREST):
        cases.append((0, filt, (53, 20), [REGIONS[0], REGIONS[6]]))                       # the horizontal pass is skipped
        cases.append((0, filt, (20, 37), [REGIONS[6], (0, 0, 0, 53, 37)]))                # the vertical one
        cases.append((0, filt, (53, 37), [REGIONS[0], REGIONS[3], REGIONS[6]]))           # both, next to a region with neither
    regions = []
    for k, (src, filt, size, regs) in enumerate(cases):
        out['rs_%d' % k] = np.stack([resize(sources[src][int(r[0])], size, filt, r[1:]) for r in regs])
        regions.extend(regs)
    out['rs_source'] = np.array([c[0] for c in cases], np.int32)
    out['rs_filter'] = np.array([c[1] for c in cases], np.int32)
    out['rs_size'] = np.array([c[2] for c in cases], np.int32)
    out['rs_count'] = np.array([len(c[3]) for c in cases], np.int32)
    out['rs_regions'] = np.array(regions, np.float64)

    # resize_frames: a batch with and without a box, a mixed-size list
    out['batch_lanczos_40x30'] = np.stack([resize(f, (40, 30), LANCZOS, None) for f in frames])
    out['batch_box'] = np.array([2.5, 1.25, 50.0, 36.5])
    out['batch_hamming_box_17x23'] = np.stack([resize(f, (17, 23), HAMMING, out['batch_box']) for f in frames])
    mixed = [frames[0], rng.integers(0, 256, (20, 31, 3), dtype=np.uint8), rng.integers(0, 256, (45, 17, 3), dtype=np.uint8)]
    out['mixed_1'], out['mixed_2'] = mixed[1], mixed[2]
    out['mixed_bilinear_32x24'] = np.stack([resize(m, (32, 24), BILINEAR, None) for m in mixed])

    # crop_faces: frames[:2], no face in frame 0, three in frame 1 (one partly outside, one wholly outside: skipped)
    faces = np.array([[4.7, 3.2, 25.9, 30.5], [40.5, 20.2, 70.0, 50.0], [-30, -30, -2, -2], [10, 8, 22.5, 21]], np.float64)
    out['chip_bbox'], out['chip_margin'] = faces, np.array(0.1)
    chips = []
    for bbox in faces:
        box = clipped_box(bbox, 37, 53, 0.1)
        if box[2] > box[0] and box[3] > box[1]:
            chips.append(resize(frames[1], (16, 20), BICUBIC, box))
    out['chips_bicubic_16x20'] = np.stack(chips)

    # pixelate scenes
    scenes = []                                         # (name, (h, w), boxes, block, margin, shape)
    two = [[5.5, 4.2, 40.9, 33.3], [30, 20, 60.7, 45]]
    scenes.append(('box_default', (48, 64), two, -1, 0.0, 'box'))
    scenes.append(('ellipse_default', (48, 64), two, -1, 0.0, 'ellipse'))
    scenes.append(('overlapping_block_3', (48, 64), two + [[20, 2, 36, 46]], 3, 0.0, 'box'))
    scenes.append(('overlapping_reversed', (48, 64), (two + [[20, 2, 36, 46]])[::-1], 3, 0.0, 'ellipse'))
    scenes.append(('block_beyond_box', (48, 64), [[3, 3, 12, 8], [20, 10, 60, 43]], 50, 0.0, 'box'))
    scenes.append(('block_beyond_box_ellipse', (48, 64), [[3, 3, 12, 8], [20, 10, 60, 43]], 50, 0.0, 'ellipse'))
    small = [[1, 1, 2, 2], [4, 1, 5, 10], [8, 1, 15, 6], [20, 1, 60, 34], [-5, 30, 9.5, 60], [50, 36, 80, 47.9]]
    scenes.append(('sizes_block_2', (48, 64), small, 2, 0.0, 'box'))
    scenes.append(('sizes_block_8_ellipse', (48, 64), small, 8, 0.0, 'ellipse'))
    scenes.append(('block_1', (48, 64), two, 1, 0.0, 'box'))
    scenes.append(('margin', (48, 64), [[20.6, 12.2, 40.1, 35.5]], -1, 0.25, 'box'))
    for s, (name, (h, w), boxes, block, margin, shape) in enumerate(scenes):
        base = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
        out['px_%d_base' % s], out['px_%d_bbox' % s] = base, np.array(boxes, np.float64).reshape(-1, 4)
        out['px_%d_expected' % s] = pixelate(base, boxes, block, margin, shape)
    out.update({'px_names': np.array([s[0] for s in scenes]), 'px_blocks': np.array([s[3] for s in scenes], np.int32),
                'px_margins': np.array([s[4] for s in scenes], np.float64), 'px_shapes': np.array([s[5] for s in scenes])})
    path = os.path.join(HERE, 'resample.npz')
    np.savez_compressed(path, **out)
    print('%s: %d resize cases, %d pixelate scenes, %d bytes, Pillow %s' % (path, len(cases), len(scenes), os.path.getsize(path), PIL.__version__))


if __name__ == '__main__':
    main()
