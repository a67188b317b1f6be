"""Generate tests/golden/jpeg_encode.npz: RGB images and the JPEG files the installed Pillow writes for them.

Needs Pillow (recorded with Pillow 12 and its bundled libjpeg-turbo 3.1).  Each fixture is `Image.fromarray(px).save(f,
'JPEG', quality=q, subsampling=s)`; s = -1 is `save(f, 'JPEG')` with Pillow's defaults.  Sizes 1 x 1 .. 250 x 33, each
subsampling, qualities 1 .. 100, flat / gradient / saturated (all 0xFF: every data byte stuffed) / noise content, and
crops of the quickstart photos rw-1.jpg / rw-2.jpg (decoded by Pillow).

npz keys: `names`, `pillow`; per name `px_<name>` (H, W, 3) uint8, `opt_<name>` [quality, subsampling],
`jpg_<name>` the file's bytes (uint8).

    python tests/golden/make_golden_jpeg_encode.py
"""
import io
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
SIZES = [(1, 1), (7, 5), (8, 8), (9, 17), (16, 16), (17, 9), (33, 250), (250, 33)]    # (H, W)
QUALITIES = [1, 5, 30, 50, 75, 90, 100]
CONTENT = ['flat', 'gradient', 'saturated', 'noise']


def content(kind, h, w, seed):
    rng = np.random.default_rng(seed)
    if kind == 'flat':
        return np.broadcast_to(rng.integers(0, 256, 3, dtype=np.uint8), (h, w, 3)).copy()
    if kind == 'gradient':
        y, x = np.mgrid[:h, :w]
        return np.stack([x * 255 // max(w - 1, 1), y * 255 // max(h - 1, 1), (x + y) * 7 % 256], -1).astype(np.uint8)
    if kind == 'saturated':
        return np.full((h, w, 3), 255, np.uint8)
    return rng.integers(0, 256, (h, w, 3), dtype=np.uint8)


def pillow_encode(px, quality, subsampling):
    from PIL import Image
    f = io.BytesIO()
    if subsampling == -1:
        Image.fromarray(px).save(f, 'JPEG')
    else:
        Image.fromarray(px).save(f, 'JPEG', quality=quality, subsampling=subsampling)
    return f.getvalue()


def fixtures():
    from PIL import Image
    out = []
    k = 0
    for si, (h, w) in enumerate(SIZES):
        for s in range(3):
            kind = CONTENT[(si + s) % 4]
            q = QUALITIES[(si * 3 + s) % len(QUALITIES)]
            out.append(('%s_%dx%d_s%d_q%d' % (kind, h, w, s, q), content(kind, h, w, k), q, s))
            k += 1
    for q in QUALITIES:                                    # every quality on every subsampling of one odd size
        for s in range(3):
            kind = CONTENT[(q + s) % 4]
            out.append(('%s_17x23_s%d_q%d' % (kind, s, q), content(kind, 17, 23, k), q, s))
            k += 1
    for kind in CONTENT:                                   # every content at the worst-case settings
        out.append(('%s_24x40_s0_q100' % kind, content(kind, 24, 40, k), 100, 0))
        k += 1
    out.append(('noise_40x24_default', content('noise', 40, 24, k), 75, -1))
    for name, (y, x, h, w), q, s in [('rw-1', (40, 60, 72, 96), 90, 2), ('rw-1', (0, 0, 33, 47), 50, 0),
                                     ('rw-2', (100, 120, 64, 81), 75, 1), ('rw-2', (7, 9, 57, 64), 95, 2)]:
        px = np.asarray(Image.open(os.path.join(HERE, name + '.jpg')).convert('RGB'))[y:y + h, x:x + w].copy()
        out.append(('%s_crop%dx%d_s%d_q%d' % (name, h, w, s, q), px, q, s))
    return out


def main():
    import PIL
    arrays = {'pillow': np.array(PIL.__version__)}
    names = []
    for name, px, q, s in fixtures():
        names.append(name)
        arrays['px_' + name] = px
        arrays['opt_' + name] = np.array([q, s], np.int32)
        arrays['jpg_' + name] = np.frombuffer(pillow_encode(px, q, s), np.uint8)
    arrays['names'] = np.array(names)
    path = os.path.join(HERE, 'jpeg_encode.npz')
    np.savez_compressed(path, **arrays)
    print('%s: %d fixtures, %d bytes' % (path, len(names), os.path.getsize(path)))


if __name__ == '__main__':
    main()
