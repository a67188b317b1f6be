"""Generate tests/golden/jpeg_encode_optimize.npz: RGB images and the JPEG files the installed Pillow writes for them
with optimize=True (per-image Huffman tables).

Needs Pillow (recorded with Pillow 12 and its bundled libjpeg-turbo 3.1).  Each fixture is `Image.fromarray(px).save(f,
'JPEG', quality=q, subsampling=s, optimize=True)`; s = -1 is `save(f, 'JPEG', optimize=True)` with Pillow's defaults.
A 1 x 1 image; 17 x 9 and 250 x 33 in every subsampling and the default; flat (one DC symbol and EOB: tables with a
single real symbol), gradient, saturated (all 0xFF), noise at q100 (hundreds of symbols) and crops of rw-1.jpg;
qualities 1, 30, 75, 90, 100; three 40 x 56 frames (flat, gradient, noise) under one set of options, for a batch; and
`deep`, built block by block in the DCT domain so that the luma AC symbol counts grow faster than Fibonacci numbers:
its unlimited Huffman tree is deeper than 16 (asserted here through the model), so the length-limiting step runs.

npz keys as in jpeg_encode.npz: `names`, `pillow`; per name `px_<name>`, `opt_<name>` [quality, subsampling],
`jpg_<name>`.

    python tests/golden/make_golden_jpeg_encode_optimize.py
"""
import io
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

from tests import jpeg_encode_model as M                       # noqa: E402
from tests import jpeg_encode_optimize_model as O              # noqa: E402
from tests.golden.make_golden_jpeg_encode import content       # noqa: E402

QUALITIES = [1, 30, 75, 90, 100]
CONTENT = ['flat', 'gradient', 'saturated', 'noise']


def deep_image(quality, seed=3):
    """Grey (so Y is the grey value, Cb = Cr = 128) blocks that each quantise, at `quality`, to chosen coefficients:
    14 symbols (one AC of size 1 or 2 after a run of 3..9) whose counts each exceed the sum of all before them but
    one, then EOB, and 0x21 / 0x11 / 0x01 from blocks with every 3rd / 2nd / every AC set to +-1."""
    rng = np.random.default_rng(seed)
    q = M.quant_tables(quality)[0].astype(np.float64)
    k = np.arange(8)
    basis = np.cos((2 * k[:, None] + 1) * k[None, :] * np.pi / 16) * np.where(k == 0, np.sqrt(0.5), 1.0)[None, :] / 2

    def block(zz):                                             # 64 quantised values in zigzag order -> 8 x 8 samples
        nat = np.zeros(64)
        nat[M.ZIGZAG] = zz
        return basis @ (nat * q).reshape(8, 8) @ basis.T
    blocks = []
    for i, count in enumerate([1, 2, 4, 6, 10, 16, 26, 42, 68, 110, 178, 288, 466, 754]):
        run, mag = 3 + i // 2, 1 + (i % 2) * 2
        for _ in range(count):
            zz = np.zeros(64)
            zz[run + 1] = mag * rng.choice([-1, 1])
            blocks.append(block(zz))
    for step, count in ((3, 105), (2, 133), (1, 102)):
        for _ in range(count):
            zz = np.zeros(64)
            idx = np.arange(step, 64, step)
            zz[idx] = rng.choice([-1, 1], idx.size)
            blocks.append(block(zz))
    side = int(np.ceil(np.sqrt(len(blocks))))
    img = np.zeros((side * 8, side * 8))
    for n, b in enumerate(blocks):
        y, x = divmod(n, side)
        img[y * 8:y * 8 + 8, x * 8:x * 8 + 8] = b
    grey = np.clip(np.rint(img + 128), 0, 255).astype(np.uint8)
    return np.repeat(grey[:, :, None], 3, 2)


def tree_depths(px, quality, subsampling):
    """Longest code of each table's Huffman tree before the limit to 16 (DC 0, AC 0, DC 1, AC 1)."""
    H, W = px.shape[:2]
    dc, ac = O.histograms(M.coefficients(px, quality, subsampling), H, W, subsampling)
    return [max(O.unlimited_lengths(f)) for f in (dc[0], ac[0], dc[1], ac[1])]


def pillow_encode(px, quality, subsampling):
    from PIL import Image
    f = io.BytesIO()
    if subsampling == -1:
        Image.fromarray(px).save(f, 'JPEG', optimize=True)
    else:
        Image.fromarray(px).save(f, 'JPEG', quality=quality, subsampling=subsampling, optimize=True)
    return f.getvalue()


def fixtures():
    from PIL import Image
    out = [('flat_1x1_s2_q75', content('flat', 1, 1, 100), 75, 2)]
    k = 0
    for si, (h, w) in enumerate([(17, 9), (250, 33)]):
        for s in (0, 1, 2, -1):
            kind = CONTENT[(si + k) % 4]
            q = 75 if s == -1 else QUALITIES[k % len(QUALITIES)]
            out.append(('%s_%dx%d_s%d_q%d' % (kind, h, w, s, q), content(kind, h, w, 200 + k), q, s))
            k += 1
    for kind in CONTENT:                                       # every content at q100 4:4:4, and on an odd size at q30
        out.append(('%s_24x40_s0_q100' % kind, content(kind, 24, 40, 300 + k), 100, 0))
        out.append(('%s_17x23_s2_q30' % kind, content(kind, 17, 23, 400 + k), 30, 2))
        k += 1
    out.append(('noise_250x33_s1_q100', content('noise', 250, 33, 500), 100, 1))
    for kind in ('flat', 'gradient', 'noise'):                 # one batch: same size, same options, tables far apart
        out.append(('batch_%s_40x56_s2_q90' % kind, content(kind, 40, 56, 600 + len(kind)), 90, 2))
    rw1 = np.asarray(Image.open(os.path.join(HERE, 'rw-1.jpg')).convert('RGB'))
    for (y, x, h, w), q, s in [((40, 60, 72, 96), 90, 2), ((0, 0, 33, 47), 1, 0), ((30, 100, 64, 81), 75, 1)]:
        out.append(('rw-1_crop%dx%d_s%d_q%d' % (h, w, s, q), rw1[y:y + h, x:x + w].copy(), q, s))
    deep = deep_image(75)
    assert max(tree_depths(deep, 75, 0)) > 16, tree_depths(deep, 75, 0)
    out.append(('deep_%dx%d_s0_q75' % deep.shape[:2], deep, 75, 0))
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
    path = os.path.join(HERE, 'jpeg_encode_optimize.npz')
    np.savez_compressed(path, **arrays)
    print('%s: %d fixtures, %d bytes' % (path, len(names), os.path.getsize(path)))


if __name__ == '__main__':
    main()
