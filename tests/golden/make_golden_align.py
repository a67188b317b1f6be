"""Generate tests/golden/align.npz with Pillow alone: what the aligned-crop kernel (csrc/arcface_post.hip warp_kernel) and
the Pillow-bicubic resize of resident frames (ta_frames_resize_bicubic on csrc/resample.hip's kernels) have to reproduce at
their edges.

    warp cases     Image.fromarray(src).transform((112, 112), Image.AFFINE, matrix, resample=Image.BILINEAR, fillcolor=0),
                   the call of the reference's aligned crop; `warp_names` lists them in order
    bicubic cases  Image.fromarray(src).resize((w, h)) with the default filter (BICUBIC)

Every source is uniform byte noise from a fixed seed: the truncation to uint8 only shows on busy pixels.  The maker asserts
what each case is there for (how much of a crop is fill colour, which source points the border cases reach).  Reads neither
the reference nor this package.

    python tests/golden/make_golden_align.py
"""
import math
import os

import numpy as np
import PIL
from PIL import Image

HERE = os.path.dirname(os.path.abspath(__file__))
SIDE = 112


def noise(seed, h, w):
    return np.random.default_rng(seed).integers(0, 256, (h, w, 3), dtype=np.uint8)


def similarity(scale, degrees, cx, cy):
    """The 6 coefficients (crop pixel -> source point) of a rotation by `degrees` and a scale, crop centre on (cx, cy)."""
    c, s = scale * math.cos(math.radians(degrees)), scale * math.sin(math.radians(degrees))
    return (c, -s, cx - (c - s) * SIDE / 2, s, c, cy - (s + c) * SIDE / 2)


def warp_cases():
    """[(name, source, matrix)]"""
    sq = noise(100, 64, 64)
    cases = [
        ('identity', noise(101, SIDE, SIDE), (1, 0, 0, 0, 1, 0)),
        ('shift_minus_half', sq, (1, 0, -0.5, 0, 1, -0.5)),         # source point 0 at crop pixel 0: tap -1 is clamped
        ('shift_plus_half', sq, (1, 0, 0.5, 0, 1, 0.5)),            # source point 64 at crop pixel 63: the first reject
    ]
    # half a source pixel per crop pixel, turned by 10 degrees, the crop's centre 12 pixels inside a corner: about half fill
    for name, cx, cy in (('corner_top_left', 12, 12), ('corner_top_right', 52, 12), ('corner_bottom_left', 12, 52),
                         ('corner_bottom_right', 52, 52)):
        cases.append((name, sq, similarity(0.5, 10, cx, cy)))
    cases += [
        ('outside', sq, (1, 0, 64 + 5, 0, 1, 0)),
        ('source_1x1', noise(102, 1, 1), (0.01, 0.002, -0.3, 0.003, 0.008, -0.2)),
        ('source_1x40', noise(103, 1, 40), (0.4, 0.03, -2.0, 0.004, 0.006, -0.2)),          # 1 row, 40 columns
        ('source_40x1', noise(104, 40, 1), (0.004, 0.006, -0.2, 0.4, 0.03, -2.0)),          # 40 rows, 1 column
        ('transpose', sq, (0, 1, 0, 1, 0, 0)),
        ('turn_180', sq, (-1, 0, 64, 0, -1, 64)),
        ('rotate_45', sq, similarity(0.5, 45, 32, 32)),
        ('magnify_20', sq, (0.05, 0, 20.3, 0, 0.05, 31.7)),          # 5.6 source pixels across the crop
        ('minify_3', noise(105, 96, 96), similarity(3.0, 7, 48, 48)),
    ]
    return cases


def source_points(matrix, h, w):
    a = [float(v) for v in matrix]
    xin, yin = np.arange(SIDE)[None, :] + 0.5, np.arange(SIDE)[:, None] + 0.5
    sx, sy = a[0] * xin + a[1] * yin + a[2], a[3] * xin + a[4] * yin + a[5]
    return sx, sy, (sx >= 0) & (sx < w) & (sy >= 0) & (sy < h)


def warp(src, matrix):
    return np.asarray(Image.fromarray(src).transform((SIDE, SIDE), Image.AFFINE, tuple(float(v) for v in matrix),
                                                     resample=Image.BILINEAR, fillcolor=0))


# (source width, source height) -> (width, height); the 40 x 31 cases share one source
BICUBIC = (((96, 80), (12, 10)),            # reduction by 8: 33 coefficients per output pixel
           ((9, 7), (45, 35)),
           ((1, 33), (5, 33)),
           ((33, 1), (33, 5)),
           ((40, 31), (40, 17)),            # width unchanged: no horizontal pass
           ((40, 31), (23, 31)),            # height unchanged: no vertical pass
           ((40, 31), (40, 31)))            # the copy


def main():
    out = {'pillow_version': np.array(PIL.__version__)}
    cases = warp_cases()
    inside_share = {}
    for k, (name, src, matrix) in enumerate(cases):
        out['warp_src_%d' % k] = src
        out['warp_out_%d' % k] = warp(src, matrix)
        inside_share[name] = source_points(matrix, *src.shape[:2])[2].mean()
    out['warp_names'] = np.array([c[0] for c in cases])
    out['warp_matrix'] = np.array([c[2] for c in cases], np.float64)
    # what the cases are there for
    assert inside_share['identity'] == 1.0 and inside_share['outside'] == 0.0
    assert not out['warp_out_%d' % [c[0] for c in cases].index('outside')].any()
    assert all(0.4 < inside_share[n] < 0.6 for n in inside_share if n.startswith('corner_')), inside_share
    assert all(0 < inside_share[n] < 1 for n in ('source_1x1', 'source_1x40', 'source_40x1', 'rotate_45', 'minify_3'))
    assert inside_share['magnify_20'] == 1.0
    assert np.array_equal(out['warp_out_0'], out['warp_src_0'])
    for k, (wh, size) in enumerate(BICUBIC):
        src = noise(200 + wh[0], wh[1], wh[0])
        out['bicubic_src_%d' % k] = src
        out['bicubic_out_%d' % k] = np.asarray(Image.fromarray(src).resize(size))
        assert out['bicubic_out_%d' % k].shape == (size[1], size[0], 3)
    out['bicubic_size'] = np.array([size for _, size in BICUBIC], np.int32)            # (width, height), as Image.resize takes it
    assert np.array_equal(out['bicubic_out_6'], out['bicubic_src_6'])
    path = os.path.join(HERE, 'align.npz')
    np.savez_compressed(path, **out)
    print('%s: %d warp cases, %d bicubic cases, %d bytes, Pillow %s'
          % (path, len(cases), len(BICUBIC), os.path.getsize(path), PIL.__version__))


if __name__ == '__main__':
    main()
