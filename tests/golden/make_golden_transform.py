"""Generate tests/golden/transform.npz with Pillow alone: the contract of ta_frames_transform / ta_frames_transpose and of
terran_amd.image.transform_frames, transpose_frames and rotate_frames.

    transform cases  Image.fromarray(src[frame]).transform((w, h), method, data, resample=filter, fillcolor=fill) for lists
                     of (frame, method, data); the sources are the formulas of tests/transform_model.py (not stored)
    transposes       Image.transpose(op), all seven
    rotates          Image.rotate(angle, resample, expand, center, translate)
    api_*            whole-batch and mixed-size-list calls of the public functions

The maker asserts that no perspective case has a denominator of exactly 0 at a pixel centre and that no NEAREST coordinate
reaches 2^31 (both are undefined behaviour in Pillow's C).  Reads neither the reference nor this package.

    python tests/golden/make_golden_transform.py
"""
import math
import os
import sys

import numpy as np
import PIL
from PIL import Image

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
from tests import transform_model as M      # noqa: E402  (the shared source formulas and the route names only)

A, P = M.AFFINE, M.PERSPECTIVE
FILTERS = (M.NEAREST, M.BILINEAR, M.BICUBIC)
FILL = (7, 8, 9)
ANGLES = (0, 90, 180, 270, 360 + 90, 30, -12.5, 45)


def matrices(W, H, ow, oh):
    """name -> (method, data) for a W x H source and an ow x oh output."""
    sx, sy = W / ow, H / oh
    c, s = math.cos(math.radians(20)), math.sin(math.radians(20))
    r0, r1, r3, r4 = c * sx, s * sx + 0.1, -s * sy, c * sy
    return {
        'identity': (A, (1, 0, 0, 0, 1, 0)),
        'shift_int': (A, (1, 0, 3, 0, 1, -2)),
        'shift_half': (A, (1, 0, 0.5, 0, 1, -0.5)),
        'scale': (A, (sx, 0, 0, 0, sy, 0)),                                     # NEAREST: the scaler route
        'rot_shear': (A, (r0, r1, W / 2 - (r0 * ow / 2 + r1 * oh / 2), r3, r4, H / 2 - (r3 * ow / 2 + r4 * oh / 2))),
        'mirror': (A, (-sx, 0, W, 0, sy, 0)),
        'outside': (A, (1, 0, W + 5, 0, 1, 0)),                                 # all fill
        'edges': (A, (1, 0, -0.5, 0, 1, -0.5)),                                 # xs = 0 at x = 0, xs = W at x = W, the same in y
        'persp_mild': (P, (sx, 0.02, 0, 0.01, sy, 0, 0.0005, 0.0003)),
        'persp_sign': (P, (sx, 0.1, -3, 0.05, sy, -2, -1 / (0.613 * ow), -0.0031)),   # the denominator changes sign inside
    }


def check_defined(method, data, ow, oh, filt):
    xin, yin = np.arange(ow)[None, :] + 0.5, np.arange(oh)[:, None] + 0.5
    a = [float(v) for v in data] + [0.0, 0.0]
    xs, ys = a[0] * xin + a[1] * yin + a[2], a[3] * xin + a[4] * yin + a[5]
    if method == P:
        d = a[6] * xin + a[7] * yin + 1
        assert (d != 0).all(), 'a perspective denominator of exactly 0 at a pixel centre'
        xs, ys = xs / d, ys / d
    assert np.isfinite(xs).all() and np.isfinite(ys).all()
    assert max(np.abs(xs).max(), np.abs(ys).max()) < 2.0 ** 31 - 1


def transform(img, size, method, data, filt, fill):
    check_defined(method, data, size[0], size[1], filt)
    return np.asarray(Image.fromarray(img).transform(size, method, tuple(float(v) for v in data), resample=filt, fillcolor=fill))


def main():
    S = M.sources()
    out = {'pillow_version': np.array(PIL.__version__)}
    cases = []                                          # (source, filter, (w, h), fill, [(frame, method, data)])
    k = 0
    for size in ((64, 48), (5, 3), (1, 1)):
        for name, (method, data) in matrices(53, 37, *size).items():
            for filt in FILTERS:
                cases.append((2, filt, size, FILL if k % 2 else None, [(0, method, data)]))
                k += 1
    big = matrices(517, 300, 131, 67)
    for filt in FILTERS:
        cases.append((3, filt, (131, 67), None if filt == M.BILINEAR else FILL, [(0,) + big['rot_shear']]))
    cases.append((3, M.NEAREST, (131, 67), None, [(0,) + big['scale']]))
    cases.append((3, M.BICUBIC, (131, 67), FILL, [(0,) + big['persp_sign']]))
    cases.append((3, M.BILINEAR, (131, 67), FILL, [(0,) + big['mirror']]))
    accumulate = (A, (256, 0.001, -33000, 0.001, 1.3, 0.2))                      # a corner beyond 32768: not fixed point
    assert M.nearest_route(A, accumulate[1], 131, 67) == 'accumulate'
    cases.append((3, M.NEAREST, (131, 67), FILL, [(0,) + accumulate]))
    for src, (h, w) in ((0, (1, 1)), (1, (2, 3)), (4, (16, 16))):
        for size in ((5, 3), (1, 1)) + (((64, 48),) if src == 4 else ()):
            m = matrices(w, h, *size)
            for name in ('identity', 'shift_half', 'scale', 'rot_shear', 'persp_mild'):
                for filt in FILTERS:
                    cases.append((src, filt, size, FILL if k % 2 else None, [(0,) + m[name]]))
                    k += 1
    # one call, 8 regions over 3 frames, frames out of order and repeated, both methods and every NEAREST route
    m = matrices(53, 37, 24, 16)
    far = (A, (3001.7, 0.01, 20 - 10.5 * 3001.7, 0.0, 2.0, 1.0))
    assert M.nearest_route(A, far[1], 24, 16) == 'accumulate'
    assert [M.nearest_route(*m[n], 24, 16) for n in ('scale', 'rot_shear', 'persp_mild')] == ['scale', 'fixed', 'generic']
    multi = [(2,) + m['rot_shear'], (0,) + m['scale'], (1,) + m['persp_mild'], (1,) + far, (0,) + m['persp_sign'], (2,) + m['mirror'],
             (2,) + m['edges'], (0,) + m['shift_half']]
    for filt in FILTERS:
        cases.append((2, filt, (24, 16), None if filt == M.BICUBIC else FILL, multi))
    regions = []
    for i, (src, filt, size, fill, regs) in enumerate(cases):
        out['tf_%d' % i] = np.stack([transform(S[src][f], size, method, data, filt, fill) for f, method, data in regs])
        regions.extend([(f, method) + tuple(float(v) for v in data) + (0.0,) * (8 - len(data)) for f, method, data in regs])
    out['tf_source'] = np.array([c[0] for c in cases], np.int32)
    out['tf_filter'] = np.array([c[1] for c in cases], np.int32)
    out['tf_size'] = np.array([c[2] for c in cases], np.int32)
    out['tf_fill'] = np.array([c[3] if c[3] is not None else (-1, -1, -1) for c in cases], np.int32)
    out['tf_count'] = np.array([len(c[4]) for c in cases], np.int32)
    out['tf_regions'] = np.array(regions, np.float64)

    tp = []
    for src in (0, 6, 5):
        for op in range(7):
            out['tp_%d' % len(tp)] = np.stack([np.asarray(Image.fromarray(f).transpose(op)) for f in S[src]])
            tp.append((src, op))
    out['tp_cases'] = np.array(tp, np.int32)

    rot = []
    for src in (6, 7):
        for angle in ANGLES:
            for expand in (False, True):
                for moved in (False, True):
                    for filt in (M.NEAREST, M.BICUBIC):
                        kw = dict(center=(10, 7), translate=(3, -2)) if moved else {}
                        out['rot_%d' % len(rot)] = np.asarray(Image.fromarray(S[src][0]).rotate(angle, filt, expand, **kw))
                        rot.append((src, angle, expand, moved, filt))
    out['rot_cases'] = np.array(rot, np.float64)

    # the public functions: one data for a batch, one per frame, a mixed-size list to one batch
    m = matrices(53, 37, 40, 30)
    out['api_one_data'] = np.array(m['persp_mild'][1], np.float64)
    out['api_one'] = np.stack([transform(f, (40, 30), P, m['persp_mild'][1], M.BICUBIC, None) for f in S[2]])
    per = [m['rot_shear'][1], m['mirror'][1], m['shift_half'][1]]
    out['api_per_data'] = np.array(per, np.float64)
    out['api_per'] = np.stack([transform(f, (40, 30), A, d, M.BILINEAR, FILL) for f, d in zip(S[2], per)])
    mixed_data = (0.9, 0.3, -4.0, -0.25, 1.1, 2.5)
    out['api_mixed_data'] = np.array(mixed_data)
    out['api_mixed'] = np.stack([transform(S[s][0], (40, 30), A, mixed_data, M.BILINEAR, FILL) for s in (2, 7, 1)])
    out['api_tilt'] = np.asarray(Image.fromarray(S[6][0]).rotate(5.0, M.BILINEAR, fillcolor=FILL))
    path = os.path.join(HERE, 'transform.npz')
    np.savez_compressed(path, **out)
    print('%s: %d transform cases, %d transposes, %d rotates, %d bytes, Pillow %s'
          % (path, len(cases), len(tp), len(rot), os.path.getsize(path), PIL.__version__))


if __name__ == '__main__':
    main()
