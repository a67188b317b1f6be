"""No GPU: the numpy restatement of csrc/transform.hip (tests/transform_model.py) against the recorded Pillow golden
(tests/golden/transform.npz) and, where Pillow is installed, against Pillow itself; image.rotate_plan (Pillow's fast paths,
matrix and expanded canvas) against Image.rotate; the argument checks of the Python layer."""
import os

import numpy as np
import pytest

from terran_amd import arcface, image, lib, vis
from tests import transform_model as M

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'transform.npz')


@pytest.fixture(scope='module')
def golden():
    return M.golden(GOLDEN)


def rotated(img, angle, filt, expand, center, translate, fill=None):
    """Image.rotate from the host functions alone: rotate_plan, then the model."""
    kind, arg, size = image.rotate_plan(img.shape[1], img.shape[0], angle, expand, center, translate)
    if kind == 'copy':
        return img.copy(), kind
    if kind == 'transpose':
        return M.transpose(img, arg), kind
    return M.transform(img, size, M.AFFINE, arg, filt, fill), kind


def test_the_model_equals_the_golden(golden):
    z, S, cases, transposes, _ = golden
    seen = set()
    for k, c in enumerate(cases):
        got = np.stack([M.transform(S[c['source']][f], c['size'], m, a, c['filter'], c['fill']) for f, m, a in c['regions']])
        assert np.array_equal(got, c['expected']), (k, c['filter'], c['size'])
        for _, m, a in c['regions']:
            seen.add((c['filter'], m, c['fill'] is None))
            if c['filter'] == M.NEAREST:
                seen.add(M.nearest_route(m, a, *c['size']))
    assert {(f, m, n) for f in (0, 2, 3) for m in (0, 2) for n in (False, True)} <= seen
    assert {'scale', 'fixed', 'accumulate', 'generic'} <= seen
    for c in transposes:
        assert np.array_equal(M.transpose(S[c['source']], c['op']), c['expected']), c['op']
    assert {c['op'] for c in transposes} == set(range(7))


def test_rotate_plan_and_the_model_equal_image_rotate(golden):
    """Angles 0, 90, 180, 270, 450, 30, -12.5, 45; expand or not; center / translate unset and set; nearest and bicubic; a
    37 x 53 and a square 48 x 48 source."""
    _, S, _, _, rotates = golden
    kinds = set()
    for c in rotates:
        got, kind = rotated(S[c['source']][0], c['angle'], c['filter'], c['expand'], c['center'], c['translate'])
        assert got.shape == c['expected'].shape, (c, got.shape)
        assert np.array_equal(got, c['expected']), {k: v for k, v in c.items() if k != 'expected'}
        kinds.add(kind)
    assert kinds == {'copy', 'transpose', 'transform'} and len(rotates) == 128
    # the fast paths: only without center and translate, 90 / 270 only with expand or a square image
    assert image.rotate_plan(53, 37, 360.0) == ('copy', None, (53, 37))
    assert image.rotate_plan(53, 37, -180) == ('transpose', lib.ROTATE_180, (53, 37))
    assert image.rotate_plan(53, 37, 90, expand=True) == ('transpose', lib.ROTATE_90, (37, 53))
    assert image.rotate_plan(48, 48, 270) == ('transpose', lib.ROTATE_270, (48, 48))
    assert image.rotate_plan(53, 37, 90)[0] == 'transform' and image.rotate_plan(53, 37, 90)[2] == (53, 37)
    assert image.rotate_plan(53, 37, 180, center=(0, 0))[0] == 'transform'
    assert image.rotate_plan(53, 37, 0, translate=(1, 0))[0] == 'transform'


def test_the_model_equals_pillow_on_seeded_maps():
    """600 seeded maps, both methods, the three filters, both fills, sources and outputs from 1 x 1, every NEAREST route."""
    Image = pytest.importorskip('PIL.Image')
    rng = np.random.default_rng(11)
    routes = set()
    for k in range(600):
        h, w = (int(v) for v in rng.integers(1, 40, 2))
        ow, oh = (int(v) for v in rng.integers(1, 48, 2))
        img = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
        filt = (M.NEAREST, M.BILINEAR, M.BICUBIC)[k % 3]
        method = (M.AFFINE, M.PERSPECTIVE)[(k // 3) % 2]
        a = [w / ow, 0.0, 0.0, 0.0, h / oh, 0.0, 0.0, 0.0]
        kind = k % 7
        if kind >= 2:                                   # 0, 1: pure scale, then with a translation, then with shear
            a[2], a[5] = rng.uniform(-3, 3, 2)
        if kind >= 4:
            a[1], a[3] = rng.uniform(-0.6, 0.6, 2)
        if kind == 6:
            a[2] -= 40000.0                             # beyond 16.16 fixed point
            a[0] += 40000.0 / ow
        if method == M.PERSPECTIVE:
            a[6], a[7] = rng.uniform(-0.004, 0.004, 2)
        data = tuple(a[:6] if method == M.AFFINE else a)
        fill = None if k % 2 else tuple(int(v) for v in rng.integers(0, 256, 3))
        want = np.asarray(Image.fromarray(img).transform((ow, oh), method, data, resample=filt, fillcolor=fill))
        got = M.transform(img, (ow, oh), method, data, filt, fill)
        assert np.array_equal(got, want), (k, (h, w), (ow, oh), filt, method, data, fill)
        if filt == M.NEAREST:
            routes.add(M.nearest_route(method, data, ow, oh))
    assert routes == {'scale', 'fixed', 'accumulate', 'generic'}


def test_rotate_plan_equals_pillow_on_more_angles():
    Image = pytest.importorskip('PIL.Image')
    rng = np.random.default_rng(12)
    img = M.noise(23, 31, 5)
    for k in range(120):
        angle = float(rng.choice([0, 90, 180, 270, -90, 720, 89.999, 1e-9])) if k % 3 == 0 else float(rng.uniform(-400, 400))
        expand = bool(k % 2)
        center = tuple(rng.uniform(-5, 35, 2)) if k % 4 == 1 else None
        translate = tuple(rng.uniform(-6, 6, 2)) if k % 5 == 2 else None
        filt = (M.NEAREST, M.BILINEAR, M.BICUBIC)[k % 3]
        want = np.asarray(Image.fromarray(img).rotate(angle, filt, expand, center, translate, fillcolor=(1, 2, 3)))
        got, _ = rotated(img, angle, filt, expand, center, translate, (1, 2, 3))
        assert got.shape == want.shape and np.array_equal(got, want), (k, angle, expand, center, translate, filt)


def test_transpose_model_equals_pillow():
    Image = pytest.importorskip('PIL.Image')
    img = M.noise(5, 7, 9)
    for op in range(7):
        assert np.array_equal(M.transpose(img, op), np.asarray(Image.fromarray(img).transpose(op))), op


def _fake_frames(n=2, h=30, w=40):
    """A lib.Frames that owns nothing: the argument checks run before anything touches the device."""
    f = lib.Frames.__new__(lib.Frames)
    f.ctx, f.h, f.shape = None, None, (n, h, w, 3)
    return f


def test_the_python_layer_checks_its_arguments():
    fr = _fake_frames()
    ident = (1, 0, 0, 0, 1, 0)
    bad_calls = [
        lambda: image.transform_frames(None, (8, 8), 'affine', ident),
        lambda: image.transform_frames([], (8, 8), 'affine', ident),
        lambda: image.transform_frames(fr, (0, 8), 'affine', ident),
        lambda: image.transform_frames(fr, (8, 16385), 'affine', ident),
        lambda: image.transform_frames(fr, 8, 'affine', ident),
        lambda: image.transform_frames(fr, (8, 8), 'quad', ident),
        lambda: image.transform_frames(fr, (8, 8), 1, ident),
        lambda: image.transform_frames(fr, (8, 8), 'affine', ident + (0, 0)),          # 8 coefficients for AFFINE
        lambda: image.transform_frames(fr, (8, 8), 'perspective', ident),              # 6 for PERSPECTIVE
        lambda: image.transform_frames(fr, (8, 8), 'affine', [ident] * 3),             # 3 tuples for 2 frames
        lambda: image.transform_frames(fr, (8, 8), 'affine', (1, 0, np.nan, 0, 1, 0)),
        lambda: image.transform_frames(fr, (8, 8), 'affine', (1, 0, np.inf, 0, 1, 0)),
        lambda: image.transform_frames(fr, (8, 8), 'affine', ident, resample='lanczos'),
        lambda: image.transform_frames(fr, (8, 8), 'affine', ident, resample=4),
        lambda: image.transform_frames(fr, (8, 8), 'affine', ident, fillcolor=(1, 2)),
        lambda: image.transform_frames(fr, (8, 8), 'affine', ident, fillcolor=(1, 2, 256)),
        lambda: image.transpose_frames(fr, 7),
        lambda: image.transpose_frames(fr, 'rotate_45'),
        lambda: image.transpose_frames(fr, True),
        lambda: image.transpose_frames('frames', 0),
        lambda: image.rotate_frames(fr, 'a lot'),
        lambda: image.rotate_frames(fr, np.nan),
        lambda: image.rotate_frames(fr, 10, resample='box'),
        lambda: image.rotate_frames(fr, 10, center=(1, 2, 3)),
        lambda: image.rotate_frames(fr, 10, translate=(np.inf, 0)),
        lambda: image.rotate_frames(fr, 10, fillcolor='red'),
        lambda: image.rotate_frames(_fake_frames(1, 16000, 16000), 45, expand=True),   # the canvas would pass 16384
        lambda: vis.align_faces(fr, [[{'bbox': [1, 2, 3, 4]}]]),                       # no landmarks
        lambda: vis.align_faces(fr, [[{'bbox': [1, 2, 3, 4], 'landmarks': np.zeros((4, 2))}]]),
        lambda: vis.align_faces(fr, [[]], size=(112, 96)),
        lambda: vis.align_faces(fr, [[]], resample='lanczos'),
        lambda: vis.align_faces(fr, [[], [], []]),                                     # more lists than frames
    ]
    for k, call in enumerate(bad_calls):
        with pytest.raises(ValueError):
            call()
            pytest.fail('call %d was accepted' % k)
    assert vis.align_faces(fr, [[], []]) == (None, [])
    assert lib.transpose_op('Rotate_90') == 2 and lib.transpose_op(np.int32(6)) == 6
    assert lib.TRANSFORM_DT.itemsize == 72 and lib.TRANSFORM_DT.fields['a'][1] == 8


def test_pack_align_scales_the_template():
    rng = np.random.default_rng(3)
    lm = arcface._TEMPLATE * 0.7 + (40, 25) + rng.normal(0, 1.5, (5, 2))
    faces = [[], [{'landmarks': lm}, {'landmarks': lm[:, ::-1] + 3}]]
    regions, index = vis.pack_align(faces)
    assert index.tolist() == [[1, 0], [1, 1]] and regions['frame'].tolist() == [1, 1] and regions['method'].tolist() == [0, 0]
    assert np.array_equal(regions['a'][:, :6], arcface.align_matrices(np.stack([lm, lm[:, ::-1] + 3])))      # the embedder's own
    assert np.array_equal(regions['a'][0, :6], arcface.align_matrix(lm)) and not regions['a'][:, 6:].any()
    # half the side: the same similarity seen from a chip of half the size
    half, _ = vis.pack_align(faces, 56)
    a, b = regions['a'][0], half['a'][0]
    assert np.allclose(b[[0, 1, 3, 4]], 2 * a[[0, 1, 3, 4]], rtol=1e-12) and np.allclose(b[[2, 5]], a[[2, 5]], rtol=1e-9, atol=1e-9)
