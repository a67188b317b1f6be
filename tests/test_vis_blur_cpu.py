"""CPU: the numpy restatement of the blur contract (tests/vis_blur_model.py) against the recorded Pillow golden
(tests/golden/vis_blur.npz) and against live Pillow; the host set-up of ta_frames_blur (ta_blur_plan: box radius, weights,
rounds) against the restatement; vis.pack_blur's clipping, margin, default radius, inputs and order."""
import os

import numpy as np
import pytest

from terran_amd import lib, vis
from tests import vis_blur_model as B

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'vis_blur.npz')
SENSITIVE = [0.25, 0.3, 1.0]                            # a double division for ww gives wrong pixels at these radii


@pytest.fixture(scope='module')
def scenes():
    return B.golden_scenes(GOLDEN)[1]


def test_model_equals_the_golden(scenes):
    assert len(scenes) >= 12
    names = ' '.join(s['name'] for s in scenes)
    for need in ('radius_0 ', 'radius_0.25', 'radius_0.3', 'radius_1 ', 'radius_2.5', 'radius_12.3', 'beyond_region', 'thin',
                 'off_every_edge', 'whole_frame', 'overlapping', 'ellipses_1xn'):
        assert need in names + ' ', need
    for s in scenes:
        assert s['base'].shape[0] <= 96 and s['base'].shape[1] <= 128
        got = B.anonymize(s['base'], s['faces'], s['radius'], s['margin'], s['shape'])
        assert np.array_equal(got, s['expected']), (s['name'], int((got != s['expected']).any(-1).sum()))
        if s['name'] != 'radius_0':
            assert not np.array_equal(s['expected'], s['base']), s['name']


def test_model_equals_live_pillow():
    pytest.importorskip('PIL')
    from PIL import Image, ImageDraw, ImageFilter
    rng = np.random.default_rng(5)
    radii = SENSITIVE + [0.1, 0.5, 1.5, 2.5, 3.7, 8, 12.3, 40, 200, 1024]
    for it in range(120):
        h, w = (int(v) for v in rng.integers(1, 70, 2))
        img = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
        radius = float(radii[it % len(radii)] if it % 3 else rng.uniform(0.1, 50))
        want = np.asarray(Image.fromarray(img).filter(ImageFilter.GaussianBlur(radius)))
        got = B.gaussian_blur(img, radius)
        assert np.array_equal(got, want), (h, w, radius, int((got != want).sum()))
    for h, w in [(1, 1), (1, 9), (9, 1), (2, 2), (3, 3), (4, 7), (7, 4), (20, 31), (33, 12), (64, 64)]:
        mask = Image.new('L', (w, h))
        ImageDraw.Draw(mask).ellipse([0, 0, w - 1, h - 1], fill=255)
        assert np.array_equal(B.ellipse_mask(h, w), np.asarray(mask) == 255), (h, w)


def test_host_plan_equals_the_model():
    """ta_blur_plan: the float32 box radius and the integer weights, bit for bit, and the rounds."""
    rng = np.random.default_rng(9)
    radii = np.r_[SENSITIVE, 0.0, 1e-30, 0.1, 0.5, 2.5, 12.3, 40.0, 1024.0, rng.uniform(0, 60, 300), rng.uniform(0, 1024, 100)]
    q = np.zeros(len(radii), lib.BLUR_DT)
    q['x1'], q['y1'], q['radius'] = 4, 4, radii
    q['frame'] = np.arange(len(q))
    rounds, fr, w = lib.blur_plan(q)
    assert not rounds.any()
    for i, radius in enumerate(q['radius']):
        want = B.box_radius(radius)
        assert fr[i] == want and fr[i] >= 0, (radius, fr[i], want)
        assert tuple(int(v) for v in w[i]) == B.weights(want)[1:], radius
    # overlaps: a chain, a region that meets two rounds, touching boxes (disjoint), other frames
    boxes = [(0, 0, 0, 10, 10), (0, 5, 5, 15, 15), (0, 12, 12, 20, 20), (0, 10, 0, 14, 5), (0, 30, 30, 40, 40),
             (0, 8, 8, 13, 35), (1, 0, 0, 10, 10), (0, 0, 0, 50, 50), (1, 9, 9, 12, 12), (0, 60, 0, 61, 1)]
    q = np.zeros(len(boxes), lib.BLUR_DT)
    for name, col in zip(('frame', 'x0', 'y0', 'x1', 'y1'), zip(*boxes)):
        q[name] = col
    q['radius'] = 2
    got = lib.blur_plan(q)[0].tolist()
    assert got == B.rounds(q) == [0, 1, 2, 0, 0, 3, 0, 4, 1, 0]
    assert lib.blur_plan(q[:0])[0].size == 0
    for field, bad in [('x1', 0), ('y1', -3), ('shape', 2), ('radius', -1.0), ('radius', np.nan), ('radius', np.inf),
                       ('radius', 1024.5)]:
        p = q[:2].copy()
        p[field][1] = bad
        with pytest.raises(lib.TerranAmdError) as e:
            lib.blur_plan(p)
        assert e.value.code == lib.E_INVALID


def test_pack_blur():
    face = {'bbox': np.array([10.7, 20.2, 50.9, 40.99], np.float32), 'track': 3}
    q = vis.pack_blur([[face]], (100, 120))
    assert q.dtype == lib.BLUR_DT and len(q) == 1
    assert q[0].tolist() == (0, 10, 20, 50, 40, lib.BLUR_BOX, 5.0)             # int(), default radius max(40, 20) / 8
    assert vis.pack_blur([face], (100, 120))[0] == q[0]                        # a dict stands for a one-element list
    assert vis.pack_blur([[face]], (1, 100, 120, 3))[0] == q[0]                # a batch's shape
    # margin: of the width left and right, of the height top and bottom, in Python floats, then int()
    m = vis.pack_blur([[face]], (100, 120), margin=0.25, shape='ellipse', radius=3.5)[0]
    x0, y0, x1, y1 = (float(v) for v in face['bbox'])
    want = (int(x0 - 0.25 * (x1 - x0)), int(y0 - 0.25 * (y1 - y0)), int(x1 + 0.25 * (x1 - x0)), int(y1 + 0.25 * (y1 - y0)))
    assert m.tolist() == (0,) + want + (lib.BLUR_ELLIPSE, 3.5)
    # clipping: int() first (towards zero), then the frame; the default radius is that of the CLIPPED region
    c = vis.pack_blur([[{'bbox': [-0.9, -30.5, 200, 16.5]}]], (64, 96))[0]
    assert c.tolist() == (0, 0, 0, 96, 16, lib.BLUR_BOX, 12.0)
    # empty after clipping, inverted, beside the frame: left out; the order and the frame index of the rest stay
    faces = [[{'bbox': [5, 5, 5.5, 9]}, {'bbox': [1, 1, 4, 4]}, {'bbox': [9, 9, 3, 20]}], [], {'bbox': [-9, 2, -1, 8]},
             [{'bbox': [70, 2, 99, 8]}, {'bbox': [60, 60, 64, 64]}, {'bbox': [2, 3, 8, 9]}]]
    q = vis.pack_blur(faces, [(64, 64), (64, 64), (64, 64), (64, 64)])
    assert q['frame'].tolist() == [0, 3, 3] and q['x0'].tolist() == [1, 60, 2]
    assert len(vis.pack_blur([[], []], (4, 4))) == 0 and vis.pack_blur([], (4, 4)).dtype == lib.BLUR_DT
    # per-frame sizes
    q = vis.pack_blur([{'bbox': [0, 0, 50, 50]}, {'bbox': [0, 0, 50, 50]}], [(20, 30), (40, 10)])
    assert q[['x1', 'y1']].tolist() == [(30, 20), (10, 40)]
    # the restatement clips the same way
    for f, hw in zip(faces, [(64, 64)] * 4):
        got = vis.pack_blur([f], hw, margin=0.1)
        assert [tuple(r)[1:5] for r in got.tolist()] == [r[:4] for r in B.face_regions(f, hw[0], hw[1], margin=0.1)]
    # overlapping faces keep the list order, and the library's rounds follow it
    over = [{'bbox': [10, 10, 50, 45]}, {'bbox': [30, 25, 75, 60]}, {'bbox': [60, 50, 80, 70]}, {'bbox': [0, 0, 9, 9]}]
    q = vis.pack_blur([over], (90, 90), radius=2)
    assert q['x0'].tolist() == [10, 30, 60, 0]
    assert lib.blur_plan(q)[0].tolist() == B.rounds(q) == [0, 1, 2, 0]
    for kw in (dict(shape='disc'), dict(radius=-1), dict(radius=float('nan')), dict(radius=2000), dict(margin=float('inf'))):
        with pytest.raises(ValueError):
            vis.pack_blur([over], (90, 90), **kw)
    with pytest.raises(ValueError):
        vis.pack_blur([{'bbox': [0, float('nan'), 5, 5]}], (90, 90))
