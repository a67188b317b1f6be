"""CPU: terran_amd.vis packing and the numpy restatement of its drawing (tests/vis_raster.py) against the reference's
terran.vis Pillow path, recorded in tests/golden/vis.npz (tests/golden/make_golden_vis.py), and -- when the Pillow that
recorded it is installed -- against the live Pillow."""
import os
import random

import numpy as np
import pytest

from terran_amd import lib, vis
from tests import vis_raster as V

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'vis.npz')


@pytest.fixture(scope='module')
def golden():
    return V.golden_scenes(GOLDEN)


def _fresh(monkeypatch, seed):
    monkeypatch.setattr(vis, 'FACE_COLORMAP', vis.build_colormap())
    random.seed(seed)


def test_restatement_reproduces_the_reference(golden):
    z, scenes = golden
    assert len(scenes) == 30
    for s in scenes:
        random.seed(s['seed'])
        if s['kind'].startswith('faces'):
            got = V.render_faces(s['base'], s['input'], s['scale'], vis.build_colormap())
        else:
            got = V.render_poses(s['base'], s['input'], s['scale'], vis.POSE_CONNECTIONS, vis.POSE_CONNECTION_COLORS,
                                 vis.POSE_KEYPOINT_COLORS)
        assert np.array_equal(got, s['expected']), (s['kind'], s['scale'])


def test_tables_are_the_reference_tables(golden):
    z, _ = golden
    assert np.array_equal(np.array(vis.PALETTE, np.uint8), z['palette'])
    assert np.array_equal(vis.POSE_CONNECTIONS, z['pose_connections'])
    assert np.array_equal(vis.POSE_CONNECTION_COLORS, z['pose_connection_colors'])
    assert np.array_equal(vis.POSE_KEYPOINT_COLORS, z['pose_keypoint_colors'])


def test_packed_primitives_reproduce_the_reference(golden, monkeypatch):
    """pack_faces / pack_poses (colours, widths, radii, skipped limbs, draw order) executed by the restatement of the
    kernel's three primitives give the reference's pixels."""
    _, scenes = golden
    for s in scenes:
        _fresh(monkeypatch, s['seed'])
        if s['kind'].startswith('faces'):
            prims = vis.pack_faces([s['input']], s['scale'])
            assert set(prims['kind']) <= {lib.DRAW_BAR} and np.all(prims['rgba'][:, 3] == 255)
        else:
            prims = vis.pack_poses([s['input']], s['scale'])
        img = s['base'][None].copy()
        V.draw_prims(img, prims)
        assert np.array_equal(img[0], s['expected']), (s['kind'], s['scale'])


def test_colormap_follows_the_reference(golden, monkeypatch):
    """First sight of a label takes the next palette colour; no label (or track 0, which is falsy) draws from `random`."""
    _, scenes = golden
    n_random = 0
    for s in scenes:
        if not s['kind'].startswith('faces'):
            continue
        _fresh(monkeypatch, s['seed'])
        faces = s['input'] if isinstance(s['input'], list) else [s['input']]
        got = [vis.FACE_COLORMAP(f.get('name') or f.get('track')) for f in faces]
        assert np.array_equal(np.array(got, np.uint8).reshape(-1, 3), s['colors'])
        n_random += sum(1 for f in faces if not (f.get('name') or f.get('track')))
    assert n_random > 10
    cm = vis.build_colormap()
    assert [cm('a'), cm('b'), cm('a'), cm(7)] == [vis.PALETTE[0], vis.PALETTE[1], vis.PALETTE[0], vis.PALETTE[2]]
    random.seed(5)
    expect = random.Random(5).choice(vis.PALETTE)
    assert cm(None) == expect


def test_pose_packing_order_widths_radii():
    k = np.zeros((2, 18, 3), np.int32)
    k[..., 0] = np.arange(18) * 10 + 5
    k[..., 1] = 50
    k[..., 2] = 1
    k[0, 14, 2] = 0                                      # right eye missing: limbs 1 and 2 of person 0 skipped
    p = vis.pack_poses([[{'keypoints': k[0]}, {'keypoints': k[1]}]], scale=1.5)
    lines, dots = p[p['kind'] == lib.DRAW_LINE], p[p['kind'] == lib.DRAW_DISC]
    assert len(lines) == 15 + 17 and len(dots) == 17 + 18
    assert np.all(p['kind'][:32] == lib.DRAW_LINE)       # every limb of every person first, then every keypoint
    assert np.all(lines['width'] == 12) and np.all(lines['rgba'][:, 3] == 180) and np.all(dots['rgba'][:, 3] == 225)
    assert np.all(dots['x1'] - dots['x0'] == 2 * 9)     # r = int(3 * int(1.5 * 4) / 2)
    assert np.array_equal(lines['rgba'][:15, :3], vis.POSE_CONNECTION_COLORS[[0, 3, 4] + list(range(5, 17))])


def test_inverted_boxes_raise(monkeypatch):
    _fresh(monkeypatch, 0)
    good = {'bbox': np.array([1, 1, 5, 5], np.float32)}
    for bad in ([5.7, 5, 3.2, 9], [5, 5.9, 9, 5.2]):
        with pytest.raises(ValueError):
            vis.pack_faces([[good, {'bbox': np.array(bad, np.float32)}]])
        with pytest.raises(ValueError):
            V.rectangle_runs(bad, 3)
    with pytest.raises(ValueError):
        vis.pack_faces([[{'bbox': [0, 0, float('nan'), 4]}]])
    assert len(vis.pack_faces([[good]], scale=0.25)) == 0   # width int(0.75) = 0 draws nothing


def test_restatement_against_live_pillow(golden):
    """Thousands of random lines (widths 0-40), ellipses and rectangle outlines, many partly or wholly off the frame,
    drawn with alpha 1 so that a pixel blended twice shows: the restatement equals Pillow pixel for pixel."""
    PIL = pytest.importorskip('PIL')
    from PIL import Image, ImageDraw
    z, _ = golden
    if PIL.__version__ != str(z['pillow_version']):
        pytest.skip('Pillow %s installed, vis.npz recorded %s' % (PIL.__version__, z['pillow_version']))
    rng = random.Random(20261016)
    H, W = 61, 83
    counts = [0, 0, 0]
    for it in range(4500):
        c = [rng.randint(-40, W + 40), rng.randint(-40, H + 40), rng.randint(-40, W + 40), rng.randint(-40, H + 40)]
        if rng.random() < 0.4:
            c[2], c[3] = c[0] + rng.randint(-6, 6), c[1] + rng.randint(-6, 6)
        width = rng.randint(0, 40) if rng.random() < 0.5 else rng.randint(0, 5)
        rgba = (rng.randint(0, 255), rng.randint(0, 255), rng.randint(0, 255), rng.choice([1, 180, 225, 255]))
        base = np.full((H, W, 3), 100, np.uint8) if rgba[3] > 1 else np.zeros((H, W, 3), np.uint8)
        im = Image.fromarray(base)
        d = ImageDraw.Draw(im, 'RGBA')
        mine = base.copy()
        k = it % 3
        if k == 0:
            d.line(c, fill=rgba, width=width)
            V.line(mine, c, rgba, width)
        elif k == 1:
            r = rng.randint(0, 30)
            r2 = max(0, r + rng.choice([0, 0, 1, -1, 3]))
            c = [c[0] - r, c[1] - r2, c[0] + r, c[1] + r2]
            d.ellipse(c, fill=rgba)
            V.ellipse(mine, c, rgba)
        else:
            c = [min(c[0], c[2]), min(c[1], c[3]), max(c[0], c[2]), max(c[1], c[3])]
            d.rectangle(c, outline=rgba, width=width)
            V.rectangle(mine, c, rgba, width)
        assert np.array_equal(np.asarray(im), mine), (k, c, width, rgba)
        counts[k] += int((mine != base).any())
    assert min(counts) > 500


def test_pillow_pins():
    """The facts the restatement was pinned on, stated once: blend, thin line, point, rectangle and ellipse sizes."""
    assert int(V.div255_blend(np.array([100]), [200], 180)[0]) == 171
    img = np.zeros((40, 40, 3), np.uint8)
    assert sum(1 for _ in V.line_runs(40, [5, 5, 20, 30], 0)) == 26 == len(V.line_runs(40, [5, 5, 20, 30], 1))
    assert V.line_runs(40, [7, 7, 7, 7], 9) == [(7, 7, 7)]
    assert V.rectangle_runs([5, 5, 9, 9], 0) == []
    V.rectangle(img, [5, 5, 6, 6], (255, 0, 0, 255), 3)
    assert (img[..., 0] > 0).sum() == 18
    assert V.ellipse_runs([3, 3, 3, 3]) == []
    assert sum(b - a + 1 for _, a, b in V.ellipse_runs([10, 10, 12, 12])) == 5
    assert sum(b - a + 1 for _, a, b in V.ellipse_runs([10, 10, 22, 22])) == 129
