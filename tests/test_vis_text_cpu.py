"""CPU: the labels of terran_amd.vis (pack_faces(..., labels=True)) executed by the numpy restatement
(tests/vis_text_model.py) against the reference's vis_faces with draw_label, recorded in tests/golden/vis_text.npz
(tests/golden/make_golden_vis_text.py) together with the font's own metrics and bitmaps, and against the live Pillow with
the live font."""
import os
import random

import numpy as np
import pytest

from terran_amd import lib, vis
from tests import vis_text_model as M

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'vis_text.npz')


@pytest.fixture(scope='module')
def golden():
    return M.golden_scenes(GOLDEN)


def _fresh(monkeypatch, seed):
    monkeypatch.setattr(vis, 'FACE_COLORMAP', vis.build_colormap())
    random.seed(seed)


def test_golden_scenes_cover_what_they_should(golden):
    z, _, scenes = golden
    assert len(scenes) == 30 and max(s['base'].shape[0] for s in scenes) <= 160 and max(s['base'].shape[1] for s in scenes) <= 240
    assert os.path.getsize(GOLDEN) < 1 << 20
    faces = [f for s in scenes for f in s['faces']]
    assert min(s['scale'] for s in scenes) * 16 < 1 and max(s['scale'] for s in scenes) == 3.0
    assert {type(f['text']) for f in faces if 'text' in f} == {str, int, float}
    assert any('text' in f and 'track' in f for f in faces) and any('track' in f and 'text' not in f for f in faces)
    assert any('name' in f and 'text' in f for f in faces) and any('name' not in f and 'track' not in f and 'text' in f for f in faces)
    assert {f['bbox'].dtype.kind if isinstance(f['bbox'], np.ndarray) else 'list' for f in faces} == {'f', 'i', 'list'}


def test_packed_labels_reproduce_the_reference(golden, monkeypatch):
    """pack_faces(labels=True) through the recorded font (metrics and bitmaps of the font that drew the goldens), executed
    by the restatement: the reference's pixels, whole image -- tab corners, text position and fractional start, the order
    of markers, tabs and texts, the colour of every face."""
    _, tables, scenes = golden
    monkeypatch.setattr(vis, 'label_font', lambda size: M.RecordedFont(tables, size))
    n_masks = 0
    for i, s in enumerate(scenes):
        _fresh(monkeypatch, s['seed'])
        prims, atlas = vis.pack_faces([s['faces']], s['scale'], labels=True)
        assert set(prims['kind']) <= {lib.DRAW_BAR, lib.DRAW_MASK} and np.all(prims['rgba'][:, 3] == 255)
        n_masks += int((prims['kind'] == lib.DRAW_MASK).sum())
        img = M.draw_prims(s['base'][None].copy(), prims, atlas)[0]
        assert np.array_equal(img, s['expected']), (i, s['scale'], int((img != s['expected']).any(-1).sum()))
    assert n_masks > 100


def test_labels_against_live_pillow(monkeypatch):
    """300 scenes of 3 random faces each (more than 300 labels) over printable ASCII, scales 0.1 - 3, float coordinates,
    off-frame placements: the packing with the live font, executed by the restatement, equals the live Pillow running
    the reference's vis_faces with its draw_label, whole image."""
    pytest.importorskip('PIL')
    rng = random.Random(20261017)
    labels = changed = 0
    for it in range(300):
        H, W = rng.randint(20, 120), rng.randint(20, 200)
        base = np.random.default_rng(it).integers(0, 256, (H, W, 3)).astype(np.uint8)
        scale = rng.choice([0.1, 0.25, 0.5, 1.0, 1.5, 2.0, 3.0, rng.uniform(0.1, 3)])
        faces = M.random_label_faces(rng, H, W, 3)
        _fresh(monkeypatch, it)
        prims, atlas = vis.pack_faces([faces], scale, labels=True)
        got = M.draw_prims(base[None].copy(), prims, atlas)[0]
        random.seed(it)
        want = M.pillow_faces(base, faces, scale, vis.build_colormap())
        assert np.array_equal(got, want), (it, scale, faces)
        labels += sum(1 for f in faces if 'text' in f or 'track' in f)
        changed += int((prims['kind'] == lib.DRAW_MASK).sum())
    assert labels >= 300 and changed > 150


def test_pillow_pins():
    """The facts the label packing rests on, against the installed Pillow: a filled rectangle's float corners are
    truncated toward zero and inclusive, and text is its coverage bitmap placed at int(xy) + offset."""
    PIL = pytest.importorskip('PIL')
    from PIL import Image, ImageDraw
    im = Image.new('RGB', (12, 12))
    ImageDraw.Draw(im, 'RGBA').rectangle([-0.9, 1.9, 4.99, 3.01], fill=(9, 9, 9, 255))
    a = np.asarray(im)[..., 0]
    assert a[1:4, 0:5].all() and a.astype(bool).sum() == 15
    font = vis.label_font(16)
    bitmap, off = font.mask('#7', (0.25, 0.75))
    base = np.full((40, 60, 3), 90, np.uint8)
    im = Image.fromarray(base)
    ImageDraw.Draw(im, 'RGBA').text([10.25, 0.75], '#7', font=font.font)
    assert np.array_equal(np.asarray(im), M.mask(base.copy(), 10 + off[0], 0 + off[1], bitmap, (255, 255, 255)))
    assert int(M.mask(np.full((1, 1, 3), 100, np.uint8), 0, 0, np.array([[127]], np.uint8), (255, 255, 255))[0, 0, 0]) == 177


def test_a_face_without_text_or_track_packs_as_before(monkeypatch):
    faces = [[{'bbox': np.array([3.5, 4, 40, 30], np.float32), 'name': 'a'}, {'bbox': [1, 2, 30, 40]}],
             [{'bbox': np.array([-5, -5, 10, 12]), 'name': 'b', 'text': None}]]
    _fresh(monkeypatch, 4)
    plain = vis.pack_faces(faces, 1.5)
    _fresh(monkeypatch, 4)
    prims, atlas = vis.pack_faces(faces, 1.5, labels=True)
    assert len(plain) == 12 and np.array_equal(prims, plain) and atlas.dtype == np.uint8 and len(atlas) == 0
    # with labels off, a labelled face packs its marker alone, and the marker is the same under both
    faces[0][1]['track'] = 3
    _fresh(monkeypatch, 4)
    plain = vis.pack_faces(faces, 1.5)
    _fresh(monkeypatch, 4)
    prims, atlas = vis.pack_faces(faces, 1.5, labels=True)
    assert len(prims) == len(plain) + 2 and len(atlas) > 0
    assert np.array_equal(prims[:8], plain[:8]) and np.array_equal(prims[10:], plain[8:])
    assert list(prims['kind'][8:10]) == [lib.DRAW_BAR, lib.DRAW_MASK] and tuple(prims['rgba'][9]) == (255, 255, 255, 255)
    assert tuple(prims['rgba'][8]) == tuple(plain['rgba'][4])          # the colour map was asked once: marker and tab agree


def test_label_errors_raise_before_anything_is_packed(monkeypatch):
    _fresh(monkeypatch, 0)
    face = {'bbox': np.array([1, 1, 5, 5], np.float32), 'track': 2}
    for scale in (0.03, 0.0, 0.01):                      # round(16 * scale) == 0: Pillow refuses the font size
        with pytest.raises(ValueError):
            vis.pack_faces([[face]], scale, labels=True)
        assert len(vis.pack_faces([[face]], scale)) == 0                 # no labels: nothing to refuse
        assert len(vis.pack_faces([[{'bbox': [1, 1, 5, 5]}]], scale, labels=True)[0]) == 0   # nor with no label to draw
    with pytest.raises(ValueError):
        vis.pack_faces([[face], [{'bbox': [1, 1, 5, 5], 'text': 'two\nlines'}]], labels=True)
    with pytest.raises(ValueError):                      # the box checks come first, as without labels
        vis.pack_faces([[{'bbox': [9, 1, 5, 5], 'text': 'x'}]], labels=True)
    assert len(vis.pack_faces([[face]], 0.04, labels=True)[0]) > 0       # round(0.64) == 1: the smallest legal size


def test_a_label_repeated_over_32_frames_is_one_mask_and_is_cached(monkeypatch):
    _fresh(monkeypatch, 0)
    monkeypatch.setattr(vis, '_masks', type(vis._masks)())
    calls = []
    real = vis.label_font(16)

    class Counting:
        key = ('counting', 16)
        measure = staticmethod(real.measure)

        @staticmethod
        def mask(text, start):
            calls.append((text, start))
            return real.mask(text, start)
    monkeypatch.setattr(vis, 'label_font', lambda size: Counting)
    faces = [[{'bbox': np.array([10, 20 + f, 90, 80], np.float32), 'track': 5},
              {'bbox': np.array([30.5, 5 * f, 60, 300], np.float32), 'track': 6}] for f in range(32)]
    prims, atlas = vis.pack_faces(faces, 1.0, labels=True)
    masks = prims[prims['kind'] == lib.DRAW_MASK]
    assert len(masks) == 64 and sorted(set(masks['frame'])) == list(range(32))
    area = (masks['x1'] - masks['x0'] + 1) * (masks['y1'] - masks['y0'] + 1)
    offs = sorted(set(zip(masks['width'].tolist(), area.tolist())))
    assert len(offs) == 2 and offs[0][0] == 0 and offs[1][0] == offs[0][1] and len(atlas) == offs[0][1] + offs[1][1]
    assert len(calls) == 2                                # one rasterisation per distinct (text, fractional start) ...
    vis.pack_faces(faces, 1.0, labels=True)
    assert len(calls) == 2                                # ... and none on the next batch of the video
    # the LRU forgets the least recently used label first
    full = len(vis._masks)                                # the two bitmaps and the metrics of 'M', 'Mq', '#5', '#6'
    monkeypatch.setattr(vis, 'LABEL_CACHE_SIZE', full)
    vis.pack_faces([[{'bbox': [0, 0, 9, 9], 'text': 'new'}]], 1.0, labels=True)     # pushes '#5' out
    assert len(calls) == 3 and len(vis._masks) == full == 6
    vis.pack_faces(faces, 1.0, labels=True)
    assert len(calls) == 5


def test_a_label_of_spaces_draws_the_tab_only(monkeypatch):
    _fresh(monkeypatch, 0)
    prims, atlas = vis.pack_faces([[{'bbox': [5, 5, 30, 30], 'text': '   ', 'name': 'a'}]], labels=True)
    assert list(prims['kind']) == [lib.DRAW_BAR] * 5 and len(atlas) == 0
    assert prims['x1'][4] > prims['x0'][4] == 5 and prims['y1'][4] > prims['y0'][4] == 5
