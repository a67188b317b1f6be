"""CPU tests (no GPU) of the pixel-value operations: the numpy model (tests/tone_model.py) against the recorded Pillow
golden (tests/golden/tone.npz) and, where Pillow is installed, against Pillow itself on seeded cases; and the host half of
the product -- terran_amd.image's table builders and histogram_stats, terran_amd.vis.pack_stats -- fed the golden's
histograms, against the golden's tables and ImageStat values, exactly."""
import numpy as np
import pytest

from terran_amd import image, lib, vis
from tests import tone_model as T


def _regions(dt, rows, **more):
    q = np.zeros(len(rows), dt)
    for k, name in enumerate(('frame', 'x0', 'y0', 'x1', 'y1', 'shape')):
        q[name] = rows[:, k] if len(rows) else 0
    for name, v in more.items():
        q[name] = v
    return q


def test_model_histograms_equal_the_golden():
    g = T.golden()
    sources = [str(s) for s in g['hist_sources']]
    assert len(sources) >= 23 and str(g['pillow_version'])
    for i, name in enumerate(sources):
        frames = T.source(name)
        q = _regions(lib.HIST_DT, g['hist_%d_regions' % i])
        assert np.array_equal(T.hist_regions(frames, q, 'RGB'), g['hist_%d_rgb' % i]), name
        assert np.array_equal(T.hist_regions(frames, q, 'L'), g['hist_%d_l' % i]), name


def test_model_point_and_saturate_equal_the_golden():
    g = T.golden()
    for name in g['point_names']:
        rows = g['point_%s_regions' % name]
        got = T.point_regions(g['point_%s_source' % name].copy(), _regions(lib.POINT_DT, rows, lut=rows[:, 6]), g['point_%s_luts' % name])
        assert np.array_equal(got, g['point_%s_expected' % name]), name
    for name in g['saturate_names']:
        q = _regions(lib.SATURATE_DT, g['saturate_%s_regions' % name], factor=g['saturate_%s_factors' % name])
        got = T.saturate_regions(g['batch'][:2].copy(), q)
        assert np.array_equal(got, g['saturate_%s_expected' % name]), name
    # the inputs can tell a fused multiply-add from Pillow's multiply and add, by the file's count and by the model's
    for f in (1.2, 1.7):
        assert int(g['saturate_factor_%g_fma' % f]) >= 1
        assert sum(T.fma_changes(img, f) for img in g['batch'][:2]) == int(g['saturate_factor_%g_fma' % f])


def _caller_frames():
    g = T.golden()
    return list(T.dim(g['batch'])[:2]) + [T.dim(g['small'])]


CALLS = {'equalize': T.equalize, 'autocontrast': T.autocontrast,
         'autocontrast_cutoff': lambda im: T.autocontrast(im, cutoff=(2, 5)),
         'autocontrast_ignore': lambda im: T.autocontrast(im, ignore=0),
         'autocontrast_tone': lambda im: T.autocontrast(im, cutoff=1, preserve_tone=True),
         'brightness': lambda im: T.brightness(im, 1.2), 'contrast': lambda im: T.contrast(im, 1.7),
         'color': lambda im: T.color(im, 1.2), 'grayscale': lambda im: T.color(im, 0.0)}


def test_model_callers_and_stats_equal_the_golden():
    g = T.golden()
    frames = _caller_frames()
    assert sorted(CALLS) == sorted(str(n) for n in g['call_names'])
    for name, fn in CALLS.items():
        want = list(g['call_%s_a' % name]) + list(g['call_%s_b' % name])
        for img, w in zip(frames, want):
            assert np.array_equal(fn(img), w), name
    for mode in ('RGB', 'L'):
        hist = np.stack([T.histogram(f, mode).reshape(-1, 256) for f in frames])
        assert np.array_equal(hist, g['stat_frames_%s_hist' % mode])
        st = T.stats_stack(hist)
        for k in T.STAT_KEYS:
            assert np.array_equal(st[k], g['stat_frames_%s_%s' % (mode, k)]), (mode, k)


def test_table_builders_equal_pillows_tables():
    g = T.golden()
    rgb, lum = g['stat_frames_RGB_hist'], g['stat_frames_L_hist']
    assert np.array_equal(np.stack([image.equalize_lut(h) for h in rgb]), g['call_equalize_luts'])
    assert np.array_equal(np.stack([image.autocontrast_lut(h) for h in rgb]), g['call_autocontrast_luts'])
    assert np.array_equal(np.stack([image.autocontrast_lut(h, cutoff=(2, 5)) for h in rgb]), g['call_autocontrast_cutoff_luts'])
    assert np.array_equal(np.stack([image.autocontrast_lut(h, ignore=0) for h in rgb]), g['call_autocontrast_ignore_luts'])
    assert np.array_equal(np.stack([np.tile(image.autocontrast_lut(h, cutoff=1), 3) for h in lum]), g['call_autocontrast_tone_luts'])
    assert g['call_equalize_luts'].max() == 255 and (g['call_autocontrast_luts'] != np.tile(np.arange(256), 3)).any()
    for in1, f, want in zip(g['blend_in1'], g['blend_factor'], g['blend_table']):
        assert np.array_equal(image.blend_lut(in1, f), want), (in1, f)
        assert np.array_equal(T.blend_lut(in1, f), want), (in1, f)
        if in1 == 0:
            assert np.array_equal(image.brightness_lut(f), want)
        assert np.array_equal(image.contrast_lut(f, in1 - 0.5), want) and np.array_equal(image.contrast_lut(f, in1 + 0.49), want)
    # the identity cases: one used bin, a step of 0, hi <= lo, an empty histogram
    one = np.zeros(256, np.int64)
    one[7] = 1000
    few = np.zeros(256, np.int64)
    few[[3, 200]] = 100, 5
    ident = np.arange(256)
    for h in (one, few, np.zeros(256, np.int64)):
        assert np.array_equal(image.equalize_lut(h), ident) and np.array_equal(T.equalize_lut(h), ident)
    assert np.array_equal(image.autocontrast_lut(one), ident) and np.array_equal(image.autocontrast_lut(one * 0), ident)
    assert np.array_equal(image.autocontrast_lut(few, cutoff=50), T.autocontrast_lut(few, cutoff=50))
    assert np.array_equal(image.invert_lut(), 255 - ident)
    assert np.array_equal(image.posterize_lut(2), ident & 0xC0) and np.array_equal(image.posterize_lut(8), ident)
    assert np.array_equal(image.solarize_lut(100), np.where(ident < 100, ident, 255 - ident))
    for bad in (np.nan, np.inf, 'x'):
        with pytest.raises(ValueError):
            image.brightness_lut(bad)
    with pytest.raises(ValueError):
        image.posterize_lut(0)
    with pytest.raises(ValueError):
        image.equalize_lut(np.zeros(255, np.int64))


def test_histogram_stats_equal_imagestat():
    g = T.golden()
    for group in ('stat_frames', 'stat_boxes', 'face_box', 'face_ellipse'):
        for mode in ('RGB', 'L'):
            st = image.histogram_stats(g['%s_%s_hist' % (group, mode)])
            for k in T.STAT_KEYS:
                want = g['%s_%s_%s' % (group, mode, k)]
                assert st[k].shape == want.shape and np.array_equal(st[k], want), (group, mode, k)
    empty = image.histogram_stats(np.zeros((2, 256), np.uint32))           # what Stat returns for a mask that covers nothing
    assert empty['count'].tolist() == [0, 0] and empty['median'].tolist() == [255, 255] and empty['extrema'].tolist() == [[255, 0]] * 2
    assert not empty['mean'].any() and not empty['var'].any() and not empty['stddev'].any() and not empty['rms'].any()
    with pytest.raises(ValueError):
        image.histogram_stats(np.zeros((3, 255), np.uint32))


def test_pack_stats_clips_as_pack_blur():
    g = T.golden()
    faces = [[], [], []]
    for f, b in zip(g['face_frames'], g['face_bboxes']):
        faces[f].append({'bbox': b})
    margin = float(g['face_margin'])
    regions, index = vis.pack_stats(faces, (3, 37, 53, 3), margin, 'ellipse')
    assert np.array_equal(index, g['face_index']) and len(regions) == 4 and (regions['shape'] == lib.BLUR_ELLIPSE).all()
    blur = vis.pack_blur(faces, (3, 37, 53, 3), radius=1.0, margin=margin)
    for k in ('frame', 'x0', 'y0', 'x1', 'y1'):
        assert np.array_equal(regions[k], blur[k])
    assert regions['x0'].min() == 0 and regions['y0'].min() == 0            # the margin pushed a box past the frame's edge
    want = [T.clipped_box(b, 37, 53, margin) for b in g['face_bboxes']]
    assert [tuple(int(v) for v in (q['x0'], q['y0'], q['x1'], q['y1'])) for q in regions] == [w for w in want if w[2] > w[0] and w[3] > w[1]]
    assert vis.pack_stats([[], []], (2, 37, 53, 3))[0].shape == (0,)
    with pytest.raises(ValueError):
        vis.pack_stats(faces, (3, 37, 53, 3), shape='disc')


def test_model_equals_pillow_on_seeded_cases():
    PIL = pytest.importorskip('PIL')
    from PIL import Image, ImageDraw, ImageEnhance, ImageOps, ImageStat
    rng = np.random.default_rng(20261019)
    for case in range(300):
        h, w = int(rng.integers(1, 24)), int(rng.integers(1, 24))
        img = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
        if case % 3 == 1:
            img = T.dim(img)
        elif case % 3 == 2:
            img = (img // int(rng.integers(16, 200))).astype(np.uint8)      # few values: the identity cases of the tables
        im = Image.fromarray(img)
        mask = None
        if case % 2:
            m = Image.new('L', (w, h))
            ImageDraw.Draw(m).ellipse([0, 0, w - 1, h - 1], fill=255)
            mask = np.asarray(m) == 255
            assert np.array_equal(mask, T.mask_of(h, w, T.ELLIPSE))
            assert im.histogram(m) == T.histogram(img, 'RGB', mask).reshape(-1).tolist()
            assert im.convert('L').histogram(m) == T.histogram(img, 'L', mask).tolist()
        assert np.array_equal(np.asarray(im.convert('L')), T.luma(img))
        assert im.histogram() == T.histogram(img).reshape(-1).tolist()
        f = float(rng.choice([0.0, 0.3, 0.5, 0.999, 1.0, 1.2, 1.7, 2.5, -0.5, 3.3333, rng.uniform(-1, 4)]))
        assert np.array_equal(np.asarray(ImageEnhance.Color(im).enhance(f)), T.color(img, f)), f
        assert np.array_equal(np.asarray(ImageEnhance.Brightness(im).enhance(f)), T.brightness(img, f)), f
        assert np.array_equal(np.asarray(ImageEnhance.Contrast(im).enhance(f)), T.contrast(img, f)), f
        assert np.array_equal(np.asarray(ImageOps.equalize(im)), T.equalize(img))
        cutoff = [0, 3, (2, 5), 7.5, 60][case % 5]
        ignore = [None, 0, [0, 255]][case % 3]
        tone = bool(case % 4 == 0)
        want = np.asarray(ImageOps.autocontrast(im, cutoff=cutoff, ignore=ignore, preserve_tone=tone))
        assert np.array_equal(want, T.autocontrast(img, cutoff, ignore, tone)), (cutoff, ignore, tone)
        hist = T.histogram(img, 'RGB', mask)
        if hist.sum():
            lut = image.autocontrast_lut(hist, cutoff, ignore)
            assert np.array_equal(lut, T.autocontrast_lut(hist, cutoff, ignore))
        st, mine, prod = ImageStat.Stat(im), T.stats(T.histogram(img)), image.histogram_stats(T.histogram(img))
        for k in T.STAT_KEYS:
            assert np.array_equal(np.array(getattr(st, k)), np.array(mine[k])), k
            assert np.array_equal(np.array(getattr(st, k)), prod[k]), k
    assert PIL.__version__
