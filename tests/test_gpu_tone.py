"""-m gpu: ta_frames_histogram / ta_frames_point / ta_frames_saturate and the pixel-value callers of terran_amd.image and
terran_amd.vis.face_stats against the recorded Pillow golden (tests/golden/tone.npz), bit for bit over whole frames, so a
pixel outside every region is checked too.  Reads no Pillow and no reference.

The shapes are the ones csrc/tone.hip can go wrong at: a row is walked as a head of 0 .. 3 single pixels up to the first
4-byte aligned one, groups of four pixels and a tail of 0 .. 3, so widths 1, 3, 5 (no group at all), 53, 64, 257 (more
units than a wave has lanes) with boxes at even and odd x0 meet every head and tail; heights 1, 2, 37 leave waves of a
workgroup without a row and give them several; the flat 300 x 517 frame puts 155 100 > 65 535 counts into one bin through
ten workgroups and every lane of a wave onto one LDS address."""
import numpy as np
import pytest

from terran_amd import image, lib, runtime, vis
from tests import tone_model as T

pytestmark = pytest.mark.gpu


def _regions(dt, rows, **more):
    q = np.zeros(len(rows), dt)
    for k, name in enumerate(('frame', 'x0', 'y0', 'x1', 'y1', 'shape')):
        q[name] = rows[:, k] if len(rows) else 0
    for name, v in more.items():
        q[name] = v
    return q


def _differing(got, want):
    return [int((g != w).any(-1).sum()) for g, w in zip(got, want)]


class _resident:
    """Host frames uploaded for the length of a `with`, freed afterwards."""

    def __init__(self, *hosts):
        self.hosts = hosts

    def __enter__(self):
        ctx = runtime.get_context(0)
        self.frames = [ctx.upload(np.ascontiguousarray(h)) for h in self.hosts]
        return self.frames if len(self.frames) > 1 else self.frames[0]

    def __exit__(self, *exc):
        for f in self.frames:
            f.free()


def test_histograms_equal_the_golden():
    g = T.golden()
    sources = [str(s) for s in g['hist_sources']]
    seen_w, seen_h, most = set(), set(), 0
    for i, name in enumerate(sources):
        host = T.source(name)
        rows = g['hist_%d_regions' % i]
        q = _regions(lib.HIST_DT, rows)
        with _resident(host) as frames:
            rgb, lum = frames.histogram(q, lib.HIST_RGB), frames.histogram(q, lib.HIST_L)
            assert np.array_equal(frames.download(), host)
        assert rgb.dtype == np.uint32 and rgb.shape == (len(q), 3, 256) and lum.shape == (len(q), 256)
        bad = [k for k in range(len(q)) if not np.array_equal(rgb[k], g['hist_%d_rgb' % i][k])]
        assert not bad, (name, 'RGB', rows[bad].tolist())
        bad = [k for k in range(len(q)) if not np.array_equal(lum[k], g['hist_%d_l' % i][k])]
        assert not bad, (name, 'L', rows[bad].tolist())
        seen_w.add(host.shape[2]), seen_h.add(host.shape[1])
        most = max(most, len(q), 0)
    # the cases the file must hold: every width and height, 40 regions in one call, frames out of order, a box twice,
    # the 1 x 1 ellipse without a pixel, a bin above 65535
    assert {1, 3, 5, 53, 64, 257} <= seen_w and {1, 2, 37} <= seen_h and most >= 40
    i = sources.index('batch')
    rows = g['hist_%d_regions' % i]
    assert rows[:, 0].tolist()[:3] == [2, 0, 1] and rows[1].tolist() == rows[4].tolist()
    assert rows[3].tolist() == [2, 11, 9, 12, 10, 1] and not g['hist_%d_rgb' % i][3].any() and g['hist_%d_rgb' % i][7].sum() == 3
    assert {(2, 2), (9, 6)} <= {(int(r[3] - r[1]), int(r[4] - r[2])) for r in rows if r[5] == 1}
    assert g['hist_%d_rgb' % sources.index('flat_517x300')].max() == 155100
    assert 'two_37x64' in sources and 'ramp_37x257' in sources


def test_histogram_of_nothing_and_invalid_regions_leave_the_output_alone():
    host = T.source('batch')
    H, W = host.shape[1:3]
    good = (1, 5, 5, 40, 30, 0)
    bad = [(3, 0, 0, 9, 9, 0), (-1, 0, 0, 9, 9, 0), (0, 9, 0, 9, 9, 0), (0, 0, 12, 9, 12, 0), (0, 9, 0, 3, 9, 0),
           (0, -1, 0, 9, 9, 0), (0, 0, 0, W + 1, 9, 0), (0, 0, 0, 9, H + 1, 0), (0, 0, -2, 9, 9, 0), (0, 0, 0, 9, 9, 2), (0, 0, 0, 9, 9, -1)]
    ctx = runtime.get_context(0)
    with _resident(host) as frames:
        assert frames.histogram(_regions(lib.HIST_DT, np.zeros((0, 6), np.int32))).shape == (0, 3, 256)       # n = 0: TA_OK
        for b in bad:
            q = _regions(lib.HIST_DT, np.array([good, b, good], np.int32))
            out = np.full((3, 3, 256), 0xDEADBEEF, np.uint32)
            rc = ctx.lib.ta_frames_histogram(ctx.h, frames.h, lib.ptr(q), 3, lib.HIST_RGB, lib.ptr(out))
            assert rc == lib.E_INVALID and b'region 1' in ctx.lib.ta_last_error(ctx.h), b
            assert (out == 0xDEADBEEF).all(), b
        out = np.full((1, 256), 0xDEADBEEF, np.uint32)
        q = _regions(lib.HIST_DT, np.array([good], np.int32))
        assert ctx.lib.ta_frames_histogram(ctx.h, frames.h, lib.ptr(q), 1, 2, lib.ptr(out)) == lib.E_INVALID     # unknown mode
        assert ctx.lib.ta_frames_histogram(ctx.h, frames.h, lib.ptr(q), 1, lib.HIST_L, None) == lib.E_INVALID   # no output
        assert (out == 0xDEADBEEF).all()
        with pytest.raises(lib.TerranAmdError):
            frames.histogram(_regions(lib.HIST_DT, np.array([bad[0]], np.int32)))
        other = runtime.new_context(0)                                      # the caller's context, as in blur
        assert np.array_equal(frames.histogram(q, lib.HIST_L, ctx=other), T.hist_regions(host, q, 'L'))


def _run_point(g, name):
    rows = g['point_%s_regions' % name]
    host = g['point_%s_source' % name]
    with _resident(host) as frames:
        frames.point(_regions(lib.POINT_DT, rows, lut=rows[:, 6]), g['point_%s_luts' % name])
        return host, frames.download()


def test_point_equals_the_golden():
    g = T.golden()
    names = [str(n) for n in g['point_names']]
    assert {'identity', 'three_bands', 'per_frame', 'invert_then_posterize', 'posterize_then_invert', 'ellipse'} <= set(names)
    for name in names:
        host, got = _run_point(g, name)
        want = g['point_%s_expected' % name]
        assert np.array_equal(got, want), (name, _differing(got, want))
        assert np.array_equal(got, host) == (name == 'identity')
    assert not np.array_equal(g['point_invert_then_posterize_expected'], g['point_posterize_then_invert_expected'])


def test_point_refuses_a_bad_table_index_before_any_pixel_changes():
    g = T.golden()
    host = g['batch']
    luts = g['point_ellipse_luts']
    rows = np.array([(0, 0, 0, 53, 37, 0, 0), (1, 0, 0, 53, 37, 0, 2), (2, 0, 0, 53, 37, 0, 1)], np.int32)
    with _resident(host) as frames:
        for index in (2, -1):
            rows[1, 6] = index
            with pytest.raises(lib.TerranAmdError) as e:
                frames.point(_regions(lib.POINT_DT, rows, lut=rows[:, 6]), luts)
            assert e.value.code == lib.E_INVALID and 'region 1' in str(e.value)
        with pytest.raises(lib.TerranAmdError):
            frames.point(_regions(lib.POINT_DT, np.array([(0, 0, 0, 54, 37, 0, 0)], np.int32), lut=0), luts)
        frames.point(_regions(lib.POINT_DT, np.zeros((0, 7), np.int32)), luts)          # n = 0: TA_OK
        assert np.array_equal(frames.download(), host)


def test_saturate_equals_the_golden():
    g = T.golden()
    names = [str(n) for n in g['saturate_names']]
    assert {'factor_%g' % f for f in T.FACTORS} | {'overlap', 'ellipse'} <= set(names)
    # a build that fuses the multiply and the add cannot pass: these inputs tell the two apart
    assert int(g['saturate_factor_1.2_fma']) >= 1 and int(g['saturate_factor_1.7_fma']) >= 1
    host = g['batch'][:2]
    for name in names:
        q = _regions(lib.SATURATE_DT, g['saturate_%s_regions' % name], factor=g['saturate_%s_factors' % name])
        with _resident(host) as frames:
            frames.saturate(q)
            got = frames.download()
        want = g['saturate_%s_expected' % name]
        assert np.array_equal(got, want), (name, _differing(got, want))
    swapped = _regions(lib.SATURATE_DT, g['saturate_overlap_regions'][[1, 0, 3, 2]], factor=g['saturate_overlap_factors'][[1, 0, 3, 2]])
    with _resident(host) as frames:
        frames.saturate(swapped)
        got = frames.download()
        assert np.array_equal(got, T.saturate_regions(host.copy(), swapped)) and not np.array_equal(got, g['saturate_overlap_expected'])
        for f in (np.nan, np.inf, -np.inf):
            with pytest.raises(lib.TerranAmdError) as e:
                frames.saturate(_regions(lib.SATURATE_DT, np.array([(0, 0, 0, 5, 5, 0), (1, 0, 0, 5, 5, 0)], np.int32), factor=[0.5, f]))
            assert e.value.code == lib.E_INVALID and 'region 1' in str(e.value)
        assert np.array_equal(frames.download(), got)


def _dim_list():
    g = T.golden()
    return T.dim(g['batch'])[:2], T.dim(g['small'])[None]


CALLS = {'equalize': image.equalize_frames, 'autocontrast': image.autocontrast_frames,
         'autocontrast_cutoff': lambda f: image.autocontrast_frames(f, cutoff=(2, 5)),
         'autocontrast_ignore': lambda f: image.autocontrast_frames(f, ignore=0),
         'autocontrast_tone': lambda f: image.autocontrast_frames(f, cutoff=1, preserve_tone=True),
         'brightness': lambda f: image.brightness_frames(f, 1.2), 'contrast': lambda f: image.contrast_frames(f, 1.7),
         'color': lambda f: image.color_frames(f, 1.2), 'grayscale': image.grayscale_frames}


@pytest.mark.parametrize('name', sorted(CALLS))
def test_callers_equal_pillow_on_a_mixed_size_list(name):
    g = T.golden()
    assert sorted(CALLS) == sorted(str(n) for n in g['call_names'])
    a, b = _dim_list()
    with _resident(a, b) as frames:
        assert CALLS[name](frames) is frames
        got = [f.download() for f in frames]
    for part, key in zip(got, 'ab'):
        want = g['call_%s_%s' % (name, key)]
        assert np.array_equal(part, want), (name, key, _differing(part, want))
    if name == 'equalize':                                                  # a single batch, and the table-only callers
        with _resident(a) as frames:
            assert image.equalize_frames(frames) is frames
            assert np.array_equal(frames.download(), g['call_equalize_a'])
            for fn, lut in ((image.invert_frames, image.invert_lut()), (lambda f: image.posterize_frames(f, 3), image.posterize_lut(3)),
                            (lambda f: image.solarize_frames(f, 99), image.solarize_lut(99))):
                before = frames.download()
                fn(frames)
                assert np.array_equal(frames.download(), np.stack([T.point(x, np.tile(lut, 3)) for x in before]))
            with pytest.raises(ValueError):
                image.point_frames(frames, np.arange(255))


def test_frame_stats_and_face_stats_equal_imagestat():
    g = T.golden()
    a, b = _dim_list()
    with _resident(a, b) as frames:
        for mode in ('RGB', 'L'):
            hist = image.histogram_frames(frames, mode)
            assert np.array_equal(hist.reshape(3, -1, 256), g['stat_frames_%s_hist' % mode])
            whole, boxed = image.frame_stats(frames, mode), image.frame_stats(frames, mode, boxes=g['stat_boxes'])
            for k in T.STAT_KEYS:
                assert np.array_equal(whole[k], g['stat_frames_%s_%s' % (mode, k)]), (mode, k)
                assert np.array_equal(boxed[k], g['stat_boxes_%s_%s' % (mode, k)]), (mode, k)
        with pytest.raises(ValueError):
            image.frame_stats(frames, 'RGB', boxes=[(0, 0, 54, 37)] * 3)
        with pytest.raises(ValueError):
            image.histogram_frames(frames, 'YCbCr')
    faces = [[], [], []]
    for f, box in zip(g['face_frames'], g['face_bboxes']):
        faces[f].append({'bbox': box})
    margin = float(g['face_margin'])
    with _resident(T.dim(g['batch'])) as frames:
        for shape in ('box', 'ellipse'):
            for mode in ('RGB', 'L'):
                st, index = vis.face_stats(frames, faces, margin=margin, shape=shape, mode=mode)
                assert np.array_equal(index, g['face_index'])
                assert np.array_equal(st['histogram'].reshape(len(index), -1, 256), g['face_%s_%s_hist' % (shape, mode)])
                for k in T.STAT_KEYS:
                    assert np.array_equal(st[k], g['face_%s_%s_%s' % (shape, mode, k)]), (shape, mode, k)
        assert vis.face_stats(frames, [[], []]) == (None, [])
