"""-m gpu: ta_frames_filter and the filter callers of terran_amd.image and terran_amd.vis against the recorded Pillow golden
(tests/golden/filter.npz), bit for bit over whole frames, so a pixel outside every region is checked too.  Reads no
Pillow and no reference.

csrc/filter.hip works in tiles of 128 x 32 pixels (TILE_W x TILE_H) with a halo of size / 2 pixels, at most 3: the frames
of 33 x 129 and 34 x 130 (height x width) are one pixel beyond the tile and at tile + halo - 1.  Widths 1 .. 6 lie below,
at and above both kernel sizes and have no group of four pixels or just one; 53, 64 and 257 give every head and tail of
the aligned walk and more units than a wave has lanes; heights 1 .. 6 and 37 the same for the rows."""
import numpy as np
import pytest

from terran_amd import image, lib, runtime, vis
from tests import filter_model as M

pytestmark = pytest.mark.gpu


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


def _case(name):
    return next(c for c in M.cases() if c[0] == name)


def test_every_golden_case_through_frames_filter():
    g = M.golden()
    specs = g['specs']
    cases = M.cases()
    assert len(cases) >= 250 and {M.TILE_H + 1, M.TILE_H + M.HALO - 1} <= {M.source(c[1]).shape[1] for c in cases}
    bad = []
    for name, src, rows, want in cases:
        with _resident(M.source(src)) as frames:
            frames.filter(M.regions_of(rows, lib.FILTER_REGION_DT), specs)
            got = frames.download()
        if not np.array_equal(got, want):
            bad.append((name, _differing(got, want)))
    assert not bad, bad[:20]


def test_many_regions_in_one_call_equal_single_region_calls():
    g = M.golden()
    name, src, rows, want = _case('many')
    assert len(rows) >= 40
    q = M.regions_of(rows, lib.FILTER_REGION_DT)
    with _resident(M.source(src)) as frames:
        for k in range(len(q)):
            frames.filter(q[k:k + 1], g['specs'])
        got = frames.download()
    assert np.array_equal(got, want), _differing(got, want)
    swapped = q[::-1].copy()                            # the order matters: rounds
    with _resident(M.source(src)) as frames:
        frames.filter(swapped, g['specs'])
        got = frames.download()
    assert np.array_equal(got, M.filter_regions(M.source(src).copy(), swapped, g['specs'])) and not np.array_equal(got, want)


def _filter_of(name):
    """A case's filter as the callers take it, without Pillow."""
    part = name.split('_')
    if part[0] == 'builtin':
        return lambda f: image.filter_frames(f, name[len('builtin_'):])
    if part[0] == 'rank':
        if (int(part[1]), int(part[2])) in ((3, 4), (5, 12), (7, 24)):
            return lambda f: image.median_frames(f, int(part[1]))
        return lambda f: image.filter_frames(f, image.rank_spec(int(part[1]), int(part[2])))
    if part[0] == 'unsharp':
        return lambda f: image.unsharp_frames(f, float(part[1]), int(part[2]), int(part[3]))
    return lambda f: image.sharpness_frames(f, float(part[1]))


def test_image_callers_equal_the_golden():
    names = [c[0] for c in M.cases() if c[1] == 'small']
    assert len(names) == 10 + len(M.RANKS) + len(M.UNSHARPS) + len(M.SHARPNESS)
    for name in names:
        _, src, rows, want = _case(name)
        with _resident(M.source(src)) as frames:
            assert _filter_of(name)(frames) is frames
            got = frames.download()
        assert np.array_equal(got, want), (name, _differing(got, want))
    with _resident(M.source('small')) as frames:
        assert image.unsharp_frames(frames) is frames and np.array_equal(frames.download(), _case('unsharp_2_150_3')[3])


def test_callers_on_a_mixed_size_list_and_boxes():
    batch, small = M.source('batch'), M.source('small')
    with _resident(batch, small) as frames:
        assert image.filter_frames(frames, 'sharpen') is frames
        got = [f.download() for f in frames]
    assert np.array_equal(got[0], _case('builtin_sharpen_batch')[3]) and np.array_equal(got[1], _case('builtin_sharpen')[3])
    boxes = [(5, 3, 40, 30), (0, 0, 53, 37), (20, 10, 35, 25), (1, 2, 30, 24)]
    spec = image.filter_spec('smooth_more')
    want = [b.copy() for b in (batch, small)]
    at = 0
    for part in want:
        q = np.zeros(len(part), lib.FILTER_REGION_DT)
        q['frame'], q['shape'] = np.arange(len(part)), 1
        for k in range(len(part)):
            q['x0'][k], q['y0'][k], q['x1'][k], q['y1'][k] = boxes[at + k]
        M.filter_regions(part, q, np.stack([spec]))
        at += len(part)
    with _resident(batch, small) as frames:
        image.filter_frames(frames, spec, boxes=boxes, shape='ellipse')
        for f, w in zip(frames, want):
            assert np.array_equal(f.download(), w)
        with pytest.raises(ValueError):
            image.filter_frames(frames, 'sharpen', boxes=[(0, 0, 54, 37)] * 4)
        with pytest.raises(ValueError):
            image.filter_frames(frames, 'sharpen', shape='disc')
        with pytest.raises(ValueError):
            image.median_frames(frames, 9)


def test_filter_faces_equals_the_golden():
    g = M.golden()
    _, src, rows, want = _case('faces')
    faces = [[], [], []]
    for f, b in zip(g['face_frames'], g['face_bboxes']):
        faces[f].append({'bbox': b})
    margin = float(g['face_margin'])
    packed = vis.pack_filter(faces, (3, 37, 53, 3), margin, 'ellipse')
    assert [tuple(int(v) for v in r)[:6] for r in packed] == [tuple(int(v) for v in r)[:6] for r in rows]
    with _resident(M.source(src)) as frames:
        assert vis.filter_faces(frames, faces, 'sharpen', margin=margin, shape='ellipse') is frames
        got = frames.download()
    assert np.array_equal(got, want), _differing(got, want)


def test_gaussian_blur_goes_through_frames_blur():
    class GaussianBlur:                                 # what filter_spec reads of Pillow's class: its name and radius
        def __init__(self, radius):
            self.radius = radius
    host = M.source('batch')
    q = np.zeros(3, lib.BLUR_DT)
    q['frame'], q['x1'], q['y1'], q['radius'] = np.arange(3), 53, 37, 2.5
    with _resident(host, host) as (a, b):
        image.filter_frames(a, GaussianBlur(2.5))
        b.blur(q)
        got = a.download()
        assert np.array_equal(got, b.download()) and not np.array_equal(got, host)


def test_invalid_calls_change_nothing_and_no_regions_is_ok():
    from tests.test_filter_cpu import BAD_ROWS, _bad_specs
    g = M.golden()
    host = M.source('batch')
    H, W = host.shape[1:3]
    ok, bad_specs = _bad_specs()
    good = (1, 5, 5, 40, 30, 0, 0)
    rows = BAD_ROWS + [(3, 0, 0, 9, 9, 0, 0), (-1, 0, 0, 9, 9, 0, 0), (0, -1, 0, 9, 9, 0, 0), (0, 0, 0, W + 1, 9, 0, 0), (0, 0, 0, 9, H + 1, 0, 0),
                       (0, 0, -2, 9, 9, 0, 0)]
    ctx = runtime.get_context(0)
    with _resident(host) as frames:
        frames.filter(np.zeros(0, lib.FILTER_REGION_DT), g['specs'])                     # n = 0: TA_OK
        frames.filter(np.zeros(0, lib.FILTER_REGION_DT), np.zeros(0, lib.FILTER_SPEC_DT))
        for row in rows:
            with pytest.raises(lib.TerranAmdError) as e:
                frames.filter(M.regions_of(np.array([good, row, good], np.int32), lib.FILTER_REGION_DT), np.stack([ok]))
            assert e.value.code == lib.E_INVALID and 'region 1' in str(e.value), row
        for s in bad_specs:
            with pytest.raises(lib.TerranAmdError) as e:
                frames.filter(M.regions_of(np.array([good], np.int32), lib.FILTER_REGION_DT), np.stack([ok, s]))
            assert e.value.code == lib.E_INVALID and 'spec 1' in str(e.value), s
        assert np.array_equal(frames.download(), host)
        other = runtime.new_context(0)                                      # the caller's context, as in blur
        frames.filter(M.regions_of(np.array([good], np.int32), lib.FILTER_REGION_DT), np.stack([ok]), ctx=other)
        want = M.filter_regions(host.copy(), M.regions_of(np.array([good], np.int32), lib.FILTER_REGION_DT), np.stack([ok]))
        assert np.array_equal(frames.download(), want)
    assert ctx is not other
