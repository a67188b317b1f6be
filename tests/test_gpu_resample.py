"""-m gpu: ta_frames_resample / ta_frames_pixelate and their callers (image.resize_frames, vis.crop_faces,
vis.blur_faces / anonymize_faces with method='pixelate') against the recorded Pillow golden (tests/golden/resample.npz),
bit for bit.  Reads no Pillow and no reference."""
import os

import numpy as np
import pytest

from terran_amd import image, lib, runtime, vis
from tests import resample_model as M

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'resample.npz')


@pytest.fixture(scope='module')
def golden():
    return M.golden(GOLDEN)


def _regions(rows, dt=lib.RESAMPLE_DT):
    q = np.zeros(len(rows), dt)
    for i, r in enumerate(rows):
        q[i] = tuple(r)
    return q


def _resample(frames, regions, size, filt):
    out = frames.resample(regions, size[1], size[0], filt)
    try:
        return out.download()
    finally:
        out.free()


def test_resample_equals_the_golden(golden):
    """Every filter; outputs 1 x 1, 5 x 3, 64 x 48; regions of three frames in one call, frames out of order; boxes on every
    border, fractional, narrower than a pixel; a 1 x 1 source; 300 x 517 -> 7 x 5 lanczos (445 and 361 taps: the horizontal
    pass's global-memory loop); one pass skipped, both skipped."""
    z, cases, _ = golden
    ctx = runtime.get_context(0)
    resident = {}
    try:
        filters, long_taps, skipped = set(), 0, 0
        for k, c in enumerate(cases):
            key = id(c['source'])
            if key not in resident:
                resident[key] = ctx.upload(c['source'])
            got = _resample(resident[key], c['regions'], c['size'], c['filter'])
            assert got.shape == c['expected'].shape, (k, got.shape)
            assert np.array_equal(got, c['expected']), (k, c['filter'], c['size'], [int((g != e).sum()) for g, e in zip(got, c['expected'])])
            filters.add(c['filter'])
            long_taps += c['source'].shape[2] == 517 and c['size'] == (7, 5)
            skipped += c['size'][0] == c['source'].shape[2] or c['size'][1] == c['source'].shape[1]
            frames = c['regions']['frame'].tolist()
            if len(frames) == 8:
                assert frames != sorted(frames) and set(frames) == {0, 1, 2}
        assert filters == set(range(6)) and long_taps == 1 and skipped >= 9
        assert resident[id(cases[0]['source'])].resample(_regions([]), 5, 5, lib.BICUBIC) is None       # n = 0
    finally:
        for f in resident.values():
            f.free()


def test_resize_frames_on_a_batch_and_on_a_mixed_list(golden):
    z, _, _ = golden
    ctx = runtime.get_context(0)
    batch = ctx.upload(z['frames'])
    others = [ctx.upload(z['mixed_1'][None]), ctx.upload(z['mixed_2'][None])]
    first = ctx.upload(z['frames'][:1])
    made = []
    try:
        out = image.resize_frames(batch, (40, 30), 'lanczos')
        made.append(out)
        assert out.shape == (3, 30, 40, 3) and np.array_equal(out.download(), z['batch_lanczos_40x30'])
        out = image.resize_frames(batch, (17, 23), lib.HAMMING, box=tuple(z['batch_box']))
        made.append(out)
        assert out.shape == (3, 23, 17, 3) and np.array_equal(out.download(), z['batch_hamming_box_17x23'])
        out = image.resize_frames([first] + others, (32, 24), resample='bilinear')
        made.append(out)
        assert isinstance(out, lib.Frames) and out.shape == (3, 24, 32, 3)
        assert np.array_equal(out.download(), z['mixed_bilinear_32x24'])              # the images in input order
        out = image.resize_frames(others[::-1] + [first], (32, 24), resample='bilinear')
        made.append(out)
        assert np.array_equal(out.download(), z['mixed_bilinear_32x24'][::-1])
        with pytest.raises(ValueError):
            image.resize_frames([first] + others, (32, 24), box=(0, 0, 40, 20))     # outside the 17-wide image
    finally:
        for f in made + others + [batch, first]:
            f.free()


def test_crop_faces_and_their_jpegs(golden):
    z, _, _ = golden
    ctx = runtime.get_context(0)
    faces = [[], [{'bbox': b.astype(np.float32)} for b in z['chip_bbox']]]
    frames = ctx.upload(z['frames'][:2])
    chips = up = None
    try:
        chips, index = vis.crop_faces(frames, faces, size=(16, 20), margin=float(z['chip_margin']))
        want = z['chips_bicubic_16x20']
        assert chips.shape == (3, 20, 16, 3) and np.array_equal(chips.download(), want)
        assert index.dtype == np.int32 and index.tolist() == [[1, 0], [1, 1], [1, 3]]      # face 2 lies outside the frame
        up = ctx.upload(want)
        files = image.encode_jpeg(chips, quality=90)
        assert len(files) == 3 and files == image.encode_jpeg(up, quality=90)
        assert vis.crop_faces(frames, [[], []])[0] is None and vis.crop_faces(frames, [[], []])[1].shape == (0, 2)
        assert np.array_equal(frames.download(), z['frames'][:2])
    finally:
        for f in (chips, up, frames):
            if f is not None:
                f.free()


def test_pixelate_equals_the_golden(golden):
    """Both shapes, overlapping faces in both orders, a block larger than the box, block 1, sides 1 .. 40, a margin; whole
    frames are compared, so pixels outside the regions are checked; a neighbour frame stays as it is."""
    _, _, scenes = golden
    ctx = runtime.get_context(0)
    shapes = set()
    for s in scenes:
        kw = dict(method='pixelate', block=s['block'], margin=s['margin'], shape=s['shape'])
        base = s['base'].copy()
        got = vis.anonymize_faces(base, s['faces'], **kw)
        assert np.array_equal(base, s['base']) and np.array_equal(got, s['expected']), s['name']
        frames = ctx.upload(np.stack([base, base, base]))
        try:
            assert vis.blur_faces(frames, [[], s['faces']], **kw) is frames
            assert np.array_equal(frames.download(), np.stack([base, s['expected'], base])), s['name']
        finally:
            frames.free()
        shapes.add(s['shape'])
    assert shapes == {'box', 'ellipse'}


def test_gaussian_stays_what_it_was(golden):
    _, _, scenes = golden
    s = scenes[0]
    ctx = runtime.get_context(0)
    outs = []
    for kw in (dict(), dict(method='gaussian')):
        frames = ctx.upload(s['base'][None])
        try:
            vis.blur_faces(frames, [s['faces']], shape='ellipse', margin=0.1, **kw)
            outs.append(frames.download())
        finally:
            frames.free()
    assert np.array_equal(outs[0], outs[1]) and not np.array_equal(outs[0][0], s['base'])
    assert np.array_equal(vis.anonymize_faces(s['base'], s['faces'], method='gaussian'), vis.anonymize_faces(s['base'], s['faces']))


def test_a_wide_region_and_many_rows():
    """More than one tile across (64 pixels) and more than one group of rows down (16), against the model."""
    rng = np.random.default_rng(4)
    host = rng.integers(0, 256, (2, 75, 150, 3), dtype=np.uint8)
    regions = _regions([(1, 3.5, 2.25, 149.0, 70.5), (0, 0, 0, 150, 75)])
    pix = _regions([(0, 5, 4, 140, 73, lib.BLUR_ELLIPSE, 2), (1, 0, 0, 150, 75, lib.BLUR_BOX, 7), (0, 100, 30, 150, 75, lib.BLUR_BOX, 5)],
                   lib.PIXELATE_DT)
    ctx = runtime.get_context(0)
    frames = ctx.upload(host)
    try:
        for filt, size in ((lib.BICUBIC, (131, 70)), (lib.BOX, (67, 33)), (lib.NEAREST, (140, 90))):
            assert np.array_equal(_resample(frames, regions, size, filt), M.resample_regions(host, regions, size, filt)), filt
        frames.pixelate(pix)
        assert np.array_equal(frames.download(), M.pixelate_regions(host.copy(), pix))
    finally:
        frames.free()
    # 2100 rows -> 2 with lanczos: 6301 taps a row, beyond what the vertical pass stages in LDS
    tall = rng.integers(0, 256, (1, 2100, 3, 3), dtype=np.uint8)
    whole = _regions([(0, 0, 0, 3, 2100)])
    frames = ctx.upload(tall)
    try:
        assert lib.resample_plan(2100, 0, 2100, 2, lib.LANCZOS)[1].shape[1] == 6301
        assert np.array_equal(_resample(frames, whole, (3, 2), lib.LANCZOS), M.resample_regions(tall, whole, (3, 2), lib.LANCZOS))
    finally:
        frames.free()


def test_invalid_regions_change_nothing():
    rng = np.random.default_rng(6)
    host = rng.integers(0, 256, (2, 30, 40, 3), dtype=np.uint8)
    ctx = runtime.get_context(0)
    frames = ctx.upload(host)
    good = (1, 2.5, 3.5, 30, 20)
    try:
        for bad in [(2, 0, 0, 9, 9), (-1, 0, 0, 9, 9), (0, -0.5, 0, 9, 9), (0, 0, 0, 40.5, 9), (0, 0, 0, 9, 30.25), (0, 9, 0, 9, 9),
                    (0, 0, 12, 9, 3), (0, np.nan, 0, 9, 9)]:
            with pytest.raises(lib.TerranAmdError) as e:
                frames.resample(_regions([good, bad]), 8, 8, lib.BICUBIC)
            assert e.value.code == lib.E_INVALID and 'region 1' in str(e.value), bad
        for filt, oh, ow in [(6, 8, 8), (-1, 8, 8), (3, 0, 8), (3, 8, 0), (3, 16385, 8), (3, 8, 16385)]:
            with pytest.raises(lib.TerranAmdError) as e:
                frames.resample(_regions([good]), oh, ow, filt)
            assert e.value.code == lib.E_INVALID, (filt, oh, ow)
        ok = (1, 5, 5, 35, 25, lib.BLUR_BOX, 4)
        for bad in [(0, 5, 5, 35, 25, 0, 0), (0, 5, 5, 35, 25, 0, -3), (0, 5, 5, 35, 25, 0, 16385), (0, 5, 5, 41, 25, 0, 4),
                    (0, -1, 5, 35, 25, 0, 4), (0, 5, 5, 5, 25, 0, 4), (2, 5, 5, 35, 25, 0, 4), (0, 5, 5, 35, 25, 2, 4)]:
            with pytest.raises(lib.TerranAmdError) as e:
                frames.pixelate(_regions([ok, bad, ok], lib.PIXELATE_DT))
            assert e.value.code == lib.E_INVALID and 'region 1' in str(e.value), bad
        frames.pixelate(_regions([], lib.PIXELATE_DT))   # n = 0: TA_OK
        frames.pixelate(_regions([(0, 0, 0, 40, 30, lib.BLUR_ELLIPSE, 1)], lib.PIXELATE_DT))      # block 1: unchanged
        assert np.array_equal(frames.download(), host)
        frames.pixelate(_regions([ok], lib.PIXELATE_DT))
        assert np.array_equal(frames.download(), M.pixelate_regions(host.copy(), _regions([ok], lib.PIXELATE_DT)))
    finally:
        frames.free()
