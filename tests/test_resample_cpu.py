"""No GPU: the host half of ta_frames_resample / ta_frames_pixelate (ta_resample_plan's tables) and the numpy
restatement of the device arithmetic (tests/resample_model.py) against the installed Pillow and the recorded golden
(tests/golden/resample.npz); vis.pack_crops / pack_pixelate and the argument checks of blur_faces / crop_faces /
resize_frames.  All comparisons are exact."""
import ctypes as C
import os

import numpy as np
import pytest

from terran_amd import image, lib, vis
from tests import resample_model as M

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'resample.npz')
FILTERS = sorted(lib.RESAMPLE_FILTERS.values())


def _f32(*v):
    return tuple(float(np.float32(x)) for x in v)


def fuzz_cases(seed=20261018, count=2400):
    """-> [(image, (ow, oh), filter, box or None)]: every filter, sides 1 .. 70 in and out, a quarter each of whole-image,
    free fractional boxes, boxes on one or more borders, and boxes narrower than a pixel."""
    rng = np.random.default_rng(seed)
    out = []
    for it in range(count):
        w, h, ow, oh = (int(v) for v in rng.integers(1, 71, 4))
        if it % 7 == 0:
            w |= 1                                      # odd widths: 3-byte pixels off every alignment
        img = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
        kind, box = it % 4, None
        if kind:
            x0, x1 = sorted(rng.uniform(0, w, 2))
            y0, y1 = sorted(rng.uniform(0, h, 2))
            if kind == 2:
                x0, x1 = (0.0 if rng.random() < .5 else x0), (float(w) if rng.random() < .5 else x1)
                y0, y1 = (0.0 if rng.random() < .5 else y0), (float(h) if rng.random() < .5 else y1)
            if kind == 3:
                x1, y1 = min(w, x0 + rng.uniform(0.01, 0.9)), min(h, y0 + rng.uniform(0.01, 0.9))
            box = _f32(x0, y0, x1, y1)
            if not (box[0] < box[2] and box[1] < box[3]):
                box = None
        out.append((img, (ow, oh), FILTERS[it % 6], box))
    return out


def test_model_on_planned_tables_equals_pillow():
    Image = pytest.importorskip('PIL.Image')
    cases = fuzz_cases()
    assert len(cases) >= 2000
    seen, boxes = set(), 0
    for img, size, filt, box in cases:
        want = np.asarray(Image.fromarray(img).resize(size, filt, box=box))
        got = M.resize(img, size, filt, box)
        assert np.array_equal(got, want), (img.shape, size, filt, box, int((got != want).sum()))
        seen.add((filt, size[0] > img.shape[1], size[1] > img.shape[0]))
        boxes += box is not None
    assert len(seen) == 24 and boxes > 1500              # every filter up and down along both axes


def test_model_equals_the_golden():
    z, cases, scenes = M.golden(GOLDEN)
    assert len(cases) >= 30 and len(scenes) >= 10 and str(z['pillow_version'])
    for k, c in enumerate(cases):
        got = M.resample_regions(c['source'], c['regions'], c['size'], c['filter'])
        assert got.shape == c['expected'].shape and np.array_equal(got, c['expected']), (k, c['filter'], c['size'])
    assert {c['filter'] for c in cases} == set(FILTERS)
    for s in scenes:
        regions = vis.pack_pixelate([s['faces']], s['base'].shape[:2], s['block'], s['margin'], s['shape'])
        got = M.pixelate_regions(s['base'][None].copy(), regions)[0]
        assert np.array_equal(got, s['expected']), s['name']


def test_nearest_accumulates_its_coordinate():
    """Pillow's affine scaler ADDS the step sample by sample; long axes are where b0 + (i + 0.5) * step would drift apart."""
    Image = pytest.importorskip('PIL.Image')
    for w, ow in [(70, 61), (69, 67), (53, 49), (1000, 997), (4000, 3977), (16000, 15999)]:
        box = _f32(0.3, 0, w - 0.45, 1)
        img = (np.arange(w * 3).reshape(1, w, 3) % 251).astype(np.uint8)
        want = np.asarray(Image.fromarray(img).resize((ow, 1), lib.NEAREST, box=box))
        assert np.array_equal(M.resize(img, (ow, 1), lib.NEAREST, box), want), (w, ow)


def test_plan_equals_the_oracle_for_whole_axis_bicubic():
    from oracle import arcface_pre
    for in_size, out_size in [(112, 112), (200, 112), (37, 112), (1080, 112), (53, 7), (5, 64), (1, 3), (300, 1)]:
        bounds, coefs = lib.resample_plan(in_size, 0, in_size, out_size, lib.BICUBIC)
        ob, oc = arcface_pre._resample_coeffs(in_size, out_size)[:2]
        ob, oc = np.asarray(ob), np.asarray(oc)
        assert np.array_equal(bounds.reshape(-1), ob.reshape(-1).astype(np.int32)), (in_size, out_size)
        assert np.array_equal(coefs.reshape(-1), oc.reshape(-1).astype(np.int32)), (in_size, out_size)


def test_plan_equals_the_oracle_on_the_axes_of_the_resize_bicubic_tests():
    """ta_frames_resize_bicubic runs on ta_frames_resample's tables: for every (in, out) axis that the GPU tests of
    Frames.resize_bicubic resize (tests/test_gpu_align.py, tests/test_gpu_pipeline.py) and the embedder's own
    1920 x 1080 -> 112 x 63, bounds and zero-padded coefficients equal oracle.arcface_pre._resample_coeffs, which
    tests/test_align_cpu.py holds to Pillow's recorded output."""
    from oracle import arcface_pre
    from tests import align_cases
    from tests.util import golden
    pins = golden('pil_pins.npz')['resize_in'].shape
    frames = [(src.shape[:2], (h, w)) for src, (w, h), _ in align_cases.bicubic_cases()]
    frames += [(shape[1:], size) for shape, size in align_cases.BICUBIC_EDGE_CASES]
    frames += [((80, 96), (10, 12)), ((450, 600), (600, 900)), ((21, 34), (40, 9)), (pins[:2], (112, 70)), (pins[:2], (40, 61))]
    axes = {(i, o) for ins, outs in frames for i, o in zip(ins, outs)} | {(1080, 63), (1920, 112), (112, 112)}
    ksizes = set()
    for in_size, out_size in sorted(axes):
        bounds, coefs = lib.resample_plan(in_size, 0, in_size, out_size, lib.BICUBIC)
        ob, oc = arcface_pre._resample_coeffs(in_size, out_size)
        assert np.array_equal(bounds, np.asarray(ob, np.int32).reshape(out_size, 2)), (in_size, out_size)
        assert np.array_equal(coefs, np.asarray(oc, np.int32).reshape(out_size, -1)), (in_size, out_size)
        ksizes.add(coefs.shape[1])
    assert {127, 129, 2045, 2049} <= ksizes              # both sides of the kernels' LDS / global coefficient switch


def test_pixelate_model_equals_the_pillow_idiom():
    Image = pytest.importorskip('PIL.Image')
    from PIL import ImageDraw
    rng = np.random.default_rng(5)
    base = rng.integers(0, 256, (50, 60, 3), dtype=np.uint8)

    def pillow(img, regions):
        im = Image.fromarray(img)
        for q in regions:
            box = tuple(int(q[k]) for k in ('x0', 'y0', 'x1', 'y1'))
            w, h, b = box[2] - box[0], box[3] - box[1], int(q['block'])
            crop = im.crop(box)
            region = crop.resize((max(1, w // b), max(1, h // b)), Image.BOX).resize((w, h), Image.NEAREST)
            if q['shape'] == lib.BLUR_ELLIPSE:
                mask = Image.new('L', (w, h))
                ImageDraw.Draw(mask).ellipse([0, 0, w - 1, h - 1], fill=255)
                region = Image.fromarray(np.where((np.asarray(mask) != 255)[..., None], np.asarray(crop), np.asarray(region)))
            im.paste(region, box)
        return np.asarray(im)

    def regions(rows):
        q = np.zeros(len(rows), lib.PIXELATE_DT)
        for i, r in enumerate(rows):
            q[i] = tuple(r)
        return q
    for w, h in [(1, 1), (1, 9), (7, 5), (40, 33)]:
        for block in (1, 2, 3, 8, 64):
            for shape in (lib.BLUR_BOX, lib.BLUR_ELLIPSE):
                q = regions([(0, 11, 9, 11 + w, 9 + h, shape, block)])
                got = M.pixelate_regions(base[None].copy(), q)[0]
                assert np.array_equal(got, pillow(base, q)), (w, h, block, shape)
                if block == 1:
                    assert np.array_equal(got, base)
    a, b = (0, 5, 5, 35, 30, lib.BLUR_BOX, 4), (0, 20, 15, 55, 45, lib.BLUR_ELLIPSE, 6)
    one, other = regions([a, b]), regions([b, a])
    got = [M.pixelate_regions(base[None].copy(), q)[0] for q in (one, other)]
    assert np.array_equal(got[0], pillow(base, one)) and np.array_equal(got[1], pillow(base, other))
    assert not np.array_equal(got[0], got[1])


def test_pack_crops_follows_pack_blur():
    rng = np.random.default_rng(9)
    faces = []
    for f in range(4):
        b = []
        for _ in range(int(rng.integers(0, 6))):
            x0, y0 = rng.uniform(-40, 90), rng.uniform(-40, 70)
            b.append({'bbox': np.array([x0, y0, x0 + rng.uniform(0.2, 60), y0 + rng.uniform(0.2, 50)], np.float32)})
        faces.append(b)
    faces[1].insert(1, {'bbox': [-90, -90, -40, -40]})   # clips to nothing, under every margin
    faces[2] = {'bbox': [3.9, 4.9, 20.1, 30.99]}         # a single dict
    for margin in (0.0, 0.15, -0.2):
        blur = vis.pack_blur(faces, (60, 80), margin=margin)
        crops, index = vis.pack_crops(faces, (60, 80), margin=margin)
        pix = vis.pack_pixelate(faces, (60, 80), margin=margin, shape='ellipse')
        assert len(crops) == len(blur) == len(index) == len(pix) and index.dtype == np.int32 and index.shape[1] == 2
        for name in ('frame', 'x0', 'y0', 'x1', 'y1'):
            assert np.array_equal(crops[name], blur[name]) and np.array_equal(pix[name], blur[name])
        assert np.array_equal(index[:, 0], blur['frame'])
        w, h = blur['x1'] - blur['x0'], blur['y1'] - blur['y0']
        assert np.array_equal(pix['block'], np.maximum(1, np.maximum(w, h) // 8)) and (pix['shape'] == lib.BLUR_ELLIPSE).all()
        assert sorted(map(tuple, index.tolist())) == list(map(tuple, index.tolist()))      # frame, then list order
        assert (1, 1) not in set(map(tuple, index.tolist()))
    crops, index = vis.pack_crops([[{'bbox': [1.5, 2.5, 30.7, 20.2]}, {'bbox': [-9, -9, -1, -1]}, {'bbox': [10, 10, 99, 99]}]], (40, 50))
    assert crops.tolist() == [(0, 1.0, 2.0, 30.0, 20.0), (0, 10.0, 10.0, 50.0, 40.0)] and index.tolist() == [[0, 0], [0, 2]]
    crops, index = vis.pack_crops([[], []], (40, 50))
    assert len(crops) == 0 and index.shape == (0, 2)


def test_argument_checks_raise_before_anything_runs():
    faces = [[{'bbox': [1, 1, 30, 30]}]]

    class Batch:                                         # stands for a lib.Frames: the checks come before any use of it
        shape = (1, 40, 50, 3)

        def __len__(self):
            return 1

        def __getattr__(self, name):
            raise AssertionError('the batch was touched: %s' % name)
    for kw in (dict(method='pixelate', radius=2.0), dict(method='mosaic'), dict(method='pixelate', block=0),
               dict(method='pixelate', block=16385), dict(method='pixelate', block=2.5), dict(method='gaussian', block=4),
               dict(method='pixelate', shape='disc'), dict(method='pixelate', margin=float('nan'))):
        with pytest.raises(ValueError):
            vis.blur_faces(Batch(), faces, **kw)
        with pytest.raises(ValueError):
            vis.anonymize_faces(np.zeros((40, 50, 3), np.uint8), faces[0], **kw)
    for kw in (dict(size=(0, 5)), dict(size=(5, 16385)), dict(size=7), dict(resample='cubic'), dict(resample=6), dict(resample=True)):
        with pytest.raises(ValueError):
            vis.crop_faces(Batch(), faces, **kw)
    with pytest.raises(ValueError):
        vis.crop_faces(Batch(), [[], []])
    with pytest.raises(ValueError):
        image.resize_frames([], (4, 4))
    with pytest.raises(ValueError):
        image.resize_frames(np.zeros((1, 4, 4, 3), np.uint8), (4, 4))
    assert [lib.resample_filter(n) for n in ('nearest', 'LANCZOS', 'bilinear', 'bicubic', 'box', 'hamming')] == [0, 1, 2, 3, 4, 5]
    assert [lib.resample_filter(c) for c in range(6)] == list(range(6))


def test_invalid_arguments_return_e_invalid():
    L = lib.load()
    k = C.c_int()
    b, c = np.zeros(2 * 8, np.int32), np.zeros(8 * 64, np.int32)

    def plan(in_size, b0, b1, out_size, filt, bounds=b, coefs=c, capacity=c.size, ksize=k):
        return L.ta_resample_plan(in_size, b0, b1, out_size, filt, lib.ptr(bounds), lib.ptr(coefs), capacity,
                                  C.byref(ksize) if ksize is not None else None)
    assert plan(10, 0, 10, 8, lib.BICUBIC) == lib.OK and k.value == 7
    for bad in [(0, 0, 1, 8, 3), (10, -0.5, 10, 8, 3), (10, 0, 10.5, 8, 3), (10, 4, 4, 8, 3), (10, 5, 4, 8, 3),
                (10, 0, 10, 0, 3), (10, 0, 10, -1, 3), (10, 0, 10, 16385, 3), (10, 0, 10, 8, 6), (10, 0, 10, 8, -1),
                (10, float('nan'), 10, 8, 3), (10, 0, float('nan'), 8, 3)]:
        assert plan(*bad) == lib.E_INVALID, bad
    assert plan(10, 0, 10, 8, 3, ksize=None) == lib.E_INVALID
    assert plan(10, 0, 10, 8, 3, bounds=None) == lib.E_INVALID
    assert plan(10, 0, 10, 8, 3, capacity=8 * 7 - 1) == lib.E_CAPACITY and k.value == 7
    assert plan(1080, 0, 1080, 8, lib.LANCZOS, capacity=0) == lib.E_CAPACITY and k.value == 2 * 405 + 1
    with pytest.raises(lib.TerranAmdError) as e:
        lib.resample_plan(10, 0, 11, 8, lib.BOX)
    assert e.value.code == lib.E_INVALID
    # the two device entries refuse a null context before they look at anything else
    assert L.ta_frames_resample(None, None, None, 0, 4, 4, 3, None) == lib.E_INVALID
    assert L.ta_frames_pixelate(None, None, None, 0) == lib.E_INVALID
