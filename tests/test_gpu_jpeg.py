"""-m gpu: ta_jpeg_decode / terran_amd.image against the reference's open_image pixels (tests/golden/jpeg.npz and the two
quickstart photos), bit for bit, in mixed-size and same-size batches; the fallback path; and the facades over resident
frame lists.  Reads only committed goldens: neither Pillow nor the reference is needed (the one Pillow test skips
without it)."""
import numpy as np
import pytest

from terran_amd import Detection, Estimation, Recognition, image, lib, runtime, synth
from tests import jpeg_model
from tests.test_jpeg_cpu import assert_matches, golden

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def fx():
    return golden()


def _device_names(fx):
    return [n for n, f in fx.items() if f['path'] == lib.JPEG_DEVICE]


def test_each_fixture_alone(fx):
    ctx = runtime.get_context(0)
    for name in _device_names(fx):
        outs, paths = ctx.jpeg_decode([fx[name]['data']])
        assert len(outs) == 1 and list(paths) == [0], name
        try:
            assert_matches(outs[0].download()[0], fx[name], name)
        finally:
            outs[0].free()


def test_mixed_sizes_in_one_call(fx):
    """Every supported fixture (the photos included) in ONE call on 16 threads: one single-image batch per image."""
    names = _device_names(fx)
    frames = image.decode_jpeg([fx[n]['data'] for n in names], threads=16)
    assert isinstance(frames, list) and len(frames) == len(names)
    ctx = runtime.get_context(0)
    assert ctx.jpeg_stats()[1]['images'] == len(names)
    for f, name in zip(frames, names):
        assert f.shape[0] == 1 and list(f.decode_paths) == [0]
        assert_matches(f.download()[0], fx[name], name)
        f.free()


def test_same_size_batch_is_one_frames(fx):
    names = [n for n in _device_names(fx) if n.endswith('97x203')]
    assert len(names) >= 8
    order = names + names[::-1]                                  # 2x each, reversed: images land in their own slots
    for threads in (1, 0):
        batch = image.decode_jpeg([fx[n]['data'] for n in order], threads=threads)
        assert isinstance(batch, lib.Frames) and batch.shape == (len(order), 97, 203, 3)
        got = batch.download()
        batch.free()
        for img, name in zip(got, order):
            assert_matches(img, fx[name], name)


def test_fallback_images_are_flagged_and_left_zero(fx):
    """The library decodes what it can; a progressive / CMYK image is reported and left zero (no Pillow involved)."""
    ctx = runtime.get_context(0)
    data = [fx['progressive_40x56']['data'], fx['s440_q90_48x48']['data'], fx['cmyk_40x56']['data']]
    outs, paths = ctx.jpeg_decode(data)
    assert list(paths) == [1, 0, 4] and len(outs) == 3
    got = [o.download()[0] for o in outs]
    for o in outs:
        o.free()
    assert not got[0].any() and not got[2].any()
    assert_matches(got[1], fx['s440_q90_48x48'], 's440_q90_48x48')
    # same size: one batch, the device image in its slot
    outs, paths = ctx.jpeg_decode([fx['progressive_40x56']['data'], fx['progressive_40x56']['data']])
    assert list(paths) == [1, 1] and outs[0].shape == (2, 40, 56, 3) and not outs[0].download().any()
    outs[0].free()


def test_fallback_through_open_images_gives_the_reference_pixels(fx):
    pytest.importorskip('PIL')
    names = ['progressive_40x56', 'cmyk_40x56', 's420_q75_17x33']
    frames = image.open_images([fx[n]['data'] for n in names])
    assert [int(f.decode_paths[0]) for f in frames] == [1, 4, 0]
    for f, n in zip(frames, names):
        assert_matches(f.download()[0], fx[n], n)
        f.free()
    batch = image.open_images([fx['progressive_40x56']['data'], fx['cmyk_40x56']['data']])
    assert list(batch.decode_paths) == [1, 4]
    got = batch.download()
    assert_matches(got[0], fx['progressive_40x56'], 'p')
    assert_matches(got[1], fx['cmyk_40x56'], 'c')


def test_invalid_data_is_refused_before_any_launch(fx):
    ctx = runtime.get_context(0)
    data = fx['s420_q75_97x203']['data']
    for bad in (b'not a jpeg', data[:len(data) // 2], b'\xff\xd8\xff\xd9'):
        with pytest.raises(lib.TerranAmdError) as e:
            ctx.jpeg_decode([data, bad])
        assert e.value.code == lib.E_INVALID and 'image 1' in str(e.value)
    outs, _ = ctx.jpeg_decode([data])                            # the context is still usable
    assert_matches(outs[0].download()[0], fx['s420_q75_97x203'], 'after')
    outs[0].free()


def _with_quant(data, values, precision):
    """`data` with every DQT table replaced by `values` (64, natural order is irrelevant: all tables get the same list)
    at 8-bit (precision 0) or 16-bit (1) precision."""
    d = bytearray(data)
    out, i = bytearray(), 0
    while True:
        j = d.find(b'\xff\xdb', i)
        if j < 0 or j > d.index(b'\xff\xda'):
            break
        seg_end = j + 2 + ((d[j + 2] << 8) | d[j + 3])
        ids, t = [], j + 4
        while t < seg_end:
            ids.append(d[t] & 15)
            t += 1 + (128 if d[t] >> 4 else 64)
        body = b''.join(bytes([precision << 4 | tq]) + b''.join(int(v).to_bytes(1 + precision, 'big') for v in values)
                        for tq in ids)
        out += d[i:j] + b'\xff\xdb' + (2 + len(body)).to_bytes(2, 'big') + body
        i = seg_end
    return bytes(out + d[i:])


def test_extreme_coefficients_equal_the_c_arithmetic(fx):
    """Quantisers no encoder of 8-bit images writes (255 on a quality-100 stream; 16-bit 65535 = -1 and 40000 as libjpeg's
    16-bit multipliers) push the IDCT past 32 bits: the device takes the 64-bit path and equals tests/jpeg_model.py (the
    C code's integer widths) bit for bit, in one call with an ordinary image."""
    ctx = runtime.get_context(0)
    base = fx['s444_q100_97x203']['data']
    crafted = [_with_quant(base, [255] * 64, 0), _with_quant(base, [65535, 40000] * 32, 1),
               _with_quant(fx['gray_q90_61x77']['data'], [65535] * 32 + [32767] * 32, 1)]
    for data in crafted:
        hdr, coefs = lib.jpeg_coefficients(data)
        want = jpeg_model.decode(hdr, coefs)
        outs, paths = ctx.jpeg_decode([fx['s420_q75_17x33']['data'], data])
        assert list(paths) == [0, 0]
        got = outs[1].download()[0]
        assert_matches(outs[0].download()[0], fx['s420_q75_17x33'], 's420_q75_17x33')
        for o in outs:
            o.free()
        assert np.array_equal(got, want), int((got != want).any(-1).sum())


def test_every_malformed_image_is_marked(fx):
    ctx = runtime.get_context(0)
    good = fx['s420_q75_17x33']['data']
    rst = bytearray(fx['rst_blocks5_s420_97x203']['data'])
    rst[rst.index(b'\xff\xd1') + 1] = 0xD3                        # restart markers out of sequence (libjpeg: a warning)
    with pytest.raises(lib.TerranAmdError) as e:
        ctx.jpeg_decode([good, b'\xff\xd8\xff\xd9', good, bytes(rst)])
    assert e.value.code == lib.E_INVALID and list(e.value.paths) == [0, lib.JPEG_INVALID, 0, lib.JPEG_INVALID]


def test_open_images_hands_refused_jpegs_to_pillow(fx):
    """What open_image accepts, open_images accepts: a file libjpeg decodes with a warning goes through Pillow, the rest of
    the batch through the library; a truncated file raises as open_image does."""
    PIL = pytest.importorskip('PIL.Image')
    import io
    rst = bytearray(fx['rst_blocks5_s420_97x203']['data'])
    rst[rst.index(b'\xff\xd1') + 1] = 0xD3
    want = np.asarray(PIL.open(io.BytesIO(bytes(rst))).convert('RGB'))
    names = ['s420_q75_97x203', 's444_q75_97x203']
    batch = image.open_images([fx[names[0]]['data'], bytes(rst), fx[names[1]]['data']])
    assert isinstance(batch, lib.Frames) and list(batch.decode_paths) == [0, lib.JPEG_INVALID, 0]
    got = batch.download()
    batch.free()
    assert_matches(got[0], fx[names[0]], names[0])
    assert np.array_equal(got[1], want)
    assert_matches(got[2], fx[names[1]], names[1])
    data = fx['s420_q75_97x203']['data']
    with pytest.raises(OSError):
        image.open_images([fx['s420_q75_17x33']['data'], data[:len(data) // 2]])


def _photo_list(fx):
    names = ['rw-1', 'rw-2', 's420_q75_97x203', 'gray_q90_61x77']
    frames = image.decode_jpeg([fx[n]['data'] for n in names])
    hosts = [f.download()[0] for f in frames]
    for h, n in zip(hosts, names):
        assert_matches(h, fx[n], n)                              # = the reference's open_image of that file
    return frames, hosts


def _same_faces(a, b):
    assert len(a) == len(b)
    for fa, fb in zip(a, b):
        assert len(fa) == len(fb)
        for x, y in zip(fa, fb):
            assert np.array_equal(x['bbox'], y['bbox']) and np.array_equal(x['landmarks'], y['landmarks'])
            assert x['score'] == y['score']


def test_detection_over_resident_list_equals_ndarray_list(fx, states):
    frames, hosts = _photo_list(fx)
    det = Detection(short_side=96, device=0, state=states('retinaface'))
    _same_faces(det(frames), det(hosts))
    assert sum(len(f) for f in det(hosts)) > 0
    with pytest.raises(ValueError):
        det([frames[0], hosts[1]])


def test_estimation_over_resident_list_equals_ndarray_list(fx, states):
    frames, hosts = _photo_list(fx)
    est = Estimation(short_side=96, device=0, state=states('openpose_decoder'))
    a, b = est(frames), est(hosts)
    assert len(a) == len(b) == len(hosts)
    for pa, pb in zip(a, b):
        assert len(pa) == len(pb)
        for x, y in zip(pa, pb):
            assert np.array_equal(x['keypoints'], y['keypoints']) and x['score'] == y['score']
    for f in frames:                                             # the caller's frames stay usable
        assert f.h is not None and f.download().shape == f.shape


def test_recognition_over_resident_list_equals_ndarray_list(fx, states):
    frames, hosts = _photo_list(fx)
    rec = Recognition(device=0, state=states('arcface'))
    faces = [[{'landmarks': l} for l in synth.landmarks(40 + i, 2 if i != 2 else 0, h.shape[0], h.shape[1])]
             for i, h in enumerate(hosts)]
    a, b = rec(frames, faces), rec(hosts, faces)
    assert len(a) == len(b) == len(hosts)
    for x, y in zip(a, b):
        assert x.dtype == y.dtype and np.array_equal(x, y)
    a, b = rec(frames), rec(hosts)                               # no landmarks: bicubic resize + centre pad
    assert np.array_equal(a, b)


def test_device_list_fanout_rejects_resident_lists(fx, states):
    frames, _ = _photo_list(fx)
    det = Detection(short_side=96, device=[0, 0], state=states('retinaface'))
    with pytest.raises(ValueError, match='resident'):
        det(frames)
