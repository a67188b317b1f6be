"""-m gpu: encode_jpeg(..., optimize=True) / ta_jpeg_encode_opt against the files Pillow writes with optimize=True
(tests/golden/jpeg_encode_optimize.npz and the live Pillow), byte for byte: every fixture alone, a same-size batch whose
images need very different tables, a mixed-size list, 2 x 1080p, repeatability, the unchanged standard path, a decode
round trip and the Motion-JPEG writer."""
import io

import numpy as np
import pytest

from terran_amd import image, lib, runtime, synth
from terran_amd.video import JpegVideoWriter
from tests import jpeg_encode_optimize_model as O
from tests.test_jpeg_encode_cpu import golden as standard_golden
from tests.test_jpeg_encode_optimize_cpu import golden

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def fx():
    return golden()


def _pillow(px, q, s, optimize=True):
    Image = pytest.importorskip('PIL.Image')
    f = io.BytesIO()
    Image.fromarray(px).save(f, 'JPEG', quality=q, subsampling=s, optimize=optimize)
    return f.getvalue()


def test_every_fixture_alone(fx):
    ctx = runtime.get_context(0)
    for name, f in fx.items():
        files = image.encode_jpeg(f['px'], f['quality'], f['subsampling'], ctx=ctx, optimize=True)
        assert len(files) == 1
        assert files[0] == f['jpg'], '%s: %d bytes, Pillow %d' % (name, len(files[0]), len(f['jpg']))


def test_every_fixture_alone_equals_live_pillow(fx):
    pytest.importorskip('PIL.Image')
    ctx = runtime.get_context(0)
    for name, f in fx.items():
        q, s = image.jpeg_options(f['quality'], f['subsampling'])
        assert image.encode_jpeg(f['px'], q, s, ctx=ctx, optimize=True) == [_pillow(f['px'], q, s)], name


def test_same_size_batch_gets_a_table_set_per_image(fx):
    """flat, gradient and noise in one call: coding every image with image 0's tables (or writing image 0's header
    before every stream) cannot give these files."""
    names = [n for n in fx if n.startswith('batch_')]
    assert len(names) == 3
    q, s = fx[names[0]]['quality'], fx[names[0]]['subsampling']
    assert all((fx[n]['quality'], fx[n]['subsampling']) == (q, s) for n in names)
    assert len({tuple(map(tuple, O.parse_dht(fx[n]['jpg'])[1][1:])) for n in names}) == 3     # three different AC 0 tables
    assert len({O.parse_dht(fx[n]['jpg'])[1][0] for n in names}) == 1
    ctx = runtime.get_context(0)
    for order in (names, names[::-1], names[1:] + names[:1]):
        frames = ctx.upload(np.stack([fx[n]['px'] for n in order]))
        try:
            files = frames.encode_jpeg(q, s, optimize=True)
        finally:
            frames.free()
        assert files == [fx[n]['jpg'] for n in order], order
    assert len({len(fx[n]['jpg'].split(b'\xff\xda')[0]) for n in names}) == 3                # header lengths differ


def test_list_of_mixed_size_batches(fx):
    names = [n for n in fx if n.startswith('rw-1')] + ['noise_24x40_s0_q100', 'flat_1x1_s2_q75', 'noise_17x9_s-1_q75']
    ctx = runtime.get_context(0)
    frames = [ctx.upload(fx[n]['px'][None]) for n in names]
    try:
        files = image.encode_jpeg(frames, 80, '4:2:2', optimize=True)
    finally:
        for f in frames:
            f.free()
    for n, got in zip(names, files):
        assert got == O.encode(fx[n]['px'], 80, 1), n


def test_two_1080p_frames_equal_pillow_and_repeat():
    pytest.importorskip('PIL.Image')
    ctx = runtime.get_context(0)
    px = synth.frames(11, 2, 1080, 1920)
    px[1, 200:600, 300:1500] = np.random.default_rng(3).integers(0, 256, (400, 1200, 3), dtype=np.uint8)
    batch = ctx.upload(px)
    try:
        files = batch.encode_jpeg(90, 2, optimize=True)
        ms, counts = ctx.jpeg_encode_stats()
        assert counts['images'] == 2 and counts['bytes'] == sum(len(f) for f in files)
        assert ms['tables'] > 0
        standard = batch.encode_jpeg(90, 2)
        assert ctx.jpeg_encode_stats()[0]['tables'] == 0
        again = batch.encode_jpeg(90, 2, optimize=True)
    finally:
        batch.free()
    for i in range(2):
        assert files[i] == _pillow(px[i], 90, 2), i
        assert standard[i] == _pillow(px[i], 90, 2, optimize=False), i
        assert len(files[i]) < len(standard[i])
    assert again == files


def test_repeated_calls_are_identical():
    ctx = runtime.get_context(0)
    px = np.random.default_rng(8).integers(0, 256, (4, 131, 257, 3), dtype=np.uint8)
    px[:, 40:90] = 255
    px[2] = 17                                                # a flat frame between noisy ones
    batch = ctx.upload(px)
    try:
        first = batch.encode_jpeg(97, 2, optimize=True)
        small = ctx.upload(px[:1, :9, :17])
        try:
            small.encode_jpeg(10, 0, optimize=True)           # a different layout in between
            batch.encode_jpeg(97, 2)                          # and the standard tables
        finally:
            small.free()
        for _ in range(3):
            assert batch.encode_jpeg(97, 2, optimize=True) == first
    finally:
        batch.free()
    assert first == [O.encode(px[i], 97, 2) for i in range(4)]


def test_standard_path_is_unchanged():
    """optimize=False (keyword, default and the ABI entry with optimize = 0): the bytes of jpeg_encode.npz."""
    import ctypes as C
    ctx = runtime.get_context(0)
    for name, f in standard_golden().items():
        q, s = image.jpeg_options(f['quality'], f['subsampling'])
        assert image.encode_jpeg(f['px'], q, s, ctx=ctx, optimize=False) == [f['jpg']], name
        assert image.encode_jpeg(f['px'], q, s, ctx=ctx) == [f['jpg']], name
        frames = ctx.upload(f['px'][None])
        try:
            out, size = C.c_void_p(), (C.c_size_t * 1)()
            ctx.check(ctx.lib.ta_jpeg_encode_opt(ctx.h, frames.h, q, s, 0, C.byref(out), size))
            assert C.string_at(out.value, size[0]) == f['jpg'], name
        finally:
            frames.free()


def test_bad_optimize_fails_before_a_launch():
    import ctypes as C
    ctx = runtime.get_context(0)
    batch = ctx.upload(np.zeros((1, 8, 8, 3), np.uint8))
    try:
        for bad in (1, 'yes', None):
            with pytest.raises(ValueError):
                batch.encode_jpeg(75, 2, optimize=bad)
        out, size = C.c_void_p(), (C.c_size_t * 1)()
        assert ctx.lib.ta_jpeg_encode_opt(ctx.h, batch.h, 75, 2, 2, C.byref(out), size) == lib.E_INVALID
    finally:
        batch.free()


def test_round_trip_through_the_decoder(fx):
    Image = pytest.importorskip('PIL.Image')
    px = synth.frames(5, 3, 120, 176)
    ctx = runtime.get_context(0)
    batch = ctx.upload(px)
    try:
        files = batch.encode_jpeg(85, 2, optimize=True)
    finally:
        batch.free()
    decoded = image.decode_jpeg(files)
    try:
        got = decoded.download()
        assert (decoded.decode_paths == lib.JPEG_DEVICE).all()
    finally:
        decoded.free()
    for i in range(3):
        assert np.array_equal(got[i], np.asarray(Image.open(io.BytesIO(files[i])).convert('RGB'))), i
    deep = next(n for n in fx if n.startswith('deep'))             # 16-bit codes through the library's own decoder
    decoded = image.decode_jpeg([fx[deep]['jpg']])
    try:
        assert (decoded.decode_paths == lib.JPEG_DEVICE).all()
        assert np.array_equal(decoded.download()[0], np.asarray(Image.open(io.BytesIO(fx[deep]['jpg'])).convert('RGB')))
    finally:
        decoded.free()


def test_video_writer_stream_is_the_concatenation_of_the_files():
    px = synth.frames(9, 5, 64, 96)
    px[3] = 200                                               # a flat frame: its header is shorter
    ctx = runtime.get_context(0)
    batch = ctx.upload(px)
    out = io.BytesIO()
    try:
        expect = batch.encode_jpeg(90, 2, optimize=True)
        with JpegVideoWriter(out, quality=90, optimize=True) as w:
            w.write_frames(batch)
            w.write_frame(lambda a: a, px[0])
    finally:
        batch.free()
    assert out.getvalue() == b''.join(expect + [expect[0]])
    assert expect == [O.encode(px[i], 90, 2) for i in range(5)]
    assert len({len(e.split(b'\xff\xda')[0]) for e in expect}) > 1
