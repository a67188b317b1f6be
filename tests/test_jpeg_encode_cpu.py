"""JPEG encode, host side (no GPU): tests/jpeg_encode_model.py (the numpy restatement of the device passes) against the
Pillow files recorded in tests/golden/jpeg_encode.npz and -- where Pillow is importable -- a few hundred seeded random
encodes; its quantisation against libjpeg-turbo's reciprocal form; ta_jpeg_encode_header; the model's coefficients
against what the library's entropy decoder reads from Pillow's files; option checking; and JpegVideoWriter with an
injected encoder."""
import io
import os
import threading

import numpy as np
import pytest

from tests import jpeg_encode_model as M

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(REPO, 'tests', 'golden')


def golden():
    g = np.load(os.path.join(GOLDEN, 'jpeg_encode.npz'))
    out = {}
    for name in g['names']:
        name = str(name)
        q, s = (int(x) for x in g['opt_' + name])
        out[name] = dict(px=g['px_' + name], quality=q, subsampling=s, jpg=g['jpg_' + name].tobytes())
    return out


@pytest.fixture(scope='module')
def fx():
    return golden()


@pytest.fixture(scope='module')
def built():
    from terran_amd import build
    build.build()


def _code(s):
    return 2 if s == -1 else s


def test_golden_covers_the_contract(fx):
    shapes = {f['px'].shape[:2] for f in fx.values()}
    for hw in [(1, 1), (7, 5), (8, 8), (9, 17), (16, 16), (17, 9), (33, 250), (250, 33)]:
        assert hw in shapes
    assert {f['quality'] for f in fx.values()} >= {1, 5, 30, 50, 75, 90, 100}
    assert {f['subsampling'] for f in fx.values()} >= {0, 1, 2, -1}
    assert any(n.startswith('rw-1') for n in fx) and any(n.startswith('rw-2') for n in fx)
    assert any(n.startswith('saturated') for n in fx)


def test_model_equals_golden_bytes(fx):
    for name, f in fx.items():
        got = M.encode(f['px'], f['quality'], _code(f['subsampling']))
        assert got == f['jpg'], name


def test_reciprocal_quantisation_is_the_rounded_division():
    x = np.arange(-32767, 32768, dtype=np.int64)
    for q in range(1, 256):
        assert np.array_equal(M.quant_reciprocal(x, q), M.quantise(x, q)), q


def _random_image(rng, kind, h, w):
    if kind == 0:
        return rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
    if kind == 1:
        y, x = np.mgrid[:h, :w]
        return np.stack([(x * 7 + y) % 256, (y * 5) % 256, ((x + y) * 3) % 256], -1).astype(np.uint8)
    if kind == 2:
        return (rng.integers(0, 2, (h, w, 3)) * 255).astype(np.uint8)
    base = rng.integers(0, 256, (max(1, h // 8), max(1, w // 8), 3), dtype=np.uint8)
    return np.repeat(np.repeat(base, 8, 0), 8, 1)[:h, :w] if h >= 8 and w >= 8 else rng.integers(0, 256, (h, w, 3),
                                                                                                   dtype=np.uint8)


def test_model_equals_live_pillow_on_random_encodes():
    Image = pytest.importorskip('PIL.Image')
    rng = np.random.default_rng(2024)
    for t in range(300):
        h, w = int(rng.integers(1, 80)), int(rng.integers(1, 80))
        q, s = int(rng.integers(1, 101)), int(rng.integers(0, 3))
        px = _random_image(rng, t % 4, h, w)
        f = io.BytesIO()
        Image.fromarray(px).save(f, 'JPEG', quality=q, subsampling=s)
        assert M.encode(px, q, s) == f.getvalue(), (t, h, w, q, s)


def test_pillow_defaults_are_q75_420():
    Image = pytest.importorskip('PIL.Image')
    px = np.random.default_rng(1).integers(0, 256, (21, 34, 3), dtype=np.uint8)
    a, b = io.BytesIO(), io.BytesIO()
    Image.fromarray(px).save(a, 'JPEG')
    Image.fromarray(px).save(b, 'JPEG', quality=75, subsampling=2)
    assert a.getvalue() == b.getvalue() == M.encode(px)


def _header_end(data):
    """Bytes up to and including the SOS segment."""
    at = 2
    while True:
        assert data[at] == 0xFF
        marker, length = data[at + 1], int.from_bytes(data[at + 2:at + 4], 'big')
        at += 2 + length
        if marker == 0xDA:
            return at


def test_header_equals_golden_prefix(built, fx):
    from terran_amd import lib
    for name, f in fx.items():
        h, w = f['px'].shape[:2]
        hd = lib.jpeg_encode_header(h, w, f['quality'], _code(f['subsampling']))
        assert hd == f['jpg'][:_header_end(f['jpg'])], name
        assert hd == M.header(h, w, f['quality'], _code(f['subsampling']))
    assert lib.jpeg_encode_header(65535, 65535, 1, 0) == M.header(65535, 65535, 1, 0)


def test_header_refuses_bad_arguments(built):
    from terran_amd import lib
    for args in [(0, 8, 75, 2), (8, 65536, 75, 2), (8, 8, 0, 2), (8, 8, 101, 2), (8, 8, 75, 3), (8, 8, 75, -1)]:
        with pytest.raises(lib.TerranAmdError):
            lib.jpeg_encode_header(*args)


def test_model_coefficients_equal_the_decoders_view_of_pillow_files(built, fx):
    """Scan order, dummy blocks and quantisation: the library's entropy decoder reads Pillow's file back into the
    coefficients the model computes (component after component, MCU grids with their dummy blocks)."""
    from terran_amd import lib
    for name, f in fx.items():
        s = _code(f['subsampling'])
        hdr, coefs = lib.jpeg_coefficients(f['jpg'])
        assert coefs is not None, name
        model = M.coefficients(f['px'], f['quality'], s)
        assert np.array_equal(coefs, model), name
        comps, _ = M.layout(*f['px'].shape[:2], s)
        assert [int(x) for x in hdr['blocks_w']] == [c[2] for c in comps], name


def test_encode_jpeg_refuses_bad_options_before_anything_runs():
    from terran_amd import image

    class Boom:
        """Not a frame batch: anything that touches it fails the test."""

        def __getattr__(self, k):
            raise AssertionError('touched before the options were checked')
    for q, s in [(0, -1), (101, -1), (75.0, -1), (True, -1), ('90', -1), (75, 3), (75, -2), (75, '4:1:1'), (75, 'keep'),
                 (75, None), (75, 2.0)]:
        with pytest.raises(ValueError):
            image.encode_jpeg(Boom(), q, s)
    for bad in [np.zeros((8, 8), np.uint8), np.zeros((8, 8, 4), np.uint8), np.zeros((8, 8, 3), np.float32),
                np.zeros((0, 8, 3), np.uint8), np.zeros((1, 70000, 1, 3), np.uint8)]:
        with pytest.raises(ValueError):
            image.encode_jpeg(bad)
    with pytest.raises(ValueError):
        image.encode_jpeg([])
    assert image.jpeg_options() == (75, 2)
    assert [image.jpeg_options(90, s)[1] for s in (-1, 0, 1, 2, '4:4:4', '4:2:2', '4:2:0')] == [2, 0, 1, 2, 0, 1, 2]


def _fake_encoder(calls):
    def enc(images, quality, subsampling):
        calls.append((len(images), quality, subsampling))
        return [b'\xff\xd8' + bytes([k]) * (k + 1) + b'\xff\xd9' for k in range(len(images))]
    return enc


def test_video_writer_frames_the_stream_in_order():
    from terran_amd.video import DEFAULT_WRITER_BUFFER_SIZE, JpegVideoWriter, VideoClosed
    assert DEFAULT_WRITER_BUFFER_SIZE == 64
    out, calls = io.BytesIO(), []
    with JpegVideoWriter(out, quality=90, subsampling='4:4:4', encoder=_fake_encoder(calls)) as w:
        w.write_frames([0, 1, 2])
        w.write_frame(lambda a, b: [a, b], 7, 8)
        w.write_frame([5])
    assert calls == [(3, 90, '4:4:4'), (2, 90, '4:4:4'), (1, 90, '4:4:4')]
    enc = _fake_encoder([])
    expect = enc([0] * 3, 90, 2) + enc([0] * 2, 90, 2) + enc([0], 90, 2)
    assert out.getvalue() == b''.join(expect) and w.frames_written == 6
    with pytest.raises(VideoClosed):
        w.write_frames([0])
    with pytest.raises(VideoClosed):
        w.write_frame([0])
    with pytest.raises(VideoClosed):
        w.close()


def test_video_writer_rejects_bad_options_at_once():
    from terran_amd.video import JpegVideoWriter
    with pytest.raises(ValueError):
        JpegVideoWriter(io.BytesIO(), quality=0)
    with pytest.raises(ValueError):
        JpegVideoWriter(io.BytesIO(), subsampling='4:1:1')


def test_video_writer_reraises_a_write_error():
    from terran_amd.video import JpegVideoWriter

    class Broken(io.RawIOBase):
        def __init__(self):
            self.failed = threading.Event()

        def write(self, b):
            self.failed.set()
            raise OSError('pipe closed')
    stream = Broken()
    w = JpegVideoWriter(stream, encoder=_fake_encoder([]))
    w.write_frames([0])
    assert stream.failed.wait(10)
    for _ in range(100):                                    # the worker records the error right after the write fails
        if w._error is not None:
            break
        threading.Event().wait(0.01)
    with pytest.raises(OSError):
        w.write_frames([0])
    w.close()


def test_video_writer_close_reraises_a_late_error():
    from terran_amd.video import JpegVideoWriter

    class Broken(io.RawIOBase):
        def write(self, b):
            raise OSError('disk full')
    w = JpegVideoWriter(Broken(), encoder=_fake_encoder([]))
    w.write_frames([0, 1])
    with pytest.raises(OSError):
        w.close()


def test_save_images_checks_paths_before_encoding(tmp_path):
    from terran_amd import image
    with pytest.raises(ValueError):
        image.save_images(np.zeros((2, 8, 8, 3), np.uint8), [str(tmp_path / 'a.jpg')])
    with pytest.raises(ValueError):
        image.save_images(np.zeros((8, 8, 3), np.uint8), [], quality=0)
    assert not list(tmp_path.iterdir())
