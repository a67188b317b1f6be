"""Raw YUV video without a GPU: the numpy model against the definition in Fractions, the shipped arithmetic
(ta_yuv_convert_samples) against the model on every triple, frame sizes, argument checks, and the reader's and writer's
framing through their test hooks."""
import io
import itertools
import threading
from fractions import Fraction as F
from math import floor

import numpy as np
import pytest

from terran_amd import image, lib, video
from tests import yuv_model

COMBOS = [(m, r) for m in ('bt601', 'bt709') for r in ('tv', 'pc')]
EDGES = (0, 1, 15, 16, 17, 127, 128, 129, 234, 235, 236, 239, 240, 241, 254, 255)
K = {'bt601': (F(299, 1000), F(114, 1000)), 'bt709': (F(2126, 10000), F(722, 10000))}


def _clip(v):
    return min(max(floor(v + F(1, 2)), 0), 255)


def _rgb_by_definition(y, cb, cr, matrix, range):
    kr, kb = K[matrix]
    kg = 1 - kr - kb
    if range == 'tv':
        yn, bn, rn = F(y - 16, 219), F(cb - 128, 224), F(cr - 128, 224)
    else:
        yn, bn, rn = F(y, 255), F(cb - 128, 255), F(cr - 128, 255)
    r = yn + 2 * (1 - kr) * rn
    b = yn + 2 * (1 - kb) * bn
    g = yn - (2 * kr * (1 - kr) / kg) * rn - (2 * kb * (1 - kb) / kg) * bn
    return [_clip(255 * v) for v in (r, g, b)]


def _yuv_by_definition(r, g, b, matrix, range):
    kr, kb = K[matrix]
    kg = 1 - kr - kb
    lum = kr * r + kg * g + kb * b
    if range == 'tv':
        v = (16 + 219 * lum / 255, 128 + 224 * (b - lum) / (255 * 2 * (1 - kb)), 128 + 224 * (r - lum) / (255 * 2 * (1 - kr)))
    else:
        v = (lum, 128 + (b - lum) / (2 * (1 - kb)), 128 + (r - lum) / (2 * (1 - kr)))
    return [_clip(x) for x in v]


def _triples():
    edge = np.array(list(itertools.product(EDGES, repeat=3)), np.uint8)
    return np.concatenate([edge, np.random.default_rng(20).integers(0, 256, (10000, 3), dtype=np.uint8)])


@pytest.mark.parametrize('matrix,range', COMBOS)
def test_model_equals_the_definition_in_fractions(matrix, range):
    t = _triples()
    got_rgb = yuv_model.yuv_to_rgb(t[:, 0], t[:, 1], t[:, 2], matrix, range)
    got_yuv = yuv_model.rgb_to_yuv(t[:, 0], t[:, 1], t[:, 2], matrix, range)
    ints = t.astype(int).tolist()
    assert got_rgb.tolist() == [_rgb_by_definition(a, b, c, matrix, range) for a, b, c in ints]
    assert got_yuv.tolist() == [_yuv_by_definition(a, b, c, matrix, range) for a, b, c in ints]


def test_model_block_mean_is_rounded_once():
    """Cb, Cr of the sums of k pixels = the definition applied to the exact mean."""
    rng = np.random.default_rng(21)
    for k in (1, 2, 4):
        sums = rng.integers(0, 255 * k + 1, (300, 3))
        got = yuv_model.rgb_to_yuv(sums[:, 0], sums[:, 1], sums[:, 2], 'bt709', 'tv', k=np.full(300, k))
        want = [_yuv_by_definition(F(int(a), k), F(int(b), k), F(int(c), k), 'bt709', 'tv') for a, b, c in sums]
        assert got.tolist() == want


@pytest.fixture(scope='module')
def all_triples():
    g = np.arange(256, dtype=np.uint8)
    return np.stack(np.meshgrid(g, g, g, indexing='ij'), -1).reshape(-1, 3)


@pytest.mark.parametrize('matrix,range', COMBOS)
def test_shipped_arithmetic_is_exact_on_all_triples(all_triples, matrix, range):
    """ta_yuv_convert_samples runs yuv_math.h, the kernels' own code, on the host: all 2^24 triples, both directions."""
    t = all_triples
    spec = image.yuv_spec('yuv444p', matrix, range)
    got = lib.yuv_convert_samples(spec, 0, t)
    want = yuv_model.yuv_to_rgb(t[:, 0], t[:, 1], t[:, 2], matrix, range)
    assert np.array_equal(got, want), int((got != want).any(1).sum())
    got = lib.yuv_convert_samples(spec, 1, t)
    want = yuv_model.rgb_to_yuv(t[:, 0], t[:, 1], t[:, 2], matrix, range)
    assert np.array_equal(got, want), int((got != want).any(1).sum())


@pytest.mark.parametrize('matrix', ('bt601', 'bt709'))
def test_grey_axis(matrix):
    y = np.arange(256)
    mid = np.full(256, 128)
    tv = yuv_model.yuv_to_rgb(y, mid, mid, matrix, 'tv')
    assert tv[16].tolist() == [0, 0, 0] and tv[235].tolist() == [255, 255, 255]
    assert (tv[:16] == 0).all() and (tv[235:] == 255).all()
    pc = yuv_model.yuv_to_rgb(y, mid, mid, matrix, 'pc')
    assert np.array_equal(pc, np.repeat(y[:, None], 3, 1))
    for range in ('tv', 'pc'):
        got = lib.yuv_convert_samples(image.yuv_spec('yuv420p', matrix, range), 0, np.stack([y, mid, mid], -1).astype(np.uint8))
        assert np.array_equal(got, tv if range == 'tv' else pc)


@pytest.mark.parametrize('w,h', [(1, 1), (2, 2), (3, 3), (5, 4), (1920, 1080)])
def test_frame_bytes_agree(w, h):
    ch, cw = (h + 1) >> 1, (w + 1) >> 1
    for fmt, want in (('yuv420p', w * h + 2 * cw * ch), ('nv12', w * h + 2 * cw * ch), ('yuv444p', 3 * w * h)):
        assert lib.yuv_frame_bytes(lib.YUV_FORMATS[fmt], h, w) == want
        assert image.yuv_frame_bytes(fmt, (w, h)) == want
        assert video.raw_frame_bytes(fmt, w, h) == want
        assert yuv_model.frame_bytes(fmt, h, w) == want
        planes = [np.zeros((h, w), np.uint8)] + [np.zeros((h, w) if fmt == 'yuv444p' else (ch, cw), np.uint8)] * 2
        assert yuv_model.join_planes(fmt, *planes).size == want


def test_model_layout_round_trip():
    rng = np.random.default_rng(22)
    for fmt in yuv_model.FORMATS:
        frame = rng.integers(0, 256, yuv_model.frame_bytes(fmt, 3, 5), dtype=np.uint8)
        assert np.array_equal(yuv_model.join_planes(fmt, *yuv_model.split_planes(fmt, frame, 3, 5)), frame)
    y, u, v = yuv_model.split_planes('nv12', np.arange(27, dtype=np.uint8), 3, 5)
    assert u[0].tolist() == [15, 17, 19] and v[1].tolist() == [22, 24, 26]


def test_frame_bytes_reject_bad_arguments():
    assert lib.yuv_frame_bytes(3, 4, 4) == 0 and lib.yuv_frame_bytes(-1, 4, 4) == 0
    for h, w in ((0, 4), (4, 0), (-1, 4), (4, -2), (65536, 4)):
        assert lib.yuv_frame_bytes(lib.YUV_420P, h, w) == 0
    with pytest.raises(ValueError, match='pix_fmt'):
        image.yuv_frame_bytes('yuv422p', (4, 4))
    for size in ((0, 4), (4, -1), (4,), 'ab', None):
        with pytest.raises(ValueError, match='size'):
            image.yuv_frame_bytes('yuv420p', size)


def test_convert_samples_rejects_bad_specs():
    t = np.zeros((1, 3), np.uint8)
    for field in np.arange(5):
        for bad in (-1, 2 if field else 3):
            spec = [0, 0, 0, 0, 0]
            spec[field] = bad
            with pytest.raises(lib.TerranAmdError) as e:
                lib.yuv_convert_samples(spec, 0, t)
            assert e.value.code == lib.E_INVALID


def test_yuv_spec_rejects_every_bad_argument_by_name():
    good = dict(pix_fmt='yuv420p', matrix='bt709', range='tv', chroma='bilinear', siting='left')
    spec = image.yuv_spec(**good)
    assert spec.dtype == lib.YUV_SPEC_DT and spec.tolist() == (0, 1, 0, 1, 0)
    assert image.yuv_spec('nv12', 'bt601', 'pc', 'nearest', 'center').tolist() == (1, 0, 1, 0, 1)
    for name in good:
        for bad in ('rgb24', 'BT709', 0, None):
            with pytest.raises(ValueError, match=name):
                image.yuv_spec(**dict(good, **{name: bad}))
    with pytest.raises(ValueError, match='pix_fmt'):
        video.RawVideoReader(io.BytesIO(b''), 4, 4, pix_fmt='yuv422p', upload=lambda a: a)
    with pytest.raises(ValueError, match='matrix'):
        video.RawVideoReader(io.BytesIO(b''), 4, 4, pix_fmt='nv12', matrix='bt2020', upload=lambda a: a)
    with pytest.raises(ValueError, match='size'):                   # in __init__, not later in the worker
        video.RawVideoReader(io.BytesIO(b''), 65536, 4, pix_fmt='yuv420p', upload=lambda a: a)
    with pytest.raises(ValueError, match='pix_fmt'):
        video.RawVideoWriter(io.BytesIO(), pix_fmt='yuv422p', download=lambda a: a)
    with pytest.raises(ValueError, match='range'):
        video.RawVideoWriter(io.BytesIO(), range='full', download=lambda a: a)


def test_reader_frames_a_yuv420p_stream():
    w, h, per = 5, 3, 27
    assert video.raw_frame_bytes('yuv420p', w, h) == per
    data = np.random.default_rng(23).integers(0, 256, 10 * per + 3, dtype=np.uint8).tobytes()
    got = []

    def upload(raw):
        assert raw.dtype == np.uint8 and raw.ndim == 2 and raw.shape[1] == per
        return raw.copy()

    reader = video.RawVideoReader(io.BytesIO(data), w, h, batch_size=4, upload=upload, pix_fmt='yuv420p')
    for batch in reader:
        got.append(batch)
    assert [len(b) for b in got] == [4, 4, 2]
    assert np.concatenate(got).tobytes() == data[:10 * per]
    reader.close()
    reader._thread.join(5)
    assert not reader._thread.is_alive()


def test_reader_worker_stops_on_close():
    class Endless(io.RawIOBase):
        def readinto(self, b):
            b[:] = bytes(len(b))
            return len(b)

    reader = video.RawVideoReader(Endless(), 5, 3, batch_size=2, upload=lambda raw: raw.copy(), pix_fmt='nv12')
    assert next(reader).shape == (2, 27)
    reader.close()
    reader._thread.join(5)
    assert not reader._thread.is_alive()
    with pytest.raises(video.VideoClosed):
        next(reader)


def test_writer_writes_frames_in_order():
    rng = np.random.default_rng(24)
    batches = [rng.integers(0, 256, (n, 27), dtype=np.uint8) for n in (3, 1, 2)]
    seen = []

    def download(batch):
        seen.append(batch)
        return batch

    out = io.BytesIO()
    with video.RawVideoWriter(out, pix_fmt='yuv420p', buffer_size=2, download=download) as writer:
        writer.write_frames(batches[0])
        writer.write_frame(lambda k: batches[k], 1)
        writer.write_frame(batches[2])
    assert out.getvalue() == b''.join(b.tobytes() for b in batches)
    assert writer.frames_written == 6 and len(seen) == 3
    writer.close()                                      # idempotent
    with pytest.raises(video.VideoClosed):
        writer.write_frames(batches[0])
    assert not writer._thread.is_alive()


def test_writer_surfaces_a_worker_error_on_the_next_call():
    failed = threading.Event()

    class Broken:
        def write(self, data):
            failed.set()
            raise OSError('pipe closed')

    writer = video.RawVideoWriter(Broken(), download=lambda b: b)
    frame = np.zeros((1, 27), np.uint8)
    writer.write_frames(frame)
    assert failed.wait(5)
    while writer._error is None and writer._thread.is_alive():      # the worker records the error right after write() raised
        failed.wait(0.001)
    with pytest.raises(OSError, match='pipe closed'):
        writer.write_frames(frame)
    writer.close()
    writer.close()


def test_writer_rgb24_writes_the_input_bytes():
    frames = np.random.default_rng(25).integers(0, 256, (3, 4, 5, 3), dtype=np.uint8)
    out = io.BytesIO()
    with video.RawVideoWriter(out, pix_fmt='rgb24') as writer:
        writer.write_frames(frames[:2])
        writer.write_frame(frames[2])
    assert out.getvalue() == frames.tobytes() and writer.frames_written == 3
