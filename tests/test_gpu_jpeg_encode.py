"""-m gpu: ta_jpeg_encode / terran_amd.image.encode_jpeg against the JPEG files Pillow writes (tests/golden/
jpeg_encode.npz), byte for byte: every fixture alone and same-size fixtures batched, 32 x 1080p synthetic frames and the
worst case (noise at q100 4:4:4) against the live Pillow, mixed-size lists, a decode round trip, encoding after a draw,
the Motion-JPEG writer and repeatability."""
import io

import numpy as np
import pytest

from terran_amd import image, runtime, synth, vis
from terran_amd.video import JpegVideoWriter
from tests.test_jpeg_encode_cpu import golden

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def fx():
    return golden()


def test_every_fixture_alone(fx):
    ctx = runtime.get_context(0)
    for name, f in fx.items():
        files = image.encode_jpeg(f['px'], f['quality'], f['subsampling'], ctx=ctx)
        assert len(files) == 1
        assert files[0] == f['jpg'], '%s: %d bytes, Pillow %d' % (name, len(files[0]), len(f['jpg']))


def test_same_size_fixtures_batched(fx):
    ctx = runtime.get_context(0)
    by_shape = {}
    for name, f in fx.items():
        by_shape.setdefault(f['px'].shape, []).append(name)
    batched = 0
    for shape, names in by_shape.items():
        if len(names) < 2:
            continue
        frames = ctx.upload(np.stack([fx[n]['px'] for n in names]))
        try:
            for n in names:                                  # the batch under each member's options
                q, s = fx[n]['quality'], fx[n]['subsampling']
                files = frames.encode_jpeg(q, image.jpeg_options(q, s)[1])
                assert len(files) == len(names)
                assert files[names.index(n)] == fx[n]['jpg'], n
                batched += 1
        finally:
            frames.free()
    assert batched >= 20


def _pillow(px, q, s):
    Image = pytest.importorskip('PIL.Image')
    f = io.BytesIO()
    Image.fromarray(px).save(f, 'JPEG', quality=q, subsampling=s)
    return f.getvalue()


def test_1080p_batch_and_worst_case_equal_pillow():
    pytest.importorskip('PIL.Image')
    ctx = runtime.get_context(0)
    frames = synth.frames(11, 32, 1080, 1920)
    batch = ctx.upload(frames)
    try:
        files = batch.encode_jpeg(90, 2)
        stats = ctx.jpeg_encode_stats()[1]
        assert stats['images'] == 32 and stats['bytes'] == sum(len(f) for f in files)
        for i in range(32):
            assert files[i] == _pillow(frames[i], 90, 2), i
    finally:
        batch.free()
    noise = np.random.default_rng(3).integers(0, 256, (2, 1080, 1920, 3), dtype=np.uint8)
    batch = ctx.upload(noise)
    try:
        files = batch.encode_jpeg(100, 0)
        for i in range(2):
            ref = _pillow(noise[i], 100, 0)
            assert len(ref) > noise[i].nbytes                  # larger than the RGB it encodes
            assert files[i] == ref, i
    finally:
        batch.free()


def test_list_of_mixed_size_batches(fx):
    names = [n for n in fx if n.startswith('rw-')] + ['noise_24x40_s0_q100', next(n for n in fx if '_17x23_' in n)]
    datas = [fx[n]['jpg'] for n in names]
    frames = image.open_images(datas)
    assert isinstance(frames, list) and len(frames) == len(names)
    try:
        files = image.encode_jpeg(frames, 80, '4:2:2')
        for f, got in zip(frames, files):
            assert got == _pillow(f.download()[0], 80, 1)
    finally:
        for f in frames:
            f.free()


def test_round_trip_through_the_decoder(fx):
    Image = pytest.importorskip('PIL.Image')
    px = synth.frames(5, 3, 120, 176)
    ctx = runtime.get_context(0)
    batch = ctx.upload(px)
    try:
        files = batch.encode_jpeg(85, 2)
    finally:
        batch.free()
    decoded = image.decode_jpeg(files)
    try:
        got = decoded.download()
    finally:
        decoded.free()
    for i in range(3):
        ref = np.asarray(Image.open(io.BytesIO(_pillow(px[i], 85, 2))).convert('RGB'))
        assert np.array_equal(got[i], ref), i


def test_encode_after_draw_sees_the_drawing():
    ctx = runtime.get_context(0)
    px = np.full((2, 96, 128, 3), 40, np.uint8)
    frames = ctx.upload(px)
    try:
        faces = [[{'bbox': np.array([10, 12, 70, 80], np.float32), 'landmarks': np.zeros((5, 2), np.float32),
                   'score': 0.9}], []]
        vis.draw_faces(frames, faces, ctx=ctx)
        files = frames.encode_jpeg(75, 2, ctx=ctx)
        drawn = frames.download()
    finally:
        frames.free()
    assert (drawn[0] != 40).any()
    assert files[0] == _pillow(drawn[0], 75, 2) and files[1] == _pillow(px[1], 75, 2)
    assert files[0] != files[1]


def test_video_writer_stream_splits_into_the_files():
    px = synth.frames(9, 5, 64, 96)
    ctx = runtime.get_context(0)
    batch = ctx.upload(px)
    out = io.BytesIO()
    try:
        expect = batch.encode_jpeg(90, 2)
        with JpegVideoWriter(out, quality=90) as w:
            w.write_frames(batch)
            w.write_frame(lambda a: a, px[0])
    finally:
        batch.free()
    data = out.getvalue()
    parts = [b'\xff\xd8' + p for p in data.split(b'\xff\xd8')[1:]]
    assert parts == expect + [expect[0]]
    assert all(p.endswith(b'\xff\xd9') for p in parts)


def test_repeated_calls_are_identical():
    ctx = runtime.get_context(0)
    px = np.random.default_rng(8).integers(0, 256, (4, 131, 257, 3), dtype=np.uint8)
    px[:, 40:90] = 255                                       # long 0xFF runs next to noise
    batch = ctx.upload(px)
    try:
        first = batch.encode_jpeg(97, 2)
        small = ctx.upload(px[:1, :9, :17])
        try:
            small.encode_jpeg(10, 0)                          # a different layout in between
        finally:
            small.free()
        for _ in range(3):
            assert batch.encode_jpeg(97, 2) == first
    finally:
        batch.free()


def test_bad_options_fail_before_a_launch():
    ctx = runtime.get_context(0)
    batch = ctx.upload(np.zeros((1, 8, 8, 3), np.uint8))
    try:
        for q, s in [(0, 2), (101, 2), (75, 3), (75, -1)]:
            with pytest.raises(ValueError):
                batch.encode_jpeg(q, s)
        with pytest.raises(ValueError):
            image.encode_jpeg(batch, 75, '4:1:1')
    finally:
        batch.free()


def test_save_images_writes_pillows_files(tmp_path, fx):
    names = [n for n in fx if n.startswith('rw-')]
    paths = [str(tmp_path / ('%s.jpg' % n)) for n in names]
    image.save_images([runtime.get_context(0).upload(fx[n]['px'][None]) for n in names], paths, 90, 2)
    for n, p in zip(names, paths):
        with open(p, 'rb') as fh:
            assert fh.read() == _pillow(fx[n]['px'], 90, 2), n
