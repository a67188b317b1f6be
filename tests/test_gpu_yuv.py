"""Raw YUV video on the device (ta_frames_from_yuv, ta_frames_to_yuv): bit for bit the numpy model (tests/yuv_model.py) at
every alignment a frame, a row and a unit can have, exhaustively over all 2^24 triples, and through the reader and the
writer."""
import io

import numpy as np
import pytest

from terran_amd import image, lib, runtime, video, vis
from tests import color_model, yuv_model

pytestmark = pytest.mark.gpu

SHAPES = [(h, w) for h in (1, 2, 3, 37) for w in (1, 2, 3, 5, 53, 64, 257)]
MODES = [('nearest', 'left'), ('bilinear', 'left'), ('bilinear', 'center')]
COMBOS = [(m, r) for m in ('bt601', 'bt709') for r in ('tv', 'pc')]
N = 3                                       # an odd frame size puts frames 1 and 2 on odd addresses


def _ctx():
    return runtime.get_context(0)


def _yuv_frames(rng, fmt, h, w):
    """N frames of seeded random planes; the chroma planes of frame 1 are a 0 / 255 checkerboard (the interpolation's rounding)."""
    frames = []
    for f in np.arange(N):
        y = rng.integers(0, 256, (h, w), dtype=np.uint8)
        ch, cw = (h, w) if fmt == 'yuv444p' else yuv_model.chroma_size(h, w)
        u, v = rng.integers(0, 256, (2, ch, cw), dtype=np.uint8)
        if f == 1:
            board = ((np.add.outer(np.arange(ch), np.arange(cw)) & 1) * 255).astype(np.uint8)
            u, v = board, 255 - board
        frames.append(yuv_model.join_planes(fmt, y, u, v))
    return np.stack(frames)


def _rgb_frames(rng, h, w):
    """N frames: random, and frame 1 of 2 x 2 blocks whose channel means differ from a grey by an odd number -- in pc range
    Cb or Cr of such a block is exactly a half (a rounding tie) -- with the pixels of a block spread around their mean."""
    frames = rng.integers(0, 256, (N, h, w, 3), dtype=np.uint8)
    ch, cw = yuv_model.chroma_size(h, w)
    grey = rng.integers(10, 240, (ch, cw))
    odd = rng.choice([-3, -1, 1, 3], (ch, cw))
    block = np.stack([grey + odd * ((np.add.outer(np.arange(ch), np.arange(cw)) & 1) == 1), grey,
                      grey + odd * ((np.add.outer(np.arange(ch), np.arange(cw)) & 1) == 0)], -1)
    tie = np.repeat(np.repeat(block, 2, 0), 2, 1)[:h, :w]
    spread = np.where((np.add.outer(np.arange(h), np.arange(w)) & 1) == 0, 1, -1)[..., None] * rng.integers(0, 3, 3)
    frames[1] = np.clip(tie + spread, 0, 255)
    return frames


def _differing(got, want):
    return [int((got[f] != want[f]).any(-1).sum()) if got.ndim == 4 else int((got[f] != want[f]).sum()) for f in np.arange(len(want))]


@pytest.mark.parametrize('fmt', yuv_model.FORMATS)
def test_from_yuv_walk(fmt):
    ctx = _ctx()
    rng = np.random.default_rng(31)
    for k, (h, w) in enumerate(SHAPES):
        matrix, range = COMBOS[k % 4]
        data = _yuv_frames(rng, fmt, h, w)
        for chroma, siting in MODES:
            spec = image.yuv_spec(fmt, matrix, range, chroma, siting)
            batch = ctx.frames_from_yuv(data, N, h, w, spec)
            got = batch.download()
            batch.free()
            want = yuv_model.from_yuv(data, N, h, w, fmt, matrix, range, chroma, siting)
            assert got.shape == want.shape
            assert np.array_equal(got, want), (fmt, h, w, chroma, siting, 'differing pixels per frame', _differing(got, want))


@pytest.mark.parametrize('fmt', yuv_model.FORMATS)
def test_to_yuv_walk(fmt):
    ctx = _ctx()
    rng = np.random.default_rng(32)
    for k, (h, w) in enumerate(SHAPES):
        matrix, range = COMBOS[(k + 1) % 4]
        frames = _rgb_frames(rng, h, w)
        batch = ctx.upload(frames)
        got = batch.to_yuv(image.yuv_spec(fmt, matrix, range))
        batch.free()
        want = yuv_model.to_yuv(frames, fmt, matrix, range)
        assert got.shape == want.shape == (N, yuv_model.frame_bytes(fmt, h, w))
        assert np.array_equal(got, want), (fmt, h, w, matrix, range, 'differing bytes per frame', _differing(got, want))


@pytest.fixture(scope='module')
def every_colour():
    return color_model.all_colours()


@pytest.mark.parametrize('matrix,range', COMBOS)
def test_every_triple_on_the_device(every_colour, matrix, range):
    ctx = _ctx()
    side = 4096
    flat = every_colour.reshape(-1, 3)
    # from_yuv: the yuv444p frame whose pixel k is the triple k
    data = np.concatenate([flat[:, 0], flat[:, 1], flat[:, 2]])
    batch = image.frames_from_yuv(data, (side, side), 'yuv444p', matrix, range, ctx=ctx)
    got = batch.download()[0].reshape(-1, 3)
    batch.free()
    want = yuv_model.yuv_to_rgb(flat[:, 0], flat[:, 1], flat[:, 2], matrix, range)
    assert np.array_equal(got, want), int((got != want).any(-1).sum())
    # to_yuv: the frame of all colours
    got = image.frames_to_yuv(every_colour, 'yuv444p', matrix, range, ctx=ctx)[0].reshape(3, -1).T
    want = yuv_model.rgb_to_yuv(flat[:, 0], flat[:, 1], flat[:, 2], matrix, range)
    assert np.array_equal(got, want), int((got != want).any(-1).sum())


def test_nv12_and_yuv420p_of_the_same_planes_agree():
    ctx = _ctx()
    rng = np.random.default_rng(33)
    h, w = 37, 53
    planes = [(rng.integers(0, 256, (h, w), dtype=np.uint8), *rng.integers(0, 256, (2, 19, 27), dtype=np.uint8)) for _ in np.arange(N)]
    for chroma, siting in MODES:
        got = []
        for fmt in ('yuv420p', 'nv12'):
            data = np.stack([yuv_model.join_planes(fmt, *p) for p in planes])
            batch = image.frames_from_yuv(data, (w, h), fmt, 'bt601', 'tv', chroma, siting, ctx=ctx)
            got.append(batch.download())
            batch.free()
        assert np.array_equal(got[0], got[1])
    frames = _rgb_frames(rng, h, w)
    a = image.frames_to_yuv(frames, 'yuv420p', ctx=ctx)
    b = image.frames_to_yuv(frames, 'nv12', ctx=ctx)
    for f in np.arange(N):
        pa, pb = yuv_model.split_planes('yuv420p', a[f], h, w), yuv_model.split_planes('nv12', b[f], h, w)
        assert all(np.array_equal(x, y) for x, y in zip(pa, pb))


def test_frames_to_yuv_of_a_list_is_the_concatenation():
    ctx = _ctx()
    frames = np.random.default_rng(34).integers(0, 256, (5, 9, 11, 3), dtype=np.uint8)
    parts = [ctx.upload(frames[:2]), ctx.upload(frames[2:3]), ctx.upload(frames[3:])]
    got = image.frames_to_yuv(parts, 'nv12', 'bt601', 'pc', ctx=ctx)
    assert np.array_equal(got, yuv_model.to_yuv(frames, 'nv12', 'bt601', 'pc'))
    assert np.array_equal(got, image.frames_to_yuv(frames, 'nv12', 'bt601', 'pc', ctx=ctx))
    other = ctx.upload(frames[:1, :4])
    with pytest.raises(ValueError, match='one frame size'):
        image.frames_to_yuv([parts[0], other], ctx=ctx)
    out = np.empty((2, 1), np.uint8)
    with pytest.raises(ValueError, match='out must be'):
        parts[0].to_yuv(image.yuv_spec('nv12'), out=out)


def test_invalid_arguments_are_refused_before_any_launch():
    ctx = _ctx()
    frames = np.random.default_rng(35).integers(0, 256, (2, 6, 8, 3), dtype=np.uint8)
    batch = ctx.upload(frames)
    data = np.zeros(2 * yuv_model.frame_bytes('yuv420p', 6, 8), np.uint8)        # two frames of format 0
    for field in np.arange(5):
        for bad in (-1, 2 if field else 3):
            spec = [0, 0, 0, 0, 0]
            spec[field] = bad
            with pytest.raises(lib.TerranAmdError) as e:
                batch.to_yuv(spec)
            assert e.value.code == lib.E_INVALID
            with pytest.raises(lib.TerranAmdError) as e:
                ctx.frames_from_yuv(data, 2, 6, 8, spec)
            assert e.value.code == lib.E_INVALID
    good = image.yuv_spec('yuv420p')
    for n, h, w in ((0, 6, 8), (-1, 6, 8), (2, 0, 8), (2, 6, -3), (2, 65536, 8)):
        with pytest.raises(lib.TerranAmdError) as e:
            ctx.frames_from_yuv(data, n, h, w, good)
        assert e.value.code == lib.E_INVALID
    with pytest.raises(ValueError, match='bytes'):
        ctx.frames_from_yuv(data[:-1], 2, 6, 8, good)
    with pytest.raises(ValueError, match='whole'):
        image.frames_from_yuv(data[:-1], (8, 6), 'yuv420p', ctx=ctx)
    assert np.array_equal(batch.download(), frames)


def test_reader_and_writer_end_to_end():
    w, h = 5, 3
    rng = np.random.default_rng(36)
    data = rng.integers(0, 256, (5, yuv_model.frame_bytes('yuv420p', h, w)), dtype=np.uint8)
    want = yuv_model.from_yuv(data, 5, h, w)
    with video.RawVideoReader(io.BytesIO(data.tobytes()), w, h, batch_size=2, pix_fmt='yuv420p') as reader:
        batches = list(reader)
    assert [b.shape for b in batches] == [(2, h, w, 3), (2, h, w, 3), (1, h, w, 3)]
    assert all(isinstance(b, lib.Frames) for b in batches)
    assert np.array_equal(np.concatenate([b.download() for b in batches]), want)
    out = io.BytesIO()
    with video.RawVideoWriter(out) as writer:
        for b in batches:
            writer.write_frames(b)
    assert out.getvalue() == yuv_model.to_yuv(want).tobytes() and writer.frames_written == 5


def test_reader_draw_writer():
    w, h, n = 64, 48, 3
    rng = np.random.default_rng(37)
    data = rng.integers(0, 256, (n, yuv_model.frame_bytes('nv12', h, w)), dtype=np.uint8)
    faces = [[{'bbox': np.array([8.0, 6.0, 40.0, 30.0], np.float32)}], [], [{'bbox': np.array([20.5, 10.0, 60.0, 44.0], np.float32)}]]
    plain = yuv_model.from_yuv(data, n, h, w, 'nv12', 'bt601', 'pc', 'nearest')
    out, drawn = io.BytesIO(), []
    with video.RawVideoReader(io.BytesIO(data.tobytes()), w, h, batch_size=2, pix_fmt='nv12', matrix='bt601', range='pc',
                              chroma='nearest') as reader, video.RawVideoWriter(out, 'nv12', 'bt601', 'pc') as writer:
        at = 0
        for batch in reader:
            vis.draw_faces(batch, faces[at:at + len(batch)], ctx=_ctx())
            drawn.append(batch.download())
            writer.write_frames(batch)
            at += len(batch)
    drawn = np.concatenate(drawn)
    changed = (drawn != plain).any(-1)
    assert changed[0].any() and not changed[1].any() and changed[2].any()
    got = np.frombuffer(out.getvalue(), np.uint8).reshape(n, -1)
    assert np.array_equal(got, yuv_model.to_yuv(drawn, 'nv12', 'bt601', 'pc'))
    # outside the drawn pixels' blocks the stream is what the undrawn frames give
    undrawn = yuv_model.to_yuv(plain, 'nv12', 'bt601', 'pc')
    for f in np.arange(n):
        y_got, u_got, v_got = yuv_model.split_planes('nv12', got[f], h, w)
        y_un, u_un, v_un = yuv_model.split_planes('nv12', undrawn[f], h, w)
        assert np.array_equal(y_got[~changed[f]], y_un[~changed[f]])
        blocks = changed[f].reshape(h // 2, 2, w // 2, 2).any(axis=(1, 3))
        assert np.array_equal(u_got[~blocks], u_un[~blocks]) and np.array_equal(v_got[~blocks], v_un[~blocks])


def test_reader_prefetches_while_the_consumer_draws_and_writes():
    """The loop of RawVideoWriter's docstring at a size where the reader thread converts the next batches (on its own
    context, in its own staging block) while this thread draws into a batch on that batch's context -- the default, the
    reader's -- and converts it back on its own: every frame in and out equals the model."""
    w, h, n, per_batch = 640, 360, 16, 4
    rng = np.random.default_rng(38)
    data = rng.integers(0, 256, (n, yuv_model.frame_bytes('yuv420p', h, w)), dtype=np.uint8)
    faces = [[{'bbox': np.array([20.0 + 30 * f, 40.0, 200.0 + 20 * f, 300.0], np.float32)}] for f in np.arange(n)]
    plain = yuv_model.from_yuv(data, n, h, w)
    out, drawn = io.BytesIO(), []
    with video.RawVideoReader(io.BytesIO(data.tobytes()), w, h, batch_size=per_batch, prefetch=2, pix_fmt='yuv420p') as reader, \
            video.RawVideoWriter(out) as writer:
        at = 0
        for batch in reader:
            assert batch.ctx is not _ctx()
            vis.draw_faces(batch, faces[at:at + len(batch)])
            drawn.append(batch.download())
            writer.write_frames(batch)
            at += len(batch)
    drawn = np.concatenate(drawn)
    changed = (drawn != plain).any(-1)
    assert changed.any(axis=(1, 2)).all() and not changed.all()
    assert np.array_equal(drawn[~changed], plain[~changed])
    assert out.getvalue() == yuv_model.to_yuv(drawn).tobytes()
