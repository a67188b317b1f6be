"""The staging that the frame region operations share (csrc/frame_regions.h) carries nothing from one call to the next:
a sequence of calls of different families on ONE context -- its scratch and pinned blocks grow and move between them --
gives, byte for byte, what the same calls give on a fresh context each."""
import numpy as np
import pytest

from terran_amd import lib, runtime

pytestmark = pytest.mark.gpu

BOX, ELLIPSE = lib.BLUR_BOX, lib.BLUR_ELLIPSE
W, H = 23, 37                                           # odd: 69-byte rows, so row starts take every byte phase


def _specs():
    specs = np.zeros(3, lib.FILTER_SPEC_DT)
    specs[0]['kind'], specs[0]['size'], specs[0]['scale'] = lib.FILTER_KERNEL, 3, 16.0
    specs[0]['kernel'][:9] = (-2, -2, -2, -2, 32, -2, -2, -2, -2)
    specs[1]['kind'], specs[1]['size'], specs[1]['rank'] = lib.FILTER_RANK, 5, 12
    specs[2]['kind'], specs[2]['radius'], specs[2]['percent'], specs[2]['threshold'] = lib.FILTER_UNSHARP, 2.0, 150, 3
    return specs


LUTS = np.stack([np.tile(np.arange(256, dtype=np.uint8), 3), np.tile(255 - np.arange(256, dtype=np.uint8), 3)])
HIST = np.array([(0, 2, 3, 20, 30, BOX), (1, 1, 2, 22, 35, ELLIPSE)], lib.HIST_DT)
# (name, what it does to a batch; a histogram returns its counts)
SEQUENCE = [
    ('histogram', lambda f, c: f.histogram(HIST, lib.HIST_RGB, ctx=c)),
    ('point', lambda f, c: f.point(np.array([(0, 3, 4, 21, 33, ELLIPSE, 1)], lib.POINT_DT), LUTS, ctx=c)),
    ('blur', lambda f, c: f.blur(np.array([(0, 1, 1, 15, 20, BOX, 2.0), (0, 8, 10, 23, 37, ELLIPSE, 1.5)], lib.BLUR_DT), ctx=c)),
    ('pixelate', lambda f, c: f.pixelate(np.array([(1, 2, 5, 21, 32, ELLIPSE, 3)], lib.PIXELATE_DT), ctx=c)),
    ('filter', lambda f, c: f.filter(np.array([(0, 0, 0, 14, 18, BOX, 0), (0, 9, 12, 23, 37, ELLIPSE, 1), (1, 3, 3, 20, 30, BOX, 2)],
                                              lib.FILTER_REGION_DT), _specs(), ctx=c)),
    ('saturate', lambda f, c: f.saturate(np.array([(1, 0, 0, 23, 37, ELLIPSE, 1.75), (0, 4, 6, 19, 29, BOX, 0.25)], lib.SATURATE_DT), ctx=c)),
    ('histogram', lambda f, c: f.histogram(HIST, lib.HIST_RGB, ctx=c)),
]


def test_region_ops_in_sequence_on_one_context():
    assert lib.blur_plan(np.array([(0, 1, 1, 15, 20, BOX, 2.0), (0, 8, 10, 23, 37, ELLIPSE, 1.5)], lib.BLUR_DT))[0].tolist() == [0, 1]
    host = np.random.default_rng(2337).integers(0, 256, (2, H, W, 3), dtype=np.uint8)

    ctx = runtime.new_context(0)
    frames = ctx.upload(host)
    try:
        together = [op(frames, ctx) for _, op in SEQUENCE]
        final = frames.download()
    finally:
        frames.free()
        ctx.close()

    apart, at = [], host
    for _, op in SEQUENCE:                              # every operation on a context of its own, through the host
        ctx = runtime.new_context(0)
        frames = ctx.upload(at)
        try:
            apart.append(op(frames, ctx))
            at = frames.download()
        finally:
            frames.free()
            ctx.close()

    assert not np.array_equal(final, host)
    assert np.array_equal(final, at)
    for (name, _), a, b in zip(SEQUENCE, together, apart):
        if name == 'histogram':
            assert a.sum() > 0 and np.array_equal(a, b)
    assert not np.array_equal(together[0], together[-1])
