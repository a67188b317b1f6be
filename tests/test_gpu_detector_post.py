"""-m gpu: rf_select_kernel through the entry that ships, ta_retinaface_run, on the painted detector of tests/detector_heads.py.

The network's logits reach the selection as float32 (cls_is_prob = 0): the in-kernel softmax, the `fg - bg < margin` shortcut, the
16-byte cell loads with the incremental (level, y, x) walk and its hop to the next level, the 64-bit mask of a thread's run
(`1ull << 63` at 1248 x 1280) and the rescoring loop of runs past 64 anchors (1280 x 1288) -- none of which
ta_retinaface_postprocess, the entry of the other selection tests, runs.  Per case (tests/test_detector_heads_cpu.py shows on the CPU
that each is what it claims) the three head tensors are first held bit for bit against the float64 reference, then

* counts and order equal oracle.retinaface_post.postprocess on the reference heads,
* bbox and landmarks are np.array_equal to it (dw = dh = 0, the file is built with -ffp-contract=off),
* every score is within SCORE_ULPS float32 ulps of float32(1 / (1 + exp(-(fg - bg)))) computed in float64.

SCORE_ULPS = 3 is the only tolerance.  The ROCm installation carries the OCML bitcode but no document with the error bound of the
device expf, so the bound is measured: the largest deviation seen on the MI355X over the distinct (fg - bg) classes of all cases
(DEVIATION_SEEN = 1 ulp; the test prints it per case) plus 2 ulps for the add and the divide of ef / (eb + ef).  Classes differ by
1/64 in fg - bg, more than 1e-3 in score, so the order never hangs on it.
DESIGN.md section 4 maps each branch of rf_select_kernel to the test id that reaches it."""
import numpy as np
import pytest

from tests import detector_heads as dh
from tests.util import retinaface_run, same

pytestmark = pytest.mark.gpu

DEVIATION_SEEN = 1
SCORE_ULPS = DEVIATION_SEEN + 2


@pytest.fixture(scope='module')
def rig():
    from terran_amd import lib
    ctx = lib.Context(0)
    model = lib.Model(ctx, dh.program())
    yield ctx, model
    model.free()
    ctx.close()


def ulps(a, b):
    """Distance in float32 ulps of two arrays of positive floats."""
    return np.abs(a.astype(np.float32).view(np.int32).astype(np.int64) - b.astype(np.float32).view(np.int32).astype(np.int64))


def run_case(rig, case, capacity=None):
    """Forward + selection of the case's frames; the heads must be the reference's bits.  -> what retinaface_run returns."""
    ctx, model = rig
    ref = dh.reference(case)
    frames = ctx.upload(case.frames())
    try:
        total = sum(len(d) for d in ref['dets'])
        out = retinaface_run(ctx, model, frames, case.thr, case.nms, total if capacity is None else capacity)
        for s in dh.STRIDES:
            same(model.read('head%d' % s), ref['heads'][s], '%s head%d' % (case.name, s))
    finally:
        frames.free()
    return out


def check_detections(case, counts, boxes, lmks, scores):
    ref = dh.reference(case)['dets']
    assert counts.tolist() == [len(d) for d in ref], (case.name, counts.tolist(), [len(d) for d in ref])
    flat = [d for img in ref for d in img]
    if not flat:
        return
    rb, rl, rs = (np.stack([d[k] for d in flat]) for k in ('bbox', 'landmarks', 'score'))
    dev = ulps(scores, rs)
    print('%s: %d detections, %d distinct scores, largest score deviation %d ulps' % (case.name, len(flat), len(np.unique(rs)), dev.max()))
    # the order first: a detection in the wrong place has another anchor's box
    assert np.array_equal(boxes, rb), (case.name, 'bbox', int(np.argmax(np.any(boxes != rb, axis=1))))
    assert np.array_equal(lmks, rl), (case.name, 'landmarks')
    assert dev.max() <= SCORE_ULPS, (case.name, 'score', int(dev.max()))


@pytest.mark.parametrize('name', [c.name for c in dh.CASE_LIST])
def test_painted_frames(rig, name):
    case = dh.CASES[name]
    rc, counts, boxes, lmks, scores, required = run_case(rig, case)
    assert rc == 0, rig[0].last_error()
    assert required == counts.sum()
    check_detections(case, counts, boxes, lmks, scores)


def test_capacity_contract(rig):
    """One short: TA_E_CAPACITY, `required` is the total and the counts are right already; exactly enough: the reference; capacity 0
    with null outputs: `required` only."""
    from terran_amd import lib
    case = dh.CASES['batch3']
    want = [len(d) for d in dh.reference(case)['dets']]
    total = sum(want)
    rc, counts, boxes, _, scores, required = run_case(rig, case, capacity=total - 1)
    assert rc == lib.E_CAPACITY and required == total and counts.tolist() == want
    assert np.isnan(boxes).all() and np.isnan(scores).all()                       # nothing was written
    rc, counts, boxes, lmks, scores, required = run_case(rig, case, capacity=required)
    assert rc == lib.OK and required == total
    check_detections(case, counts, boxes, lmks, scores)
    ctx, model = rig
    frames = ctx.upload(case.frames())
    rc, counts, _, _, _, required = retinaface_run(ctx, model, frames, case.thr, case.nms, 0, outputs=False)
    frames.free()
    assert rc == lib.E_CAPACITY and required == total and counts.tolist() == want
    empty = dh.CASES['c0']
    frames = ctx.upload(empty.frames())
    rc, counts, _, _, _, required = retinaface_run(ctx, model, frames, empty.thr, empty.nms, 0, outputs=False)
    frames.free()
    assert rc == lib.OK and required == 0 and counts.tolist() == [0]
