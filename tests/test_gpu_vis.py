"""-m gpu: terran_amd.vis / ta_frames_draw against the reference's terran.vis (tests/golden/vis.npz) and the numpy
restatement of its primitives (tests/vis_raster.py), bit for bit over whole frames.  Reads no Pillow and no reference."""
import os
import random

import numpy as np
import pytest

from terran_amd import lib, results, runtime, synth, vis
from tests import vis_raster as V

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'vis.npz')


def _fresh(monkeypatch, seed):
    monkeypatch.setattr(vis, 'FACE_COLORMAP', vis.build_colormap())
    random.seed(seed)


def _scene_prims(seed, n, h, w, scale=1.0):
    """The bench's scene: 4 synth people and 2 named boxes per frame -> (faces_per_frame, poses_per_frame)."""
    rng = np.random.default_rng(seed)
    faces, poses = [], []
    for i in range(n):
        kps, v = synth.people(seed + i, 4, h, w)
        k = np.concatenate([kps, v[..., None]], -1).astype(np.int32)
        poses.append([{'keypoints': x, 'score': 1.0} for x in k])
        b = []
        for j in range(2):
            x0, y0 = rng.uniform(-50, w - 100), rng.uniform(-50, h - 100)
            b.append({'bbox': np.array([x0, y0, x0 + rng.uniform(20, 300), y0 + rng.uniform(20, 300)], np.float32),
                      'name': 'p%d' % rng.integers(0, 5)})
        faces.append(b)
    return faces, poses


def test_vis_faces_and_poses_reproduce_the_reference(monkeypatch):
    _, scenes = V.golden_scenes(GOLDEN)
    for s in scenes:
        _fresh(monkeypatch, s['seed'])
        fn = vis.vis_faces if s['kind'].startswith('faces') else vis.vis_poses
        base = s['base'].copy()
        got = fn(base, s['input'], scale=s['scale'])
        assert got is not base and np.array_equal(base, s['base'])
        assert np.array_equal(got, s['expected']), (s['kind'], s['scale'], (got != s['expected']).any(-1).sum())


def test_resident_1080p_batch_equals_restatement(monkeypatch):
    """32 x 1080 x 1920 resident frames: draw_faces + draw_poses in place equal the restatement over every pixel of every
    frame (so nothing outside the primitives changed either)."""
    n, h, w = 32, 1080, 1920
    host = synth.frames(77, n, h, w)
    faces, poses = _scene_prims(77, n, h, w)
    ctx = runtime.get_context(0)
    frames = ctx.upload(host)
    try:
        _fresh(monkeypatch, 1)
        vis.draw_faces(frames, faces)
        vis.draw_poses(frames, poses)
        got = frames.download()
    finally:
        frames.free()
    _fresh(monkeypatch, 1)
    prims = np.concatenate([vis.pack_faces(faces), vis.pack_poses(poses)])
    assert len(prims) > 32 * 60
    want = V.draw_prims(host.copy(), prims)
    assert (want != host).any(-1).sum() > 32 * 20000
    assert np.array_equal(got, want), [int((got[i] != want[i]).any(-1).sum()) for i in range(n)]


def test_random_primitives_and_interleaved_frames():
    """Random bars, lines (widths 0-40) and discs, on and off odd-sized frames, any alpha: equal to the restatement; the
    result does not depend on how the primitives of different frames are interleaved."""
    rng = np.random.default_rng(3)
    n, h, w, m = 6, 61, 83, 1800
    p = np.zeros(m, lib.PRIM_DT)
    p['frame'] = rng.integers(0, n, m)
    p['kind'] = rng.integers(0, 3, m)
    x0, y0 = rng.integers(-40, w + 40, m), rng.integers(-40, h + 40, m)
    short = rng.random(m) < 0.4
    x1 = np.where(short, x0 + rng.integers(-6, 7, m), rng.integers(-40, w + 40, m))
    y1 = np.where(short, y0 + rng.integers(-6, 7, m), rng.integers(-40, h + 40, m))
    box = p['kind'] != lib.DRAW_LINE
    p['x0'], p['x1'] = np.where(box, np.minimum(x0, x1), x0), np.where(box, np.maximum(x0, x1), x1)
    p['y0'], p['y1'] = np.where(box, np.minimum(y0, y1), y0), np.where(box, np.maximum(y0, y1), y1)
    p['width'] = np.where(rng.random(m) < 0.5, rng.integers(0, 41, m), rng.integers(0, 6, m))
    p['rgba'] = rng.integers(0, 256, (m, 4))
    host = synth.frames(5, n, h, w)
    want = V.draw_prims(host.copy(), p)
    ctx = runtime.get_context(0)
    rank = np.zeros(m, np.int64)                        # position of a primitive within its frame's sequence
    for f in range(n):
        rank[p['frame'] == f] = np.arange((p['frame'] == f).sum())
    for order in (np.arange(m), np.argsort(p['frame'], kind='stable'), np.lexsort((-p['frame'], rank))):
        q = p[order]
        assert all(np.array_equal(p[p['frame'] == f], q[q['frame'] == f]) for f in range(n))
        frames = ctx.upload(host)
        try:
            frames.draw(q)
            got = frames.download()
        finally:
            frames.free()
        assert np.array_equal(got, want), [int((got[i] != want[i]).any(-1).sum()) for i in range(n)]


def test_overlapping_limbs_blend_in_list_order():
    """Hundreds of alpha-180 limbs piled on one spot: every pixel must see them in list order."""
    rng = np.random.default_rng(11)
    m = 400
    p = np.zeros(m, lib.PRIM_DT)
    p['kind'] = lib.DRAW_LINE
    c = rng.integers(28, 36, (m, 4))
    p['x0'], p['y0'] = c[:, 0] - rng.integers(0, 30, m), c[:, 1] - rng.integers(0, 30, m)
    p['x1'], p['y1'] = c[:, 2] + rng.integers(0, 30, m), c[:, 3] + rng.integers(0, 30, m)
    p['width'] = rng.integers(1, 20, m)
    p['rgba'][:, :3] = rng.integers(0, 256, (m, 3))
    p['rgba'][:, 3] = 180
    host = synth.frames(9, 1, 64, 64)
    ctx = runtime.get_context(0)
    frames = ctx.upload(host)
    try:
        frames.draw(p)
        got = frames.download()
    finally:
        frames.free()
    want = V.draw_prims(host.copy(), p)
    assert np.array_equal(got, want)
    assert not np.array_equal(want, V.draw_prims(host.copy(), p[::-1]))    # the order does matter here


def test_edge_cases_and_errors(monkeypatch):
    img = synth.frames(4, 1, 50, 70)[0]
    out = vis.vis_faces(img, [])
    assert out is not img and np.array_equal(out, img)
    assert np.array_equal(vis.vis_poses(img, []), img)
    # a single dict equals a one-element list
    face = {'bbox': np.array([3.5, 4, 40, 30], np.float32), 'name': 'x'}
    _fresh(monkeypatch, 0)
    a = vis.vis_faces(img, face, scale=2.0)
    _fresh(monkeypatch, 0)
    assert np.array_equal(a, vis.vis_faces(img, [face], scale=2.0)) and not np.array_equal(a, img)
    # LazyFaces (the detector's opt-in lazy results) draw like the plain list they stand for
    boxes = np.array([[5, 5, 30, 20], [-10, 30, 20, 60], [50, 2, 69, 49]], np.float32)
    lazy = results.LazyFaces(boxes, np.zeros((3, 5, 2), np.float32), np.ones(3, np.float32))
    plain = [{'bbox': b} for b in boxes]
    _fresh(monkeypatch, 3)
    a = vis.vis_faces(img, lazy)
    _fresh(monkeypatch, 3)
    assert np.array_equal(a, vis.vis_faces(img, plain))
    # a bad box raises before anything is drawn into a resident batch
    ctx = runtime.get_context(0)
    frames = ctx.upload(np.stack([img, img]))
    try:
        with pytest.raises(ValueError):
            vis.draw_faces(frames, [[face], [face, {'bbox': np.array([9, 9, 3, 20], np.float32)}]])
        vis.draw_faces(frames, [[], []])
        vis.draw_poses(frames, [[]])
        assert np.array_equal(frames.download(), np.stack([img, img]))
        # TA_E_INVALID: frame index out of range, unknown kind
        p = np.zeros(1, lib.PRIM_DT)
        p['frame'], p['x1'], p['y1'] = 2, 3, 3
        with pytest.raises(lib.TerranAmdError) as e:
            frames.draw(p)
        assert e.value.code == lib.E_INVALID and 'frame 2 out of range' in str(e.value)
        p['frame'], p['kind'] = 0, 7
        with pytest.raises(lib.TerranAmdError) as e:
            frames.draw(p)
        assert e.value.code == lib.E_INVALID
        assert np.array_equal(frames.download(), np.stack([img, img]))
    finally:
        frames.free()


def test_stream_pipeline_resident_batches_drawn_after_each_triple(states, monkeypatch):
    """Batches stay resident through StreamPipeline.run (free_resident=False); drawing each one after its triple was
    yielded, on the caller's own context, equals vis_faces / vis_poses on the host copies."""
    from terran_amd.pipeline import StreamPipeline
    kw = dict(detection_kw=dict(short_side=96, state=states('retinaface')), recognition_kw=dict(state=states('arcface')),
              estimation_kw=dict(short_side=96, state=states('openpose_decoder')))
    batches = [synth.pose_code_frames(900 + 10 * i, n, 96, 128, 3) for i, n in enumerate([5, 4, 3])]
    pipe = StreamPipeline([0], inflight=2, pick_faces=lambda dets: [d[:2] for d in dets], **kw)
    ctx = runtime.new_context(0)
    drawn = []
    try:
        resident = [pipe.scatter(b) for b in batches]
        for i, ((d, _, p), r) in enumerate(zip(pipe.run(iter(resident), free_resident=False), resident)):
            _fresh(monkeypatch, 50 + i)
            vis.draw_faces(r[0], d, ctx=ctx)
            vis.draw_poses(r[0], p, ctx=ctx)
            drawn.append((r[0].download(), d, p))
        for r in resident:
            r[0].free()
    finally:
        pipe.close()
    n_faces = n_people = 0
    for i, (got, d, p) in enumerate(drawn):
        _fresh(monkeypatch, 50 + i)
        want = [vis.vis_faces(img, faces) for img, faces in zip(batches[i], d)]
        want = np.stack([vis.vis_poses(img, people) for img, people in zip(want, p)])
        assert np.array_equal(got, want), i
        n_faces += sum(len(x) for x in d)
        n_people += sum(len(x) for x in p)
    assert n_faces > 10 and n_people > 10
