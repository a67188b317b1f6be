"""-m gpu: face labels on the device -- terran_amd.vis with labels=True and ta_frames_draw_masks' DRAW_MASK primitive
against the reference's vis_faces with draw_label (tests/golden/vis_text.npz, through its recorded font) and the numpy
restatement (tests/vis_text_model.py), bit for bit over whole frames.  Reads no reference; Pillow only as the live font."""
import io
import os
import random

import numpy as np
import pytest

from terran_amd import image, lib, runtime, synth, vis
from terran_amd.video import JpegVideoWriter
from tests import vis_text_model as M

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'vis_text.npz')
COVERAGE = np.array([0, 1, 127, 254, 255], np.uint8)       # a blend done twice, or skipped, shows at every one but 0


def _fresh(monkeypatch, seed):
    monkeypatch.setattr(vis, 'FACE_COLORMAP', vis.build_colormap())
    random.seed(seed)


def _draw(host, prims, masks=None):
    frames = runtime.get_context(0).upload(host)
    try:
        frames.draw(prims, masks)
        return frames.download()
    finally:
        frames.free()


def _diff(got, want):
    return [int((g != w).any(-1).sum()) for g, w in zip(got, want)]


def test_vis_faces_with_labels_reproduces_the_reference(monkeypatch):
    _, tables, scenes = M.golden_scenes(GOLDEN)
    monkeypatch.setattr(vis, 'label_font', lambda size: M.RecordedFont(tables, size))
    for i, s in enumerate(scenes):
        _fresh(monkeypatch, s['seed'])
        base = s['base'].copy()
        got = vis.vis_faces(base, s['faces'], scale=s['scale'], labels=True)
        assert got is not base and np.array_equal(base, s['base'])
        assert np.array_equal(got, s['expected']), (i, s['scale'], int((got != s['expected']).any(-1).sum()))


def test_live_font_random_labels_equal_the_restatement(monkeypatch):
    """Printable-ASCII labels rasterised by the installed font, scales 0.1 - 3, float boxes on and off the frame: the
    device equals the restatement over the whole frame."""
    pytest.importorskip('PIL')
    rng = random.Random(7)
    n_masks = 0
    for it in range(40):
        H, W = rng.randint(20, 120), rng.randint(20, 200)
        base = synth.frames(200 + it, 1, H, W)[0]
        scale = rng.choice([0.1, 0.5, 1.0, 1.5, 3.0, rng.uniform(0.1, 3)])
        faces = M.random_label_faces(rng, H, W, 4)
        _fresh(monkeypatch, it)
        got = vis.vis_faces(base, faces, scale=scale, labels=True)
        _fresh(monkeypatch, it)
        prims, atlas = vis.pack_faces([faces], scale, labels=True)
        n_masks += int((prims['kind'] == lib.DRAW_MASK).sum())
        want = M.draw_prims(base[None].copy(), prims, atlas)[0]
        assert np.array_equal(got, want), (it, scale, faces)
    assert n_masks > 40


@pytest.mark.parametrize('W', [1, 63, 64, 65, 130])
def test_synthetic_masks_at_lane_and_frame_edges(W):
    """Masks 1, 64, 65 and 200 wide inside (where they fit), over each edge and each corner and wholly outside frames
    1, 63, 64, 65 and 130 wide, coverage from {0, 1, 127, 254, 255}, piled on each other in list order."""
    rng = np.random.default_rng(100 + W)
    H, mh = 11, 5
    bitmaps = {mw: rng.choice(COVERAGE, (mh, mw)) for mw in (1, 64, 65, 200)}
    offs, atlas, at = {}, [], 3
    atlas.append(np.full(3, 255, np.uint8))                 # the offsets are bytes: nothing is aligned
    for mw, b in bitmaps.items():
        offs[mw] = at
        atlas.append(b.ravel())
        at += b.size
    atlas = np.concatenate(atlas)
    rows = []
    for mw in bitmaps:
        xs = {'in': min(max((W - mw) // 2, 0), W - 1), 'left': -(mw // 2) - 1 if mw > 1 else -1, 'right': W - (mw + 1) // 2,
              'out_left': -mw, 'out_right': W, 'one_in_left': 1 - mw, 'one_in_right': W - 1, 'at_lane': 63, 'at_lane1': 64 - mw}
        ys = {'in': 3, 'top': -2, 'bottom': H - 2, 'out_top': -mh, 'out_bottom': H, 'one_in_top': 1 - mh, 'one_in_bottom': H - 1}
        for x0 in xs.values():
            for y0 in ys.values():
                rows.append((mw, x0, y0))
    p = np.zeros(len(rows), lib.PRIM_DT)
    p['kind'] = lib.DRAW_MASK
    p['frame'] = rng.integers(0, 2, len(rows))
    for q, (mw, x0, y0) in zip(p, rows):
        q['x0'], q['y0'], q['x1'], q['y1'], q['width'] = x0, y0, x0 + mw - 1, y0 + mh - 1, offs[mw]
    p['rgba'][:, :3] = rng.integers(0, 256, (len(rows), 3))
    p['rgba'][:, 3] = 255
    p = p[rng.permutation(len(p))]
    host = synth.frames(W, 2, H, W)
    want = M.draw_prims(host.copy(), p, atlas)
    assert (want != host).any()
    got = _draw(host, p, atlas)
    assert np.array_equal(got, want), _diff(got, want)
    # coverage 0 leaves a pixel untouched, coverage 255 replaces it, whatever lies under it
    q = np.zeros(2, lib.PRIM_DT)
    q['kind'], q['x1'], q['y1'] = lib.DRAW_MASK, W - 1, H - 1
    q['width'] = [0, H * W]
    q['rgba'] = [(1, 2, 3, 255), (9, 8, 7, 255)]
    got = _draw(host, q, np.concatenate([np.zeros(H * W, np.uint8), np.full(H * W, 255, np.uint8)]))
    assert np.array_equal(got[1], host[1]) and np.all(got[0] == (9, 8, 7))
    assert np.array_equal(_draw(host, q[:1], np.zeros(H * W, np.uint8)), host)


def _mixed(seed, n, h, w, m):
    """m random bars, lines, discs (any alpha) and masks (4 bitmaps, shared by primitives of every frame) over n frames."""
    rng = np.random.default_rng(seed)
    shapes = [(1, 1), (7, 64), (3, 65), (4, 200)]
    bitmaps = [np.where(rng.random(s) < 0.5, rng.choice(COVERAGE, s), rng.integers(0, 256, s)).astype(np.uint8) for s in shapes]
    starts = np.cumsum([0] + [b.size for b in bitmaps])
    p = np.zeros(m, lib.PRIM_DT)
    p['frame'] = rng.integers(0, n, m)
    p['kind'] = rng.integers(0, 4, m)
    x0, y0 = rng.integers(-40, w + 40, m), rng.integers(-40, h + 40, m)
    x1, y1 = rng.integers(-40, w + 40, m), rng.integers(-40, h + 40, m)
    box = p['kind'] != lib.DRAW_LINE
    p['x0'], p['x1'] = np.where(box, np.minimum(x0, x1), x0), np.where(box, np.maximum(x0, x1), x1)
    p['y0'], p['y1'] = np.where(box, np.minimum(y0, y1), y0), np.where(box, np.maximum(y0, y1), y1)
    p['width'] = rng.integers(0, 12, m)
    p['rgba'] = rng.integers(0, 256, (m, 4))
    which = rng.integers(0, len(shapes), m)
    for i in np.nonzero(p['kind'] == lib.DRAW_MASK)[0]:
        bh, bw = shapes[which[i]]
        p[i]['x0'], p[i]['y0'] = rng.integers(-bw, w), rng.integers(-bh, h)
        p[i]['x1'], p[i]['y1'] = p[i]['x0'] + bw - 1, p[i]['y0'] + bh - 1
        p[i]['width'] = starts[which[i]]
        p[i]['rgba'][3] = 255
    return p, np.concatenate([b.ravel() for b in bitmaps])


def test_masks_mixed_with_other_primitives_in_three_submission_orders():
    """One list in its own order, stably sorted by frame, and with the frames reversed (each frame's order kept): the
    same frames, equal to the restatement; every bitmap is used by primitives of all three frames."""
    n, h, w, m = 3, 37, 130, 420
    p, atlas = _mixed(21, n, h, w, m)
    masks = p[p['kind'] == lib.DRAW_MASK]
    assert all(set(masks['frame'][masks['width'] == o]) == {0, 1, 2} for o in set(masks['width'])) and len(set(masks['width'])) == 4
    host = synth.frames(6, n, h, w)
    want = M.draw_prims(host.copy(), p, atlas)
    rank = np.zeros(m, np.int64)
    for f in range(n):
        rank[p['frame'] == f] = np.arange((p['frame'] == f).sum())
    for order in (np.arange(m), np.argsort(p['frame'], kind='stable'), np.lexsort((-p['frame'], rank))):
        q = p[order]
        assert all(np.array_equal(p[p['frame'] == f], q[q['frame'] == f]) for f in range(n))
        got = _draw(host, q, atlas)
        assert np.array_equal(got, want), _diff(got, want)
    assert not np.array_equal(want, M.draw_prims(host.copy(), p[::-1], atlas))     # the order does matter here


def test_mask_errors_leave_every_pixel_unchanged():
    host = synth.frames(4, 2, 20, 30)
    ctx = runtime.get_context(0)
    frames = ctx.upload(host)
    atlas = np.full(40, 255, np.uint8)
    good = np.zeros(2, lib.PRIM_DT)                          # a bar that would draw, then the mask under test
    good['kind'] = [lib.DRAW_BAR, lib.DRAW_MASK]
    good['x0'], good['y0'], good['x1'], good['y1'] = 2, 2, 9, 5     # the mask: 8 x 4 = 32 bytes
    good['rgba'] = 255
    good['frame'] = [0, 1]

    def refused(p, masks, word=None):
        with pytest.raises(lib.TerranAmdError) as e:
            frames.draw(p, masks)
        assert e.value.code == lib.E_INVALID and (word is None or word in str(e.value)), str(e.value)
        assert np.array_equal(frames.download(), host)
    try:
        p = good.copy()
        p['width'][1] = 9                                   # 9 + 32 > 40
        refused(p, atlas, 'reaches')
        refused(good, atlas[:31], 'reaches')
        refused(good, np.zeros(0, np.uint8))                # no buffer at all
        p = good.copy()
        p['rgba'][1, 3] = 254
        refused(p, atlas, 'alpha')
        p = good.copy()
        p['width'][1] = -1
        refused(p, atlas, 'negative')
        p = good.copy()
        p['x1'][1] = 1                                      # inverted, like every other box
        refused(p, atlas)
        refused(good, None, 'unknown kind')                 # ta_frames_draw takes no masks: kind 3 is unknown there
        with pytest.raises(lib.TerranAmdError) as e:        # and ta_frames_draw_masks NULL masks with a mask primitive
            ctx.check(ctx.lib.ta_frames_draw_masks(ctx.h, frames.h, lib.ptr(good), 2, None, 40))
        assert e.value.code == lib.E_INVALID and np.array_equal(frames.download(), host)
        # the same list is fine with its buffer, to the last byte; primitives of no mask kind need no buffer
        p = good.copy()
        p['width'][1] = 8
        frames.draw(p, atlas)
        want = M.draw_prims(host.copy(), p, atlas)
        assert np.array_equal(frames.download(), want) and (want != host).any(-1).sum() == 64
        ctx.check(ctx.lib.ta_frames_draw_masks(ctx.h, frames.h, lib.ptr(good[:1]), 1, None, 0))
        # label errors surface before any launch
        with pytest.raises(ValueError):
            vis.draw_faces(frames, [[{'bbox': [1, 1, 9, 9], 'track': 1}], [{'bbox': [1, 1, 9, 9], 'text': 'a\nb'}]], labels=True)
        with pytest.raises(ValueError):
            vis.draw_faces(frames, [[{'bbox': [1, 1, 9, 9], 'track': 1}]], scale=0.01, labels=True)
        assert np.array_equal(frames.download(), want)
    finally:
        frames.free()


def test_resident_batch_with_labels_and_the_video_writer(monkeypatch):
    """draw_faces(labels=True) into a resident batch on the caller's own context equals vis_faces on the host copies frame
    by frame; the batch then goes through JpegVideoWriter and decodes to what encode_jpeg of the host-drawn frames does."""
    pytest.importorskip('PIL')
    n, h, w = 5, 96, 136
    host = synth.frames(31, n, h, w)
    rng = np.random.default_rng(8)
    tracked = []
    for i in range(n):                                      # as face_tracking returns them: float32 boxes, a track id each
        faces = []
        for t in (1, 2, 7):
            x0, y0 = rng.uniform(-20, w - 20), rng.uniform(-10, h - 10)
            faces.append({'bbox': np.array([x0, y0, x0 + rng.uniform(10, 50), y0 + rng.uniform(10, 50)], np.float32),
                          'landmarks': np.zeros((5, 2), np.float32), 'score': np.float32(0.9), 'track': t})
        tracked.append(faces[:3 - i % 2])
    ctx = runtime.new_context(0)
    frames = runtime.get_context(0).upload(host)
    out = io.BytesIO()
    try:
        _fresh(monkeypatch, 2)
        assert vis.draw_faces(frames, tracked, labels=True, ctx=ctx) is frames
        got = frames.download()
        with JpegVideoWriter(out, quality=90) as writer:
            writer.write_frames(frames)
    finally:
        frames.free()
    _fresh(monkeypatch, 2)
    want = np.stack([vis.vis_faces(img, faces, labels=True) for img, faces in zip(host, tracked)])
    assert np.array_equal(got, want), _diff(got, want)
    _fresh(monkeypatch, 2)
    plain = np.stack([vis.vis_faces(img, faces) for img, faces in zip(host, tracked)])
    assert all((a != b).any() for a, b in zip(want, plain))               # every frame did get a label
    files = image.encode_jpeg(want, quality=90)
    assert out.getvalue() == b''.join(files)
    ends = np.cumsum([len(f) for f in files])
    written = [out.getvalue()[e - len(f):e] for e, f in zip(ends, files)]
    a, b = image.decode_jpeg(written), image.decode_jpeg(files)
    try:
        assert np.array_equal(a.download(), b.download())
    finally:
        a.free()
        b.free()


def test_labels_are_new():
    """On the parent of this change vis_faces took no `labels` and the library had no ta_frames_draw_masks."""
    assert hasattr(lib.load(), 'ta_frames_draw_masks') and lib.DRAW_MASK == 3
    img = synth.frames(1, 1, 40, 80)[0]
    out = vis.vis_faces(img, {'bbox': [5, 5, 30, 30], 'track': 4}, labels=True)
    assert (out != vis.vis_faces(img, {'bbox': [5, 5, 30, 30], 'track': 4})).any()
