"""-m gpu: tiled detection.  The cutter (ta_frames_tiles) against numpy slicing at every byte alignment; the merge
(ta_detections_merge) against the numpy model of tests/tiles_model.py, bit for bit, at the wave, workgroup and bit-word seams of its
kernels (there is one path: a bit matrix in the context's scratch block at every size); RetinaFace.detect_tiles on the painted
detector of tests/detector_heads.py against the float64 reference on each tile's pixels; TiledDetection on the seeded network
against the same steps made by hand with the calls that existed before; and the one-tile identity."""
import ctypes as C

import numpy as np
import pytest

from tests import detector_heads as dh
from tests import tiles_model as tm

pytestmark = pytest.mark.gpu

NAMES = ('counts', 'boxes', 'landmarks', 'scores', 'source')


@pytest.fixture(scope='module')
def ctx():
    from terran_amd import lib
    c = lib.Context(0)
    yield c
    c.close()


# ---- the cutter ----------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def small(ctx):
    fr = np.random.default_rng(5).integers(0, 256, (3, 37, 53, 3), dtype=np.uint8)
    frames = ctx.upload(fr)
    yield fr, frames
    frames.free()


def cut(ctx, frames, tiles, th, tw):
    from terran_amd import lib
    out = ctx.frames_tiles(frames, np.array(tiles, np.int32).reshape(-1, 3).view(lib.TILE_DT).reshape(-1), th, tw)
    try:
        return out.download()
    finally:
        out.free()


def test_cutter_every_alignment(ctx, small):
    """Rows of 63 bytes from byte 3 x of rows of 159 bytes into a batch whose rows start every 63 bytes: every pairing of the four
    byte alignments (and of the sixteen positions in a 16-byte block) on both sides; flush right, flush bottom, every frame."""
    fr, frames = small
    tiles = [(f, y, x) for f in range(3) for y in (0, 21) for x in (0, 1, 2, 3, 32)]
    tiles = [tiles[i] for i in np.random.default_rng(1).permutation(len(tiles))]
    got = cut(ctx, frames, tiles, 16, 21)
    assert got.shape == (30, 16, 21, 3)
    for i, (f, y, x) in enumerate(tiles):
        assert np.array_equal(got[i], fr[f, y:y + 16, x:x + 21]), (i, f, y, x)


def test_cutter_whole_frame_and_one_column(ctx, small):
    fr, frames = small
    assert np.array_equal(cut(ctx, frames, [(1, 0, 0)], 37, 53)[0], fr[1])
    tiles = [(f, y, x) for f in (0, 2) for y in (0, 5, 21) for x in (0, 1, 2, 3, 17, 52)]
    got = cut(ctx, frames, tiles, 16, 1)                                              # tw = 1: rows of three bytes
    for i, (f, y, x) in enumerate(tiles):
        assert np.array_equal(got[i], fr[f, y:y + 16, x:x + 1]), (i, f, y, x)
    tiles = [(2, 36, x) for x in range(0, 50, 7)]
    got = cut(ctx, frames, tiles, 1, 4)                                               # th = 1
    for i, (f, y, x) in enumerate(tiles):
        assert np.array_equal(got[i], fr[f, y:y + 1, x:x + 4]), (i, f, y, x)


def test_cutter_nothing_and_errors(ctx, small):
    from terran_amd import lib
    fr, frames = small
    assert ctx.frames_tiles(frames, np.zeros(0, lib.TILE_DT), 16, 21) is None
    for bad in ((0, 22, 0), (0, 0, 33), (0, -1, 0), (0, 0, -1), (3, 0, 0), (-1, 0, 0)):
        with pytest.raises(lib.TerranAmdError, match='tile 1') as e:
            cut(ctx, frames, [(0, 0, 0), bad], 16, 21)
        assert e.value.code == lib.E_INVALID


# ---- the merge against the model -------------------------------------------------------------------------------------------------------
def check(ctx, groups, n_frames, boxes, lm, scores, thr, metric=0, edge=0.0, stats=None):
    want = tm.merge_model(groups, n_frames, boxes, lm, scores, thr, metric, edge, stats)
    got = ctx.detections_merge(tm.records(groups), n_frames, boxes, lm, scores, thr, metric, edge)
    for a, b, what in zip(got, want, NAMES):
        assert a.dtype == b.dtype and a.shape == b.shape, (what, a.shape, b.shape)
        assert np.array_equal(a, b), (what, int(np.argmax(np.any((a != b).reshape(len(a), -1), axis=1))))
    return got


SEAM_COUNTS = (65, 0, 1, 63, 2049, 64, 1025)          # per frame; frame 1 is empty between two that are not


@pytest.fixture(scope='module')
def seams():
    """Seven frames with SEAM_COUNTS candidates, each frame's split over up to three groups with their own zoom (1.3 among them),
    non-integer origins and interior bits; clusters of near-duplicates, a quarter of them exact duplicates with equal scores."""
    rng = np.random.default_rng(11)
    groups, parts, first = [], [], 0
    for f, n in enumerate(SEAM_COUNTS):
        cuts = sorted(rng.integers(0, n + 1, 2).tolist()) if n > 2 else [n, n]
        for k, count in enumerate((cuts[0], cuts[1] - cuts[0], n - cuts[1])):
            if count == 0 and k:
                continue
            ox, oy = float(rng.integers(0, 500)) + 0.3 * k, float(rng.integers(0, 500)) + 0.7 * (k == 2)
            groups.append(tm.group(f, first, count, ox=ox, oy=oy, zoom=(1.3, 1.0, 0.8)[k], rect=(ox, oy, ox + 900, oy + 900),
                                   interior=int(rng.integers(0, 16))))
            b, l, s = tm.clustered_candidates(rng, count, extent=1200.0 if n > 1000 else 300.0, exact=k == 1)
            parts.append((b, l, s))
            first += count
    boxes, lm, scores = (np.concatenate([p[k] for p in parts]) for k in range(3))
    return groups, boxes, lm, scores


@pytest.mark.parametrize('metric,edge,thr', [(0, 0.0, 0.4), (0, 40.0, 0.4), (1, 0.0, 0.5), (1, 25.0, 0.3)])
def test_merge_seams(ctx, seams, metric, edge, thr):
    groups, boxes, lm, scores = seams
    stats = {}
    counts = check(ctx, groups, len(SEAM_COUNTS), boxes, lm, scores, thr, metric, edge, stats)[0]
    print('metric %d edge %g: %s -> %s' % (metric, edge, stats, counts.tolist()))
    assert stats['candidates'] == sum(SEAM_COUNTS) and stats['suppressed'] > 100 and (stats['cut'] > 0) == (edge > 0)
    assert counts[1] == 0 and (counts[[0, 4, 6]] > 0).all()


def test_merge_in_batches_of_frames(ctx, seams, monkeypatch):
    """The matrices of a call are cut in batches of frames that fit a budget of scratch memory: with room for one frame's at a time
    the answer is the same."""
    groups, boxes, lm, scores = seams
    monkeypatch.setenv('TA_DM_MATRIX_BYTES', str(2049 * 33 * 8))
    check(ctx, groups, len(SEAM_COUNTS), boxes, lm, scores, 0.4)


def test_merge_exact_duplicates_keep_the_lowest_row(ctx):
    rng = np.random.default_rng(3)
    b, l, s = tm.clustered_candidates(rng, 300, extent=400.0, exact=True)
    groups = [tm.group(0, 0, 100), tm.group(0, 100, 50), tm.group(2, 150, 150)]
    counts, _, _, _, src = check(ctx, groups, 3, b, l, s, 0.4)
    assert counts[1] == 0 and counts[0] < 150 and counts[2] < 150
    for r in src:                                       # of equal boxes with equal scores in one frame, the first row stays
        f0 = r < 150
        same = np.nonzero((b == b[r]).all(axis=1) & (s == s[r]) & ((np.arange(300) < 150) == f0))[0]
        assert r == same.min()


def test_merge_threshold_is_strict(ctx):
    """Integer boxes whose overlap equals the threshold exactly stay both; a pair just above it loses its second."""
    boxes = np.array([[0, 0, 2, 2], [0, 0, 2, 1], [10, 0, 12, 2], [10, 0, 12, 1.5], [20, 0, 22, 2], [20, 0, 22, 1.0000001]], np.float32)
    assert boxes[5, 3] > 1
    scores = np.array([0.9, 0.8, 0.9, 0.8, 0.7, 0.6], np.float32)
    counts, _, _, _, src = check(ctx, [tm.group(0, 0, 6)], 1, boxes, np.zeros((6, 5, 2), np.float32), scores, 0.5)
    assert counts.tolist() == [4] and src.tolist() == [0, 2, 1, 4]


def test_merge_edge_rule_per_side(ctx):
    """Frame f takes bit f.  Rows 3 f, 3 f + 1: a box well inside and one pushed into the band of that side, in a group whose side is
    interior (the pushed one is dropped).  Row 3 f + 2: the pushed box again in a group where that side alone lies on the frame's
    border (kept; it overlaps the inside box by 0.32 at the most).  edge == 0 drops nothing: the two pushed boxes then meet in the NMS."""
    rect, edge = (100.0, 100.0, 200.0, 200.0), 10.0
    inside = [130, 130, 170, 170]
    pushed = {1: [105, 130, 145, 170], 2: [130, 109.5, 170, 149.5], 4: [155, 130, 190.5, 170], 8: [130, 155, 170, 195]}
    groups, boxes = [], []
    for f, bit in enumerate((1, 2, 4, 8)):
        groups += [tm.group(f, 3 * f, 2, rect=rect, interior=bit), tm.group(f, 3 * f + 2, 1, rect=rect, interior=15 - bit)]
        boxes += [inside, pushed[bit], pushed[bit]]
    boxes = np.array(boxes, np.float32)
    lm, scores = np.zeros((12, 5, 2), np.float32), np.linspace(0.9, 0.6, 12).astype(np.float32)
    stats = {}
    counts, _, _, _, src = check(ctx, groups, 4, boxes, lm, scores, 0.4, 0, edge, stats)
    assert counts.tolist() == [2, 2, 2, 2] and src.tolist() == [0, 2, 3, 5, 6, 8, 9, 11] and stats['cut'] == 4
    counts, _, _, _, src = check(ctx, groups, 4, boxes, lm, scores, 0.4, 0, 0.0)
    assert counts.tolist() == [2, 2, 2, 2] and src.tolist() == [0, 1, 3, 4, 6, 7, 9, 10]
    # exactly on the band's limit is not inside it: bx1 == x0 + edge stays
    on = np.array([[110, 130, 150, 170]], np.float32)
    assert check(ctx, [tm.group(0, 0, 1, rect=rect, interior=15)], 1, on, lm[:1], scores[:1], 0.4, 0, edge)[0].tolist() == [1]


def test_merge_ios_removes_a_box_inside_another(ctx):
    boxes = np.array([[0, 0, 100, 100], [40, 40, 50, 50]], np.float32)
    lm, scores = np.zeros((2, 5, 2), np.float32), np.array([0.9, 0.8], np.float32)
    assert check(ctx, [tm.group(0, 0, 2)], 1, boxes, lm, scores, 0.5, 0)[0].tolist() == [2]      # IoU 0.01
    assert check(ctx, [tm.group(0, 0, 2)], 1, boxes, lm, scores, 0.5, 1)[0].tolist() == [1]      # IoS 1


def raw_merge(ctx, groups, n_frames, boxes, lm, scores, thr, capacity, outputs=True):
    from terran_amd import lib
    g = tm.records(groups)
    counts = np.full(max(n_frames, 1), -1, np.int32)
    cap = max(capacity, 1)
    ob, ol = np.full((cap, 4), np.nan, np.float32), np.full((cap, 5, 2), np.nan, np.float32)
    osc, src = np.full(cap, np.nan, np.float32), np.full(cap, -1, np.int32)
    req = C.c_int32(-1)
    out = [lib.ptr(a) if outputs else None for a in (ob, ol, osc, src)]
    rc = ctx.lib.ta_detections_merge(ctx.h, lib.ptr(g) if len(g) else None, len(g), n_frames, lib.ptr(boxes), lib.ptr(lm), lib.ptr(scores),
                                     len(scores), float(thr), 0, 0.0, int(capacity), lib.ptr(counts), *out, C.byref(req))
    return rc, counts[:n_frames], ob, ol, osc, src, int(req.value)


def test_merge_capacity_protocol(ctx):
    from terran_amd import lib
    rng = np.random.default_rng(8)
    b, l, s = tm.clustered_candidates(rng, 200, extent=300.0)
    groups = [tm.group(0, 0, 120), tm.group(2, 120, 80)]
    want = tm.merge_model(groups, 3, b, l, s, 0.4)
    total = int(want[0].sum())
    rc, counts, ob, _, osc, _, required = raw_merge(ctx, groups, 3, b, l, s, 0.4, total - 1)
    assert rc == lib.E_CAPACITY and required == total and np.array_equal(counts, want[0])
    assert np.isnan(ob).all() and np.isnan(osc).all()                                 # nothing was written
    rc, counts, ob, ol, osc, src, required = raw_merge(ctx, groups, 3, b, l, s, 0.4, total)
    assert rc == lib.OK and required == total
    for a, w in zip((counts, ob, ol, osc, src), want):
        assert np.array_equal(a, w)
    rc, counts, _, _, _, _, required = raw_merge(ctx, groups, 3, b, l, s, 0.4, 0, outputs=False)
    assert rc == lib.E_CAPACITY and required == total and np.array_equal(counts, want[0])
    rc, counts, _, _, _, _, required = raw_merge(ctx, [], 3, b, l, s, 0.4, 0, outputs=False)   # nothing to merge
    assert rc == lib.OK and required == 0 and counts.tolist() == [0, 0, 0]


def test_merge_errors(ctx):
    from terran_amd import lib
    n = lib.MERGE_MAX_PER_FRAME + 1                      # the limit is checked on the host, before any launch
    b, l, s = np.zeros((n, 4), np.float32), np.zeros((n, 5, 2), np.float32), np.zeros(n, np.float32)
    with pytest.raises(lib.TerranAmdError, match=str(lib.MERGE_MAX_PER_FRAME)) as e:
        ctx.detections_merge(tm.records([tm.group(0, 0, n - 5), tm.group(0, n - 5, 5)]), 1, b, l, s, 0.4)
    assert e.value.code == lib.E_OVERFLOW
    for groups, what in (([tm.group(1, 0, 2), tm.group(0, 2, 2)], 'sorted'), ([tm.group(0, 0, 3), tm.group(0, 2, 2)], 'belongs to groups'),
                         ([tm.group(0, 0, 2, zoom=0.0)], 'zoom'), ([tm.group(2, 0, 2)], 'frame 2'), ([tm.group(0, 8, 3)], 'not inside')):
        with pytest.raises(lib.TerranAmdError, match=what) as e:
            ctx.detections_merge(tm.records(groups), 2, b[:10], l[:10], s[:10], 0.4)
        assert e.value.code == lib.E_INVALID
    with pytest.raises(lib.TerranAmdError, match='metric'):
        ctx.detections_merge(tm.records([tm.group(0, 0, 2)]), 1, b[:2], l[:2], s[:2], 0.4, metric=2)


# ---- end to end on painted heads -------------------------------------------------------------------------------------------------------
def painted_detector(ctx):
    """A RetinaFace whose network is the painted detector's program."""
    from terran_amd import lib
    from terran_amd.retinaface import RetinaFace
    det = RetinaFace.__new__(RetinaFace)
    det.device, det.lazy_results, det.precision, det.nms_threshold, det.ctx = 0, False, 'f32', 0.4, ctx
    det.model = lib.Model(ctx, dh.program())
    det._init_fallback('retinaface', None)
    return det


def paint_faces(seed, faces):
    """A 96 x 160 frame on which anchor 1 (the 16-pixel box) of the stride-8 cell at each (y, x) of `faces` scores exactly 0.5 -- a
    margin of 0 goes through expf(0) alone, so the device's score IS the reference's -- with the other anchor's byte `other`, which
    sets the box's x offset: the box is [x - 32 + other / 4, x - 17 + other / 4] x [y, y + 15]."""
    geo = dh.Geometry(96, 160)
    p = dh.Painter(geo, seed)
    for y, x, other in faces:
        p.set(geo.anchor(8, y // 8, x // 8, 1), 0)
        assert other < dh.FAIL_TOP
        p.fr[y, x, 2] = other                                                         # B: anchor 0 of the cell fails
    return p.fr


def test_detect_tiles_on_painted_heads(ctx):
    """Two frames of 96 x 160, tile 64, overlap 32 (origins y 0, 32; x 0, 32, 64, 96), edge 4.  Boxes are 15 x 15, so one lies wholly
    in every tile that holds its pixel unless it is within 4 pixels of an interior side.  Frame 0: a face in one tile only (pixel
    (8, 8)); one in the overlap of two tiles (8, 56: box x 38.75 .. 53.75, clear of x = 36 and x = 60) ; one in the overlap of four
    (40, 56); one whose box (x 22.75 .. 37.75 at pixel (8, 40)) is within the band of the left side of the tile at x = 32 and whole in
    the tile at x = 0.  Frame 1: the same kinds elsewhere, and two faces whose boxes (x 98 .. 113 from pixel (48, 120), x 102 .. 117
    from pixel (48, 128); IoU 11 / 19) survive in two DIFFERENT tiles, x = 64 and x = 96: equal scores, the lower row stays."""
    from terran_amd import tiles
    thr, nms, edge = 0.5, 0.4, 4.0
    fr = np.stack([paint_faces(1, [(8, 8, 59), (8, 56, 59), (40, 56, 59), (8, 40, 59)]),
                   paint_faces(2, [(72, 136, 59), (40, 104, 59), (48, 120, 40), (48, 128, 24), (16, 72, 59)])])
    origins = tiles.tile_grid(96, 160, 64, 32)
    assert origins.tolist() == [[y, x] for y in (0, 32) for x in (0, 32, 64, 96)]
    # the reference: the float64 heads of every cropped tile, the oracle's selection on them, then the model of the merge
    geo = dh.Geometry(64, 64)
    crops = np.stack([fr[f, y:y + 64, x:x + 64] for f in range(2) for y, x in origins])
    dets = dh.orp.postprocess(dh.reference_layout(dh.heads64(geo, crops)), 64, 64, thr, nms)
    tile_counts = [len(d) for d in dets]
    flat = [d for t in dets for d in t]
    boxes, lm, scores = (np.stack([d[k] for d in flat]) for k in ('bbox', 'landmarks', 'score'))
    assert (scores == np.float32(0.5)).all()
    groups = tiles.merge_groups(2, 96, 160, origins, 64, 64, 1.0, tile_counts)
    stats = {}
    want = tm.merge_model(groups, 2, boxes, lm, scores, nms, 0, edge, stats)
    print('painted tiles: %d candidates in %d tiles, %s -> %s' % (len(flat), len(dets), stats, want[0].tolist()))
    assert stats['cut'] >= 1 and stats['suppressed'] >= 3, stats                         # never vacuous
    assert want[0].tolist() == [4, 4]
    det = painted_detector(ctx)
    frames = ctx.upload(fr)
    try:
        got = det.detect_tiles(frames, 64, 32, 1.0, thr, None, edge, 'iou', max_tiles=5)    # four chunks: 5 + 5 + 5 + 1 tiles
        for a, b, what in zip(got, want[:4], NAMES):
            assert a.dtype == b.dtype and np.array_equal(a, b), what
    finally:
        frames.free()
        det.model.free()


# ---- the facade on the seeded network ----------------------------------------------------------------------------------------------------
FACADE_THRESHOLD = 0.5


def test_tiled_detection_equals_the_steps_by_hand(ctx, states):
    """Two frames of 160 x 224, tile 128, overlap 32, zoom 1.5, a whole-frame pass at short side 160.  Expected: the tiles cropped on
    the host, uploaded, resized and detected a chunk at a time with the calls `Detection` makes, the model of the merge, the rounding."""
    from terran_amd import TiledDetection, synth, tiles
    fr = synth.frames(21, 2, 160, 224)
    td = TiledDetection(tile=128, overlap=32, zoom=1.5, full_frame=True, short_side=160, device=0, state=states('retinaface'),
                        threshold=FACADE_THRESHOLD, max_tiles=5)
    mctx = td._ctx()
    model = td.model
    origins = tiles.tile_grid(160, 224, 128, 32)
    assert origins.tolist() == [[0, 0], [0, 96], [32, 0], [32, 96]]                   # step 96; eight tiles in chunks of 5 and 3
    crops = np.stack([fr[f, y:y + 128, x:x + 128] for f in range(2) for y, x in origins])
    parts = []
    for lo in range(0, len(crops), 5):
        up = mctx.upload(crops[lo:lo + 5])
        big = up.resize(int(128 * 1.5), int(128 * 1.5))
        parts.append(model.detect_arrays(big, FACADE_THRESHOLD))
        up.free(), big.free()
    tile_counts = np.concatenate([p[0] for p in parts])
    up = mctx.upload(fr)
    whole = up.resize(int(160 * (160 / 160)), int(224 * (160 / 160)))
    parts.append(model.detect_arrays(whole, FACADE_THRESHOLD))
    up.free(), whole.free()
    groups = tiles.merge_groups(2, 160, 224, origins, 128, 128, 1.5, tile_counts, parts[-1][0], 160 / 160)
    boxes, lm, scores = (np.concatenate([p[k] for p in parts]) for k in (1, 2, 3))
    stats = {}
    counts, wb, wl, ws, _ = tm.merge_model(groups, 2, boxes, lm, scores, model.nms_threshold, 0, 0.0, stats)
    print('seeded tiles: %s -> %s' % (stats, counts.tolist()))
    assert counts.sum() >= 5 and stats['suppressed'] >= 1
    wb, wl = np.around(wb).astype(np.int32), np.around(wl).astype(np.int32)
    for images in (fr, mctx.upload(fr), [fr[1], fr[0][:100], fr[0]]):
        got = td(images)
        if isinstance(images, list):
            assert len(got) == 3 and isinstance(got[1], list)
            got = [got[2], got[0]]                                                      # a mixed-size list answers in input order
        assert [len(g) for g in got] == counts.tolist()
        flat = [d for g in got for d in g]
        assert all(d['bbox'].dtype == np.int32 and d['landmarks'].dtype == np.int32 for d in flat)
        assert np.array_equal(np.stack([d['bbox'] for d in flat]), wb)
        assert np.array_equal(np.stack([d['landmarks'] for d in flat]), wl)
        assert np.array_equal(np.stack([d['score'] for d in flat]), ws)
    one = td(fr[0])
    assert len(one) == counts[0] and np.array_equal(np.stack([d['bbox'] for d in one]), wb[:counts[0]])


def test_one_tile_is_detect_arrays(ctx, states):
    """A frame no larger than one tile, zoom 1, no whole-frame pass: exactly what one detect_arrays call gives."""
    from terran_amd import TiledDetection, synth
    fr = synth.frames(22, 2, 120, 200)
    td = TiledDetection(tile=256, overlap=0.2, zoom=1.0, full_frame=False, device=0, state=states('retinaface'), threshold=FACADE_THRESHOLD)
    frames = td._ctx().upload(fr)
    try:
        want = td.model.detect_arrays(frames, FACADE_THRESHOLD)
        got = td.model.detect_tiles(frames, 256, 0.2, 1.0, FACADE_THRESHOLD)
        assert want[0].sum() >= 1
        for a, b, what in zip(got, want, NAMES):
            assert a.dtype == b.dtype and np.array_equal(a, b), what
        dicts = td(frames)
        assert [len(d) for d in dicts] == want[0].tolist()
        assert np.array_equal(np.stack([d['bbox'] for f in dicts for d in f]), np.around(want[1]).astype(np.int32))
    finally:
        frames.free()
