"""-m gpu: the face-to-skeleton link.  ta_faces_poses_link against the model of tests/link_model.py with np.array_equal and no
tolerance anywhere: every edge of the predicate, the order and its ties, costs beyond 2^54, chains that take one round per link,
seeded crowds at the wave and workgroup seams in two frame orders and with the scratch matrix cut to one frame a batch, the
per-frame limit, every error, the empty cases; and link_faces_poses / head_boxes end to end behind the two networks."""
import ctypes as C

import numpy as np
import pytest

from tests import link_model as lm

pytestmark = pytest.mark.gpu

NAMES = ('pose_of_face', 'face_of_pose', 'links', 'rounds')


@pytest.fixture(scope='module')
def ctx():
    from terran_amd import lib
    c = lib.Context(0)
    yield c
    c.close()


def same(got, want):
    for a, b, what in zip(got, want, NAMES):
        if what == 'rounds':
            assert a == b, (what, a, b)
            continue
        assert a.dtype == b.dtype == np.int32 and a.shape == b.shape, (what, a.dtype, b.dtype, a.shape, b.shape)
        assert np.array_equal(a, b), (what, int(np.argmax(a != b)))


def check(ctx, fc, boxes, pc, kp, margin=250, min_inside=1, want=None):
    if want is None:
        want = lm.link_rounds_model(fc, boxes, pc, kp, margin, min_inside)
    got = ctx.faces_poses_link(fc, boxes, pc, kp, margin, min_inside)
    same(got, want)
    return got


def frames_of(pairs):
    """[(boxes of a frame, rows of a frame)] -> (face_counts, boxes, pose_counts, keypoints)."""
    fc, pc = [len(b) for b, _ in pairs], [len(k) for _, k in pairs]
    boxes = np.array([b for bs, _ in pairs for b in bs], np.int32).reshape(-1, 4)
    kp = np.array([k for _, ks in pairs for k in ks], np.int32).reshape(-1, 18, 3)
    return np.array(fc, np.int32), boxes, np.array(pc, np.int32), kp


# ---- edges of the predicate ----------------------------------------------------------------------------------------------------
BOX = (100, 200, 140, 260)              # w = 40, h = 60; 250 permille: mx = 10, my = 15 -> 90 .. 150 x 185 .. 275
NARROW = (10, 0, 17, 20)                # w = 7: mx = 7 * 250 / 1000 = 1 -> 9 .. 18
ABSENT_INSIDE = lm.pose_row({0: (300, 300)})
ABSENT_INSIDE[14] = (120, 230, 0)       # absent, with coordinates in the middle of BOX
# (box, joints or a ready row, linked at min_inside = 1?, linked at min_inside = 2?)
EDGES = [
    (BOX, {0: (90, 230)}, True, False), (BOX, {0: (89, 230)}, False, False),
    (BOX, {14: (150, 230)}, True, False), (BOX, {14: (151, 230)}, False, False),
    (BOX, {15: (120, 185)}, True, False), (BOX, {15: (120, 184)}, False, False),
    (BOX, {17: (120, 275)}, True, False), (BOX, {17: (120, 276)}, False, False),
    (NARROW, {0: (9, 10)}, True, False), (NARROW, {0: (8, 10)}, False, False),
    (NARROW, {16: (18, 10)}, True, False), (NARROW, {16: (19, 10)}, False, False),
    ((12, 3, 12, 9), {0: (12, 5)}, True, False), ((12, 3, 12, 9), {0: (13, 5)}, False, False),             # w = 0
    ((12, 3, 12, 3), {0: (12, 3)}, True, False),                                                           # w = h = 0
    ((17, 0, 10, 20), {0: (12, 3)}, False, False), ((10, 20, 17, 0), {0: (12, 3)}, False, False),          # x1 < x0; y1 < y0
    (BOX, {0: (120, 230), 14: (500, 230), 15: (500, 240)}, False, False),                                  # n = 3, inside = 1
    (BOX, {0: (120, 230), 14: (500, 230)}, True, False),                                                   # n = 2, inside = 1
    (BOX, {0: (120, 230), 14: (125, 230)}, True, True),                                                    # n = 2, inside = 2
    (BOX, {0: (120, 230), 14: (125, 230), 15: (115, 230), 16: (500, 0), 17: (500, 9)}, True, True),        # n = 5, inside = 3
    (BOX, {0: (120, 230), 14: (125, 230), 15: (500, 230), 16: (500, 0), 17: (500, 9)}, False, False),      # n = 5, inside = 2
    (BOX, ABSENT_INSIDE, False, False),                                                                    # only an absent joint is inside
    (BOX, {1: (120, 230), 2: (121, 231), 8: (119, 229)}, False, False),                                    # body joints are no head
]


@pytest.mark.parametrize('min_inside', [1, 2])
def test_edges_of_the_predicate(ctx, min_inside):
    rows = [j if isinstance(j, np.ndarray) else lm.pose_row(j) for _, j, _, _ in EDGES]
    fc, boxes, pc, kp = frames_of([([b], [r]) for (b, _, _, _), r in zip(EDGES, rows)])
    pof, fop, links, rounds = check(ctx, fc, boxes, pc, kp, 250, min_inside)
    expected = [e[1 + min_inside] for e in EDGES]
    assert (pof >= 0).tolist() == expected == (fop >= 0).tolist() == (links > 0).tolist()
    assert rounds == 2


def test_margin_truncates_and_reaches_its_limits(ctx):
    # 999 permille of w = 1 is 0; 1000 is 1; 4000 of w = 3 is 12
    cases = [((10, 10, 11, 11), (9, 10), 999, False), ((10, 10, 11, 11), (9, 10), 1000, True), ((10, 10, 13, 13), (-2, 25), 4000, True),
             ((10, 10, 13, 13), (-3, 25), 4000, False), ((10, 10, 13, 13), (10, 14), 0, False)]
    for box, at, margin, linked in cases:
        fc, boxes, pc, kp = frames_of([([box], [lm.pose_row({0: at})])])
        assert (check(ctx, fc, boxes, pc, kp, margin, 1)[0] >= 0).tolist() == [linked], (box, at, margin)


# ---- the order -------------------------------------------------------------------------------------------------------------------
def test_order_and_ties(ctx):
    sym = [lm.pose_row({0: (115, 230)}), lm.pose_row({0: (125, 230)})]           # equally far from the centre (120, 230)
    # one face, two poses of equal cost: the lower p; one pose, two faces of equal cost (the same box twice): the lower f;
    # both at once: f0 takes p0, f1 takes p1
    fc, boxes, pc, kp = frames_of([([BOX], sym), ([BOX, BOX], sym[:1]), ([BOX, BOX], sym), ([BOX], sym[::-1])])
    pof, fop, links, _ = check(ctx, fc, boxes, pc, kp)
    assert pof.tolist() == [0, 0, -1, 0, 1, 0] and fop.tolist() == [0, -1, 0, 0, 1, 0, -1] and links.tolist() == [1, 1, 2, 1]
    # n = 1 .. 5 joints, all of pose n at distance 12 - n from the centre: S = 4 n (12 - n)^2 is smallest for n = 1, the cost
    # 240 (12 - n)^2 for n = 5
    poses = [lm.pose_row({j: (120 + 12 - n, 230) for j in lm.HEAD[:n]}) for n in range(1, 6)]
    s = [sum((2 * x - 240) ** 2 + (2 * y - 460) ** 2 for x, y in lm.head_joints(r)) for r in poses]
    assert int(np.argmin(s)) == 0 and int(np.argmin([v * (60 // n) for n, v in enumerate(s, 1)])) == 4
    fc, boxes, pc, kp = frames_of([([BOX], poses), ([BOX] * 5, poses)])
    pof, fop, _, _ = check(ctx, fc, boxes, pc, kp)
    assert pof.tolist() == [4, 4, 3, 2, 1, 0]


def test_costs_beyond_32_bits_and_beyond_float32(ctx):
    """Coordinates just below 2^22: a small box in one corner, 4000 permille, two single-nose skeletons in the opposite corner.
    Their costs, 60 S, lie above 2^54 and differ by 480, the least two such neighbours differ by; the cheaper one has the HIGHER
    index, so any tie links the wrong one.  Restated in the test: float32 ties them, and int32 arithmetic wraps a third skeleton,
    cheaper than both, to a larger number, so the case bites on both.  float64 does NOT tie them, and cannot: below the coordinate bound every cost is a multiple
    of 4 under 2^55 -- (2x - cx)^2 = cx^2 mod 4, so S = n (cx^2 + cy^2) mod 4 and S (60 / n) = 0 mod 4 for every n -- hence
    representable, and distinct costs are at least 12 apart.  The figures are printed; the kernel keeps int64 throughout."""
    L = (1 << 22) - 1
    w = 1677721
    box = (-L, -L, -L + w, -L + w)
    hi = -L + 5 * w                                     # the far side of the widened box
    assert hi == L - 1
    a, b = (hi - 37, hi - 39), (hi - 38, hi - 38)       # b is the cheaper
    cx = cy = -2 * L + w
    cost = [60 * ((2 * x - cx) ** 2 + (2 * y - cy) ** 2) for x, y in (a, b)]
    assert cost[1] < cost[0] and cost[0] - cost[1] == 480 and cost[1] > 1 << 54
    f32 = [np.float32(60) * (np.float32(2 * x - cx) ** 2 + np.float32(2 * y - cy) ** 2) for x, y in (a, b)]
    f64 = [60.0 * (float(2 * x - cx) ** 2 + float(2 * y - cy) ** 2) for x, y in (a, b)]
    wrap = lambda v: (int(v) + (1 << 31)) % (1 << 32) - (1 << 31)
    c = (hi - 105, hi - 105)                            # cheaper than both
    cost.append(60 * ((2 * c[0] - cx) ** 2 + (2 * c[1] - cy) ** 2))
    i32 = [wrap(60 * wrap(wrap((2 * x - cx) ** 2) + wrap((2 * y - cy) ** 2))) for x, y in (a, b, c)]
    print('costs', cost, 'float32', f32, 'float64', f64, 'int32', i32)
    assert f32[0] == f32[1]                             # would link pose 0 of (a, b)
    assert 1 << 54 < cost[2] < cost[1] and i32[2] > i32[1]      # would link pose 0 of (b, c)
    assert f64[1] < f64[0]                              # see above
    fc, boxes, pc, kp = frames_of([([box], [lm.pose_row({0: a}), lm.pose_row({0: b})]), ([box], [lm.pose_row({0: b}), lm.pose_row({0: c})]),
                                   ([box, box], [lm.pose_row({0: a}), lm.pose_row({0: b}), lm.pose_row({0: (L, L)})])])
    pof, fop, _, _ = check(ctx, fc, boxes, pc, kp, 4000, 1)
    assert pof.tolist() == [1, 1, 1, 0] and fop.tolist() == [-1, 0, -1, 0, 1, 0, -1]
    # the mirror image, at the negative end of the range
    fc, boxes, pc, kp = frames_of([([tuple(-v for v in box[2:] + box[:2])], [lm.pose_row({0: (-a[0], -a[1])}), lm.pose_row({0: (-b[0], -b[1])})])])
    assert check(ctx, fc, boxes, pc, kp, 4000, 1)[0].tolist() == [1]


# ---- chains ------------------------------------------------------------------------------------------------------------------------
def test_chains_take_one_round_per_link(ctx):
    lengths = (1, 63, 64, 65, 257)
    fc, boxes, pc, kp = frames_of([lm.chain(n, x_at=-1000 * k, y_at=3 * k) for k, n in enumerate(lengths)])
    want = lm.link_rounds_model(fc, boxes, pc, kp, 0, 1)
    assert want[3] == 258 and want[2].tolist() == list(lengths)
    pof, _, _, rounds = check(ctx, fc, boxes, pc, kp, 0, 1, want)
    assert rounds == 258 and pof.tolist() == [i for n in lengths for i in range(n)]


# ---- seeded crowds -----------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def crowd():
    call = lm.crowd_call()
    want = lm.link_rounds_model(*call)
    per_frame = [lm.link_rounds_model(call[0][k:k + 1], call[1][a:a + n], call[2][k:k + 1], call[3][b:b + m])
                 for k, (a, n, b, m) in enumerate(zip(np.cumsum(call[0]) - call[0], call[0], np.cumsum(call[2]) - call[2], call[2]))]
    return call, want, per_frame


def test_crowds(ctx, crowd):
    call, want, per_frame = crowd
    assert call[0].tolist() == list(lm.CROWD_FACES) and call[2].tolist() == list(lm.CROWD_FACES[::-1])
    q = lm.qualifying_per_face(*call)
    assert (q >= 2).sum() * 4 >= len(q) and max(r[3] for r in per_frame) >= 3
    walk = lm.link_model(*call)
    assert all(np.array_equal(a, b) for a, b in zip(walk, want[:3]))
    check(ctx, *call, want=want)
    # the same frames in another order: every frame's own answer
    order = [7, 2, 5, 0, 3, 6, 1, 4]
    got = ctx.faces_poses_link(*lm.reorder(*call, order))
    fo, po = np.concatenate([[0], np.cumsum(call[0][order])]), np.concatenate([[0], np.cumsum(call[2][order])])
    for slot, k in enumerate(order):
        same((got[0][fo[slot]:fo[slot + 1]], got[1][po[slot]:po[slot + 1]], got[2][slot:slot + 1]), per_frame[k][:3])
    assert got[3] == want[3]
    # other parameters on the same frames
    for margin, min_inside in ((0, 1), (1000, 3), (4000, 5)):
        check(ctx, *call, margin, min_inside)


def test_crowds_one_frame_per_scratch_batch(ctx, crowd, monkeypatch):
    """Any frame's matrices alone exceed 8 bytes, so every frame is its own batch."""
    call, want, _ = crowd
    monkeypatch.setenv('TA_FL_MATRIX_BYTES', '8')
    check(ctx, *call, want=want)
    monkeypatch.setenv('TA_FL_MATRIX_BYTES', '4096')    # and a few frames a batch
    check(ctx, *call, want=want)


# ---- the limit -----------------------------------------------------------------------------------------------------------------------
def raw_link(ctx, fc, boxes, nf, pc, kp, npose, margin=250, min_inside=1, outputs=True):
    from terran_amd import lib
    p = lambda a: lib.ptr(a) if a is not None and len(a) else None
    pof, fop = np.full(max(nf, 1), -7, np.int32), np.full(max(npose, 1), -7, np.int32)
    links, rounds = np.full(max(len(fc), 1), -7, np.int32), C.c_int32(-7)
    rc = ctx.lib.ta_faces_poses_link(ctx.h, len(fc), p(fc), p(boxes), nf, p(pc), p(kp), npose, margin, min_inside,
                                     lib.ptr(pof) if outputs else None, lib.ptr(fop) if outputs else None, lib.ptr(links), C.byref(rounds))
    return rc, pof, fop, links, int(rounds.value)


def test_the_limit_per_frame(ctx):
    from terran_amd import lib
    n = lib.LINK_MAX_PER_FRAME
    assert n == lm.MAX_PER_FRAME == 16384
    rng = np.random.default_rng(5)
    many_boxes, few_kp = lm.crowd(rng, n, 4, extent=2048, box=(300, 900))
    few_boxes, many_kp = lm.crowd(rng, 4, n, extent=2048, box=(300, 900))
    fc, pc = np.array([n, 4], np.int32), np.array([4, n], np.int32)
    boxes, kp = np.concatenate([many_boxes, few_boxes]), np.concatenate([few_kp, many_kp])
    pof, fop, links, _ = check(ctx, fc, boxes, pc, kp)
    assert links.tolist() == [4, 4]
    for fc1, pc1 in (((n + 1,), (4,)), ((4,), (n + 1,))):
        fc1, pc1 = np.array(fc1, np.int32), np.array(pc1, np.int32)
        b1, k1 = np.zeros((fc1[0], 4), np.int32), np.zeros((pc1[0], 18, 3), np.int32)
        rc, pof, fop, links, rounds = raw_link(ctx, fc1, b1, len(b1), pc1, k1, len(k1))
        assert rc == lib.E_OVERFLOW and '16384' in ctx.last_error()
        assert (pof == -7).all() and (fop == -7).all() and (links == -7).all() and rounds == -7      # checked before any launch


# ---- errors and empty cases ------------------------------------------------------------------------------------------------------------
def test_errors(ctx):
    from terran_amd import lib
    fc, pc = np.array([2, 1], np.int32), np.array([1, 3], np.int32)
    boxes, kp = np.zeros((3, 4), np.int32), np.zeros((4, 18, 3), np.int32)
    kp[:, :, 2] = 1
    big, small = 1 << 22, -(1 << 22)

    def wild(arr, index, value):
        out = arr.copy()
        out[index] = value
        return out

    cases = [
        (dict(fc=np.array([-1, 4], np.int32)), 'negative'), (dict(pc=np.array([5, -1], np.int32)), 'negative'),
        (dict(fc=np.array([2, 2], np.int32)), 'sum'), (dict(pc=np.array([1, 2], np.int32)), 'sum'), (dict(nf=4), 'sum'), (dict(npose=3), 'sum'),
        (dict(boxes=None), 'null'), (dict(kp=None), 'null'), (dict(outputs=False), 'null'),
        (dict(margin=-1), 'margin_permille'), (dict(margin=4001), 'margin_permille'), (dict(min_inside=0), 'min_inside'), (dict(min_inside=6), 'min_inside'),
        (dict(boxes=wild(boxes, (2, 0), big)), 'face row 2'), (dict(boxes=wild(boxes, (1, 3), small)), 'face row 1'),
        (dict(kp=wild(kp, (3, 0, 0), big)), 'pose row 3'), (dict(kp=wild(kp, (0, 17, 1), small)), 'pose row 0'),
        (dict(kp=wild(kp, (2, 9, 1), big)), 'pose row 2'),                                     # a body joint counts too
        (dict(kp=wild(wild(kp, (1, 14, 2), 0), (1, 14, 0), big)), 'pose row 1'),               # and so does an absent joint
    ]
    for change, what in cases:
        a = dict(fc=fc, boxes=boxes, nf=3, pc=pc, kp=kp, npose=4, margin=250, min_inside=1, outputs=True)
        a.update(change)
        rc, pof, fop, links, rounds = raw_link(ctx, a['fc'], a['boxes'], a['nf'], a['pc'], a['kp'], a['npose'], a['margin'], a['min_inside'], a['outputs'])
        assert rc == lib.E_INVALID and what in ctx.last_error(), (what, rc, ctx.last_error())
        assert (pof == -7).all() and (fop == -7).all() and (links == -7).all() and rounds == -7
    # the bound itself is 2^22 - 1 in size, and the third value of a joint is free
    ok_kp = wild(wild(kp, (3, 0, 0), big - 1), (0, 17, 1), small + 1)
    ok_kp[2, 5, 2] = big
    check(ctx, fc, wild(boxes, (2, 0), small + 1), pc, ok_kp)
    with pytest.raises(lib.TerranAmdError) as e:
        ctx.faces_poses_link(fc, boxes, pc, kp, 250, 9)
    assert e.value.code == lib.E_INVALID
    with pytest.raises(ValueError, match='counts'):
        ctx.faces_poses_link(fc, boxes, pc[:1], kp)


def test_empty_cases(ctx):
    from terran_amd import lib
    none = np.zeros(0, np.int32)
    pof, fop, links, rounds = ctx.faces_poses_link(none, none.reshape(0, 4), none, none.reshape(0, 18, 3))
    assert len(pof) == len(fop) == len(links) == 0 and rounds == 0
    rc, _, _, _, rounds = raw_link(ctx, none, None, 0, none, None, 0, outputs=False)
    assert rc == lib.OK and rounds == 0
    boxes, kp = np.array([BOX] * 3, np.int32), np.stack([lm.pose_row({0: (120, 230)})] * 2)
    # faces and no pose at all; poses and no face at all: nothing is launched
    same(ctx.faces_poses_link([3], boxes, [0], kp[:0]), lm.link_rounds_model([3], boxes, [0], kp[:0]))
    same(ctx.faces_poses_link([0, 0], boxes[:0], [1, 1], kp), lm.link_rounds_model([0, 0], boxes[:0], [1, 1], kp))
    # frames with faces but no poses, and the reverse, beside a frame that has both
    pof, fop, links, rounds = check(ctx, [3, 0, 1, 0], np.concatenate([boxes, boxes[:1]]), [0, 2, 1, 0], np.concatenate([kp, kp[:1]]))
    assert pof.tolist() == [-1, -1, -1, 0] and fop.tolist() == [-1, -1, 0] and links.tolist() == [0, 0, 1, 0] and rounds == 2
    assert ctx.faces_poses_link([3], boxes, [2], np.zeros((2, 18, 3), np.int32))[3] == 1      # nothing qualifies: the silent round only


# ---- end to end --------------------------------------------------------------------------------------------------------------------------
def test_end_to_end_behind_the_two_networks(states):
    """Coded frames (the decoder weights assemble people on them; the plain seeded pose network assembles nobody) through Detection
    and Estimation on the seeded weights, then link_faces_poses.  Whatever the seeded detector finds is acceptable; on these two
    frames the CPU oracle gives 16 and 19 faces, 4 and 3 people and 1 and 3 links, so the link is not empty."""
    from terran_amd import Detection, Estimation, link_faces_poses, head_boxes, runtime, synth, vis
    rctx = runtime.get_context(0)
    fr = synth.upscale_for_resize(synth.pose_code_frames(60, 2, 96, 128, 3), 288, 384)
    faces = Detection(short_side=128, device=0, state=states('retinaface'))(fr)
    poses = Estimation(short_side=96, device=0, state=states('openpose_decoder'))(fr)
    assert len(faces) == len(poses) == 2 and sum(map(len, poses)) >= 3 and sum(map(len, faces)) >= 3
    fc, pc = [len(v) for v in faces], [len(v) for v in poses]
    boxes = np.array([f['bbox'] for v in faces for f in v], np.int32).reshape(-1, 4)
    kp = np.array([p['keypoints'] for v in poses for p in v], np.int32).reshape(-1, 18, 3)
    want = lm.link_model(fc, boxes, pc, kp, 250, 1)
    print('faces', fc, 'poses', pc, 'links', want[2].tolist())
    assert want[2].sum() >= 1
    flat_faces = [f for v in faces for f in v]
    first = int(np.argmax(want[0] >= 0))                 # a face that will link: its name must arrive on its skeleton
    frame = int(np.searchsorted(np.cumsum(fc), first, side='right'))
    flat_faces[first]['text'] = 'ada'
    poses[-1][-1]['face'] = 99                           # stale, whether it links or not
    got = link_faces_poses(faces, poses, device=0)
    assert np.array_equal(np.concatenate(got), want[0]) and all(g.dtype == np.int32 for g in got)
    assert [f.get('pose', -1) for f in flat_faces] == want[0].tolist()
    assert [p.get('face', -1) for v in poses for p in v] == want[1].tolist()
    for fl, pl in zip(faces, poses):
        assert all(pl[f['pose']]['face'] == k for k, f in enumerate(fl) if 'pose' in f)
        assert all(fl[p['face']]['pose'] == k for k, p in enumerate(pl) if 'face' in p)
    assert [p is poses[frame][want[0][first]] for v in poses for p in v if p.get('text') == 'ada'] == [True]
    assert np.array_equal(link_faces_poses(faces[0], poses[0], device=0), got[0])      # the single-image form
    # the people whose face was not found, blurred through their head boxes: nothing else changes
    every, heads = head_boxes(poses), head_boxes(poses, only_unlinked=True)
    assert [[d['pose'] for d in v] for v in heads] == [[d['pose'] for d in v if 'face' not in pl[d['pose']]] for v, pl in zip(every, poses)]
    shown = heads if sum(map(len, heads)) else every
    assert sum(map(len, shown)) >= 1
    up = rctx.upload(fr)
    try:
        out = vis.blur_faces(up, shown).download()
    finally:
        up.free()
    changed = (out != fr).any(-1)
    allowed = np.zeros_like(changed)
    for k, v in enumerate(shown):
        for d in v:
            x0, y0, x1, y1 = (max(int(c), 0) for c in d['bbox'])
            allowed[k, y0:y1, x0:x1] = True
    assert changed.any() and not (changed & ~allowed).any()
