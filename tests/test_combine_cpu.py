"""No GPU: tests/combine_model.py (the contract of ta_frames_combine in numpy) against the recorded Pillow golden
(tests/golden/combine.npz) and, where Pillow is installed, against Pillow itself; the golden's power to tell the wrong
arithmetic from the right one; and the host halves of the callers: pack_combine, the clipping of paste_frames, the boxes
of composite_faces and the layout of inset_chips."""
import numpy as np
import pytest

from terran_amd import image, lib, vis
from tests import combine_model as M
from tests import tone_model as T


def _run(c, **wrong):
    dst = c['dst'].copy()
    src = dst if isinstance(c['src'], str) else c['src']
    mf = dst if isinstance(c['mask_frames'], str) else c['mask_frames']
    return M.combine_regions(dst, src, M.records(M.MODEL_DT, c['rows'], c['alpha']), c['masks'], mf, **wrong)


def test_binding_matches_the_model_columns():
    assert set(lib.COMBINE_DT.names) == set(M.MODEL_DT.names) and lib.COMBINE_DT.itemsize == 72
    assert [lib.COMBINE_OPS[n] for n in M.OP_NAMES] == list(range(14))
    assert (lib.MASK_NONE, lib.MASK_CONSTANT, lib.MASK_BITMAP, lib.MASK_FRAMES) == (0, 1, 2, 3)


def test_model_equals_the_golden():
    g = M.golden()
    assert str(g['pillow_version']) == '12.2.0'
    names = [str(n) for n in g['case_names']]
    assert len(names) == len(set(names)) >= 50
    for name in names:
        c = M.case(g, name)
        got = _run(c)
        assert np.array_equal(got, c['expected']), (name, int((got != c['expected']).any(-1).sum()))


def test_the_golden_tells_the_wrong_arithmetic_from_the_right_one():
    """The counts of pixels that paste as two MULDIV255s, add / subtract with a reciprocal multiply and blend with a fused
    multiply-add would change are recorded by the generator (its own emulation) and reproduced by the model here."""
    g = M.golden()
    seen = []
    for name in (str(n) for n in g['case_names']):
        _run(M.case(g, name), seen=seen)
    counts = M.wrong_counts(seen)
    assert counts == (int(g['count_paste_two_divisions']), int(g['count_add_reciprocal']), int(g['count_blend_fma']))
    assert min(counts) >= 1
    # and a whole case goes wrong under each of them
    right = {n: _run(M.case(g, n)) for n in ('mask_constant', 'ramp_add_1.7', 'blend_1.7')}
    assert not np.array_equal(_run(M.case(g, 'mask_constant'), paste=M.paste_two_divisions), right['mask_constant'])
    assert not np.array_equal(_run(M.case(g, 'ramp_add_1.7'), add_reciprocal=True), right['ramp_add_1.7'])
    assert not np.array_equal(_run(M.case(g, 'blend_1.7'), blend=T.blend_fused), right['blend_1.7'])


def test_the_golden_holds_the_shapes_the_kernel_can_go_wrong_at():
    cover = M.coverage(M.golden())
    assert cover['pairs'] == {(d, s) for d in range(4) for s in range(4)}
    assert cover['bitmap'] == {0, 1, 2, 3} and cover['mask_frames'] == {0, 1, 2, 3}
    assert cover['tails'] == {0, 1, 2, 3}
    assert {1, 3, 5, 53, 64, 257} <= cover['widths'] and {1, 2, 37} <= cover['heights']
    assert cover['ops'] == {(op, shape) for op in range(14) for shape in (0, 1)}
    assert cover['kinds'] == {(k, shape) for k in range(4) for shape in (0, 1)}
    assert cover['most_regions'] >= 40 and cover['other_size']


def test_model_equals_pillow_on_every_pair_of_samples():
    pytest.importorskip('PIL')
    from PIL import Image, ImageChops
    y, x = np.mgrid[:256, :256]
    a = np.stack([y, y, y], -1).astype(np.uint8)
    b = np.stack([x, x, 255 - x], -1).astype(np.uint8)
    ia, ib = Image.fromarray(a), Image.fromarray(b)
    for op in range(M.LIGHTER, M.OVERLAY + 1):
        if op in (M.ADD, M.SUBTRACT):
            continue
        want = np.asarray(getattr(ImageChops, M.OP_NAMES[op])(ia, ib))
        assert np.array_equal(M.chop(op, a, b), want), M.OP_NAMES[op]
    for scale, offset in ((1.0, 0), (1.7, -7), (3.0, -40), (0.3, 11), (-2.5, 100), (7.0, 0)):
        assert np.array_equal(M.chop(M.ADD, a, b, scale, offset), np.asarray(ImageChops.add(ia, ib, scale, offset))), (scale, offset)
        assert np.array_equal(M.chop(M.SUBTRACT, a, b, scale, offset), np.asarray(ImageChops.subtract(ia, ib, scale, offset))), (scale, offset)
    for alpha in (0.0, 0.3, 0.5, 0.999, 1.0, 1.2, 1.7, -0.5):
        assert np.array_equal(M.chop(M.BLEND, a, b, alpha), np.asarray(Image.blend(ia, ib, alpha))), alpha
    for m in (0, 1, 77, 128, 254, 255):
        out = ia.copy()
        out.paste(ib, (0, 0), Image.new('L', (256, 256), m))
        assert np.array_equal(M.paste_mask(a, b, np.int64(m)), np.asarray(out)), m
    rng = np.random.default_rng(3)
    mask = rng.integers(0, 256, (256, 256), dtype=np.uint8)
    assert np.array_equal(M.paste_mask(a, b, mask[..., None].astype(np.int64)), np.asarray(Image.composite(ib, ia, Image.fromarray(mask))))


def test_pack_combine_clips_as_paste_does():
    q, masks = image.pack_combine((3, 37, 53, 3), (1, 37, 53, 3), 'paste', (-5, 11))
    assert masks is None and len(q) == 3 and q['frame'].tolist() == [0, 1, 2] and q['src_frame'].tolist() == [0, 0, 0]
    assert [tuple(int(q[0][k]) for k in ('x0', 'y0', 'x1', 'y1', 'src_x', 'src_y'))] == [(0, 11, 48, 37, 5, 0)]
    q, _ = image.pack_combine((2, 20, 31, 3), (2, 37, 53, 3), 'paste', (40, -3), mask=90)
    assert len(q) == 0                                                       # the box lies right of the frame
    q, _ = image.pack_combine((2, 20, 31, 3), (2, 37, 53, 3), 'paste', (25, -3), mask=90)
    assert q['src_frame'].tolist() == [0, 1] and q['mask_kind'].tolist() == [1, 1] and q['mask_value'].tolist() == [90, 90]
    assert (int(q[1]['x0']), int(q[1]['y0']), int(q[1]['x1']), int(q[1]['y1']), int(q[1]['src_x']), int(q[1]['src_y'])) == (25, 0, 31, 20, 0, 3)
    # a bitmap is cropped like the piece, and packed once per distinct clipping
    bitmap = np.arange(12 * 17, dtype=np.uint8).reshape(12, 17)
    q, masks = image.pack_combine((3, 37, 53, 3), (1, 37, 53, 3), 'paste', [(45, 30, 62, 42), (45, 30, 62, 42), (2, 3, 19, 15)], (3, 2), bitmap)
    assert q['mask_value'].tolist() == [0, 0, 56] and len(masks) == 56 + 12 * 17
    assert np.array_equal(masks[:56].reshape(7, 8), bitmap[:7, :8]) and np.array_equal(masks[56:].reshape(12, 17), bitmap)
    assert (q['src_x'].tolist(), q['src_y'].tolist()) == ([3, 3, 3], [2, 2, 2])
    assert (q['x1'] - q['x0']).tolist() == [8, 8, 17]
    # a 4-tuple takes the piece's size from the box; a resident mask batch is read from its corner, shifted by the clipping
    q, _ = image.pack_combine((1, 37, 53, 3), (1, 41, 59, 3), 'paste', (-2, -1, 10, 9), (7, 5), (1, 41, 59, 3), mask_band=2)
    r = q[0]
    assert (r['x0'], r['y0'], r['x1'], r['y1'], r['src_x'], r['src_y'], r['mask_x'], r['mask_y'], r['mask_band']) == (0, 0, 10, 9, 9, 6, 2, 1, 2)
    q, _ = image.pack_combine((2, 8, 8, 3), (2, 8, 8, 3), 'add', alpha=1.7, offset=-3, shape='ellipse')
    assert q['op'].tolist() == [lib.COMBINE_ADD] * 2 and q['shape'].tolist() == [1, 1] and q['offset'].tolist() == [-3, -3]
    assert q['alpha'].tolist() == [np.float32(1.7)] * 2
    for bad in (dict(op='nope'), dict(op='add', alpha=0.0), dict(op='blend', alpha=np.nan), dict(op='blend', mask=3), dict(mask=256),
                dict(mask=np.zeros((3, 3), np.uint8)), dict(box=(0, 0, 0, 5)), dict(source=(50, 0), box=(0, 0, 9, 9)),
                dict(shape='disc'), dict(box=[(0, 0)] * 3), dict(mask=(3, 8, 8, 3))):
        with pytest.raises(ValueError):
            image.pack_combine((2, 37, 53, 3), (2, 37, 53, 3), **bad)
    with pytest.raises(ValueError):
        image.pack_combine((2, 37, 53, 3), (3, 37, 53, 3))


def test_pack_combine_agrees_with_the_model_on_the_caller_goldens():
    """paste_frames' clipping against Pillow's own: the records of pack_combine, applied by the model, give what Pillow's
    paste gave for a box that leaves the frame."""
    g = M.golden()
    one = g['one']
    for key, frames in (('a', g['pair']), ('b', g['small'])):
        for name, args in (('paste_corner', dict(box=(-5, 11))), ('paste_constant', dict(box=(40, -3), mask=90)),
                           ('paste_bitmap', dict(box=(45, 30, 62, 42), source=(3, 2), mask=np.array(g['call_bitmap'])))):
            q, masks = image.pack_combine(frames.shape, one.shape, 'paste', **args)
            got = M.combine_regions(frames.copy(), one, q, masks)
            assert np.array_equal(got, g['call_%s_%s' % (name, key)]), (name, key)


def test_composite_faces_boxes_and_inset_layout():
    g = M.golden()
    faces = [[], [], []]
    for f, box in zip(g['face_frames'], g['face_bboxes']):
        faces[f].append({'bbox': box})
    margin = float(g['face_margin'])
    batch = g['batch']
    other = np.ascontiguousarray(batch[::-1])
    for shape in ('box', 'ellipse'):
        for alpha, key in ((None, 'paste'), (0.4, 'alpha')):
            q = vis.pack_composite(faces, batch.shape, 3, margin, shape, alpha)
            blur = vis.pack_blur(faces, batch.shape, 1.0, margin, shape)
            assert all(np.array_equal(q[k], blur[k]) for k in ('frame', 'x0', 'y0', 'x1', 'y1', 'shape'))
            assert np.array_equal(q['src_frame'], q['frame']) and np.array_equal(q['src_x'], q['x0'])
            assert set(q['mask_value'].tolist()) == ({0} if alpha is None else {102})
            got = M.combine_regions(batch.copy(), other, q)
            assert np.array_equal(got, g['faces_%s_%s' % (shape, key)]), (shape, key)
    assert vis.pack_composite(faces, batch.shape, 1)['src_frame'].tolist() == [0] * 4
    with pytest.raises(ValueError):
        vis.pack_composite(faces, batch.shape, 3, alpha=1.5)
    # chips in rows of three; the seventh of frame 0 would start a third row that no longer fits
    chips, index = g['inset_chips'], g['inset_index']
    q = vis.pack_insets(index, chips.shape, batch.shape, origin=(3, 2), gap=2)
    want = [(k, int(index[k][0])) + tuple(int(v) for v in p) for k, p in enumerate(g['inset_places']) if p[0] >= 0]
    assert [(int(r['src_frame']), int(r['frame']), int(r['x0']), int(r['y0'])) for r in q] == want
    assert want == M.inset_layout(index, 14, 12, 37, 53, (3, 2), 2) and len(want) == 7
    assert np.array_equal(M.combine_regions(batch.copy(), chips, q), g['inset_expected'])
    assert len(vis.pack_insets(index, chips.shape, batch.shape, origin=(50, 2))) == 0      # no chip fits: none is pasted
    with pytest.raises(ValueError):
        vis.pack_insets(index[:3], chips.shape, batch.shape)
