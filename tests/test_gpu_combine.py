"""-m gpu: ta_frames_combine and the two-image callers of terran_amd.image and terran_amd.vis against the recorded Pillow
golden (tests/golden/combine.npz), bit for bit over whole frames, so a pixel outside every region is checked too.  Reads
no Pillow and no reference.

The shapes are the ones csrc/combine.hip can go wrong at.  The destination row is walked as a head of 0 .. 3 single pixels,
groups of four pixels and a tail of 0 .. 3, and a group aligns its source's and its mask's bytes out of the dwords that
cover them: so widths 1, 3, 5 (no group at all), 53, 64, 257 and heights 1, 2, 37; all 16 pairs of (destination, source)
address mod 4 and every mask address mod 4 for bitmaps and mask batches; a source of another size and batch length; a
last group that ends at the last byte of its source batch at every alignment (the covering dwords must stay inside the
allocation); every op and mask kind under both shapes; 40 overlapping regions in one call.  That the golden's regions reach
all of them is asserted from the regions themselves."""
import numpy as np
import pytest

from terran_amd import image, lib, runtime, vis
from tests import combine_model as M

pytestmark = pytest.mark.gpu

GROUPS = ['size', 'op', 'mask', 'align', 'tail', 'ramp', 'blend', 'many', 'self']


def _differing(got, want):
    return [int((g != w).any(-1).sum()) for g, w in zip(got, want)]


class _resident:
    """Host frames uploaded for the length of a `with`, freed afterwards."""

    def __init__(self, *hosts):
        self.hosts = hosts

    def __enter__(self):
        ctx = runtime.get_context(0)
        self.frames = [ctx.upload(np.ascontiguousarray(h)) for h in self.hosts]
        return self.frames if len(self.frames) > 1 else self.frames[0]

    def __exit__(self, *exc):
        for f in self.frames:
            f.free()


def _run_case(c, ctx=None):
    hosts = [c['dst']] + [c[k] for k in ('src', 'mask_frames') if isinstance(c[k], np.ndarray)]
    with _resident(*hosts) as up:
        up = up if isinstance(up, list) else [up]
        dst, rest = up[0], up[1:]
        src = dst if isinstance(c['src'], str) else rest.pop(0)
        mf = dst if isinstance(c['mask_frames'], str) else rest.pop(0) if c['mask_frames'] is not None else None
        dst.combine(src, M.records(lib.COMBINE_DT, c['rows'], c['alpha']), c['masks'], mask_frames=mf, ctx=ctx)
        return dst.download()


@pytest.mark.parametrize('group', GROUPS)
def test_combine_equals_the_golden(group):
    g = M.golden()
    names = [str(n) for n in g['case_names']]
    assert {n.split('_')[0] for n in names} == set(GROUPS)
    mine = [n for n in names if n.split('_')[0] == group]
    assert mine
    for name in mine:
        c = M.case(g, name)
        got = _run_case(c)
        assert np.array_equal(got, c['expected']), (name, _differing(got, c['expected']))
    if group == 'op':                                                        # the 1 x 1 ellipse changes nothing
        assert np.array_equal(g['case_op_paste_expected'][0, 36, 52], g['one'][0, 36, 52])
        assert {'op_' + n for n in M.OP_NAMES} <= set(mine)
    if group == 'mask':
        assert {'mask_constant', 'mask_bitmap', 'mask_frames'} <= set(mine)
    if group == 'ramp':
        assert {'ramp_%s_%s' % (o, s) for o in ('add', 'subtract') for s in ('1', '1.7', '3')} <= set(mine)
        assert (g['case_ramp_add_1.7_rows'][:, M.COLUMNS.index('offset')] < 0).all()
        a, b = (x.astype(int) for x in M.ramp_pair())
        assert set(range(511)) <= set((a + b).ravel().tolist()) and set(range(-255, 256)) <= set((a - b).ravel().tolist())
    if group == 'blend':
        assert {'blend_%g' % a for a in (0.3, 0.5, 1.7, -0.5)} <= set(mine)
    if group == 'self':                                                      # the frame that is read stays as it was
        assert np.array_equal(got[1], g['batch'][1]) and isinstance(M.case(g, 'self')['src'], str)


def test_the_golden_reaches_every_alignment_shape_op_and_mask_kind():
    g = M.golden()
    cover = M.coverage(g)
    assert cover['pairs'] == {(d, s) for d in range(4) for s in range(4)}
    assert cover['bitmap'] == {0, 1, 2, 3} and cover['mask_frames'] == {0, 1, 2, 3}
    assert cover['tails'] == {0, 1, 2, 3}
    assert {1, 3, 5, 53, 64, 257} <= cover['widths'] and {1, 2, 37} <= cover['heights']
    assert cover['ops'] == {(op, shape) for op in range(14) for shape in (0, 1)}
    assert cover['kinds'] == {(k, shape) for k in range(4) for shape in (0, 1)}
    assert cover['most_regions'] >= 40 and cover['other_size']
    # the inputs tell the wrong arithmetic from the right one
    assert min(int(g['count_paste_two_divisions']), int(g['count_add_reciprocal']), int(g['count_blend_fma'])) >= 1
    rows = g['case_many_rows']
    assert rows[:3, 0].tolist() == [2, 0, 1]
    shared = rows[rows[:, M.COLUMNS.index('mask_kind')] == M.MASK_BITMAP][:, M.COLUMNS.index('mask_value')]
    assert len(set(shared.tolist())) >= 3 and len(shared) >= 2 * len(set(shared.tolist()))


def _three(bad=None, **fields):
    """[good, bad, good]: the middle region is a good one with `fields` changed."""
    q = np.zeros(3, lib.COMBINE_DT)
    for k, (f, x0, y0, x1, y1, sf, sx, sy, op) in enumerate([(0, 1, 1, 11, 9, 0, 0, 0, lib.COMBINE_PASTE), (1, 2, 2, 12, 10, 1, 4, 4, lib.COMBINE_PASTE),
                                                             (2, 5, 5, 20, 20, 1, 3, 3, lib.COMBINE_DIFFERENCE)]):
        r = q[k]
        r['frame'], r['x0'], r['y0'], r['x1'], r['y1'], r['src_frame'], r['src_x'], r['src_y'], r['op'] = f, x0, y0, x1, y1, sf, sx, sy, op
    q['alpha'] = 1.0
    for name, v in fields.items():
        q[name][1] = v
    return q


FRAMES_MASK = dict(mask_kind=lib.MASK_FRAMES, mask_frame=1, mask_x=3, mask_y=3, mask_band=1)
INVALID = [
    # what ta_check_regions refuses
    dict(frame=3), dict(frame=-1), dict(x1=2), dict(y1=1), dict(x0=-1), dict(x1=54), dict(y1=38), dict(y0=-2), dict(shape=2), dict(shape=-1),
    # a source or mask box not inside its frame, a frame index out of range
    dict(src_x=50), dict(src_y=34), dict(src_x=-1), dict(src_y=-1), dict(src_frame=2), dict(src_frame=-1),
    dict(FRAMES_MASK, mask_x=50), dict(FRAMES_MASK, mask_y=-1), dict(FRAMES_MASK, mask_frame=2), dict(FRAMES_MASK, mask_frame=-1),
    # an unknown op or mask kind, a mask on another op
    dict(op=14), dict(op=-1), dict(mask_kind=4), dict(mask_kind=-1), dict(op=lib.COMBINE_BLEND, mask_kind=lib.MASK_CONSTANT, mask_value=9),
    # alpha / scale
    dict(op=lib.COMBINE_BLEND, alpha=np.nan), dict(op=lib.COMBINE_ADD, alpha=np.inf), dict(op=lib.COMBINE_SUBTRACT, alpha=-np.inf),
    dict(op=lib.COMBINE_ADD, alpha=0.0), dict(op=lib.COMBINE_SUBTRACT, alpha=0.0),
    # mask values
    dict(FRAMES_MASK, mask_band=3), dict(FRAMES_MASK, mask_band=-1), dict(mask_kind=lib.MASK_CONSTANT, mask_value=256),
    dict(mask_kind=lib.MASK_BITMAP, mask_value=121), dict(mask_kind=lib.MASK_BITMAP, mask_value=-1),
]


def test_invalid_regions_are_named_before_any_pixel_changes():
    g = M.golden()
    host = g['batch']
    ctx = runtime.get_context(0)
    masks = np.arange(200, dtype=np.uint8)                                   # a 10 x 8 bitmap fits up to offset 120
    with _resident(host, g['src_big'], M.matte(2, 41, 59)) as (dst, src, mattes):
        def call(q, src=src, mattes=mattes, masks=masks):
            return ctx.lib.ta_frames_combine(ctx.h, dst.h, src.h, mattes.h if mattes is not None else None, lib.ptr(q), len(q),
                                             lib.ptr(masks) if masks is not None else None, len(masks) if masks is not None else 0)

        def refused(rc, what):
            assert rc == lib.E_INVALID and b'region 1' in ctx.lib.ta_last_error(ctx.h), (what, ctx.lib.ta_last_error(ctx.h))
            assert np.array_equal(dst.download(), host), what
        for fields in INVALID:
            refused(call(_three(**fields)), fields)
        # masks or mask_frames NULL where a region needs them
        refused(call(_three(mask_kind=lib.MASK_BITMAP, mask_value=0), masks=None), 'masks NULL')
        refused(call(_three(**FRAMES_MASK), mattes=None), 'mask_frames NULL')
        # a frame both written and read: dst as src, dst as mask batch
        q = _three(frame=2, src_frame=0, src_x=0, src_y=0)
        q['frame'][2], q['src_frame'][0], q['src_frame'][2], q['op'][2] = 0, 1, 1, lib.COMBINE_PASTE
        refused(call(q, src=dst), 'dst as src')
        q = _three(frame=2, mask_kind=lib.MASK_FRAMES, mask_frame=0)
        q['frame'][2] = 0
        refused(call(q, mattes=dst), 'dst as mask batch')
        # the valid neighbours of all these: the bitmap that just fits, n = 0, and the three good regions themselves
        assert call(_three()[:0]) == lib.OK and np.array_equal(dst.download(), host)
        assert call(_three(mask_kind=lib.MASK_BITMAP, mask_value=120)) == lib.OK
        with pytest.raises(lib.TerranAmdError) as e:
            dst.combine(src, _three(op=99))
        assert e.value.code == lib.E_INVALID and 'region 1' in str(e.value)


def test_the_callers_own_context_and_a_second_call():
    g = M.golden()
    c = M.case(g, 'many')
    other = runtime.new_context(0)                                           # the caller's context, as in blur
    got = _run_case(c, ctx=other)
    assert np.array_equal(got, c['expected']), _differing(got, c['expected'])
    with _resident(g['batch']) as frames:
        copy = image.copy_frames(frames, ctx=other)
        assert copy is not frames and copy.shape == frames.shape and np.array_equal(copy.download(), g['batch'])
        image.difference_frames(copy, frames)
        assert not copy.download().any() and np.array_equal(frames.download(), g['batch'])
        copy.free()


def test_a_one_frame_other_is_applied_to_every_frame():
    g = M.golden()
    with _resident(g['batch'], g['one']) as (frames, one):
        assert image.blend_frames(frames, one, 0.25) is frames
        assert np.array_equal(frames.download(), g['call_blend_one'])
    with _resident(g['batch'], g['one']) as (frames, one):
        image.difference_frames(frames, one)
        assert np.array_equal(frames.download(), g['call_difference_one'])
        with pytest.raises(ValueError):
            image.blend_frames(frames, frames, np.nan)
    # boxes and the ellipse shape, against the model
    boxes = np.array([(3, 2, 41, 30), (0, 0, 53, 1), (30, 19, 31, 20)])
    with _resident(g['batch'], g['one']) as (frames, one):
        image.chop_frames(frames, one, 'multiply', boxes=boxes, shape='ellipse')
        q, _ = image.pack_combine(frames.shape, one.shape, 'multiply', boxes, boxes[:, :2], shape='ellipse')
        assert np.array_equal(frames.download(), M.combine_regions(g['batch'].copy(), g['one'], q))
        with pytest.raises(ValueError):
            image.chop_frames(frames, one, 'paste')


CALLS = {'difference': lambda f, o, m, one, bm: image.difference_frames(f, o),
         'composite': lambda f, o, m, one, bm: image.composite_frames(f, o, m),
         'screen': lambda f, o, m, one, bm: image.chop_frames(f, o, 'screen'),
         'add': lambda f, o, m, one, bm: image.chop_frames(f, o, 'add', 1.7, -5),
         'blend': lambda f, o, m, one, bm: image.blend_frames(f, o, 1.7),
         'paste_corner': lambda f, o, m, one, bm: image.paste_frames(f, one, (-5, 11)),
         'paste_constant': lambda f, o, m, one, bm: image.paste_frames(f, one, (40, -3), 90),
         'paste_bitmap': lambda f, o, m, one, bm: image.paste_frames(f, one, (45, 30, 62, 42), bm, source=(3, 2))}


@pytest.mark.parametrize('name', sorted(CALLS))
def test_callers_equal_pillow_on_a_mixed_size_list(name):
    g = M.golden()
    assert sorted(CALLS) == sorted(str(n) for n in g['call_names'])
    with _resident(g['pair'], g['small'], g['one'], g['small_b'], M.matte(1, 37, 53), M.matte(1, 20, 31)) as up:
        frames, others, mattes = up[:2], [up[2], up[3]], up[4:]
        assert CALLS[name](frames, others, mattes, up[2], np.array(g['call_bitmap'])) is frames
        got = [f.download() for f in frames]
        assert np.array_equal(up[2].download(), g['one'])                    # the other batch is only read
    for part, key in zip(got, 'ab'):
        want = g['call_%s_%s' % (name, key)]
        assert np.array_equal(part, want), (name, key, _differing(part, want))


def test_composite_faces_and_inset_chips_equal_pillow():
    g = M.golden()
    faces = [[], [], []]
    for f, box in zip(g['face_frames'], g['face_bboxes']):
        faces[f].append({'bbox': box})
    margin = float(g['face_margin'])
    other_host = np.ascontiguousarray(g['batch'][::-1])
    for shape in ('box', 'ellipse'):
        for alpha, key in ((None, 'paste'), (0.4, 'alpha')):
            with _resident(g['batch'], other_host) as (frames, other):
                assert vis.composite_faces(frames, other, faces, margin=margin, shape=shape, alpha=alpha) is frames
                got = frames.download()
            want = g['faces_%s_%s' % (shape, key)]
            assert np.array_equal(got, want), (shape, key, _differing(got, want))
    with _resident(g['batch'], g['inset_chips']) as (frames, chips):
        assert vis.inset_chips(frames, chips, g['inset_index'], origin=(3, 2), gap=2) is frames
        got = frames.download()
        assert np.array_equal(got, g['inset_expected']), _differing(got, g['inset_expected'])
        assert vis.inset_chips(frames, None, []) is frames
        with pytest.raises(ValueError):
            vis.composite_faces(frames, chips, faces)
