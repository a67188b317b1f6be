"""-m gpu: ta_frames_color and the colour callers of terran_amd.image and terran_amd.vis.color_faces against the recorded
Pillow golden (tests/golden/color.npz), bit for bit over whole frames, so a pixel outside every region is checked too.
Reads no Pillow and no reference.

The shapes are test_gpu_tone's, for the same walk (csrc/pixel_walk.h): widths 1, 3, 5 (no group of four at all), 53, 64,
257 (more units than a wave has lanes) with boxes at even and odd x0 meet every head and tail, heights 1, 2, 37 leave waves
of a workgroup without a row and give them several; every op kind walks all of them under both shapes.  The arithmetic is
checked on the frame of all 2^24 colours, by the SHA-256 of the downloaded bytes against Pillow's; the 3-D table sizes 2^3,
(3, 5, 7) and 17^3 take the LDS path, 33^3 and 65^3 the cached one."""
import numpy as np
import pytest

from terran_amd import image, lib, runtime, vis
from tests import color_model as M

pytestmark = pytest.mark.gpu


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


def _run_case(g, name, source=None):
    host = g[source or name + '_source']
    with _resident(host) as frames:
        frames.color(M.case_regions(g[name + '_regions'], lib.COLOR_REGION_DT), M.case_ops(g, name, lib.COLOR_OP_DT), M.case_tables(g, name))
        return host, frames.download()


@pytest.mark.parametrize('kind', ['matrix', 'ycbcr', 'rgb_from_ycbcr', 'hsv', 'rgb_from_hsv', 'lut'])
def test_every_op_walks_every_width_and_height(kind):
    g = M.golden()
    assert kind in [str(k) for k in g['walk_kinds']]
    sizes = [tuple(int(v) for v in s) for s in g['walk_sizes']]
    assert {w for _, w in sizes} == {1, 3, 5, 53, 64, 257} and {h for h, _ in sizes} == {1, 2, 37}
    for h, w in sizes:
        name = 'walk_%s_%dx%d' % (kind, h, w)
        rows = g[name + '_regions']
        assert {0, 1} <= set(rows[:, 5].tolist()) and (w == 1 or {0, 1} <= {int(x) % 2 for x in rows[:, 1]})
        host, got = _run_case(g, name, 'walk_source_%dx%d' % (h, w))
        want = g[name + '_expected']
        assert np.array_equal(got, want), (name, _differing(got, want))
        assert not np.array_equal(got, host)


@pytest.fixture(scope='module')
def every_colour():
    """The 4096 x 4096 frame of all colours, resident once for the digest tests; it is uploaded again by none of them."""
    host = M.all_colours()
    ctx = runtime.get_context(0)
    frames = ctx.upload(host[None])
    yield host, frames
    frames.free()


DIGESTS = {'ycbcr': 'ycbcr', 'rgb_from_ycbcr': 'rgb_from_ycbcr', 'hsv': 'hsv', 'rgb_from_hsv': 'rgb_from_hsv', 'matrix_sepia': M.SEPIA,
           'matrix_wild': M.WILD, 'lut_17': (17, 17, 17), 'lut_33': (33, 33, 33)}


@pytest.mark.parametrize('name', sorted(DIGESTS))
def test_all_colours_digest_equals_pillows(name, every_colour):
    g = M.golden()
    assert sorted(DIGESTS) == sorted(str(n) for n in g['digest_names'])
    host, resident = every_colour
    op = DIGESTS[name]
    rec, table = image.color_spec((op, M.formula_lut(op)) if name.startswith('lut') else op)
    work = image.copy_frames(resident)
    try:
        whole = np.zeros(1, lib.COLOR_REGION_DT)
        whole['x1'], whole['y1'] = 4096, 4096
        work.color(whole, rec, table)
        got = work.download()[0]
    finally:
        work.free()
    assert np.array_equal(resident.download()[0, :2], host[:2])             # the shared frame is as it was
    if M.digest(got) != str(g['digest_' + name]):
        ops = np.zeros(1, lib.COLOR_OP_DT)
        ops[0] = rec
        want = M.apply_op(host, ops[0], table)
        bad = (got != want).any(-1)
        pytest.fail('%s: %d of 2^24 colours differ from the model; first: %s -> %s, model %s'
                    % (name, int(bad.sum()), host[bad][:4].tolist(), got[bad][:4].tolist(), want[bad][:4].tolist()))


def test_lut_sizes_take_both_table_paths():
    g = M.golden()
    sizes = [tuple(int(v) for v in op[1:4]) for op in g['lut_sizes_ops']]
    assert sizes == [(2, 2, 2), (3, 5, 7), (17, 17, 17), (33, 33, 33), (65, 65, 65)]
    assert 17 ** 3 * 8 <= 65536 < 33 ** 3 * 8                                # LDS_TABLE_BYTES lies between them
    host, got = _run_case(g, 'lut_sizes')
    want = g['lut_sizes_expected']
    assert np.array_equal(got, want), _differing(got, want)
    # one op a call: nothing depends on what else the call carried
    rows = g['lut_sizes_regions']
    tables = M.case_tables(g, 'lut_sizes')
    ops = M.case_ops(g, 'lut_sizes', lib.COLOR_OP_DT)
    with _resident(host) as frames:
        for r in rows:
            one = ops[[r[6]]].copy()
            n = 3 * int(np.prod(one['size'][0]))
            sub = tables[one['table'][0]:one['table'][0] + n]
            one['table'] = 0
            q = M.case_regions(r[None].copy(), lib.COLOR_REGION_DT)
            q['op'] = 0
            frames.color(q, one, sub)
        assert np.array_equal(frames.download(), want)


def test_overlapping_regions_apply_in_list_order():
    g = M.golden()
    names = [str(n) for n in g['order_names']]
    assert names == ['order_ycbcr_then_matrix', 'order_matrix_then_ycbcr']
    for name in names:
        rows = g[name + '_regions']
        assert rows[:, 0].tolist()[:2] == [2, 0] and rows[1].tolist() == rows[5].tolist()       # frames out of order, a box twice
        assert len(set(rows[:, 6].tolist())) == 3                                               # three op kinds in one call
        host, got = _run_case(g, name)
        want = g[name + '_expected']
        assert np.array_equal(got, want), (name, _differing(got, want))
    assert not np.array_equal(g[names[0] + '_expected'], g[names[1] + '_expected'])


def _call(ctx, frames, q, ops, tables):
    ops = np.ascontiguousarray(ops, lib.COLOR_OP_DT).reshape(-1)
    tables = np.ascontiguousarray(tables, np.float32)
    return ctx.lib.ta_frames_color(ctx.h, frames.h, lib.ptr(q) if len(q) else None, len(q), lib.ptr(ops) if len(ops) else None, len(ops),
                                   lib.ptr(tables) if len(tables) else None, len(tables))


def test_invalid_calls_are_refused_before_any_pixel_changes():
    g = M.golden()
    host = g['batch']
    H, W = host.shape[1:3]
    good = (1, 5, 5, 40, 30, 0, 0)
    ctx = runtime.get_context(0)
    ops = np.zeros(3, lib.COLOR_OP_DT)
    ops['kind'] = [lib.COLOR_RGB2YCBCR, lib.COLOR_MATRIX, lib.COLOR_LUT3D]
    ops['size'][2] = (2, 2, 2)
    ops['table'] = [0, 0, 12]
    tables = np.concatenate([np.asarray(M.SEPIA, np.float32), M.formula_lut((2, 2, 2))])

    def regions(*rows):
        return M.case_regions(np.array(rows, np.int32).reshape(-1, 7), lib.COLOR_REGION_DT)
    with _resident(host) as frames:
        assert _call(ctx, frames, regions(), ops, tables) == lib.OK                              # n = 0: TA_OK
        # every region defect of ta_frames_point, and an op index out of range
        bad = [(3, 0, 0, 9, 9, 0, 0), (-1, 0, 0, 9, 9, 0, 0), (0, 9, 0, 9, 9, 0, 0), (0, 0, 12, 9, 12, 0, 0), (0, 9, 0, 3, 9, 0, 0),
               (0, -1, 0, 9, 9, 0, 0), (0, 0, 0, W + 1, 9, 0, 0), (0, 0, 0, 9, H + 1, 0, 0), (0, 0, -2, 9, 9, 0, 0), (0, 0, 0, 9, 9, 2, 0),
               (0, 0, 0, 9, 9, -1, 0), (0, 0, 0, 9, 9, 0, 3), (0, 0, 0, 9, 9, 0, -1)]
        for b in bad:
            assert _call(ctx, frames, regions(good, b, good), ops, tables) == lib.E_INVALID, b
            assert b'region 1' in ctx.lib.ta_last_error(ctx.h), b
        # the ops: an unknown kind, an axis below 2 or above 65, a missing or short table, NaN or infinity
        def broken(index, **fields):
            o = ops.copy()
            for k, v in fields.items():
                o[k][index] = v
            return o
        nan_m, inf_t = tables.copy(), tables.copy()
        nan_m[7], inf_t[12 + 5] = np.nan, -np.inf
        cases = [(broken(0, kind=6), tables, 0), (broken(0, kind=-1), tables, 0), (broken(2, size=(2, 1, 2)), tables, 2),
                 (broken(2, size=(66, 2, 2)), tables, 2), (broken(1, table=-1), tables, 1), (broken(2, table=13), tables, 2),
                 (broken(1, table=len(tables) - 11), tables, 1), (ops, tables[:-1], 2), (ops, np.zeros(0, np.float32), 1),
                 (ops, nan_m, 1), (ops, inf_t, 2)]
        for o, t, which in cases:
            assert _call(ctx, frames, regions(good), o, t) == lib.E_INVALID, (o, len(t))
            assert ('op %d' % which).encode() in ctx.lib.ta_last_error(ctx.h), (o, ctx.lib.ta_last_error(ctx.h))
        with pytest.raises(lib.TerranAmdError) as e:
            frames.color(regions(good, bad[0]), ops, tables)
        assert e.value.code == lib.E_INVALID and 'region 1' in str(e.value)
        assert np.array_equal(frames.download(), host)                                          # nothing changed so far
        other = runtime.new_context(0)                                                          # the caller's context, as in blur
        q = regions(good, (0, 1, 1, 9, 9, 1, 2))
        frames.color(q, ops, tables, ctx=other)
        assert np.array_equal(frames.download(), M.color_regions(host.copy(), q, ops, tables))


def _mixed():
    g = M.golden()
    return g['batch'][:2], g['small'][None]


CALLS = {'hue': lambda f, g: image.hue_frames(f, int(g['call_hue_shift'])), 'ycbcr': lambda f, g: image.convert_frames(f, 'YCbCr'),
         'hsv': lambda f, g: image.convert_frames(f, 'HSV'), 'matrix': lambda f, g: image.matrix_frames(f, M.SEPIA),
         'lut': lambda f, g: image.color_lut_frames(f, (17, M.formula_lut((17, 17, 17)))),
         'round_trip': lambda f, g: image.convert_frames(image.convert_frames(f, 'YCbCr'), 'RGB', source='YCbCr')}


@pytest.mark.parametrize('name', sorted(CALLS))
def test_callers_equal_pillow_on_a_mixed_size_list(name):
    g = M.golden()
    assert sorted(CALLS) == sorted(str(n) for n in g['call_names'])
    a, b = _mixed()
    with _resident(a, b) as frames:
        assert CALLS[name](frames, g) is frames
        got = [f.download() for f in frames]
    for part, key in zip(got, 'ab'):
        want = g['call_%s_%s' % (name, key)]
        assert np.array_equal(part, want), (name, key, _differing(part, want))
    if name == 'matrix':                                   # boxes under the ellipse, a matrix through convert_frames
        with _resident(a, b) as frames:
            image.convert_frames(frames, 'RGB', matrix=M.WILD, boxes=g['call_boxes'], shape='ellipse')
            for f, key in zip(frames, 'ab'):
                assert np.array_equal(f.download(), g['call_boxed_matrix_' + key]), key
            with pytest.raises(ValueError):
                image.convert_frames(frames, 'LAB')
            with pytest.raises(ValueError):
                image.convert_frames(frames, 'RGB', matrix=M.SEPIA[:4])


def test_color_faces_equals_pillow():
    g = M.golden()
    faces = [[], [], []]
    for f, box in zip(g['face_frames'], g['face_bboxes']):
        faces[f].append({'bbox': box})
    for shape in ('box', 'ellipse'):
        with _resident(g['batch']) as frames:
            assert vis.color_faces(frames, faces, M.SEPIA, margin=float(g['face_margin']), shape=shape) is frames
            got = frames.download()
        want = g['face_%s_expected' % shape]
        assert np.array_equal(got, want), (shape, _differing(got, want))
        assert not np.array_equal(got, g['batch'])
