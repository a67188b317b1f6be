"""CPU tests (no GPU) of the colour operations: tests/color_model.py against the recorded Pillow golden and, over all 2^24
colours, against live Pillow; ta_color_plan's rounds and quantised tables against the model; the refusals of
terran_amd.image.color_spec and its callers."""
import numpy as np
import pytest

from terran_amd import image, lib
from tests import color_model as M


def _pil():
    return pytest.importorskip('PIL.Image')


def _case(g, name, source=None):
    host = g[source or name + '_source'].copy()
    q = M.case_regions(g[name + '_regions'], lib.COLOR_REGION_DT)
    return M.color_regions(host, q, M.case_ops(g, name, lib.COLOR_OP_DT), M.case_tables(g, name))


def test_model_equals_the_golden_on_the_small_cases():
    g = M.golden()
    assert str(g['pillow_version'])
    for kind in (str(k) for k in g['walk_kinds']):
        for h, w in g['walk_sizes']:
            name = 'walk_%s_%dx%d' % (kind, h, w)
            assert np.array_equal(_case(g, name, 'walk_source_%dx%d' % (h, w)), g[name + '_expected']), name
    for name in ['lut_sizes'] + [str(n) for n in g['order_names']]:
        assert np.array_equal(_case(g, name), g[name + '_expected']), name
    hue = M.hue_lut(int(g['call_hue_shift']))
    fns = {'hue': lambda a: M.hsv_to_rgb(_point(M.rgb_to_hsv(a), hue)), 'ycbcr': M.rgb_to_ycbcr, 'hsv': M.rgb_to_hsv, 'matrix': lambda a: M.matrix(a, M.SEPIA),
           'lut': lambda a: M.lut3d(a, (17, 17, 17), M.formula_lut((17, 17, 17))),
           'round_trip': lambda a: M.ycbcr_to_rgb(M.rgb_to_ycbcr(a))}
    assert sorted(fns) == sorted(str(n) for n in g['call_names'])
    for name, fn in fns.items():
        for key, part in (('a', g['batch'][:2]), ('b', g['small'][None])):
            assert np.array_equal(fn(part), g['call_%s_%s' % (name, key)]), (name, key)


def _point(a, lut):
    lut = lut.reshape(3, 256)
    return np.stack([lut[c][a[..., c]] for c in range(3)], -1)


def test_formula_tables_leave_0_to_1_at_both_ends_and_saturate():
    for size in [(2, 2, 2), (3, 5, 7), (17, 17, 17)]:
        t = M.formula_lut(size)
        q = M.quantise(t)
        assert t.dtype == np.float32 and len(t) == 3 * size[0] * size[1] * size[2]
        assert t.min() < 0 and t.max() > 2.0 and q.max() == 0x7fff and q.min() < 0
    # the ends of the quantisation, item = t * 16320 as a float32 product
    edge = np.array([0x7fff - 0.5, 0x7fff - 0.51, -0x7fff + 0.5, -0x7fff + 0.51, 0.5, -0.5, 0.49, 1e9, -1e9], np.float64) / 16320
    item = edge.astype(np.float32) * np.float32(16320)
    want = [0x7fff if i >= 0x7fff - 0.5 else -0x7fff if i <= -0x7fff + 0.5 else int(i + (0.5 if i >= 0 else -0.5)) for i in item.astype(np.float64)]
    assert M.quantise(edge).tolist() == want


@pytest.mark.parametrize('name', ['ycbcr', 'rgb_from_ycbcr', 'hsv', 'rgb_from_hsv', 'matrix_sepia', 'matrix_wild'])
def test_model_equals_live_pillow_and_the_digest_over_all_colours(name):
    Image = _pil()
    g = M.golden()
    a = M.all_colours()
    im = Image.fromarray(a)
    raw = lambda mode: Image.frombytes(mode, im.size, a.tobytes())      # noqa: E731
    if name == 'ycbcr':
        got, want = M.rgb_to_ycbcr(a), im.convert('YCbCr')
    elif name == 'rgb_from_ycbcr':
        got, want = M.ycbcr_to_rgb(a), raw('YCbCr').convert('RGB')
    elif name == 'hsv':
        got, want = M.rgb_to_hsv(a), im.convert('HSV')
    elif name == 'rgb_from_hsv':
        got, want = M.hsv_to_rgb(a), raw('HSV').convert('RGB')
    else:
        m = M.SEPIA if name == 'matrix_sepia' else M.WILD
        got, want = M.matrix(a, m), im.convert('RGB', m)
    want = np.asarray(want)
    bad = (got != want).any(-1)
    assert not bad.any(), (int(bad.sum()), a[bad][:4].tolist(), got[bad][:4].tolist(), want[bad][:4].tolist())
    assert M.digest(got) == str(g['digest_' + name])


@pytest.mark.parametrize('size', [17, 33])
def test_model_lut_digest_over_all_colours(size):
    g = M.golden()
    a = M.all_colours()
    table = M.formula_lut((size,) * 3)
    got = np.concatenate([M.lut3d(a[y:y + 512], (size,) * 3, table) for y in range(0, 4096, 512)])
    assert M.digest(got) == str(g['digest_lut_%d' % size])


def test_color_plan_equals_the_model():
    g = M.golden()
    for name in ['lut_sizes'] + [str(n) for n in g['order_names']]:
        q = M.case_regions(g[name + '_regions'], lib.COLOR_REGION_DT)
        ops, tables = M.case_ops(g, name, lib.COLOR_OP_DT), M.case_tables(g, name)
        rounds, nodes = lib.color_plan(q, ops, tables)
        assert np.array_equal(rounds, M.plan_rounds(q)), name
        assert rounds.max() >= 1
        for op, n in zip(ops, nodes):
            if op['kind'] != lib.COLOR_LUT3D:
                assert n is None
                continue
            s0, s1, s2 = (int(v) for v in op['size'])
            want = M.quantise(tables[op['table']:op['table'] + 3 * s0 * s1 * s2]).reshape(s2, s1, s0, 3)
            assert n.dtype == np.int16 and np.array_equal(n[..., :3], want) and not n[..., 3].any(), (name, s0, s1, s2)
    # the ends of the quantisation through the C code
    edge = (np.array([0x7fff - 0.5, 0x7fff - 0.51, -0x7fff + 0.5, -0x7fff + 0.51, 0.5, -0.5, 0.49, 1e9, -1e9, 0, 1, 0.1] * 2, np.float64) / 16320).astype(np.float32)
    ops = np.zeros(1, lib.COLOR_OP_DT)
    ops['kind'], ops['size'] = lib.COLOR_LUT3D, (2, 2, 2)
    _, nodes = lib.color_plan(np.zeros(0, lib.COLOR_REGION_DT), ops, edge)
    assert np.array_equal(nodes[0][..., :3].reshape(-1), M.quantise(edge))


def test_color_plan_refuses_what_the_call_refuses():
    good = M.case_regions(np.array([(0, 0, 0, 9, 9, 0, 0)], np.int32), lib.COLOR_REGION_DT)
    ops = np.zeros(2, lib.COLOR_OP_DT)
    ops['kind'], ops['size'][1] = [lib.COLOR_MATRIX, lib.COLOR_LUT3D], (2, 3, 2)
    ops['table'] = [0, 12]
    tables = np.concatenate([np.asarray(M.SEPIA, np.float32), M.formula_lut((2, 3, 2))])
    assert lib.color_plan(good, ops, tables)[0].tolist() == [0]

    def refused(q=good, o=ops, t=tables):
        with pytest.raises(lib.TerranAmdError) as e:
            lib.color_plan(q, o, t)
        assert e.value.code == lib.E_INVALID
    for row in [(0, 9, 0, 9, 9, 0, 0), (0, 0, 9, 9, 3, 0, 0), (0, 0, 0, 9, 9, 2, 0), (0, 0, 0, 9, 9, 0, 2), (0, 0, 0, 9, 9, 0, -1)]:
        refused(q=M.case_regions(np.array([row], np.int32), lib.COLOR_REGION_DT))
    for field, index, value in [('kind', 0, 6), ('kind', 1, -1), ('size', 1, (1, 3, 2)), ('size', 1, (2, 3, 66)), ('table', 0, -1),
                                ('table', 1, 13), ('table', 0, len(tables) - 11)]:
        o = ops.copy()
        o[field][index] = value
        refused(o=o)
    refused(t=tables[:-1])
    refused(t=None)
    for at in (3, 12 + 7):
        for v in (np.nan, np.inf, -np.inf):
            t = tables.copy()
            t[at] = v
            refused(t=t)


def test_color_spec_packs_and_refuses():
    rec, t = image.color_spec(M.SEPIA)
    assert rec['kind'] == lib.COLOR_MATRIX and t.dtype == np.float32 and np.array_equal(t, np.asarray(M.SEPIA, np.float32))
    for name, kind in M.CONVERSIONS.items():
        rec, t = image.color_spec(name)
        assert rec['kind'] == kind and len(t) == 0
    table = M.formula_lut((3, 5, 7))
    for op in ((( 3, 5, 7), table), ((3, 5, 7), table.reshape(7, 5, 3, 3).tolist())):
        rec, t = image.color_spec(op)
        assert rec['kind'] == lib.COLOR_LUT3D and rec['size'].tolist() == [3, 5, 7] and np.array_equal(t, table)
    rec, t = image.color_spec((2, np.zeros(24)))
    assert rec['size'].tolist() == [2, 2, 2] and image.color_spec((rec, t))[0] == rec
    bad = [M.SEPIA[:4], M.SEPIA[:11], 'lab', 'YCbCr', None, 7, (1, np.zeros(3)), (66, np.zeros(3)), ((2, 2), np.zeros(12)),
           (2, np.zeros(8)), (2, np.zeros(32)), (2, np.zeros(23)), M.SEPIA[:11] + (np.nan,), M.SEPIA[:11] + (np.inf,),
           (2, [np.nan] * 24), (2, [1e39] * 24), M.SEPIA[:11] + ('x',)]
    for op in bad:
        with pytest.raises(ValueError):
            image.color_spec(op)
    with pytest.raises(ValueError):
        image.hue_lut(0.5)
    assert np.array_equal(image.hue_lut(77), M.hue_lut(77)) and np.array_equal(image.hue_lut(-179), M.hue_lut(77))


def test_color_spec_takes_pillows_color3dlut():
    pytest.importorskip('PIL.Image')
    from PIL import ImageFilter
    table = M.formula_lut((2, 3, 4))
    rec, t = image.color_spec(ImageFilter.Color3DLUT((2, 3, 4), table.tolist()))
    assert rec['kind'] == lib.COLOR_LUT3D and rec['size'].tolist() == [2, 3, 4] and np.array_equal(t, table)
    with pytest.raises(ValueError):                                         # (a 1-channel one Pillow itself refuses to build)
        image.color_spec(ImageFilter.Color3DLUT(2, [0.0] * 32, channels=4))
    with pytest.raises(ValueError, match='Color3DLUT'):                     # the filter route still refuses it
        image.filter_spec(ImageFilter.Color3DLUT(2, [0.0] * 24))
