"""CPU tests (no GPU) of the neighbourhood filters: ta_filter_plan's host arithmetic and refusals, terran_amd.image's
filter_spec, and the numpy model (tests/filter_model.py) against the recorded Pillow golden (tests/golden/filter.npz)."""
import numpy as np
import pytest

from terran_amd import image, lib
from tests import filter_model as M


def _one_region(spec=0):
    return M.regions_of(np.array([(0, 0, 0, 5, 5, 0, spec)], np.int32), lib.FILTER_REGION_DT)


def test_plan_normalises_kernels_in_float32():
    g = M.golden()
    specs = g['specs']
    rounds, kernels, offsets = lib.filter_plan(_one_region(), specs)
    assert rounds.tolist() == [0] and kernels.dtype == np.float32 and offsets.dtype == np.float32
    seen = 0
    for s, k, off in zip(specs, kernels, offsets):
        if s['kind'] != lib.FILTER_KERNEL:
            assert not k.any() and off == 0
            continue
        n = int(s['size']) ** 2
        want_k, want_off = M.normalise(s)
        assert k[:n].tobytes() == want_k.tobytes() and not k[n:].any() and off.tobytes() == want_off.tobytes()
        seen += 1
    assert seen >= 19                                   # ten built-ins, two random kernels, seven sharpness factors


def test_plan_rounds_follow_list_order_within_a_frame():
    g = M.golden()
    names = [str(n) for n in g['case_names']]
    rows = g['case_%d_regions' % names.index('many')]
    assert len(rows) >= 40
    q = M.regions_of(rows, lib.FILTER_REGION_DT)
    rounds = lib.filter_plan(q, g['specs'])[0]
    want = []
    for i, a in enumerate(rows):
        k = 0
        for j, b in enumerate(rows[:i]):
            if a[0] == b[0] and a[1] < b[3] and b[1] < a[3] and a[2] < b[4] and b[2] < a[4]:
                k = max(k, want[j] + 1)
        want.append(k)
    assert rounds.tolist() == want and max(want) >= 3 and rounds[3] == rounds[1] + 1


def _bad_specs():
    ok = image.filter_spec('sharpen').copy()
    out = []

    def bad(base=ok, **fields):
        s = base.copy()
        for k, v in fields.items():
            if k == 'entry':
                s['kernel'][4] = v
            else:
                s[k] = v
        out.append(s)
    bad(kind=3), bad(kind=-1), bad(size=4), bad(size=7), bad(entry=np.nan), bad(entry=np.inf), bad(offset=np.nan), bad(scale=0)
    bad(scale=np.inf), bad(scale=np.nan), bad(has_factor=1, factor=np.nan), bad(has_factor=1, factor=-np.inf)
    rank = image.rank_spec(3, 4)
    bad(rank, size=4), bad(rank, size=9), bad(rank, size=0), bad(rank, size=-1), bad(rank, rank=9), bad(rank, rank=-1)
    un = image.unsharp_spec(2, 150, 3)
    bad(un, radius=-1), bad(un, radius=np.nan), bad(un, radius=np.inf), bad(un, radius=1025), bad(un, percent=-1), bad(un, threshold=-1)
    return ok, out


BAD_ROWS = [(0, 9, 0, 9, 9, 0, 0), (0, 0, 12, 9, 12, 0, 0), (0, 9, 0, 3, 9, 0, 0), (0, 0, 0, 9, 9, 2, 0), (0, 0, 0, 9, 9, -1, 0),
            (0, 0, 0, 9, 9, 0, 1), (0, 0, 0, 9, 9, 0, -1)]


def test_plan_refuses_invalid_specs_and_regions_with_outputs_untouched():
    load = lib.load()
    ok, bad = _bad_specs()
    assert len(bad) == 24

    def call(regions, specs):
        rounds, kernels, offsets = np.full(len(regions), -7, np.int32), np.full((len(specs), 25), -7, np.float32), np.full(len(specs), -7, np.float32)
        rc = load.ta_filter_plan(lib.ptr(regions), len(regions), lib.ptr(specs), len(specs), lib.ptr(rounds), lib.ptr(kernels), lib.ptr(offsets))
        return rc, (rounds == -7).all() and (kernels == -7).all() and (offsets == -7).all()
    assert call(_one_region(), np.stack([ok])) == (lib.OK, False)
    for s in bad:
        assert call(_one_region(), np.stack([ok, s])) == (lib.E_INVALID, True), s    # every spec is checked, used or not
    for row in BAD_ROWS:
        q = M.regions_of(np.array([(0, 0, 0, 5, 5, 0, 0), row], np.int32), lib.FILTER_REGION_DT)
        assert call(q, np.stack([ok])) == (lib.E_INVALID, True), row
    with pytest.raises(lib.TerranAmdError):
        lib.filter_plan(_one_region(1), np.stack([ok]))
    assert lib.filter_plan(np.zeros(0, lib.FILTER_REGION_DT), np.zeros(0, lib.FILTER_SPEC_DT))[0].shape == (0,)


def test_filter_spec_of_names_and_records():
    g = M.golden()
    by_name = {str(n): s for n, s in zip(g['spec_names'], g['specs'])}
    for name in image.FILTER_BUILTINS:
        assert image.filter_spec(name).tobytes() == by_name['builtin_' + name].tobytes(), name
    assert len(image.FILTER_BUILTINS) == 10
    for s, r in M.RANKS:
        assert image.rank_spec(s, r).tobytes() == by_name['rank_%d_%d' % (s, r)].tobytes()
    for u in M.UNSHARPS:
        assert image.unsharp_spec(*u).tobytes() == by_name['unsharp_%g_%d_%d' % u].tobytes()
    size, scale, offset, kernel = image.FILTER_BUILTINS['smooth']
    for f in M.SHARPNESS:
        assert image.kernel_spec(size, kernel, scale, offset, factor=f).tobytes() == by_name['sharpness_%g' % f].tobytes()
    spec = image.filter_spec('emboss')
    assert image.filter_spec(spec) is spec
    for bad in ('SHARPEN', 'median', 7, None, np.zeros(3)):
        with pytest.raises(ValueError):
            image.filter_spec(bad)
    for bad in ((9, 40), (4, 3), (3, 9), (3, -1), (3.0, 1)):
        with pytest.raises(ValueError):
            image.rank_spec(*bad)
    for bad in (((1, 2), 150, 3), (-1, 150, 3), (np.nan, 150, 3), (2, -1, 3), (2, 150, -1), (2, 1.5, 3), (1025, 1, 1)):
        with pytest.raises(ValueError):
            image.unsharp_spec(*bad)
    for bad in ((3, [1] * 8), (4, [1] * 16), (3, [np.nan] * 9), (3, [1, -1, 0] * 3), ((3, 5), [1] * 15)):
        with pytest.raises(ValueError):
            image.kernel_spec(*bad)


def test_filter_spec_of_pillow_filters():
    pytest.importorskip('PIL')
    from PIL import ImageFilter as F
    g = M.golden()
    by_name = {str(n): s for n, s in zip(g['spec_names'], g['specs'])}
    for name, (size, scale, offset, kernel) in image.FILTER_BUILTINS.items():
        cls = getattr(F, name.upper())
        assert cls.filterargs == ((size, size), scale, offset, kernel), name       # the tables are Pillow's
        assert image.filter_spec(cls).tobytes() == image.filter_spec(cls()).tobytes() == by_name['builtin_' + name].tobytes()
    for s, r in M.RANKS:
        assert image.filter_spec(F.RankFilter(s, r)).tobytes() == by_name['rank_%d_%d' % (s, r)].tobytes()
    assert image.filter_spec(F.MinFilter).tobytes() == by_name['rank_3_0'].tobytes()
    assert image.filter_spec(F.MedianFilter(5)).tobytes() == by_name['rank_5_12'].tobytes()
    assert image.filter_spec(F.MaxFilter(7)).tobytes() == by_name['rank_7_48'].tobytes()
    for u in M.UNSHARPS:
        assert image.filter_spec(F.UnsharpMask(*u)).tobytes() == by_name['unsharp_%g_%d_%d' % u].tobytes()
    assert image.filter_spec(F.UnsharpMask).tobytes() == by_name['unsharp_2_150_3'].tobytes()
    k = F.Kernel((3, 3), [0.5, -1, 2, 0, 1.25, 0, 3, 1, -2], offset=-1.5)
    spec = image.filter_spec(k)
    assert spec['scale'] == np.float32(4.75) and spec['offset'] == np.float32(-1.5) and spec['kernel'][:9].tolist() == list(k.filterargs[3])
    blur = image.filter_spec(F.GaussianBlur(2.5))
    assert blur['kind'] == image.FILTER_GAUSSIAN and blur['radius'] == np.float32(2.5)
    refused = [(F.ModeFilter(3), 'ModeFilter'), (F.BoxBlur(2), 'BoxBlur'), (F.GaussianBlur((1, 2)), 'GaussianBlur'), (F.UnsharpMask((1, 2)), 'UnsharpMask'),
               (F.Color3DLUT.generate(2, lambda r, g, b: (r, g, b)), 'Color3DLUT'), (F.RankFilter(9, 3), 'RankFilter'), (F.MedianFilter(9), 'MedianFilter'),
               (F.RankFilter, 'RankFilter')]
    for flt, name in refused:
        with pytest.raises(ValueError, match=name):
            image.filter_spec(flt)


def test_model_equals_the_golden():
    g = M.golden()
    specs = g['specs']
    cases = M.cases()
    names = [c[0] for c in cases]
    assert str(g['pillow_version']) and len(cases) >= 250
    for name, src, rows, want in cases:
        got = M.filter_regions(M.source(src).copy(), M.regions_of(rows, lib.FILTER_REGION_DT), specs)
        assert np.array_equal(got, want), (name, int((got != want).any(-1).sum()))
    # the cases the file must hold
    for h in M.HEIGHTS:
        for w in M.WIDTHS:
            assert {'%s_%dx%d' % (n, h, w) for n in ('k3', 'k5', 'rank_5_12', 'unsharp_1.3_73_0')} <= set(names)
    fma = dict(zip(names, g['case_fma']))
    for n in ('builtin_detail', 'builtin_smooth_more', 'k3_37x53', 'k5_37x53', 'k5_tile_33x129', 'k5_tile_34x130', 'sharpness_1.7'):
        assert fma[n] >= 1, n                           # a contracted build cannot pass these
    for n in ('builtin_emboss', 'builtin_contour'):
        e = cases[names.index(n)][3][0, 1:-1, 1:-1]
        assert (e == 0).any() and (e == 255).any()
