"""-m gpu: the device gallery (terran_amd/csrc/gallery.hip, lib.Gallery, FaceGallery) against tests/gallery_model.py.

Exact cases: integer components in [-8, 8], normalize=0 -- every dot is an integer below 2^24 in magnitude, exact in float32
in any summation order, so rows, ids and distances must EQUAL the model's; many rows are duplicates, so ties are everywhere.
Real-valued cases: ATOL = (dim + 8) 2^-24, the forward bound of a length-dim float32 dot of unit vectors plus the two
normalisations (derived, not tuned; numpy's own float32 on the same data is off by 3e-7).
"""
import ctypes as C

import numpy as np
import pytest

from tests.gallery_model import GalleryModel
from tests.util import golden

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def ctx():
    from terran_amd import runtime
    return runtime.get_context(0)


def _tg():
    from terran_amd import lib
    return lib.GALLERY_ROW_TILE, lib.GALLERY_QUERY_GROUP


def _exact_data(seed, n, nq, dim, pool=24):
    """n rows drawn (with many repeats) from a pool of integer vectors, ids that repeat too, nq queries of which some ARE
    pool vectors."""
    rng = np.random.default_rng(seed)
    base = rng.integers(-8, 9, (pool, dim)).astype(np.float32)
    rows = base[rng.integers(0, pool, n)]
    ids = rng.integers(0, 9, n).astype(np.int32)
    q = rng.integers(-8, 9, (nq, dim)).astype(np.float32)
    q[::3] = base[rng.integers(0, pool, len(q[::3]))]
    return rows, ids, q


def _build(ctx, dim, rows, ids, normalize, reserve=0):
    from terran_amd import lib
    g = lib.Gallery(ctx, dim, reserve)
    m = GalleryModel(dim)
    g.add(rows, ids, normalize)
    m.add(rows, ids)
    return g, m


def _same(g, m, q, k, what):
    row, ident, dist = g.search(q, k, normalize=False)
    mrow, mid, mdist = m.search(q, k, normalize=False)
    assert row.shape == ident.shape == dist.shape == (len(q), k) and dist.dtype == np.float32
    assert np.array_equal(row, mrow), what
    assert np.array_equal(ident, mid), what
    assert np.array_equal(dist, mdist.astype(np.float32)), what
    return row, ident, dist


def _row_counts():
    T, _ = _tg()
    return [T - 1, T, T + 1, 3 * T + 1, 1]


def _query_counts():
    _, G = _tg()
    return [1, G - 1, G, G + 1, 2 * G + 1, 130]


@pytest.mark.parametrize('k', [1, 5, 16])
@pytest.mark.parametrize('n', _row_counts())
def test_exact_row_counts_and_k(ctx, n, k):
    """Tile edges (T - 1, T, T + 1, several tiles, one row) under every k: with one row, and with k = 16 over 24 distinct
    vectors, k exceeds what can be told apart by distance alone or what exists at all."""
    rows, ids, q = _exact_data(n, n, 5, 512)
    g, m = _build(ctx, 512, rows, ids, False)
    row, _, dist = _same(g, m, q, k, (n, k))
    if n < k:
        assert (row[:, n:] == -1).all() and np.isinf(dist[:, n:]).all()
    g.free()


@pytest.mark.parametrize('nq', _query_counts())
def test_exact_query_counts(ctx, nq):
    """Query group edges (G - 1, G, G + 1), more groups than one pass holds (2 G + 1, 130) and a single query."""
    T, _ = _tg()
    rows, ids, q = _exact_data(100 + nq, 3 * T + 1, nq, 512)
    g, m = _build(ctx, 512, rows, ids, False)
    _same(g, m, q, 5, nq)
    g.free()


@pytest.mark.parametrize('dim', [1, 2, 63, 64, 65, 512, 1024])
def test_exact_dims(ctx, dim):
    """K tails (the stored row is zero-filled to the kernel's K step) and the widest row, which holds one query group per pass."""
    T, G = _tg()
    rows, ids, q = _exact_data(200 + dim, T + 1, G + 1, dim)
    g, m = _build(ctx, dim, rows, ids, False)
    _same(g, m, q, 5, dim)
    got_rows, got_ids = g.download()
    assert np.array_equal(got_rows, rows) and np.array_equal(got_ids, ids)
    g.free()


@pytest.mark.parametrize('n', [40001, 70003])
def test_exact_more_tiles_than_workgroups(ctx, n):
    """The grid is one workgroup per CU at the most (256 on the MI355X), so above 256 T rows a
    workgroup walks several tiles, tile w, w + grid, ...: the first chunk of its next tile is prefetched behind the last
    of this one, and candidates meet an owner's list that earlier tiles filled.  40 001 rows are 313 tiles (57 workgroups
    take two, the others one), 70 003 are 547 (35 take three, the others two).  Every vector of the pool occurs about eight
    times anywhere in the gallery, so the 16 best of a query that IS a pool vector are ties that span the tiles of one
    workgroup and those of others; 2 G + 1 queries make the walk happen in two passes."""
    T, G = _tg()
    cus = 256
    rows, ids, q = _exact_data(n, n, 2 * G + 1, 64, pool=n // 8)
    g, m = _build(ctx, 64, rows, ids, False)
    row, _, _ = _same(g, m, q, 16, n)
    tiles = row // T
    assert (tiles >= cus).any() and (tiles < cus).any()                 # results come from first and from later tiles
    assert (tiles.max(1) - tiles.min(1) >= cus).any()                   # ... within one query's list
    g.free()


@pytest.fixture(scope='module')
def real_case(ctx):
    """3001 Gaussian rows, 67 queries of which 20 are noisy copies of rows; the float64 model's full distance matrix."""
    rng = np.random.default_rng(77)
    dim, n, nq, k = 512, 3001, 67, 8
    rows = rng.normal(size=(n, dim)).astype(np.float32)
    q = rng.normal(size=(nq, dim)).astype(np.float32)
    src = rng.choice(n, 20, replace=False)
    q[:20] = rows[src] + rng.normal(0, 0.05, (20, dim)).astype(np.float32)
    ids = (np.arange(n) % 1000).astype(np.int32)
    g, m = _build(ctx, dim, rows, ids, True)
    got = g.search(q, k, normalize=True)
    g.free()
    return dict(dim=dim, k=k, ids=ids, src=src, got=got, full=m.distances(q, True), want=m.search(q, k, True))


def test_real_valued_distances_and_ranks(real_case):
    c = real_case
    atol = (c['dim'] + 8) * 2.0 ** -24
    row, ident, dist = c['got']
    _, _, wdist = c['want']
    assert (row >= 0).all() and np.array_equal(ident, c['ids'][row])
    err = np.abs(dist.astype(np.float64) - wdist)                       # every query, every rank
    own = np.take_along_axis(c['full'], row.astype(np.int64), 1)        # the returned row's own float64 distance
    err_own = np.abs(own - wdist)
    print('gallery: worst distance error %.3g, worst own-distance error %.3g (ATOL %.3g, numpy float32: 3e-7)'
          % (err.max(), err_own.max(), atol))
    assert (err <= atol).all(), err.max()
    assert (err_own <= 2 * atol).all(), err_own.max()
    assert np.array_equal(row[:20, 0], c['src'])                       # a noisy copy finds its source first
    for i in range(len(row)):
        assert len(set(row[i].tolist())) == c['k']
        keys = list(zip(dist[i].tolist(), row[i].tolist()))
        assert keys == sorted(keys), (i, keys)


def test_tombstones_remove_add_clear_size(ctx):
    T, G = _tg()
    rows, ids, q = _exact_data(5, 2 * T + 9, G + 3, 512)
    g, m = _build(ctx, 512, rows, ids, False)
    assert g.size() == m.size() == (2 * T + 9, 2 * T + 9)
    gone = [2, 7]
    want_removed = m.remove(gone)
    assert g.remove(gone) == want_removed > 0
    assert g.remove(gone) == 0                                          # nothing left under those ids
    assert g.size() == m.size() and g.size()[1] == 2 * T + 9 - want_removed
    _, ident, _ = _same(g, m, q, 16, 'after remove')
    assert not np.isin(ident, gone).any()
    assert np.array_equal(g.download()[1], m.ids)
    sel = np.isin(ids, gone)
    g.add(rows[sel], ids[sel], False)                                   # the same vectors again: new rows at the end
    m.add(rows[sel], ids[sel])
    assert g.size() == m.size()
    row, ident, _ = _same(g, m, q, 16, 'after re-add')
    assert np.isin(ident, gone).any() and not np.isin(row, np.nonzero(sel)[0]).any()
    live = np.unique(ids)                                               # fewer live rows than k
    m.remove(live[1:])
    g.remove(live[1:])
    m.remove([0])
    g.remove([0])
    g.add(rows[:3], np.array([4, 4, 5], np.int32), False)
    m.add(rows[:3], [4, 4, 5])
    row, _, dist = _same(g, m, q, 5, 'three live rows')
    assert (row[:, 3:] == -1).all() and np.isinf(dist[:, 3:]).all() and g.size()[1] == 3
    g.clear()
    assert g.size() == (0, 0)
    row, ident, dist = g.search(q, 3, normalize=False)
    assert (row == -1).all() and (ident == -1).all() and np.isinf(dist).all()
    g.add(rows[:T], ids[:T], False)                                     # a cleared gallery starts at row 0 again
    m.clear()
    m.add(rows[:T], ids[:T])
    _same(g, m, q, 5, 'after clear')
    g.free()


def test_growth_in_steps_equals_reserved(ctx):
    from terran_amd import lib
    T, G = _tg()
    rng = np.random.default_rng(9)
    n, dim = 3 * T + 1, 512
    rows = rng.normal(size=(n, dim)).astype(np.float32)
    ids = np.arange(n, dtype=np.int32)
    q = rng.normal(size=(G + 1, dim)).astype(np.float32)
    whole = lib.Gallery(ctx, dim, reserve=n)
    whole.add(rows, ids)
    steps = lib.Gallery(ctx, dim, reserve=0)
    for i in range(0, n, 7):
        steps.add(rows[i:i + 7], ids[i:i + 7])
    assert steps.size() == whole.size() == (n, n)
    a, b = whole.search(q, 8), steps.search(q, 8)
    again = steps.search(q, 8)
    for x, y, z in zip(a, b, again):
        assert np.array_equal(x, y) and np.array_equal(y, z)
    for x, y in zip(whole.download(), steps.download()):
        assert np.array_equal(x, y)
    whole.free()
    steps.free()


def test_identify_end_to_end(states):
    """Enrol the faces of one frame, identify the same faces: each gets its own name at a distance within ATOL; a face of
    another frame under threshold 0.0 gets none."""
    from terran_amd import FaceGallery, Recognition, synth
    a = golden('arcface_call.npz')
    image, lms = a['image'], a['landmarks']
    marks = [lms[0], lms[1], lms[0] + np.array([9, -6]), lms[1] + np.array([-7, 8])]
    rec = Recognition(device=0, state=states('arcface'))
    feats = rec(image, [{'landmarks': m} for m in marks])
    assert feats.shape == (4, 512)
    gallery = FaceGallery(dim=512, device=0)
    names = ['ada', 'bob', 'cy', 'dee']
    for name, f in zip(names, feats):
        gallery.add(name, f)
    assert len(gallery) == 4 and gallery.names == names
    faces = [{'landmarks': m} for m in marks]
    assert gallery.identify(faces, feats) is faces
    atol = (512 + 8) * 2.0 ** -24
    print('gallery: identify distances %s (ATOL %.3g)' % ([f.get('distance') for f in faces], atol))
    assert [f.get('text') for f in faces] == names
    assert all(abs(f['distance']) <= atol for f in faces)
    other = synth.frames(31, 1, image.shape[0], image.shape[1])[0]
    strangers = [[{'landmarks': marks[0]}], [{'landmarks': marks[1]}]]
    gallery.identify(strangers, rec([other, other], strangers), threshold=0.0)
    assert all('text' not in f and 'distance' not in f for per in strangers for f in per)
    gallery.free()


def test_errors_and_empty_calls(ctx):
    from terran_amd import lib
    L = ctx.lib
    g = lib.Gallery(ctx, 16)
    q = np.ones((2, 16), np.float32)
    row, ident, dist = g.search(q, 4)                                   # an empty gallery answers with padding
    assert (row == -1).all() and (ident == -1).all() and np.isinf(dist).all()
    g.add(q, [1, 2])
    assert g.search(np.empty((0, 16), np.float32), 3)[0].shape == (0, 3)  # no queries: success, nothing written
    out = [np.zeros((2, 1), np.int32), np.zeros((2, 1), np.int32), np.zeros((2, 1), np.float32)]
    po = [lib.ptr(x) for x in out]
    for k in (0, 17, -1):
        with pytest.raises(lib.TerranAmdError) as e:
            g.search(q, k)
        assert e.value.code == lib.E_INVALID
    for bad in (np.ones((2, 15), np.float32), np.ones((2, 17), np.float32), np.ones(16, np.float32)):
        with pytest.raises(lib.TerranAmdError) as e:
            g.search(bad, 1)
        assert e.value.code == lib.E_INVALID
        with pytest.raises(lib.TerranAmdError) as e:
            g.add(bad, [1, 2][:len(bad)])
        assert e.value.code == lib.E_INVALID
    assert L.ta_gallery_search(g.h, None, 2, 1, 0, *po) == lib.E_INVALID
    for i in range(3):
        args = list(po)
        args[i] = None
        assert L.ta_gallery_search(g.h, lib.ptr(q), 2, 1, 0, *args) == lib.E_INVALID
    assert L.ta_gallery_search(None, lib.ptr(q), 2, 1, 0, *po) == lib.E_INVALID
    ids = np.array([1, 2], np.int32)
    assert L.ta_gallery_add(g.h, None, lib.ptr(ids), 2, 0) == lib.E_INVALID
    assert L.ta_gallery_add(g.h, lib.ptr(q), None, 2, 0) == lib.E_INVALID
    assert L.ta_gallery_add(g.h, lib.ptr(q), lib.ptr(np.array([1, -2], np.int32)), 2, 0) == lib.E_INVALID
    assert L.ta_gallery_add(g.h, lib.ptr(q), lib.ptr(ids), 2 ** 31, 0) == lib.E_INVALID     # more than 2^31-1 rows: refused before any copy
    assert L.ta_gallery_remove(g.h, None, 2, None) == lib.E_INVALID
    assert L.ta_gallery_download(g.h, None, None) == lib.E_INVALID
    h = C.c_void_p()
    for dim in (0, -1, 1025):
        assert L.ta_gallery_create(ctx.h, dim, 0, C.byref(h)) == lib.E_INVALID and not h.value
    assert L.ta_gallery_create(ctx.h, 16, 2 ** 31, C.byref(h)) == lib.E_INVALID
    assert L.ta_gallery_create(ctx.h, 16, 0, None) == lib.E_INVALID
    assert g.size() == (2, 2)                                           # none of the refused calls changed anything
    g.free()
