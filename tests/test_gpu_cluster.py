"""-m gpu: ta_gallery_cluster (terran_amd/csrc/gallery_cluster.hip, lib.Gallery.cluster, cluster_faces) against
tests/cluster_model.py.

Exact cases: integer components, normalize=0 -- every dot is an integer below 2^24 in magnitude, exact in float32 in any
summation order, and the thresholds are 1 - t for an integer t, so labels, degree and the number of clusters must EQUAL the
model's.  The real-valued case picks its threshold in the middle of a gap of the model's distances that is asserted to be
at least 8 ATOL wide, ATOL = (dim + 8) 2^-24 as in test_gpu_gallery.py: no pair can change sides within the kernel's
error, so the answer must be equal there too.
"""
import ctypes as C
import os

import numpy as np
import pytest

from tests import cluster_model
from tests.util import GOLDEN

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def ctx():
    from terran_amd import runtime
    return runtime.get_context(0)


def _T():
    from terran_amd import lib
    return lib.GALLERY_ROW_TILE


def _pool_rows(seed, n, dim, pool=24):
    rng = np.random.default_rng(seed)
    base = rng.integers(-8, 9, (pool, dim)).astype(np.float32)
    return base[rng.integers(0, pool, n)]


def _check(g, rows, ids, threshold, min_samples, what):
    labels, degree, count, rounds = g.cluster(threshold, min_samples)
    wl, wd, wc = cluster_model.cluster(rows, ids, threshold, min_samples)
    assert labels.dtype == degree.dtype == np.int32 and labels.shape == degree.shape == (len(rows),)
    assert np.array_equal(degree, wd), what
    assert np.array_equal(labels, wl), what
    assert count == wc and 1 <= rounds <= len(rows) + 1, (what, count, wc, rounds)
    return labels, degree, count, rounds


def _exact_case(ctx, seed, n, dim, want_degree, ms, pool=24):
    from terran_amd import lib
    rows = _pool_rows(seed, n, dim, pool)
    ids = np.zeros(n, np.int32)
    threshold, mean = cluster_model.threshold_for_degree(rows, ids, want_degree)
    g = lib.Gallery(ctx, dim)
    g.add(rows, ids, False)
    out = [_check(g, rows, ids, threshold, m, (n, dim, m, threshold)) for m in ms]
    g.free()
    return out, mean


def _row_counts():
    T = _T()
    return [T - 1, T, T + 1, 3 * T + 1, 1, 2, 63, 64, 65]


@pytest.mark.parametrize('n', _row_counts())
def test_exact_tile_and_word_edges(ctx, n):
    """Tile edges (T - 1, T, T + 1, several tiles, one and two rows) and bit-word edges (63, 64, 65) under min_samples
    1, 2 and 4; duplicates everywhere, mean degree about 2."""
    out, mean = _exact_case(ctx, n, n, 512, 2.0, (1, 2, 4))
    assert n < 3 or out[0][2] >= 1, mean                                 # the threshold leaves something to cluster


@pytest.mark.parametrize('dim', [1, 2, 63, 64, 65, 1024])
def test_exact_dims(ctx, dim):
    """K tails (the stored row is zero-filled to the kernel's 64-float chunk), one chunk, two chunks and the widest row."""
    _exact_case(ctx, 300 + dim, _T() + 1, dim, 2.0, (1, 2, 4))


def _chain(n, first=0, dim=1024):
    rows = np.zeros((n, dim), np.float32)
    rows[np.arange(n), first + np.arange(n)] = 1
    rows[np.arange(n), first + np.arange(n) + 1] = 1
    return rows


@pytest.mark.parametrize('order', ['in order', 'permuted'])
def test_exact_chain_is_the_worst_diameter(ctx, order):
    """row_i = e_i + e_(i+1): 1023 rows in a path, threshold 1 (edge iff dot > 0).  Stored in order and under a fixed
    permutation (the component minimum then sits mid-chain and the jumps cross tiles)."""
    from terran_amd import lib
    n = 1023
    rows = _chain(n)
    perm = np.arange(n) if order == 'in order' else np.random.default_rng(5).permutation(n)
    rows = rows[perm]
    ids = np.zeros(n, np.int32)
    g = lib.Gallery(ctx, 1024)
    g.add(rows, ids, False)
    ends = np.nonzero((perm == 0) | (perm == n - 1))[0]
    for m in (1, 2, 3, 4):
        labels, degree, count, rounds = _check(g, rows, ids, 1.0, m, (order, m))
        print('cluster: chain of %d %s, min_samples %d: %d rounds' % (n, order, m, rounds))
        assert rounds <= 1024
        if m <= 3:
            assert count == 1 and (labels == 0).all()
            assert sorted(np.nonzero(degree < 3)[0].tolist()) == sorted(ends.tolist())   # at m = 3 the two ends are border rows
        else:
            assert count == 0 and (labels == -1).all()
    g.free()


def test_exact_two_interleaved_chains(ctx):
    """Two paths of 500, row by row in turn: two clusters, numbered by their smallest row."""
    from terran_amd import lib
    a, b = _chain(500, 0), _chain(500, 501)
    rows = np.empty((1000, 1024), np.float32)
    rows[0::2], rows[1::2] = a, b
    ids = np.zeros(1000, np.int32)
    g = lib.Gallery(ctx, 1024)
    g.add(rows, ids, False)
    for m in (1, 3):
        labels, _, count, rounds = _check(g, rows, ids, 1.0, m, m)
        print('cluster: two interleaved chains of 500, min_samples %d: %d rounds' % (m, rounds))
        assert count == 2 and labels.tolist() == [0, 1] * 500
    g.free()


def test_exact_border_rows_between_two_clusters(ctx):
    """Nine rows, an edge = a shared basis vector, min_samples 4.  Rows 1, 2, 3, 8 are a clique (cluster 0: smallest core
    row 1), rows 4, 6, 7 a triangle made core by their border neighbours (cluster 1).  Row 5 is not core and has core
    neighbours 4 (cluster 1, the lower ROW) and 8 (cluster 0): it joins cluster 0.  Row 0 is not core and has core
    neighbours 6 and 7 only: cluster 1."""
    from terran_amd import lib
    edges = [(1, 2), (1, 3), (1, 8), (2, 3), (2, 8), (3, 8), (4, 6), (4, 7), (6, 7), (5, 8), (5, 4), (0, 6), (0, 7)]
    rows = np.zeros((9, 9 + len(edges)), np.float32)
    rows[np.arange(9), np.arange(9)] = 1
    for k, (i, j) in enumerate(edges):
        rows[i, 9 + k] = rows[j, 9 + k] = 1
    ids = np.arange(9, dtype=np.int32)
    g = lib.Gallery(ctx, rows.shape[1])
    g.add(rows, ids, False)
    labels, degree, count, _ = _check(g, rows, ids, 1.0, 4, 'border')
    assert labels.tolist() == [1, 0, 0, 0, 1, 0, 1, 1, 0]
    assert degree.tolist() == [3, 4, 4, 4, 4, 3, 4, 4, 5] and count == 2
    g.free()


def test_exact_more_tile_pairs_than_workgroups(ctx):
    """5 003 rows are 40 tiles and 820 tile pairs for at most 256 workgroups: every workgroup walks three or four pairs,
    with the first chunk of its next pair prefetched behind the last of this one."""
    out, mean = _exact_case(ctx, 17, 5003, 64, 3.0, (1, 3), pool=300)
    print('cluster: 5003 rows, mean degree %.2f, %d / %d clusters' % (mean, out[0][2], out[1][2]))
    assert out[0][2] > 1


def test_tombstones_and_re_adding(ctx):
    """A path whose every ninth row carries id 4: removing the id cuts the path into pieces that are numbered by their new
    smallest rows; adding the same vectors again joins the pieces through NEW rows and leaves the old indices removed."""
    from terran_amd import lib
    n = 2 * _T() + 9
    rows = _chain(n, dim=512)
    ids = (np.arange(n) % 9).astype(np.int32)
    g = lib.Gallery(ctx, 512)
    g.add(rows, ids, False)
    labels, _, count, _ = _check(g, rows, ids, 1.0, 1, 'whole')
    assert count == 1
    gone = ids == 4
    assert g.remove([4]) == gone.sum()
    mids = np.where(gone, -1, ids).astype(np.int32)
    labels, degree, count, _ = _check(g, rows, mids, 1.0, 1, 'cut')
    assert (labels[gone] == -1).all() and (degree[gone] == 0).all() and count == gone.sum() + 1
    assert labels[0] == 0 and labels[5] == 1 and labels[14] == 2                     # pieces 0..3, 5..12, 14..21, ...
    _check(g, rows, mids, 1.0, 3, 'cut, min_samples 3')
    g.add(rows[gone], ids[gone], False)
    rows2, ids2 = np.concatenate([rows, rows[gone]]), np.concatenate([mids, ids[gone]])
    labels, degree, count, _ = _check(g, rows2, ids2, 1.0, 1, 're-added')
    assert count == 1 and (labels[:n][gone] == -1).all() and (degree[:n][gone] == 0).all() and (labels[n:] == 0).all()
    g.clear()
    labels, degree, count, rounds = g.cluster(1.0, 1)
    assert labels.shape == degree.shape == (0,) and count == 0 and rounds == 0
    g.add(rows[:7], ids[:7], False)                                     # a cleared gallery forgets the rows it held
    _check(g, rows[:7], ids[:7], 1.0, 1, 'after clear')
    g.free()


def test_growth_in_steps_equals_reserved(ctx):
    from terran_amd import lib
    rng = np.random.default_rng(9)
    n, dim = 3 * _T() + 1, 512
    rows = rng.normal(size=(n, dim)).astype(np.float32)
    ids = np.arange(n, dtype=np.int32)
    whole = lib.Gallery(ctx, dim, reserve=n)
    whole.add(rows, ids)
    steps = lib.Gallery(ctx, dim, reserve=0)
    for i in range(0, n, 7):
        steps.add(rows[i:i + 7], ids[i:i + 7])
    for threshold, m in ((1.0, 1), (0.95, 3)):
        a, b, again = whole.cluster(threshold, m), steps.cluster(threshold, m), steps.cluster(threshold, m)
        for x, y, z in zip(a[:3], b[:3], again[:3]):
            assert np.array_equal(x, y) and np.array_equal(y, z)
        assert a[1].max() > 1
    whole.free()
    steps.free()


def test_refusals(ctx, monkeypatch):
    from terran_amd import lib
    L = ctx.lib
    g = lib.Gallery(ctx, 16)
    g.add(np.eye(6, 16, dtype=np.float32), np.arange(6), False)
    for threshold, m in ((0.5, 0), (0.5, -1), (float('nan'), 1), (float('inf'), 1), (float('-inf'), 1)):
        with pytest.raises(lib.TerranAmdError) as e:
            g.cluster(threshold, m)
        assert e.value.code == lib.E_INVALID
    count, rounds = C.c_int32(7), C.c_int32(7)
    assert L.ta_gallery_cluster(g.h, 0.5, 1, None, None, C.byref(count), C.byref(rounds)) == lib.E_INVALID
    assert count.value == 0 and rounds.value == 0
    assert L.ta_gallery_cluster(None, 0.5, 1, None, None, None, None) == lib.E_INVALID
    labels = np.full(6, 9, np.int32)
    assert L.ta_gallery_cluster(g.h, 0.5, 1, lib.ptr(labels), None, None, None) == lib.OK   # every optional output left out
    assert labels.tolist() == [0, 1, 2, 3, 4, 5]
    monkeypatch.setenv('TA_GALLERY_CLUSTER_MAX_ROWS', '5')                # the test-only switch: six rows are one too many
    labels[:] = 9
    with pytest.raises(lib.TerranAmdError, match=r'limit is 2\^18 rows') as e:
        g.cluster(0.5, 1)
    assert e.value.code == lib.E_INVALID
    assert L.ta_gallery_cluster(g.h, 0.5, 1, lib.ptr(labels), None, None, None) == lib.E_INVALID and (labels == 9).all()
    monkeypatch.delenv('TA_GALLERY_CLUSTER_MAX_ROWS')
    assert g.cluster(0.5, 1)[2] == 6 and g.size() == (6, 6)              # the gallery is as it was
    g.free()


def _sphere_walks():
    """385 rows at dim 512: five random walks on the sphere, 77 steps each, then one permutation of all rows."""
    rng = np.random.default_rng(1)
    dim, rows = 512, []
    for walk in range(5):
        x = rng.normal(size=dim)
        x /= np.linalg.norm(x)
        for step in range(77):
            x = x + rng.uniform(0.3, 1.1) * rng.normal(size=dim) / np.sqrt(dim)
            x /= np.linalg.norm(x)
            rows.append(x.copy())
    rows = np.asarray(rows)
    return rows[rng.permutation(len(rows))].astype(np.float32)


@pytest.fixture(scope='module')
def real_case(ctx):
    """The walks, normalised on the device; the model's distances of the STORED rows and the widest gap between
    consecutive ones in (0.40, 0.60)."""
    from terran_amd import lib
    rows = _sphere_walks()
    g = lib.Gallery(ctx, 512)
    g.add(rows, np.zeros(len(rows), np.int32), True)
    stored, ids = g.download()
    d = np.unique(cluster_model.distances(stored).astype(np.float32).astype(np.float64))
    d = d[(d > 0.40) & (d < 0.60)]
    k = int(np.argmax(np.diff(d)))
    yield dict(g=g, stored=stored, ids=ids, gap=float(d[k + 1] - d[k]), threshold=float((d[k] + d[k + 1]) / 2))
    g.free()


@pytest.mark.parametrize('m', [1, 3, 4])
def test_real_valued_rows_normalised_on_the_device(real_case, m):
    c = real_case
    atol = (512 + 8) * 2.0 ** -24
    assert len(c['stored']) == 385
    assert np.abs(np.linalg.norm(c['stored'].astype(np.float64), axis=1) - 1).max() < 1e-6
    print('cluster: walks: threshold %.4f in a gap of %.1f ATOL' % (c['threshold'], c['gap'] / atol))
    assert c['gap'] >= 8 * atol, c['gap'] / atol
    labels, degree, count, rounds = _check(c['g'], c['stored'], c['ids'], c['threshold'], m, m)
    core = degree >= m
    print('cluster: walks, min_samples %d: %d core, %d clusters, %d border, %d noise, %d rounds'
          % (m, core.sum(), count, (~core & (labels >= 0)).sum(), (labels < 0).sum(), rounds))
    assert count > 1


def test_cluster_faces_end_to_end(states):
    """The face of rw-1.jpg embedded twice and the face of rw-2.jpg once, through Recognition and cluster_faces: the two
    embeddings of one face share a cluster, every face gets its cluster and, asked for, its 'person %d'."""
    from PIL import Image
    from terran_amd import Recognition, cluster_faces
    ims = [np.asarray(Image.open(os.path.join(GOLDEN, name)).convert('RGB')) for name in ('rw-1.jpg', 'rw-2.jpg')]
    h, w = min(im.shape[0] for im in ims), min(im.shape[1] for im in ims)
    ims = [np.ascontiguousarray(im[:h, :w]) for im in ims]
    lms = np.array([[38, 52], [74, 52], [56, 72], [42, 92], [70, 92]], np.float32) + np.array([w // 3, h // 4], np.float32)
    frames = [ims[0], ims[1], ims[0]]
    faces = [[{'landmarks': lms}], [{'landmarks': lms, 'text': 'kept'}], [{'landmarks': lms}]]
    rec = Recognition(device=0, state=states('arcface'))
    feats = rec(frames, faces)
    labels, reps = cluster_faces(faces, feats, threshold=0.5, min_samples=1, text='person %d', device=0)
    print('cluster: end to end labels %s representatives %s' % (labels.tolist(), reps.tolist()))
    assert labels.shape == (3,) and labels[0] == labels[2] == 0 and labels[1] in (0, 1)
    assert reps[0] == 0 and len(reps) == labels.max() + 1
    assert [f[0]['cluster'] for f in faces] == labels.tolist()
    assert faces[0][0]['text'] == faces[2][0]['text'] == 'person 0' and faces[1][0]['text'] == 'kept'
