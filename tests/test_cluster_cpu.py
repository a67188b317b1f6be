"""CPU tests (no GPU): the numpy model of ta_gallery_cluster (tests/cluster_model.py) against sklearn's DBSCAN on the same
adjacency, cluster_representatives, FaceGallery.cluster and cluster_faces over a stand-in for lib.Gallery that answers from
the model, and the host half of the C call (argument checks, renumbering) as a stand-alone program under ASan + UBSan."""
import os
import subprocess

import numpy as np
import pytest

from tests import cluster_model
from tests.test_gallery_cpu import FakeGallery
from tests.util import REPO


class FakeClusterGallery(FakeGallery):
    """FakeGallery plus `cluster` from the model; counts the cluster calls and remembers which instances were freed."""
    clusters = 0
    made = []
    fail = None

    def __init__(self, ctx, dim, reserve=0):
        super().__init__(ctx, dim, reserve)
        self.freed = 0
        FakeClusterGallery.made.append(self)

    def cluster(self, threshold, min_samples=1):
        FakeClusterGallery.clusters += 1
        if FakeClusterGallery.fail is not None:
            raise FakeClusterGallery.fail
        rows = self.model.rows.astype(np.float32)            # the library keeps float32 rows
        labels, degree, count = cluster_model.cluster(rows, self.model.ids, threshold, min_samples)
        return labels, degree, count, 1

    def free(self):
        self.freed += 1


@pytest.fixture
def fake(monkeypatch):
    from terran_amd import lib
    monkeypatch.setattr(lib, 'Gallery', FakeClusterGallery)
    FakeClusterGallery.clusters, FakeClusterGallery.made, FakeClusterGallery.fail = 0, [], None
    return FakeClusterGallery


def _random_graph(seed, n=60, p=0.06):
    rng = np.random.default_rng(seed)
    upper = np.triu(rng.random((n, n)) < p, 1)
    adj = upper | upper.T
    np.fill_diagonal(adj, True)                              # a row is its own neighbour
    adj[:, rng.random(n) < 0.05] = False                     # a few rows that are nobody's neighbour (removed, zero, NaN)
    return adj & adj.T


def _two_cluster_borders(adj, min_samples):
    """Border rows whose core neighbours lie in more than one cluster."""
    labels, degree, _ = cluster_model.cluster_adjacency(adj, min_samples)
    core = degree >= min_samples
    return [i for i in np.nonzero(~core & (labels >= 0))[0] if len(set(labels[adj[i] & core])) > 1]


@pytest.mark.parametrize('m', [1, 2, 4])
def test_model_equals_sklearn_dbscan(m):
    """Labels array-equal, numbering included, on random graphs; for m > 1 some of them hold border rows with core
    neighbours in two clusters (the lowest-numbered one wins in both)."""
    DBSCAN = pytest.importorskip('sklearn.cluster').DBSCAN
    contested = 0
    for seed in range(40):
        adj = _random_graph(seed, p=0.03 + 0.002 * seed)
        labels, degree, count = cluster_model.cluster_adjacency(adj, m)
        want = DBSCAN(eps=0.5, min_samples=m, metric='precomputed').fit(np.where(adj, 0.0, 1.0)).labels_
        assert np.array_equal(labels, want), (seed, m)
        assert count == want.max() + 1 and np.array_equal(degree, adj.sum(1))
        contested += len(_two_cluster_borders(adj, m))
    # (a row counts itself, so a row with any neighbour but itself has degree >= 2: border rows exist from m = 3 on)
    assert contested > 0 or m < 3


def test_model_definition_on_rows():
    """Distances in float64, compared in float32 with <; removed rows, a zero row and a NaN row are nobody's neighbour."""
    e = np.eye(6, dtype=np.float32)
    rows = np.stack([e[0], e[0], e[1], 0 * e[0], e[2], e[2]])
    rows[4, 5] = np.nan
    ids = np.array([0, 1, 2, 3, 4, -1], np.int32)
    labels, degree, count = cluster_model.cluster(rows, ids, 0.5, 1)
    assert labels.tolist() == [0, 0, 1, -1, -1, -1] and degree.tolist() == [2, 2, 1, 0, 0, 0] and count == 2
    half = np.array([[1, 0], [0.5, np.sqrt(0.75)]], np.float32)           # distance 0.5 in float32: no edge at 0.5
    assert cluster_model.cluster(half, [0, 0], 0.5, 1)[0].tolist() == [0, 1]
    assert cluster_model.cluster(half, [0, 0], float(np.nextafter(np.float32(0.5), np.float32(1))), 1)[0].tolist() == [0, 0]
    assert cluster_model.cluster(np.empty((0, 4)), [], 0.5, 1)[2] == 0


def test_cluster_representatives_and_ties():
    from terran_amd.gallery import cluster_representatives
    labels = np.array([1, 0, -1, 0, 1, 0, 1, -1], np.int32)
    degree = np.array([3, 2, 9, 4, 3, 4, 1, 0], np.int32)
    assert cluster_representatives(labels, degree).tolist() == [3, 0]      # ties go to the lower row; noise never represents
    assert cluster_representatives([], []).tolist() == []
    assert cluster_representatives([-1, -1], [0, 0]).tolist() == []
    assert cluster_representatives([0], [0]).tolist() == [0]
    with pytest.raises(ValueError):
        cluster_representatives([0, 0], [1])


def _unit(i, dim=8):
    v = np.zeros(dim, np.float32)
    v[i] = 1
    return v


def test_cluster_faces_is_exported():
    import terran_amd
    from terran_amd.gallery import cluster_faces
    assert terran_amd.cluster_faces is cluster_faces


def test_face_gallery_cluster(fake):
    from terran_amd.gallery import FaceGallery
    g = FaceGallery(dim=8, ctx=object())
    g.add('ada', np.stack([_unit(0), _unit(0) + 0.1 * _unit(1)]))
    g.add('bob', _unit(2))
    g.add('adah', _unit(0) + 0.1 * _unit(3))                               # the same person under a second name
    labels, degree = g.cluster()
    assert labels.tolist() == [0, 0, 1, 0] and degree.tolist() == [3, 3, 1, 3] and labels.dtype == np.int32
    assert g.cluster(min_samples=2)[0].tolist() == [0, 0, -1, 0]
    g.remove('ada')
    assert g.cluster()[0].tolist() == [-1, -1, 0, 1]                        # removed rows keep their index and are noise
    assert fake.clusters == 3


def test_cluster_faces_flat_text_and_noise(fake):
    from terran_amd.gallery import cluster_faces
    feats = np.stack([_unit(0), 3 * _unit(1), _unit(0) + 0.1 * _unit(2), _unit(1), _unit(5)]).astype(np.float32)
    faces = [{'i': 0}, {'i': 1, 'text': 'bob'}, {'i': 2}, {'i': 3}, {'i': 4}]
    labels, reps = cluster_faces(faces, feats, min_samples=2, text='person %d', ctx=object())
    assert labels.tolist() == [0, 1, 0, 1, -1] and reps.tolist() == [0, 1]
    assert [f.get('cluster') for f in faces] == [0, 1, 0, 1, None]
    assert [f.get('text') for f in faces] == ['person 0', 'bob', 'person 0', 'person 1', None]   # a name from identify stays
    assert faces[4] == {'i': 4}                                            # noise: untouched
    assert fake.clusters == 1 and len(fake.made) == 1 and fake.made[0].freed == 1
    assert fake.made[0].add_flags == [True]                                # normalised on the way in
    faces = [{'i': 0}, {'i': 1}]
    cluster_faces(faces, feats[:2], ctx=object())                          # no text asked for: none written
    assert faces == [{'i': 0, 'cluster': 0}, {'i': 1, 'cluster': 1}]
    single = [{'i': 0}]
    labels, reps = cluster_faces(single, feats[0], ctx=object())           # one (dim,) embedding
    assert labels.tolist() == [0] and reps.tolist() == [0]


def test_cluster_faces_nested(fake):
    from terran_amd.gallery import cluster_faces
    nested = [[{'i': 0}], [], [{'i': 1}, {'i': 2}]]
    feats = [_unit(0)[None], np.empty((0, 8), np.float32), np.stack([_unit(3), _unit(0)])]
    labels, reps = cluster_faces(nested, feats, text='person %d', ctx=object())
    assert labels.tolist() == [0, 1, 0] and reps.tolist() == [0, 1] and fake.clusters == 1
    assert nested[0][0]['cluster'] == 0 and nested[2][0]['cluster'] == 1 and nested[2][1]['text'] == 'person 0'


def test_cluster_faces_empty_and_mismatched(fake):
    from terran_amd.gallery import cluster_faces
    for faces, feats in (([], np.empty((0, 8), np.float32)), ([[], []], [np.empty((0, 8), np.float32)] * 2)):
        labels, reps = cluster_faces(faces, feats, ctx=None)               # no context is even looked up
        assert labels.shape == (0,) and labels.dtype == np.int32 and reps.shape == (0,)
    assert fake.clusters == 0 and fake.made == []
    with pytest.raises(ValueError, match='2 feature arrays for 3 images'):
        cluster_faces([[{'i': 0}], [], [{'i': 1}]], [_unit(0)[None], _unit(1)[None]], ctx=object())
    with pytest.raises(ValueError, match='3 embeddings for 2 faces'):
        cluster_faces([{'i': 0}, {'i': 1}], np.stack([_unit(0), _unit(1), _unit(2)]), ctx=object())
    assert fake.made == []


def test_cluster_faces_frees_the_gallery_when_cluster_raises(fake):
    from terran_amd.gallery import cluster_faces
    fake.fail = RuntimeError('device lost')
    faces = [{'i': 0}, {'i': 1}]
    with pytest.raises(RuntimeError, match='device lost'):
        cluster_faces(faces, np.stack([_unit(0), _unit(1)]), text='person %d', ctx=object())
    assert len(fake.made) == 1 and fake.made[0].freed == 1
    assert faces == [{'i': 0}, {'i': 1}]


def test_host_half_under_sanitizers(tmp_path):
    """Argument checks and renumbering of ta_gallery_cluster (csrc/gallery_cluster_host.h), built as a program of their own
    with -fsanitize=address,undefined and run: nothing is loaded into Python."""
    exe = str(tmp_path / 'cluster_host_check')
    cmd = ['g++', '-std=c++17', '-O1', '-g', '-fsanitize=address,undefined', '-fno-sanitize-recover=all', '-static-libasan', '-static-libubsan',
           '-I', os.path.join(REPO, 'terran_amd', 'csrc'), os.path.join(REPO, 'tests', 'native', 'cluster_host_check.cpp'), '-o', exe]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    assert r.returncode == 0, r.stdout.decode(errors='replace')
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    assert r.returncode == 0 and r.stdout.decode().strip().endswith('ok'), r.stdout.decode(errors='replace')
