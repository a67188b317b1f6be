"""CPU tests (no GPU): FaceGallery's host side -- names and ids, remove, identify on flat and nested face lists, the
threshold edge, empty lists, save / load -- over a stand-in for lib.Gallery that answers from tests/gallery_model.py."""
import numpy as np
import pytest

from tests.gallery_model import GalleryModel


class FakeGallery:
    """lib.Gallery's interface on the numpy model; counts the searches.  Like the library it keeps float32 rows, normalised
    in float32 when they are added so (a zero row stays zero)."""
    searches = 0

    def __init__(self, ctx, dim, reserve=0):
        self.ctx, self.dim, self.model, self.add_flags = ctx, int(dim), GalleryModel(dim), []

    def add(self, rows, ids, normalize=True):
        rows = np.asarray(rows, np.float32)
        if normalize:
            nrm = np.sqrt((rows * rows).sum(1, dtype=np.float32))
            nrm[nrm == 0] = 1
            rows = rows / nrm[:, None]
        self.add_flags.append(bool(normalize))
        self.model.add(rows, ids)

    def remove(self, ids):
        return self.model.remove(ids)

    def clear(self):
        self.model.clear()

    def size(self):
        return self.model.size()

    def download(self):
        return self.model.rows.astype(np.float32), self.model.ids.copy()

    def search(self, queries, k=1, normalize=True):
        FakeGallery.searches += 1
        row, ident, dist = self.model.search(queries, k, normalize)
        return row, ident, dist.astype(np.float32)

    def free(self):
        pass


@pytest.fixture
def gallery(monkeypatch):
    from terran_amd import gallery as gallery_mod, lib
    monkeypatch.setattr(lib, 'Gallery', FakeGallery)
    FakeGallery.searches = 0
    return gallery_mod.FaceGallery(dim=8, ctx=object())


def _unit(i, dim=8):
    v = np.zeros(dim, np.float32)
    v[i] = 1
    return v


def test_face_gallery_is_exported():
    import terran_amd
    from terran_amd.gallery import FaceGallery
    assert terran_amd.FaceGallery is FaceGallery


def test_names_ids_and_remove(gallery):
    assert len(gallery) == 0 and gallery.names == []
    assert gallery.add('ada', _unit(0)) == 1
    assert gallery.add('bob', np.stack([_unit(1), _unit(2)])) == 2
    assert gallery.add('ada', 3 * _unit(3)) == 1                                   # a second embedding under a known name
    assert gallery.add('eve', np.empty((0, 8), np.float32)) == 0 and gallery.names == ['ada', 'bob']
    assert len(gallery) == 4 and gallery._g.model.ids.tolist() == [0, 1, 1, 0]
    names, dist, rows = gallery.search(np.stack([_unit(3), _unit(2), _unit(7)]), k=2)
    assert names.shape == dist.shape == rows.shape == (3, 2)
    assert names[0, 0] == 'ada' and rows[0, 0] == 3 and dist[0, 0] == 0
    assert names[1, 0] == 'bob' and rows[1, 0] == 2
    assert rows[2].tolist() == [0, 1] and np.all(dist[2] == 1)                     # orthogonal to all: ties go to the lower row
    with pytest.raises(ValueError):
        gallery.add('ada', np.zeros(7, np.float32))
    for name in (7, ('ada', 1), None):                                             # save / load keep names as text
        with pytest.raises(TypeError):
            gallery.add(name, _unit(0))
    assert len(gallery) == 4 and gallery.names == ['ada', 'bob']
    with pytest.raises(KeyError):
        gallery.remove('nobody')
    assert gallery.remove('bob') == 2
    assert gallery.names == ['ada'] and len(gallery) == 2
    with pytest.raises(KeyError):
        gallery.remove('bob')
    names, dist, rows = gallery.search(_unit(2), k=3)
    assert names[0].tolist() == ['ada', 'ada', None] and rows[0].tolist() == [0, 3, -1] and np.isinf(dist[0, 2])
    gallery.add('bob', _unit(2))                                                   # the name comes back under its old id
    assert gallery.search(_unit(2))[0][0, 0] == 'bob' and gallery.names == ['ada', 'bob']
    gallery.clear()
    assert len(gallery) == 0 and gallery.names == []
    assert gallery.search(_unit(0), k=2)[0].tolist() == [[None, None]]


def test_identify_flat_nested_and_the_threshold_edge(gallery):
    gallery.add('ada', _unit(0))
    gallery.add('bob', _unit(1))
    half = np.array([0.5, 0, np.sqrt(0.75), 0, 0, 0, 0, 0], np.float64)           # cosine distance to ada: 0.5 in float32
    near = np.array([0.9, 0, np.sqrt(1 - 0.81), 0, 0, 0, 0, 0], np.float64)       # 0.1
    feats = np.stack([_unit(1), half, near]).astype(np.float32)
    faces = [{'bbox': 0}, {'bbox': 1}, {'bbox': 2, 'text': 'kept'}]
    d_half = gallery.search(feats[1])[1][0, 0]
    assert d_half.dtype == np.float32 and abs(d_half - 0.5) < 1e-6
    out = gallery.identify(faces, feats, threshold=float(d_half))
    assert out is faces and FakeGallery.searches == 2                              # one search for the three faces
    assert faces[0]['text'] == 'bob' and faces[0]['distance'] == 0.0
    assert 'text' not in faces[1] and 'distance' not in faces[1]                   # a distance EQUAL to the threshold is no match
    assert faces[2]['text'] == 'ada' and abs(faces[2]['distance'] - 0.1) < 1e-6
    faces = [{'bbox': 1}]
    gallery.identify(faces, feats[1:2], threshold=float(np.nextafter(d_half, np.float32(1))))
    assert faces[0]['text'] == 'ada' and faces[0]['distance'] == float(d_half)

    FakeGallery.searches = 0
    nested = [[{'i': 0}], [], [{'i': 1}, {'i': 2}]]
    out = gallery.identify(nested, [feats[0:1], np.empty((0, 8), np.float32), feats[1:3]], threshold=0.2)
    assert out is nested and FakeGallery.searches == 1
    assert nested[0][0]['text'] == 'bob' and 'text' not in nested[2][0] and nested[2][1]['text'] == 'ada'
    with pytest.raises(ValueError):
        gallery.identify(nested, [feats[0:1], feats[1:3]])
    with pytest.raises(ValueError):
        gallery.identify([{'i': 0}, {'i': 1}], feats)


def test_identify_empty_lists_make_no_search(gallery):
    gallery.add('ada', _unit(0))
    FakeGallery.searches = 0
    assert gallery.identify([], np.empty((0, 8), np.float32)) == []
    assert gallery.identify([[], []], [np.empty((0, 8), np.float32)] * 2) == [[], []]
    assert FakeGallery.searches == 0
    empty = type(gallery)(dim=8, ctx=object())
    faces = [{'i': 0}]
    empty.identify(faces, _unit(0)[None])                                          # nothing enrolled: nobody is named
    assert faces == [{'i': 0}]


def test_save_load_round_trip(gallery, tmp_path):
    rng = np.random.default_rng(3)
    for name in ('ada', 'bob', 'zoë', 'dan'):
        gallery.add(name, rng.normal(size=(3, 8)).astype(np.float32))
    gallery.remove('bob')
    path = str(tmp_path / 'gallery.npz')
    gallery.save(path)
    again = type(gallery).load(path, ctx=object())
    assert again.dim == 8 and again.names == gallery.names == ['ada', 'zoë', 'dan'] and len(again) == len(gallery) == 9
    a, b = gallery._g.download(), again._g.download()
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])               # the same rows at the same indices
    assert again._g.add_flags == [False]                                           # loaded as stored: no second normalisation
    q = rng.normal(size=(5, 8)).astype(np.float32)
    for x, y in zip(gallery.search(q, k=4), again.search(q, k=4)):
        assert np.array_equal(x, y)
    again.add('bob', _unit(0))                                                     # ids go on where they stopped
    assert again.search(_unit(0))[0][0, 0] == 'bob' and again.names == ['ada', 'bob', 'zoë', 'dan']
    fresh = type(gallery)(dim=8, ctx=object())
    fresh.save(path)
    assert len(type(gallery).load(path, ctx=object())) == 0
