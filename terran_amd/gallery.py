"""Who is this face?  A gallery of named embeddings resident on the GPU, searched by cosine distance.

    gallery = FaceGallery()
    gallery.add('ada', extract_features(image, face))
    ...
    faces = face_detection(frames)
    gallery.identify(faces, extract_features(frames, faces))     # sets face['text'] = name where distance < 0.5
    vis.draw_faces(frames, faces, labels=True)

`examples/match.py` of the reference compares one face with every face of a directory through
`scipy.spatial.distance.cosine` and keeps those under 0.5; here the known faces stay on the device (lib.Gallery:
ta_gallery_* in include/terran_amd.h) and one call finds the k nearest of every query.  Names live on the host: every name
owns one int32 id, and the rows added under it carry that id.

Without a watch-list -- who appears in this video, and which faces are the same person? -- `cluster_faces` groups the
faces of any number of frames by their embeddings (DBSCAN on the device, ta_gallery_cluster) and
`cluster_representatives` picks the face to show for each group; `FaceGallery.cluster` does the same over an enrolled
gallery, where two names in one cluster are probably one person.
"""
import numpy as np

from . import lib


class FaceGallery:
    def __init__(self, dim=512, ctx=None, device=None, reserve=0):
        if ctx is None:
            from . import runtime
            ctx = runtime.get_context(device)
        self.ctx = ctx
        self.dim = int(dim)
        self._g = lib.Gallery(ctx, self.dim, reserve)
        self._names = []                  # id -> name
        self._ids = {}                    # name -> id
        self._count = {}                  # name -> live rows

    # ---- bookkeeping ----------------------------------------------------------------------
    def _features(self, features):
        f = np.asarray(features, dtype=np.float32)
        if f.ndim == 1:
            f = f[None]
        if f.ndim != 2 or f.shape[1] != self.dim:
            raise ValueError('features of shape %s are not (%d,) or (n, %d)' % (np.shape(features), self.dim, self.dim))
        return np.ascontiguousarray(f)

    def add(self, name, features, normalize=True):
        """One (dim,) or many (n, dim) embeddings under one name; returns the number of rows added."""
        if not isinstance(name, str):
            raise TypeError('a name is a str (save / load keep names as text), not %r' % (name,))
        f = self._features(features)
        if not len(f):
            return 0
        ident = self._ids.get(name)
        if ident is None:
            ident = len(self._names)
            self._names.append(name)
            self._ids[name] = ident
        self._g.add(f, np.full(len(f), ident, np.int32), normalize)
        self._count[name] = self._count.get(name, 0) + len(f)
        return len(f)

    def remove(self, name):
        """Forget every embedding of `name` (KeyError if it has none); returns how many rows that were."""
        if not self._count.get(name):
            raise KeyError(name)
        removed = self._g.remove([self._ids[name]])
        self._count[name] = 0
        return removed

    def clear(self):
        self._g.clear()
        self._names, self._ids, self._count = [], {}, {}

    def __len__(self):
        """Embeddings held (removed ones do not count)."""
        return self._g.size()[1]

    @property
    def names(self):
        """The names that have embeddings, in the order they were first added."""
        return [n for n in self._names if self._count.get(n)]

    # ---- queries --------------------------------------------------------------------------
    def search(self, features, k=1, normalize=True):
        """(names, distances, rows), each (n, k): the k nearest embeddings of every query by (distance, row) ascending.
        With fewer than k embeddings held the tail is (None, +inf, -1)."""
        f = self._features(features)
        rows, ids, dist = self._g.search(f, k, normalize)
        names = np.empty(ids.shape, object)
        for i, j in zip(*np.nonzero(ids >= 0)):
            names[i, j] = self._names[ids[i, j]]
        return names, dist, rows

    def identify(self, faces, features, threshold=0.5):
        """faces: one image's list of face dicts, or a list of such lists (one per image); features: what
        `extract_features` returned for them.  ONE search for all faces; a face whose nearest embedding lies at a distance
        < threshold (match.py's comparison) gets face['text'] = that name and face['distance']; the others are left as they
        are.  Returns `faces`."""
        nested = any(isinstance(f, (list, tuple)) for f in faces)
        if nested:
            if len(features) != len(faces):
                raise ValueError('%d feature arrays for %d images' % (len(features), len(faces)))
            flat = [face for per_image in faces for face in per_image]
            parts = [self._features(f) for per_image, f in zip(faces, features) if len(per_image)]
            feats = np.concatenate(parts) if parts else np.empty((0, self.dim), np.float32)
        else:
            flat = list(faces)
            feats = self._features(features) if len(flat) else np.empty((0, self.dim), np.float32)
        if len(feats) != len(flat):
            raise ValueError('%d embeddings for %d faces' % (len(feats), len(flat)))
        if not flat:
            return faces
        names, dist, _ = self.search(feats, k=1)
        for face, name, d in zip(flat, names[:, 0], dist[:, 0]):
            if name is not None and d < threshold:
                face['text'] = name
                face['distance'] = float(d)
        return faces

    def cluster(self, threshold=0.5, min_samples=1):
        """(labels, degree) over the stored rows, removed ones included: DBSCAN with cosine distance < threshold as the
        neighbourhood (lib.Gallery.cluster).  labels[i] is row i's cluster, numbered by ascending smallest core row, or
        -1 (noise, removed); degree[i] the number of rows within the threshold, the row itself included.
        min_samples=1 is single linkage.  Two names in one cluster are probably one person, enrolled twice:

            labels, _ = gallery.cluster()
            _, ids = gallery._g.download()
            for c in range(labels.max() + 1):
                names = {gallery._names[i] for i in ids[labels == c] if i >= 0}
                if len(names) > 1:
                    print('one person?', sorted(names))
        """
        labels, degree, _, _ = self._g.cluster(threshold, min_samples)
        return labels, degree

    # ---- persistence ----------------------------------------------------------------------
    def save(self, path):
        """One .npz: the stored (normalised) rows, their ids (-1: removed) and the names."""
        rows, ids = self._g.download()
        names = np.array(self._names, dtype=str) if self._names else np.empty(0, '<U1')
        with open(path, 'wb') as fh:
            np.savez(fh, rows=rows, ids=ids, names=names, dim=np.int32(self.dim))

    @classmethod
    def load(cls, path, ctx=None, device=None, reserve=0):
        """The gallery `save` wrote: same rows at the same indices, stored as they were (no second normalisation), so that
        it answers bit for bit as before."""
        with np.load(path, allow_pickle=False) as z:
            rows, ids, names, dim = z['rows'], z['ids'].astype(np.int32), [str(n) for n in z['names']], int(z['dim'])
        g = cls(dim=dim, ctx=ctx, device=device, reserve=max(int(reserve), len(rows)))
        g._names = names
        g._ids = {n: i for i, n in enumerate(names)}
        g._count = {n: int((ids == i).sum()) for i, n in enumerate(names)}
        if len(rows):
            gone = len(names)                        # removed rows keep their index: added under a spare id, removed again
            g._g.add(rows, np.where(ids < 0, gone, ids).astype(np.int32), False)
            if (ids < 0).any():
                g._g.remove([gone])
        return g

    def free(self):
        self._g.free()


def cluster_representatives(labels, degree):
    """One row per cluster, (n_clusters,) int64: the member with the most neighbours, ties to the lower row -- the chip to
    show for "person 3".  Host only."""
    labels, degree = np.asarray(labels).reshape(-1), np.asarray(degree).reshape(-1)
    if len(labels) != len(degree):
        raise ValueError('%d labels for %d degrees' % (len(labels), len(degree)))
    n = int(labels.max()) + 1 if len(labels) else 0
    reps = np.full(max(n, 0), -1, np.int64)
    best = np.full(max(n, 0), -1, np.int64)
    for row in np.nonzero(labels >= 0)[0]:
        c = labels[row]
        if degree[row] > best[c]:
            best[c], reps[c] = degree[row], row
    return reps


def _rows_2d(f):
    f = np.asarray(f, dtype=np.float32)
    return f[None] if f.ndim == 1 else f


def cluster_faces(faces, features, threshold=0.5, min_samples=1, text=None, ctx=None, device=None):
    """Which faces are the same person?  faces: one image's list of face dicts, or a list of such lists (one per image);
    features: what `extract_features` returned for them -- as `FaceGallery.identify` takes them.  The embeddings go into a
    temporary gallery on the device and ONE cluster call groups them (DBSCAN, cosine distance < threshold, see
    `FaceGallery.cluster`).  Every clustered face gets face['cluster'] = int; noise faces are left as they are.  With
    text='person %d' a clustered face that has no face['text'] yet gets one, which `draw_faces(..., labels=True)`
    writes; names from `identify` stay.  Returns (labels, representatives): labels (n_faces,) int32 in flat order,
    representatives (n_clusters,) flat indices of the face to show per cluster (`cluster_representatives`)."""
    nested = any(isinstance(f, (list, tuple)) for f in faces)
    if nested:
        if len(features) != len(faces):
            raise ValueError('%d feature arrays for %d images' % (len(features), len(faces)))
        flat = [face for per_image in faces for face in per_image]
        parts = [_rows_2d(f) for per_image, f in zip(faces, features) if len(per_image)]
        feats = np.concatenate(parts) if parts else np.empty((0, 0), np.float32)
    else:
        flat = list(faces)
        feats = _rows_2d(features) if len(flat) else np.empty((0, 0), np.float32)
    if feats.ndim != 2 or len(feats) != len(flat):
        raise ValueError('%d embeddings for %d faces' % (len(feats) if feats.ndim else 0, len(flat)))
    if not flat:
        return np.empty(0, np.int32), np.empty(0, np.int64)
    if ctx is None:
        from . import runtime
        ctx = runtime.get_context(device)
    g = lib.Gallery(ctx, feats.shape[1], len(feats))
    try:
        g.add(np.ascontiguousarray(feats), np.zeros(len(feats), np.int32), True)
        labels, degree, _, _ = g.cluster(threshold, min_samples)
    finally:
        g.free()
    for face, label in zip(flat, labels):
        if label >= 0:
            face['cluster'] = int(label)
            if text is not None and 'text' not in face:
                face['text'] = text % int(label)
    return labels, cluster_representatives(labels, degree)
