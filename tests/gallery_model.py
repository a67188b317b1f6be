"""A numpy model of the gallery (terran_amd/csrc/gallery.hip): float64 distances, selection by (distance, row).

Distances come from `oracle.arcface_pre.cosine_distance` -- 1 - u.v / (|u| |v|), the restatement of match.py's
scipy call.  With `normalize=False` on both sides the library takes its operands as unit vectors and computes 1 - u.v;
the model then does the same in float64 (cosine_distance's formula with both norms equal to one), which is exact for the
integer data of the exact tests.  Removed rows never come back; with fewer than k live rows the tail is (-1, -1, +inf).
"""
import numpy as np

from oracle.arcface_pre import cosine_distance


class GalleryModel:
    def __init__(self, dim):
        self.dim = int(dim)
        self.clear()

    def clear(self):
        self.rows = np.empty((0, self.dim), np.float64)
        self.ids = np.empty(0, np.int32)

    def add(self, rows, ids):
        rows = np.asarray(rows, np.float64).reshape(-1, self.dim)
        ids = np.asarray(ids, np.int32).reshape(-1)
        assert len(rows) == len(ids) and (ids >= 0).all()
        self.rows = np.concatenate([self.rows, rows])
        self.ids = np.concatenate([self.ids, ids])

    def remove(self, ids):
        hit = np.isin(self.ids, np.asarray(ids, np.int32)) & (self.ids >= 0)
        self.ids = np.where(hit, np.int32(-1), self.ids)
        return int(hit.sum())

    def size(self):
        return len(self.ids), int((self.ids >= 0).sum())

    def distances(self, queries, normalize=True):
        """(nq, rows) float64, +inf at removed rows."""
        q = np.asarray(queries, np.float64).reshape(-1, self.dim)
        if not len(self.ids):
            return np.empty((len(q), 0), np.float64)
        if normalize:
            with np.errstate(invalid='ignore', divide='ignore'):
                d = cosine_distance(q, self.rows)
        else:
            d = 1.0 - q @ self.rows.T
        d[:, self.ids < 0] = np.inf
        return d

    def search(self, queries, k, normalize=True):
        """(row, id, distance): (nq, k) int32, int32, float64; ties go to the lower row."""
        d = self.distances(queries, normalize)
        nq, n = d.shape
        row = np.full((nq, k), -1, np.int32)
        ident = np.full((nq, k), -1, np.int32)
        dist = np.full((nq, k), np.inf, np.float64)
        live = np.nonzero(self.ids >= 0)[0]
        for i in range(nq):
            order = live[np.lexsort((live, d[i, live]))][:k]
            row[i, :len(order)] = order
            ident[i, :len(order)] = self.ids[order]
            dist[i, :len(order)] = d[i, order]
        return row, ident, dist
