"""A numpy model of ta_gallery_cluster (terran_amd/csrc/gallery_cluster.hip): the definition, applied literally.

    d(i, j)   1 - row_i . row_j in float64 (gallery_model.py's line for normalize=0), cast to float32 for the comparison
    i ~ j     both rows live (id >= 0) and d(i, j) < float32(threshold); j = i like any other pair; NaN is no neighbour
    degree    number of j with i ~ j; core iff degree >= min_samples
    clusters  connected components of ~ among core rows, numbered by ascending smallest core row
    border    a live non-core row with a core neighbour joins the lowest-numbered cluster among its core neighbours'
    noise     everything else, removed rows included: -1
"""
import numpy as np


def distances(rows):
    """(n, n) float64."""
    r = np.asarray(rows, np.float64)
    with np.errstate(invalid='ignore', over='ignore'):
        return 1.0 - r @ r.T


def adjacency(rows, ids, threshold):
    """(n, n) bool, symmetric."""
    ids = np.asarray(ids).reshape(-1)
    with np.errstate(invalid='ignore', over='ignore'):
        adj = distances(rows).astype(np.float32) < np.float32(threshold)
    live = ids >= 0
    return adj & live[:, None] & live[None, :]


def cluster_adjacency(adj, min_samples):
    """(labels int32, degree int32, n_clusters) of a symmetric boolean adjacency."""
    adj = np.asarray(adj, bool)
    n = len(adj)
    assert adj.shape == (n, n) and np.array_equal(adj, adj.T)
    degree = adj.sum(1).astype(np.int32)
    core = degree >= min_samples
    labels = np.full(n, -1, np.int32)
    count = 0
    for i in range(n):                                    # ascending smallest core row: the first unlabelled core row opens a cluster
        if not core[i] or labels[i] >= 0:
            continue
        labels[i] = count
        stack = [i]
        while stack:
            a = stack.pop()
            for b in np.nonzero(adj[a] & core & (labels < 0))[0]:
                labels[b] = count
                stack.append(b)
        count += 1
    for i in np.nonzero(~core & (degree > 0))[0]:
        near = labels[adj[i] & core]
        if len(near):
            labels[i] = near.min()
    return labels, degree, count


def cluster(rows, ids, threshold, min_samples):
    """(labels, degree, n_clusters) of stored rows (n, dim) with ids (n,), -1 = removed."""
    if not len(rows):
        return np.empty(0, np.int32), np.empty(0, np.int32), 0
    return cluster_adjacency(adjacency(rows, ids, threshold), min_samples)


def threshold_for_degree(rows, ids, want):
    """For integer rows: the integer t whose threshold 1 - t (edge iff dot > t) brings the mean degree of the live rows
    closest to `want`, among the t that leave at least one edge; -> (float threshold, mean degree)."""
    r = np.asarray(rows, np.float64)
    live = np.asarray(ids) >= 0
    dots = (r @ r.T)[np.ix_(live, live)]
    vals, counts = np.unique(dots, return_counts=True)
    ts = np.concatenate([[vals[0] - 1], vals[:-1]])       # every t that gives another graph and keeps an edge
    above = counts[::-1].cumsum()[::-1]                    # edges at ts[k]: the dots >= vals[k], that is > ts[k]
    mean = above / live.sum()
    k = int(np.argmin(np.abs(mean - want)))
    return 1.0 - float(ts[k]), float(mean[k])
