"""DBSCAN restated in numpy from a distance matrix: the oracle of tests/test_gpu_cluster.py, itself
checked against scikit-learn in tests/test_cluster_ref.py.  The rules are those of
include/reidmi.h (reidmi_dbscan_f32): adjacency, union by smaller root, relabel, borders by the
smallest label."""
import numpy as np


def dbscan_ref(dm, eps, min_samples):
    """(labels int32 [N], core bool [N], counts int32 [N], n_clusters) from the [N][N] matrix dm.
    eps is compared in dm's dtype (fp32 distances: eps rounded to fp32)."""
    dm = np.asarray(dm)
    n = dm.shape[0]
    assert dm.shape == (n, n)
    adj = dm <= dm.dtype.type(eps)
    adj[np.arange(n), np.arange(n)] = True  # the diagonal counts whatever its rounding gave
    counts = adj.sum(1).astype(np.int32)
    core = counts >= min_samples
    parent = np.arange(n)

    def find(a):
        while parent[a] != a:
            a = parent[a]
        return a
    for i, j in zip(*np.nonzero(np.triu(adj & core[:, None] & core[None, :], 1))):
        a, b = find(i), find(j)
        if a != b:
            parent[max(a, b)] = min(a, b)
    root = np.array([find(i) for i in range(n)])
    roots = np.flatnonzero(core & (root == np.arange(n)))  # ascending: numbered by lowest core index
    number = np.full(n, -1, np.int64)
    number[roots] = np.arange(len(roots))
    labels = np.where(core, number[root], -1)
    for i in np.flatnonzero(~core):
        near = np.flatnonzero(adj[i] & core)
        if near.size:
            labels[i] = labels[near].min()
    return labels.astype(np.int32), core, counts, len(roots)


def contested(dm, eps, labels, core):
    """The border points whose core neighbours lie in more than one cluster."""
    dm = np.asarray(dm)
    adj = dm <= dm.dtype.type(eps)
    return [i for i in np.flatnonzero(~core & (labels >= 0)) if len(set(labels[adj[i] & core])) > 1]
