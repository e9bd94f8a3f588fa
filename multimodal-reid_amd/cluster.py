"""Group an unlabelled set of embeddings into identities: exact DBSCAN on the GPU, computed from
the features without the N x N distance matrix (reidmi_dbscan_f32, include/reidmi.h).

    dbscan_device(x, eps, min_samples=4, normalize=False) -> (labels, core, counts) on the device
    dbscan(x, eps, min_samples=4, normalize=False)        -> (labels, core, counts, n_clusters), numpy
    label_groups(labels)                                  -> (offsets, idx) of the non-noise labels
    cluster_centroids(x, labels, normalize=True)          -> fp32 [n_clusters][D], numpy

eps is in the units of evaluate.euclidean_distance: the SQUARED Euclidean distance, the scale of
search(max_dist=).  On L2-normalised rows that is 2 - 2 cos: a cosine of at least c is eps = 2 - 2 c,
and scikit-learn's DBSCAN(eps=e) on Euclidean distances is eps = e ** 2 here.

The labels are those of sklearn.cluster.DBSCAN(metric="precomputed") on euclidean_distance_device(x,
x): a point's neighbours are the points within eps (<=) and itself, a core point has at least
min_samples of them, clusters are the connected components of the core points numbered by their
lowest core index, a border point joins the lowest-numbered cluster among its core neighbours',
and the rest is noise (-1).  Memory grows linearly in N and the result is the same on every run.

The same rules on the k-reciprocal Jaccard distance of the set against itself, the distance
unsupervised and two-stage ReID pipelines cluster on (reidmi_dbscan_jaccard, from the sparse V_qe
rows of the re-rank, again without an N x N matrix):

    dbscan_jaccard_device(x, eps=0.6, min_samples=4, k1=30, k2=6, normalize=False, chunk_bytes=None)
    dbscan_jaccard(...)                                   -> as dbscan_device / dbscan
    jaccard_distance_device(x, k1=30, k2=6, rows=None, normalize=False) -> fp16 [rows][N], small N

That distance is the Jaccard term of this package's re_ranking, the reference's definition; eps is
compared in fp16 and must round to less than 1.
"""
import math

import numpy as np
import torch

from . import _lib
from .evaluate import _pitch, _rows_f32, combine_rows_device, l2_normalize_device


def _run(x, eps, min_samples, normalize):
    x = l2_normalize_device(x) if normalize else _rows_f32(x, "x")
    if x.dim() != 2:
        raise _lib.ReidmiError("dbscan: x must be [N][D]")
    eps = float(eps)
    if isinstance(min_samples, bool) or not isinstance(min_samples, (int, np.integer)):
        raise _lib.ReidmiError(f"dbscan: min_samples must be an integer, not {min_samples!r}")
    if not (math.isfinite(eps) and eps >= 0.0):
        raise _lib.ReidmiError(f"dbscan: eps must be finite and >= 0, not {eps!r}")
    n, d = x.shape
    dev = x.device
    labels = torch.empty(n, device=dev, dtype=torch.int32)
    counts = torch.empty(n, device=dev, dtype=torch.int32)
    core = torch.empty(n, device=dev, dtype=torch.uint8)
    n_clusters = torch.empty(1, device=dev, dtype=torch.int32)
    nb = _lib.load().reidmi_dbscan_workspace_bytes(n, d)
    ws = torch.empty(max(nb, 1), device=dev, dtype=torch.uint8)
    _lib.call("reidmi_dbscan_f32", _lib.ptr(x), n, d, _pitch(x), eps, int(min_samples), _lib.ptr(labels),
              _lib.ptr(counts), _lib.ptr(core), _lib.ptr(n_clusters), _lib.ptr(ws), nb, _lib.stream())
    return labels, core.view(torch.bool), counts, n_clusters


def dbscan_device(x, eps, min_samples=4, normalize=False):
    """DBSCAN of the rows of x (fp32 [N][D]; a device view with a row pitch is used in place): device
    (labels int32 [N], core bool [N], counts int32 [N]).  labels: the cluster number, -1 for noise;
    counts[i]: the points within eps of i, itself included.  eps is a SQUARED Euclidean distance
    (rounded to fp32, as the distances are); normalize=True clusters l2_normalize_device(x)."""
    return _run(x, eps, min_samples, normalize)[:3]


def dbscan(x, eps, min_samples=4, normalize=False):
    """dbscan_device as numpy arrays, plus the number of clusters: (labels, core, counts, n_clusters)."""
    labels, core, counts, n_clusters = _run(x, eps, min_samples, normalize)
    return labels.cpu().numpy(), core.cpu().numpy(), counts.cpu().numpy(), int(n_clusters.item())


# ------------------------------------------------- on the k-reciprocal Jaccard distance
def _int_arg(who, name, v, least=1):
    if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or v < least:
        raise _lib.ReidmiError(f"{who}: {name} must be an integer >= {least}, not {v!r}")
    return int(v)


def _jaccard_stages(who, x, k1, k2, normalize, chunk_bytes):
    """V_qe of all N rows of x and its inverted index, through the re-rank's stages (R2-R5 of
    reranking.HipStages over the rows 0..N; the number of queries plays no part in them):
    (N, device, (qoff, qcol, qval), (coff, irow, ival))."""
    from .reranking import HipStages
    k1, k2 = _int_arg(who, "k1", k1), _int_arg(who, "k2", k2)
    x = l2_normalize_device(x) if normalize else _rows_f32(x, "x")
    if x.dim() != 2 or x.shape[0] < 1 or x.shape[1] < 1:
        raise _lib.ReidmiError(f"{who}: x must be [N][D] with N >= 1 and D >= 1")
    if x.shape[0] == 1:
        # a lone row is its own k-reciprocal set, with weight 1: V_qe = [[1]] and jd(0, 0) = 0.  (The
        # stages divide a distance row by its maximum, which is 0 here; the reference fails earlier.)
        off = torch.tensor([0, 1], device=x.device, dtype=torch.int64)
        col = torch.zeros(1, device=x.device, dtype=torch.int32)
        val = torch.ones(1, device=x.device, dtype=torch.float16).view(torch.int16)
        return 1, x.device, (off, col, val), (off.clone(), col.clone(), val.clone())
    st = HipStages(x, x.shape[0], k1, k2, 0.0, chunk_bytes)
    n = st.N
    R, rmax = st.rank_rows(0, n)
    nnz, col, val = st.v_rows(R, rmax, 0, n)  # R3
    Vq = (st.offsets(nnz), col, val)
    if k2 != 1 and st.k2e >= 2:  # R4 (as staged_rerank: otherwise the mean is V itself)
        nnz, col, val = st.qe_rows(R, Vq, 0, n)
        Vq = (st.offsets(nnz), col, val)
    csc = st._csc(Vq)  # R5
    st.check()
    return n, st.dev, Vq, csc


def jaccard_distance_device(x, k1=30, k2=6, rows=None, normalize=False):
    """The k-reciprocal Jaccard distance of the rows of x against themselves, dense: fp16
    [hi - lo][N] on the device for rows = (lo, hi), all N rows by default.  The small-N form (2 N^2
    bytes for all rows); dbscan_jaccard_device clusters on the same values without it.  This is
    the Jaccard term of this package's re_ranking, the reference's definition (reranking.py:86-93
    on V_qe of all N items, every operation in fp16): other code bases' compute_jaccard_distance
    variants build V differently and give other values.  The matrix is bit-symmetric, its
    diagonal is small but not exactly zero, and some entries are slightly negative."""
    who = "jaccard_distance"
    lo, hi = (0, len(x)) if rows is None else rows
    lo, hi = _int_arg(who, "rows[0]", lo, 0), _int_arg(who, "rows[1]", hi, 0)
    if not lo <= hi <= len(x):
        raise _lib.ReidmiError(f"{who}: rows must satisfy 0 <= lo <= hi <= N, not {(lo, hi)!r}")
    n, dev, Vq, csc = _jaccard_stages(who, x, k1, k2, normalize, None)
    out = torch.empty((hi - lo, n), device=dev, dtype=torch.float16)
    if hi > lo:
        bb = int(_lib.load().reidmi_rr_jaccard_bounds_bytes(n, n))
        bounds = torch.empty((bb + 7) // 8, device=dev, dtype=torch.int64)
        _lib.call("reidmi_rr_jaccard_self_rows", n, lo, hi, *(_lib.ptr(t) for t in Vq + csc), _lib.ptr(out), n,
                  _lib.ptr(bounds), bb, _lib.stream())
    return out


def _run_jaccard(x, eps, min_samples, k1, k2, normalize, chunk_bytes):
    who = "dbscan_jaccard"
    eps = float(eps)
    min_samples = _int_arg(who, "min_samples", min_samples)
    with np.errstate(over="ignore"):
        if not (math.isfinite(eps) and eps >= 0.0 and np.float16(eps) < 1):
            raise _lib.ReidmiError(f"{who}: eps must be >= 0 and round to less than 1 in fp16, not {eps!r}")
    n, dev, Vq, csc = _jaccard_stages(who, x, k1, k2, normalize, chunk_bytes)
    labels = torch.empty(n, device=dev, dtype=torch.int32)
    counts = torch.empty(n, device=dev, dtype=torch.int32)
    core = torch.empty(n, device=dev, dtype=torch.uint8)
    n_clusters = torch.empty(1, device=dev, dtype=torch.int32)
    nb = int(_lib.load().reidmi_dbscan_jaccard_workspace_bytes(n))
    ws = torch.empty(nb, device=dev, dtype=torch.uint8)
    _lib.call("reidmi_dbscan_jaccard", n, *(_lib.ptr(t) for t in Vq + csc), eps, min_samples, _lib.ptr(labels),
              _lib.ptr(counts), _lib.ptr(core), _lib.ptr(n_clusters), _lib.ptr(ws), nb, _lib.stream())
    return labels, core.view(torch.bool), counts, n_clusters


def dbscan_jaccard_device(x, eps=0.6, min_samples=4, k1=30, k2=6, normalize=False, chunk_bytes=None):
    """DBSCAN of the rows of x on their k-reciprocal Jaccard distance (jaccard_distance_device's
    values and definition), what unsupervised and two-stage ReID pipelines cluster on: device
    (labels int32 [N], core bool [N], counts int32 [N]) as dbscan_device.  The stages of the re-rank
    build V_qe of all N rows and its inverted index (chunk_bytes: their distance scratch per row
    pass, as re_ranking_search_device), then one reidmi_dbscan_jaccard call clusters from those
    sparse rows: no N x N matrix.  eps is rounded to fp16, as the distance is, and must round to
    less than 1 (at 1 every pair would be a neighbour)."""
    return _run_jaccard(x, eps, min_samples, k1, k2, normalize, chunk_bytes)[:3]


def dbscan_jaccard(x, eps=0.6, min_samples=4, k1=30, k2=6, normalize=False, chunk_bytes=None):
    """dbscan_jaccard_device as numpy arrays, plus the number of clusters: (labels, core, counts,
    n_clusters)."""
    labels, core, counts, n_clusters = _run_jaccard(x, eps, min_samples, k1, k2, normalize, chunk_bytes)
    return labels.cpu().numpy(), core.cpu().numpy(), counts.cpu().numpy(), int(n_clusters.item())


def label_groups(labels):
    """The members of every cluster as the lists combine_rows_device takes (the form pool_features
    builds from its group keys): offsets int64 [n_clusters + 1] and idx int32, cluster c's rows are
    idx[offsets[c]:offsets[c + 1]] in ascending row index.  Noise (-1) is in no list; a cluster
    number without a member gets an empty one."""
    labels = np.asarray(labels.cpu() if isinstance(labels, torch.Tensor) else labels).reshape(-1)
    if labels.dtype.kind not in "iu":
        raise _lib.ReidmiError("label_groups: labels must be integers")
    labels = labels.astype(np.int64)
    kept = np.flatnonzero(labels >= 0)
    n_clusters = int(labels.max()) + 1 if kept.size else 0
    offsets = np.zeros(n_clusters + 1, np.int64)
    np.cumsum(np.bincount(labels[kept], minlength=n_clusters), out=offsets[1:])
    idx = kept[np.argsort(labels[kept], kind="stable")].astype(np.int32)
    return offsets, idx


def cluster_centroids(x, labels, normalize=True):
    """The mean of every cluster's rows of x, L2-normalised unless normalize=False: fp32
    [n_clusters][D] as a numpy array; row c is cluster c (the pseudo-label), noise takes no part.
    One reidmi_combine_rows_f32 call over label_groups(labels), so the arithmetic is
    combine_rows_device's: the rows of a cluster added in ascending row index into one fp32
    accumulator per column, divided by the count, then normalised."""
    offsets, idx = label_groups(labels)
    return combine_rows_device(x, offsets, idx, mode="mean", normalize=normalize).cpu().numpy()
