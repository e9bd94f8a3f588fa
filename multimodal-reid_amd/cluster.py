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
