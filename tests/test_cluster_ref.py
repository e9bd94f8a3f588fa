"""tests/dbscan_ref.py (the oracle of tests/test_gpu_cluster.py) against scikit-learn's
DBSCAN(metric="precomputed") on a host distance matrix of the GPU tests' 300-row set, clamped at 0
with a zero diagonal (what scikit-learn accepts).  No GPU."""
import numpy as np
import pytest

from dbscan_ref import contested, dbscan_ref
from multimodal_reid_amd import synthetic as syn

N = 300


def _host_matrix(D):
    qp, gp, _, _ = syn.labels(10, N, num_ids=12, num_cams=6, seed=D)
    x = syn.features(qp, gp, dim=D, seed=D)[1]
    x = (x / np.linalg.norm(x, axis=1, keepdims=True)).astype(np.float32)
    sq = (x * x).sum(1)
    dm = np.maximum(sq[:, None] + sq[None, :] - np.float32(2) * (x @ x.T), np.float32(0)).astype(np.float32)
    dm = np.minimum(dm, dm.T)  # BLAS need not be symmetric to the last bit
    np.fill_diagonal(dm, 0)
    return dm


@pytest.mark.parametrize("D", [36, 33])
@pytest.mark.parametrize("min_samples,quantile", [(4, 0.01), (8, 0.02)])
def test_restatement_equals_sklearn(D, min_samples, quantile):
    cluster = pytest.importorskip("sklearn.cluster")
    dm = _host_matrix(D)
    eps = float(np.float32(np.quantile(dm, quantile)))
    labels, core, counts, n_clusters = dbscan_ref(dm, eps, min_samples)
    sk = cluster.DBSCAN(eps=eps, min_samples=min_samples, metric="precomputed").fit(dm)
    sk_core = np.zeros(N, bool)
    sk_core[sk.core_sample_indices_] = True
    assert np.array_equal(core, sk_core)
    assert np.array_equal(labels, sk.labels_.astype(np.int32))
    assert n_clusters == sk.labels_.max() + 1 and n_clusters >= 2
    assert np.array_equal(counts, (dm <= np.float32(eps)).sum(1))
    # the case is worth something: noise, border points, and border points two clusters contest
    assert (labels < 0).any() and (~core & (labels >= 0)).any()
    assert len(contested(dm, eps, labels, core)) > 0
