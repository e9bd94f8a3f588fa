"""tests/jaccard_ref.py against the C oracle: the oracle's `jac` with num_query = N (lambda 0) is the
self-Jaccard matrix, bit for bit what both numpy restatements give from its V_qe, and the matrix is
bit-symmetric.  These pin the reference of tests/test_gpu_cluster_jaccard.py."""
import numpy as np
import pytest

import oracle
from dbscan_ref import contested, dbscan_ref
from jaccard_ref import dense_to_csr, fixture, jaccard_self_csr, jaccard_self_dense

K = [(20, 6), (6, 1), (70, 6)]
_cache = {}


def _oracle(D, k1, k2):
    if (D, k1, k2) not in _cache:
        x = fixture(D)
        _, _, vqe, jac = oracle.rerank_from_dist(oracle.distmat(x, x), len(x), k1, k2, 0.0, debug=True)
        for a in (vqe, jac):
            a.setflags(write=False)
        _cache[D, k1, k2] = vqe, jac
    return _cache[D, k1, k2]


@pytest.mark.parametrize("D", [32, 33])
@pytest.mark.parametrize("k1,k2", K)
def test_helpers_equal_the_oracle(D, k1, k2):
    vqe, jac = _oracle(D, k1, k2)
    assert jac.shape == (232, 232) and np.array_equal(jac, jac.T)
    assert np.array_equal(jaccard_self_dense(vqe).view(np.uint16), jac)
    assert np.array_equal(jaccard_self_csr(*dense_to_csr(vqe)).view(np.uint16), jac)


@pytest.mark.parametrize("D", [32, 33])
def test_the_matrix_is_what_the_clustering_tests_assume(D):
    """Small nonzero diagonal, negative entries, jd = 1 exactly without a shared column."""
    for k1, k2 in K:
        vqe, jac = _oracle(D, k1, k2)
        J = jac.view(np.float16)
        assert 0 < J.diagonal().max() < 0.01 and -0.01 < J.min() < 0
        share = ((vqe & 0x7fff) != 0).astype(np.float32)
        assert np.array_equal(J == 1, share @ share.T == 0)


def test_the_fixture_has_clusters_borders_and_noise():
    """The counts the GPU cases rely on, from the oracle and dbscan_ref alone."""
    seen_contested = False
    for D in (32, 33):
        for k1, k2 in K[:2]:
            J = _oracle(D, k1, k2)[1].view(np.float16)
            for eps in (0.4, 0.6):
                for min_samples in (2, 4):
                    labels, core, _, n = dbscan_ref(J, eps, min_samples)
                    assert 18 <= n <= 32 and 4 <= (labels < 0).sum() <= 67 and (~core & (labels >= 0)).sum() <= 3
                    seen_contested |= len(contested(J, eps, labels, core)) > 0
        assert dbscan_ref(_oracle(D, 70, 6)[1].view(np.float16), 0.6, 4)[3] <= 2
    assert seen_contested
