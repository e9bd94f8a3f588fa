"""reidmi_rr_jaccard_self_rows, reidmi_dbscan_jaccard and their cluster.py forms: the k-reciprocal
Jaccard distance of a set against itself, and exact DBSCAN on it from the sparse rows.

Base data: tests/jaccard_ref.fixture, 232 rows (24 identities of 8, 40 outliers), D = 32 and 33.
Reference of the distance: the C oracle's `jac` with num_query = N and lambda 0 (uint16 fp16 bits,
[N][N]); of the clustering: tests/dbscan_ref.py on that matrix viewed as fp16, so eps is compared in
fp16 there as in the kernel.  Everything is compared as integers.  (k1, k2) = (70, 6) takes the
generic V kernel (k1 > 61) and at eps 0.6 joins nearly everything into one cluster; (6, 1) has
V_qe = V.

Two chunks: 8492 rows (one 8192-column chunk and 300 more), about 1000 identities in a random row
order so that neighbours lie on both sides of the boundary.  The oracle's dense path takes about
20 s there, so the reference is jaccard_ref.jaccard_self_csr on the V_qe the re-rank stages built
(pinned to the oracle by the re-rank tests; tests/test_jaccard_ref.py pins the helper), once per
module."""
import numpy as np
import pytest
import torch

import oracle
from dbscan_ref import contested, dbscan_ref
from jaccard_ref import fixture, identities, jaccard_self_csr

pytestmark = pytest.mark.gpu

N = 232
K = [(20, 6), (6, 1), (70, 6)]
JCH = 8192
BIG_N = JCH + 300
_cache = {}


def _cl():
    from multimodal_reid_amd import cluster
    return cluster


def _ref(D, k1, k2, n=N):
    """(x, the oracle's self-Jaccard matrix as fp16) of the first n fixture rows, left unchanged."""
    if (D, k1, k2, n) not in _cache:
        x = np.ascontiguousarray(fixture(D)[:n])
        jac = oracle.rerank_from_dist(oracle.distmat(x, x), n, k1, k2, 0.0, debug=True)[3]
        assert np.array_equal(jac, jac.T)
        J = jac.view(np.float16)
        for a in (J,):
            a.setflags(write=False)
        _cache[D, k1, k2, n] = x, J
    return _cache[D, k1, k2, n]


def _check(x, J, eps, min_samples, k1, k2, expect="clusters and noise"):
    """cluster.dbscan_jaccard against dbscan_ref on J; returns the (equal) result.  expect: what the
    reference alone must show for the case to mean something: at least two clusters and a noise
    point; "connected": at most two clusters; None: a second run of a case (min_samples = 1 leaves
    no noise by definition, a raised min_samples may leave any number of clusters)."""
    want = dbscan_ref(J, eps, min_samples)
    border = ~want[1] & (want[0] >= 0)
    print(f"[dbscan_jaccard] N {len(x)} k ({k1}, {k2}) eps {eps:.6g} min_samples {min_samples}: {want[3]} clusters, "
          f"{int((want[0] < 0).sum())} noise, {int(border.sum())} border")
    if expect == "connected":
        assert want[3] <= 2
    elif expect is not None:
        assert want[3] >= 2 and (want[0] < 0).any()
    labels, core, counts, n_clusters = _cl().dbscan_jaccard(x, eps, min_samples, k1, k2)
    assert labels.dtype == np.int32 and core.dtype == np.bool_ and counts.dtype == np.int32
    assert np.array_equal(counts, want[2])
    assert np.array_equal(core, want[1])
    assert n_clusters == want[3]
    assert np.array_equal(labels, want[0])
    return want


# ----------------------------------------------------------------------- 1. the rows
@pytest.mark.parametrize("D", [32, 33])
@pytest.mark.parametrize("k1,k2", K)
def test_rows_equal_the_oracle(gpu, D, k1, k2):
    x, J = _ref(D, k1, k2)
    got = _cl().jaccard_distance_device(torch.from_numpy(x.copy()).cuda(), k1, k2)
    assert got.is_cuda and got.dtype == torch.float16 and got.shape == (N, N)
    assert np.array_equal(got.cpu().numpy().view(np.uint16), J.view(np.uint16))
    sub = _cl().jaccard_distance_device(x, k1, k2, rows=(37, 101))
    assert sub.shape == (64, N)
    assert np.array_equal(sub.cpu().numpy().view(np.uint16), J[37:101].view(np.uint16))
    assert _cl().jaccard_distance_device(x, k1, k2, rows=(5, 5)).shape == (0, N)


# --------------------------------------------------------------------- 2. clustering
@pytest.mark.parametrize("D", [32, 33])
@pytest.mark.parametrize("k1,k2", K[:2])
@pytest.mark.parametrize("eps", [0.4, 0.6])
@pytest.mark.parametrize("min_samples", [2, 4])
def test_dbscan_equals_the_reference(gpu, D, k1, k2, eps, min_samples):
    x, J = _ref(D, k1, k2)
    _check(x, J, eps, min_samples, k1, k2)


def test_contested_border_point(gpu):
    x, J = _ref(32, 20, 6)
    labels, core, _, _ = dbscan_ref(J, 0.6, 4)
    assert len(contested(J, 0.6, labels, core)) >= 1  # it takes the smaller cluster number
    want = _check(x, J, 0.6, 4, 20, 6)
    # the device form returns the same arrays
    got = _cl().dbscan_jaccard_device(torch.from_numpy(x.copy()).cuda(), 0.6, 4, 20, 6)
    assert got[0].dtype == torch.int32 and got[1].dtype == torch.bool and got[2].dtype == torch.int32
    assert all(g.is_cuda for g in got)
    assert all(np.array_equal(g.cpu().numpy(), w) for g, w in zip(got, want[:3]))


@pytest.mark.parametrize("D", [32, 33])
@pytest.mark.parametrize("min_samples", [2, 4])
def test_everything_connected(gpu, D, min_samples):
    """(70, 6) at eps 0.6: one or two clusters and no noise; most unions meet in one tree."""
    x, J = _ref(D, 70, 6)
    _check(x, J, 0.6, min_samples, 70, 6, expect="connected")


@pytest.mark.parametrize("D,k1,k2", [(32, 20, 6), (33, 20, 6), (33, 6, 1)])
def test_pairs_exactly_at_eps_are_neighbours(gpu, D, k1, k2):
    x, J = _ref(D, k1, k2)
    off = ~np.eye(N, dtype=bool)
    vals, n_at = np.unique(J[off & (J > 0.3) & (J < 0.7)], return_counts=True)
    eps = float(vals[np.argmax(n_at)])  # an fp16 value: fp32 and the fp16 rounding keep it
    at = (J == np.float16(eps)) & off
    assert at.sum() >= 2
    want = _check(x, J, eps, 4, k1, k2)
    # the pairs at eps are in the counts (<=): a strict compare would lose them
    assert np.array_equal(want[2] - at.sum(1), ((J < np.float16(eps)) | ~off).sum(1))
    i = int(np.argmax(at.sum(1)))
    strict = ((J < np.float16(eps)) | ~off).sum(1)
    assert strict[i] < want[2][i]
    again = _check(x, J, eps, int(want[2][i]), k1, k2, expect=None)
    assert again[1][i]  # row i is a core point only with the pairs at eps


def test_eps_is_rounded_to_fp16(gpu):
    """0.6 is not an fp16 value: the threshold is float16(0.6) = 0.60009765625, and pairs there hit."""
    x, J = _ref(33, 20, 6)
    assert (J == np.float16(0.6)).sum() >= 2 and float(np.float16(0.6)) > 0.6
    _check(x, J, 0.6, 4, 20, 6)
    _check(x, J, float(np.float16(0.6)), 4, 20, 6)


@pytest.mark.parametrize("D,k1,k2", [(32, 20, 6), (33, 70, 6)])
def test_eps_zero(gpu, D, k1, k2):
    """Only the diagonal and the non-positive entries hit."""
    x, J = _ref(D, k1, k2)
    off = ~np.eye(N, dtype=bool)
    assert (J[off] <= 0).any() and (J.diagonal() > 0).any()
    want = _check(x, J, 0.0, 2, k1, k2)
    assert np.array_equal(want[2], ((J <= 0) | ~off).sum(1)) and want[2].max() > 1
    labels = _check(x, J, 0.0, 1, k1, k2, expect=None)[0]
    assert (labels >= 0).all()


# ------------------------------------------------------------------------- 3. edges
@pytest.mark.parametrize("D,k1,k2", [(32, 20, 6), (33, 6, 1)])
def test_min_samples_one_leaves_no_noise(gpu, D, k1, k2):
    x, J = _ref(D, k1, k2)
    labels, core, _, n_clusters = _check(x, J, 0.4, 1, k1, k2, expect=None)
    assert core.all() and (labels >= 0).all() and n_clusters > 2


def test_one_row(gpu):
    """A lone row is its own k-reciprocal set: jd(0, 0) = 0, and the diagonal counts in any case.
    (The reference fails on one row, and the oracle with it, so the expectation is written out.)"""
    x = fixture(32)[:1]
    J = np.zeros((1, 1), np.float16)
    assert _check(x, J, 0.6, 1, 20, 6, expect=None)[0].tolist() == [0]
    assert _check(x, J, 0.0, 1, 20, 6, expect=None)[0].tolist() == [0]
    assert _check(x, J, 0.6, 2, 20, 6, expect=None)[0].tolist() == [-1]
    assert _cl().jaccard_distance_device(x, 20, 6).cpu().numpy().view(np.uint16).tolist() == [[0]]


def test_fewer_rows_than_min_samples(gpu):
    """Three rows, k1 = 2 (the reference needs k1 < N), min_samples = 4."""
    x, J = _ref(33, 2, 2, n=3)
    labels, core, counts, n_clusters = _check(x, J, 0.9, 4, 2, 2, expect=None)
    assert n_clusters == 0 and (labels == -1).all() and not core.any() and (counts == 3).all()
    assert np.array_equal(_cl().jaccard_distance_device(x, 2, 2).cpu().numpy().view(np.uint16), J.view(np.uint16))


def test_normalize(gpu):
    """normalize=True clusters l2_normalize_device(x)."""
    from multimodal_reid_amd import evaluate
    x, _ = _ref(32, 20, 6)
    scaled = x * np.linspace(0.5, 3.0, N, dtype=np.float32)[:, None]
    xn = evaluate.l2_normalize_device(scaled).cpu().numpy()
    want = _cl().dbscan_jaccard(xn, 0.6, 4, 20, 6)
    got = _cl().dbscan_jaccard(scaled, 0.6, 4, 20, 6, normalize=True)
    assert all(np.array_equal(g, w) for g, w in zip(got[:3], want[:3])) and got[3] == want[3] >= 2


def test_argument_errors(gpu):
    from multimodal_reid_amd._lib import ReidmiError
    x, _ = _ref(32, 20, 6)
    for kw in (dict(eps=-0.1), dict(eps=1.0), dict(eps=0.9998), dict(eps=float("nan")), dict(eps=float("inf")),
               dict(min_samples=0), dict(min_samples=2.5), dict(min_samples=True), dict(k1=0), dict(k2=0),
               dict(k1=2.0)):
        with pytest.raises(ReidmiError):
            _cl().dbscan_jaccard(x, **kw)
    for rows in ((5, 3), (-1, 4), (0, N + 1)):
        with pytest.raises(ReidmiError):
            _cl().jaccard_distance_device(x, 20, 6, rows=rows)
    with pytest.raises(ReidmiError):
        _cl().dbscan_jaccard(x[0], 0.6)


# -------------------------------------------------------------------- 4. two chunks
def _big():
    """(x, V_qe and its inverted index on the device, J, the labels of dbscan_ref), once."""
    if "big" not in _cache:
        from multimodal_reid_amd import reranking as rr
        x = identities(1000, 8, BIG_N - 8000, 32, seed=1)
        x = np.ascontiguousarray(x[np.random.default_rng(2).permutation(BIG_N)])
        st = rr.HipStages(torch.from_numpy(x).cuda(), BIG_N, 20, 6, 0.0)
        R, rmax = st.rank_rows(0, BIG_N)
        V = rr._gather_csr(st, *st.v_rows(R, rmax, 0, BIG_N), BIG_N)
        Vq = rr._gather_csr(st, *st.qe_rows(R, V, 0, BIG_N), BIG_N)
        st.check()
        off, col, val = (t.cpu().numpy() for t in Vq)
        J = jaccard_self_csr(off, col, val)
        assert np.array_equal(J.view(np.uint16), J.view(np.uint16).T)
        want = dbscan_ref(J, 0.6, 4)
        for a in (J,) + want[:3]:
            a.setflags(write=False)
        _cache["big"] = x, J, want
    return _cache["big"]


def test_two_chunks(gpu):
    x, J, want = _big()
    labels, core, counts, n_clusters = want
    # neighbours on both sides of the chunk boundary, in both directions, and clusters across it
    near = (J <= np.float16(0.6))
    assert near[:JCH, JCH:].sum() >= 100 and near[JCH:, :JCH].sum() >= 100
    both = np.intersect1d(labels[:JCH][labels[:JCH] >= 0], labels[JCH:][labels[JCH:] >= 0])
    print(f"[dbscan_jaccard] N {BIG_N}: {n_clusters} clusters, {int((labels < 0).sum())} noise, "
          f"{int((~core & (labels >= 0)).sum())} border, {len(both)} clusters on both sides of column {JCH}")
    assert n_clusters >= 500 and (labels < 0).any() and len(both) >= 50
    got = _cl().dbscan_jaccard(x, 0.6, 4, 20, 6)
    assert np.array_equal(got[2], counts)
    assert np.array_equal(got[1], core)
    assert got[3] == n_clusters
    assert np.array_equal(got[0], labels)


def test_two_chunks_rows(gpu):
    x, J, _ = _big()
    lo, hi = JCH - 100, JCH + 100  # rows whose own column lies in the first and in the second chunk
    got = _cl().jaccard_distance_device(x, 20, 6, rows=(lo, hi)).cpu().numpy()
    assert np.array_equal(got.view(np.uint16), J[lo:hi].view(np.uint16))
    assert (J[lo:hi, :JCH] < 1).any() and (J[lo:hi, JCH:] < 1).any()


# ------------------------------------------------- 5. determinism, surroundings, pooling
def test_two_runs_are_identical(gpu):
    """A repeat for equality (the unions land in whatever order the hardware runs them)."""
    for D, k1, k2 in ((32, 20, 6), (33, 70, 6)):
        x, _ = _ref(D, k1, k2)
        a = _cl().dbscan_jaccard(x, 0.6, 4, k1, k2)
        b = _cl().dbscan_jaccard(x, 0.6, 4, k1, k2)
        assert all(np.array_equal(u, v) for u, v in zip(a[:3], b[:3])) and a[3] == b[3]


def test_untouched_surroundings(gpu):
    """The C calls: outputs and workspace pre-filled, one spare entry behind each."""
    from multimodal_reid_amd import _lib
    x, J = _ref(33, 20, 6)
    want = dbscan_ref(J, 0.6, 4)
    n, _, Vq, csc = _cl()._jaccard_stages("test", x, 20, 6, False, None)
    sparse = [_lib.ptr(t) for t in Vq + csc]
    labels = torch.full((N + 1,), -77, device="cuda", dtype=torch.int32)
    counts = torch.full((N + 1,), -77, device="cuda", dtype=torch.int32)
    core = torch.full((N + 1,), 0xAB, device="cuda", dtype=torch.uint8)
    n_clusters = torch.full((2,), -77, device="cuda", dtype=torch.int32)
    nb = _lib.load().reidmi_dbscan_jaccard_workspace_bytes(N)
    ws = torch.full((nb + 16,), 0xFF, device="cuda", dtype=torch.uint8)
    _lib.call("reidmi_dbscan_jaccard", N, *sparse, 0.6, 4, _lib.ptr(labels), _lib.ptr(counts), _lib.ptr(core),
              _lib.ptr(n_clusters), _lib.ptr(ws), nb, _lib.stream())
    torch.cuda.synchronize()
    assert np.array_equal(labels[:N].cpu().numpy(), want[0]) and labels[N].item() == -77
    assert np.array_equal(core[:N].cpu().numpy(), want[1].astype(np.uint8)) and core[N].item() == 0xAB
    assert np.array_equal(counts[:N].cpu().numpy(), want[2]) and counts[N].item() == -77
    assert n_clusters.tolist() == [want[3], -77]
    assert (ws[nb:] == 0xFF).all().item()
    # the rows: a pitch beyond N, the rows before and behind the range, the bounds scratch
    ld, lo, hi = N + 5, 37, 101
    out = torch.full((hi - lo + 2, ld), 0x7777, device="cuda", dtype=torch.int16)
    bb = _lib.load().reidmi_rr_jaccard_bounds_bytes(N, N)
    bounds = torch.full((bb + 8,), 0xFF, device="cuda", dtype=torch.uint8)
    _lib.call("reidmi_rr_jaccard_self_rows", N, lo, hi, *sparse, _lib.ptr(out[1:]), ld, _lib.ptr(bounds), bb,
              _lib.stream())
    torch.cuda.synchronize()
    got = out.cpu().numpy().view(np.uint16)
    assert np.array_equal(got[1:-1, :N], J[lo:hi].view(np.uint16))
    assert (got[0] == 0x7777).all() and (got[-1] == 0x7777).all() and (got[:, N:] == 0x7777).all()
    assert (bounds[bb:] == 0xFF).all().item()


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def test_label_groups_and_centroids(gpu):
    x, J = _ref(32, 20, 6)
    labels, _, _, n_clusters = _cl().dbscan_jaccard(x, 0.6, 4, 20, 6)
    assert n_clusters >= 2 and (labels < 0).any()
    offsets, idx = _cl().label_groups(labels)
    assert len(offsets) == n_clusters + 1 and offsets[-1] == (labels >= 0).sum() == len(idx)
    want = np.zeros((n_clusters, x.shape[1]), np.float32)
    for c in range(n_clusters):
        members = np.flatnonzero(labels == c)  # ascending row index
        assert np.array_equal(idx[offsets[c]:offsets[c + 1]], members)
        acc = np.zeros(x.shape[1], np.float32)
        for i in members:
            acc = acc + x[i]
        want[c] = acc / np.float32(len(members))
    assert np.array_equal(_bits(_cl().cluster_centroids(x, labels, normalize=False)), _bits(want))
    assert np.array_equal(_bits(_cl().cluster_centroids(torch.from_numpy(x.copy()).cuda(), torch.from_numpy(labels))),
                          _bits(oracle.l2norm(want)))
