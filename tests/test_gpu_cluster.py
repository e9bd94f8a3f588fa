"""reidmi_dbscan_f32 and multimodal_reid_amd.cluster: exact DBSCAN from the features.

Base data: N = 300 rows (three 128-row bands, the last ragged: diagonal tiles, off-diagonal tiles and
unions across workgroups), synthetic identity-clustered features, L2-normalised; D = 36 runs the
pipelined mainloop and D = 33 the single-stage one.

Oracle: euclidean_distance_device(x, x) (the clustering's own distance bits, asserted symmetric),
then tests/dbscan_ref.py on the host (checked against scikit-learn in tests/test_cluster_ref.py).
Labels, core flags, counts and the number of clusters are compared as integers.  eps is always a
value fp32 holds exactly, so the oracle and the kernel compare against the same number."""
import numpy as np
import pytest
import torch

import oracle
from dbscan_ref import contested, dbscan_ref
from multimodal_reid_amd import synthetic as syn

pytestmark = pytest.mark.gpu

N = 300
MAIN = [(4, 0.01), (8, 0.02)]  # (min_samples, the quantile of the distance matrix eps sits at)
_cache = {}


def _cl():
    from multimodal_reid_amd import cluster
    return cluster


def _ev():
    from multimodal_reid_amd import evaluate
    return evaluate


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _matrix(x):
    dm = _ev().euclidean_distance_device(x, x).cpu().numpy()
    assert np.isfinite(dm).all() and np.array_equal(dm, dm.T)  # the contract's precondition
    return dm


def _cached(key, make):
    """(x, its distance matrix), computed once and left unchanged."""
    if key not in _cache:
        x = np.ascontiguousarray(make(), dtype=np.float32)
        dm = _matrix(x)
        dm.setflags(write=False)
        _cache[key] = (x, dm)
    return _cache[key]


def _base(D):
    def make():
        qp, gp, _, _ = syn.labels(10, N, num_ids=12, num_cams=6, seed=D)
        return _ev().l2_normalize_device(syn.features(qp, gp, dim=D, seed=D)[1]).cpu().numpy()
    return _cached(("base", D), make)


def _dup(D):
    """The base rows with copies (as tests/test_gpu_search_bounded.py's _base_data): a copy's
    distances to a third row are its original's bit for bit, also across the band borders."""
    def make():
        x = _base(D)[0].copy()
        x[0] = x[1]
        for b in (128, 256):
            for i in range(8):
                x[b + i] = x[b - 1 - i]
        return x
    return _cached(("dup", D), make)


def _chain():
    """300 points on a line at unit spacing, in a random order of the rows: every distance is a
    small integer (exact in fp32), 1 to the two neighbours on the line and >= 4 to the rest."""
    def make():
        x = np.zeros((N, 36), np.float32)
        x[np.random.default_rng(5).permutation(N), 5] = np.arange(N, dtype=np.float32)
        return x
    return _cached("chain", make)


def _quantile_eps(dm, q):
    return float(np.float32(np.quantile(dm, q)))


def _check(x, dm, eps, min_samples):
    """cluster.dbscan against the oracle; returns the (equal) result."""
    want = dbscan_ref(dm, eps, min_samples)
    labels, core, counts, n_clusters = _cl().dbscan(x, eps, min_samples)
    assert labels.dtype == np.int32 and core.dtype == np.bool_ and counts.dtype == np.int32
    assert np.array_equal(counts, want[2])
    assert np.array_equal(core, want[1])
    assert n_clusters == want[3]
    assert np.array_equal(labels, want[0])
    return want


# --------------------------------------------------------------------- 1. main case
@pytest.mark.parametrize("D", [36, 33])
@pytest.mark.parametrize("min_samples,quantile", MAIN)
def test_main(gpu, D, min_samples, quantile):
    x, dm = _base(D)
    eps = _quantile_eps(dm, quantile)
    labels, core, counts, n_clusters = dbscan_ref(dm, eps, min_samples)
    border = ~core & (labels >= 0)
    n_contested = len(contested(dm, eps, labels, core))
    print(f"[dbscan] D {D} eps {eps:.6g} min_samples {min_samples}: {n_clusters} clusters, "
          f"{int((labels < 0).sum())} noise, {int(border.sum())} border, {n_contested} contested")
    assert n_clusters >= 2 and (labels < 0).any() and border.any() and n_contested >= 1
    _check(x, dm, eps, min_samples)
    # the device form returns the same arrays
    got = _cl().dbscan_device(torch.from_numpy(x).cuda(), eps, min_samples)
    assert got[0].dtype == torch.int32 and got[1].dtype == torch.bool and got[2].dtype == torch.int32
    assert all(g.is_cuda for g in got)
    assert np.array_equal(got[0].cpu().numpy(), labels) and np.array_equal(got[1].cpu().numpy(), core)
    assert np.array_equal(got[2].cpu().numpy(), counts)


def test_normalize(gpu):
    """normalize=True clusters l2_normalize_device(x)."""
    x, dm = _base(36)
    eps = _quantile_eps(dm, 0.01)
    scaled = x * np.linspace(0.5, 3.0, N, dtype=np.float32)[:, None]
    xn = _ev().l2_normalize_device(scaled).cpu().numpy()
    want = dbscan_ref(_matrix(xn), eps, 4)
    got = _cl().dbscan(scaled, eps, 4, normalize=True)
    assert all(np.array_equal(g, w) for g, w in zip(got[:3], want[:3])) and got[3] == want[3]


# -------------------------------------------------------------- 2. threshold equality
@pytest.mark.parametrize("D", [36, 33])
def test_pairs_exactly_at_eps_are_neighbours(gpu, D):
    x, dm = _dup(D)
    # row 128 is a copy of row 127: eps = d(128, k) is also d(127, k), and both once more transposed
    others = np.setdiff1d(np.arange(N), [127, 128])
    k = others[np.argmin(np.abs(dm[128, others] - np.quantile(dm, 0.01)))]
    eps = float(dm[128, k])
    at = (dm == np.float32(eps)) & ~np.eye(N, dtype=bool)
    assert at[128, k] and at[127, k] and at[k, 128] and at[k, 127] and at.sum() >= 4
    want = _check(x, dm, eps, 4)
    # the pairs at eps are in the counts (<=): a strict compare would lose them
    assert np.array_equal(want[2] - at.sum(1), ((dm < np.float32(eps)) | np.eye(N, dtype=bool)).sum(1))
    _check(x, dm, eps, int(want[2][128]))  # row 128 is a core point only with the pairs at eps


# ------------------------------------------------------------------------- 3. chain
@pytest.mark.parametrize("min_samples", [2, 3])
def test_chain_is_one_cluster(gpu, min_samples):
    x, dm = _chain()
    eps = 2.0  # the neighbours on the line are at 1, the next ones at 4
    assert ((dm <= 2.0).sum(1) <= 3).all()
    labels, core, counts, n_clusters = _check(x, dm, eps, min_samples)
    assert n_clusters == 1 and (labels == 0).all()
    assert (~core).sum() == (0 if min_samples == 2 else 2)  # the ends of the line: border points


# ------------------------------------------------------------------------- 4. edges
def test_one_row(gpu):
    x = _base(36)[0][:1]
    dm = _matrix(x)
    assert _check(x, dm, 0.5, 1)[0].tolist() == [0]
    assert _check(x, dm, 0.0, 1)[0].tolist() == [0]  # the diagonal counts whatever its rounding
    assert _check(x, dm, 0.5, 2)[0].tolist() == [-1]


def test_fewer_rows_than_min_samples(gpu):
    x = _base(33)[0][:3]
    labels, core, counts, n_clusters = _check(x, _matrix(x), 10.0, 4)
    assert n_clusters == 0 and (labels == -1).all() and not core.any() and (counts == 3).all()


@pytest.mark.parametrize("D", [36, 33])
def test_eps_zero_with_duplicated_rows(gpu, D):
    x, dm = _dup(D)
    _check(x, dm, 0.0, 2)
    _check(x, dm, 0.0, 1)


def test_eps_beyond_every_distance(gpu):
    x, dm = _base(36)
    labels, core, counts, n_clusters = _check(x, dm, float(np.float32(dm.max() * 2)), 4)
    assert n_clusters == 1 and (labels == 0).all() and core.all() and (counts == N).all()


@pytest.mark.parametrize("D", [36, 33])
def test_min_samples_one_leaves_no_noise(gpu, D):
    x, dm = _base(D)
    labels, core, _, n_clusters = _check(x, dm, _quantile_eps(dm, 0.01), 1)
    assert core.all() and (labels >= 0).all() and n_clusters > 2


# ------------------------------------------------------------------------ 5. layout
@pytest.mark.parametrize("D,ld", [(36, 40), (36, 37), (33, 40)])  # (36, 37): the single-stage mainloop
def test_row_pitch_and_untouched_surroundings(gpu, D, ld):
    from multimodal_reid_amd import _lib
    x, dm = _base(D)
    eps = _quantile_eps(dm, 0.01)
    want = _cl().dbscan(x, eps, 4)  # the contiguous run
    buf = torch.full((N, ld), float("nan"), device="cuda")
    buf[:, :D] = torch.from_numpy(x).cuda()
    got = _cl().dbscan(buf[:, :D], eps, 4)  # the view is used in place
    assert all(np.array_equal(g, w) for g, w in zip(got[:3], want[:3])) and got[3] == want[3]
    # the C call: outputs and workspace pre-filled, one spare entry behind each output
    labels = torch.full((N + 1,), -77, device="cuda", dtype=torch.int32)
    counts = torch.full((N + 1,), -77, device="cuda", dtype=torch.int32)
    core = torch.full((N + 1,), 0xAB, device="cuda", dtype=torch.uint8)
    n_clusters = torch.full((2,), -77, device="cuda", dtype=torch.int32)
    nb = _lib.load().reidmi_dbscan_workspace_bytes(N, D)
    ws = torch.full((nb + 16,), 0xFF, device="cuda", dtype=torch.uint8)
    _lib.call("reidmi_dbscan_f32", _lib.ptr(buf), N, D, ld, eps, 4, _lib.ptr(labels), _lib.ptr(counts),
              _lib.ptr(core), _lib.ptr(n_clusters), _lib.ptr(ws), nb, _lib.stream())
    torch.cuda.synchronize()
    assert np.array_equal(labels[:N].cpu().numpy(), want[0]) and labels[N].item() == -77
    assert np.array_equal(core[:N].cpu().numpy(), want[1].astype(np.uint8)) and core[N].item() == 0xAB
    assert np.array_equal(counts[:N].cpu().numpy(), want[2]) and counts[N].item() == -77
    assert n_clusters.tolist() == [want[3], -77]
    assert (ws[nb:] == 0xFF).all().item()
    assert torch.isnan(buf[:, D:]).all().item()


# ------------------------------------------------------------------- 6. determinism
def test_two_runs_are_identical(gpu):
    """A repeat for equality (the unions land in whatever order the hardware runs them)."""
    x, dm = _base(36)
    cx, _ = _chain()
    for data, eps, min_samples in ((x, _quantile_eps(dm, 0.01), 4), (cx, 2.0, 3)):
        a = _cl().dbscan(data, eps, min_samples)
        b = _cl().dbscan(data, eps, min_samples)
        assert all(np.array_equal(u, v) for u, v in zip(a[:3], b[:3])) and a[3] == b[3]


# --------------------------------------------------------------------- 7. centroids
def test_label_groups_and_centroids(gpu):
    x, dm = _base(36)
    labels, _, _, n_clusters = dbscan_ref(dm, _quantile_eps(dm, 0.01), 4)
    offsets, idx = _cl().label_groups(labels)
    assert offsets.dtype == np.int64 and idx.dtype == np.int32 and len(offsets) == n_clusters + 1
    assert offsets[0] == 0 and offsets[-1] == (labels >= 0).sum() == len(idx)
    want = np.zeros((n_clusters, x.shape[1]), np.float32)
    for c in range(n_clusters):
        members = np.flatnonzero(labels == c)  # ascending row index
        assert np.array_equal(idx[offsets[c]:offsets[c + 1]], members)
        acc = np.zeros(x.shape[1], np.float32)
        for i in members:
            acc = acc + x[i]
        want[c] = acc / np.float32(len(members))
    assert np.array_equal(_bits(_cl().cluster_centroids(x, labels, normalize=False)), _bits(want))
    assert np.array_equal(_bits(_cl().cluster_centroids(torch.from_numpy(x).cuda(), torch.from_numpy(labels))),
                          _bits(oracle.l2norm(want)))
    # noise only: no cluster, no centroid
    assert _cl().label_groups(np.full(5, -1))[0].tolist() == [0] and len(_cl().label_groups(np.full(5, -1))[1]) == 0
