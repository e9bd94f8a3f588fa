"""reidmi_combine_rows_f32 and what evaluate.py builds on it (query expansion, database
augmentation, group pooling, R1_mAP_eval's two keyword arguments) against a numpy restatement.

The oracle is the float32 loop below, in the order include/reidmi.h states: one accumulator per
column, base_w * base first, then acc = acc + (w * src[j]) for the kept entries in list order
(numpy rounds the product and the sum separately), mean's division, fmax for max; the
normalisation is the oracle's l2norm (the C restatement of reidmi_l2norm_f32).  Every comparison is
np.array_equal on the bit patterns.  No accuracy claim is tested."""
import numpy as np
import pytest
import torch

import oracle
from multimodal_reid_amd import synthetic as syn

pytestmark = pytest.mark.gpu

ROWS, N_SRC = 37, 97
LENGTHS = (0, 1, 2, 63, 64, 65, 130)  # across a wave and the 64-entry chunk of the list walk


def _ev():
    from multimodal_reid_amd import evaluate
    return evaluate


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def ref_combine(src, n_src, offsets, idx, w, base, base_w, mode):
    """(out fp32 [rows][d], entries >= n_src) in the stated order."""
    rows, d = len(offsets) - 1, src.shape[1]
    out = np.zeros((rows, d), np.float32)
    bad = 0
    for r in range(rows):
        ent = range(int(offsets[r]), int(offsets[r + 1]))
        bad += sum(int(idx[t]) >= n_src for t in ent)
        kept = [t for t in ent if 0 <= idx[t] < n_src]
        if mode == "max":
            parts = ([base[r]] if base is not None else []) + [src[idx[t]] for t in kept]
            if parts:
                acc = parts[0].astype(np.float32)
                for p in parts[1:]:
                    acc = np.fmax(acc, p)
                out[r] = acc
            continue
        acc = np.float32(base_w) * base[r] if base is not None else np.zeros(d, np.float32)
        for t in kept:
            acc = acc + (src[idx[t]] if w is None else np.float32(w[t]) * src[idx[t]])
        n = len(kept) + (base is not None)
        if mode == "mean" and n:
            acc = acc / np.float32(n)
        assert acc.dtype == np.float32
        out[r] = acc
    return out, bad


def _lists(seed):
    """37 lists with every length of LENGTHS, -1 entries, repeated indices, zero and negative weights."""
    r = np.random.default_rng(seed)
    lens = np.concatenate([np.array(LENGTHS), r.choice(LENGTHS, ROWS - len(LENGTHS))])
    lens = lens[r.permutation(ROWS)]
    offsets = np.zeros(ROWS + 1, np.int64)
    np.cumsum(lens, out=offsets[1:])
    n = int(offsets[-1])
    idx = r.integers(0, N_SRC, n).astype(np.int32)
    idx[r.random(n) < 0.15] = -1
    rep = np.flatnonzero(r.random(n) < 0.1)
    idx[rep[rep > 0]] = idx[rep[rep > 0] - 1]  # an index twice in a row (or a second -1)
    w = r.standard_normal(n).astype(np.float32)
    w[r.random(n) < 0.1] = 0.0
    two = np.flatnonzero(lens == 2)[0]  # a row whose entries are all skipped
    idx[offsets[two]:offsets[two + 1]] = -1
    return offsets, idx, w


_grid = {}


def _grid_case(d):
    if d not in _grid:
        r = np.random.default_rng(d)
        src = r.standard_normal((N_SRC, d)).astype(np.float32)
        base = r.standard_normal((ROWS, d)).astype(np.float32)
        _grid[d] = (src, base) + _lists(1000 + d)
    return _grid[d]


def _pitched(a, pad):
    """The rows of a on the device at a pitch of d + pad floats."""
    if not pad:
        return torch.from_numpy(a).cuda()
    buf = torch.full((a.shape[0], a.shape[1] + pad), float("nan"), device="cuda", dtype=torch.float32)
    buf[:, :a.shape[1]] = torch.from_numpy(a).cuda()
    return buf[:, :a.shape[1]]


MODES = [("sum", True), ("sum", False), ("mean", True), ("max", False)]


@pytest.mark.parametrize("pad", [0, 3], ids=["ld=d", "ld=d+3"])
@pytest.mark.parametrize("d", [1, 5, 64, 133, 256, 1280, 1792])
def test_kernel_grid(gpu, d, pad):
    """Both kernels (d < 256: a wave per row; d >= 256: a workgroup per row), the 16-byte and the
    4-byte path, with and without a base, all modes, normalised and not."""
    ev = _ev()
    src, base, offsets, idx, w = _grid_case(d)
    dsrc, dbase = _pitched(src, pad), _pitched(base, pad)
    for mode, weighted in MODES:
        for with_base in (False, True):
            ww = w if weighted else None
            want, bad = ref_combine(src, N_SRC, offsets, idx, ww, base if with_base else None, -0.75, mode)
            assert bad == 0
            kw = dict(w=ww, base=dbase if with_base else None, base_w=-0.75, mode=mode)
            plain = ev.combine_rows_device(dsrc, offsets, idx, normalize=False, **kw)
            assert np.array_equal(_bits(plain.cpu().numpy()), _bits(want)), (mode, weighted, with_base)
            normed = ev.combine_rows_device(dsrc, offsets, idx, normalize=True, **kw)
            assert torch.equal(normed.view(torch.int32), ev.l2_normalize_device(plain).view(torch.int32)), \
                (mode, weighted, with_base)
            assert np.array_equal(_bits(normed.cpu().numpy()), _bits(oracle.l2norm(want)))


def test_rows_wider_than_one_pass(gpu):
    """d = 2052 > the 2048 columns a workgroup holds in registers: two passes over the list, the
    squared-norm chain carried across them."""
    ev = _ev()
    r = np.random.default_rng(5)
    d = 2052
    src = r.standard_normal((N_SRC, d)).astype(np.float32)
    offsets, idx, w = _lists(77)
    want, _ = ref_combine(src, N_SRC, offsets, idx, w, None, 1.0, "mean")
    for normalize in (False, True):
        got = ev.combine_rows_device(src, offsets, idx, w=w, mode="mean", normalize=normalize).cpu().numpy()
        assert np.array_equal(_bits(got), _bits(oracle.l2norm(want) if normalize else want))


@pytest.mark.parametrize("d", [133, 1280])
def test_out_of_range_entries_are_skipped_and_counted(gpu, d):
    """src holds N_SRC + 8 rows and N_SRC is passed: entries N_SRC .. N_SRC + 7 point at allocated
    memory, so a missing guard gives wrong bits, not a fault."""
    ev = _ev()
    from multimodal_reid_amd import _lib
    r = np.random.default_rng(d)
    src = r.standard_normal((N_SRC + 8, d)).astype(np.float32)
    offsets, idx, w = _lists(2000 + d)
    hit = r.choice(len(idx), 11, replace=False)
    idx[hit] = N_SRC + r.integers(0, 8, len(hit))
    want, n_bad = ref_combine(src, N_SRC, offsets, idx, w, None, 1.0, "sum")
    assert n_bad == 11
    dsrc = torch.from_numpy(src).cuda()
    doff, didx, dw = torch.from_numpy(offsets).cuda(), torch.from_numpy(idx).cuda(), torch.from_numpy(w).cuda()
    out = torch.empty((ROWS, d), device="cuda", dtype=torch.float32)
    bad = torch.zeros(1, device="cuda", dtype=torch.int32)
    _lib.call("reidmi_combine_rows_f32", _lib.ptr(dsrc), N_SRC, d, d, _lib.ptr(doff), _lib.ptr(didx), _lib.ptr(dw),
              ROWS, None, 0, 1.0, 0, 0, _lib.ptr(out), d, _lib.ptr(bad), _lib.stream())
    assert int(bad.item()) == 11
    assert np.array_equal(_bits(out.cpu().numpy()), _bits(want))
    with pytest.raises(_lib.ReidmiError, match="11 list entries"):
        ev.combine_rows_device(dsrc[:N_SRC], doff, didx, w=dw)
    past = doff.clone()
    past[-1] += 1  # the last list would run off idx: refused before the kernel runs
    with pytest.raises(_lib.ReidmiError, match="offsets"):
        ev.combine_rows_device(dsrc[:N_SRC], past, didx, w=dw)


# ------------------------------------------------------------------ expansion
Q, G = 70, 300
_feat = {}


def _features(D):
    """Unit rows; 30 gallery rows are exact copies of others (tied distances, ordered by index)."""
    if D not in _feat:
        qp, gp, _, _ = syn.labels(Q, G, num_ids=25, num_cams=6, seed=D)
        qf, gf = syn.features(qp, gp, dim=D, seed=D)
        gf = gf.copy()
        gf[200:230] = gf[20:50]
        _feat[D] = (oracle.l2norm(qf), oracle.l2norm(gf))
    return _feat[D]


def ref_expand(xf, gf, idx, dist, alpha, include_x):
    """The restatement, fed the lists search itself returned."""
    k = idx.shape[1]
    w = None
    if alpha:
        s = np.maximum(np.float32(1) - dist * np.float32(0.5), np.float32(0))
        w = s
        for _ in range(alpha - 1):
            w = w * s
        assert w.dtype == np.float32
        w = w.reshape(-1)
    offsets = np.arange(len(xf) + 1, dtype=np.int64) * k
    out, _ = ref_combine(gf, len(gf), offsets, idx.reshape(-1), w, xf if include_x else None, 1.0, "sum")
    return oracle.l2norm(out)


@pytest.mark.parametrize("alpha", [0, 1, 3])
@pytest.mark.parametrize("k", [1, 10, 128])
@pytest.mark.parametrize("D", [133, 1280])
def test_expand_features(gpu, D, k, alpha):
    ev = _ev()
    qf, gf = _features(D)
    idx, dist = ev.search(qf, gf, k)
    got = ev.expand_features(qf, gf, k, alpha)
    assert np.array_equal(_bits(got), _bits(ref_expand(qf, gf, idx, dist, alpha, True)))


def test_expand_features_refuses_a_fractional_alpha(gpu):
    from multimodal_reid_amd import _lib
    qf, gf = _features(133)
    for alpha in (0.5, 3.0, -1, True):
        with pytest.raises(_lib.ReidmiError, match="alpha"):
            _ev().expand_features(qf, gf, 5, alpha)


@pytest.mark.parametrize("alpha", [0, 3])
def test_database_augmentation(gpu, alpha):
    ev = _ev()
    _, gf = _features(133)
    got = ev.database_augmentation(gf, 10, alpha)
    assert np.array_equal(_bits(got), _bits(ev.expand_features(gf, gf, 10, alpha, include_x=False)))
    idx, dist = ev.search(gf, gf, 10)
    assert np.array_equal(_bits(got), _bits(ref_expand(gf, gf, idx, dist, alpha, False)))


# ------------------------------------------------------------------ pooling
@pytest.mark.parametrize("D", [133, 1280])
def test_pool_features(gpu, D):
    """Groups of 1 .. 40 rows, keys neither sorted nor dense, rows of a group scattered."""
    ev = _ev()
    r = np.random.default_rng(D)
    keys = r.permutation(np.arange(-20, 100) * 7)[:40].astype(np.int64)
    groups = np.repeat(keys, np.arange(1, 41))
    groups = groups[r.permutation(len(groups))]
    feat = r.standard_normal((len(groups), D)).astype(np.float32)
    uk, inv = np.unique(groups, return_inverse=True)
    want = {m: np.zeros((len(uk), D), np.float32) for m in ("mean", "max")}
    for u, key in enumerate(uk):
        members = np.flatnonzero(groups == key)  # ascending row index
        acc = np.zeros(D, np.float32)
        for i in members:
            acc = acc + feat[i]
        want["mean"][u] = acc / np.float32(len(members))
        mx = feat[members[0]]
        for i in members[1:]:
            mx = np.fmax(mx, feat[i])
        want["max"][u] = mx
    for mode in ("mean", "max"):
        pooled, k2, inv2 = ev.pool_features(feat, groups, mode=mode)
        assert np.array_equal(k2, uk) and np.array_equal(inv2, inv.reshape(-1))
        assert np.array_equal(_bits(pooled), _bits(want[mode])), mode
    pooled, _, _ = ev.pool_features(torch.from_numpy(feat).cuda(), torch.from_numpy(groups), mode="mean",
                                    normalize=True)
    assert np.array_equal(_bits(pooled), _bits(oracle.l2norm(want["mean"])))


def test_multi_query_groups():
    pids = np.array([3, 3, 1, 1, 3, -1, 1, 3])
    cams = np.array([2, 5, 2, 2, 2, 4, 5, 5])
    key = _ev().multi_query_groups(pids, cams)
    assert key.dtype == np.int64 and key.shape == (8,)
    for i in range(8):
        for j in range(8):
            assert (key[i] == key[j]) == (pids[i] == pids[j] and cams[i] == cams[j])
    # np.unique's order is (pid, camera) order
    uk, first = np.unique(key, return_index=True)
    assert [(int(pids[i]), int(cams[i])) for i in first] == [(-1, 4), (1, 2), (1, 5), (3, 2), (3, 5)]


# ------------------------------------------------------------------ R1_mAP_eval
def test_r1_map_eval_with_expansion(gpu):
    ev = _ev()
    from multimodal_reid_amd import _lib
    qp, gp, qc, gc = syn.labels(100, 500, num_ids=60, num_cams=6, seed=1, distractor_frac=0.1, junk_frac=0.04)
    qf, gf = syn.features(qp, gp, dim=1280, seed=1, noise=4.0)
    m = ev.R1_mAP_eval(100, max_rank=50, feat_norm=True, query_expansion=(5, 3), db_augmentation=(5, 3))
    m.reset()
    m.update((torch.from_numpy(qf), qp, qc))
    m.update((torch.from_numpy(gf), gp, gc))
    n = ev.l2_normalize_device(torch.from_numpy(np.concatenate([qf, gf])))
    ge = ev.database_augmentation_device(n[100:], 5, 3)
    qe = ev.expand_features_device(n[:100], ge, 5, 3)
    cmc, mAP = m.compute()
    wcmc, wmap = ev.eval_func_device(ev.euclidean_distance_device(qe, ge), qp, gp, qc, gc)
    assert np.array_equal(cmc, wcmc) and mAP == wmap
    idx, dist = m.rank_lists(10)
    widx, wdist = ev.search(qe, ge, 10, qp, qc, gp, gc)
    assert np.array_equal(idx, widx) and np.array_equal(_bits(dist), _bits(wdist))
    # the expanded features are not the plain ones
    assert not torch.equal(qe, n[:100]) and not torch.equal(ge, n[100:])
    with pytest.raises(_lib.ReidmiError, match="sharded"):
        ev.R1_mAP_eval(100, sharded=True, query_expansion=(5, 3))
    with pytest.raises(_lib.ReidmiError, match="sharded"):
        ev.R1_mAP_eval(100, sharded=True, db_augmentation=(5, 0))
