"""reidmi_search_prefiltered_f32 and search(prefilter=True) on top of it: the rank lists of the exact
search, bit for bit (torch.equal on idx and dist, no tolerance).

The reference is evaluate.search_device (reidmi_search_f32 / reidmi_search_bounded_f32) on the same
tensors.  Base data: Q = 130 (a partial 256-row GEMM tile), G = 1100 (a partial 256-column tile),
D = 130 (not a multiple of 64, nor of 4), synthetic identity-clustered features, L2-normalised;
sample stride 2, so the sample is 512 items.  G <= 4096 (the survivor capacity): no row may be left
to the exact search for size there, which the tests assert."""
import ctypes

import numpy as np
import pytest
import torch

from multimodal_reid_amd import synthetic as syn

pytestmark = pytest.mark.gpu

Q, G, D, S = 130, 1100, 130, 2
INT_MAX = 2 ** 31 - 1
_cache = {}


def _ev():
    from multimodal_reid_amd import evaluate
    return evaluate


def _L():
    from multimodal_reid_amd import _lib
    return _lib


def _base():
    """Normalised device features and the labels of the base shape (few identities, 2 cameras)."""
    if "base" not in _cache:
        qp, gp, qc, gc = syn.labels(Q, G, num_ids=4, num_cams=2, seed=5)
        qf, gf = syn.features(qp, gp, dim=D, seed=5)
        f = _ev().l2_normalize_device(torch.from_numpy(np.concatenate([qf, gf])))
        _cache["base"] = (f[:Q].contiguous(), f[Q:].contiguous(), qp, gp, qc, gc)
    return _cache["base"]


def _ref(key, fn):
    if key not in _cache:
        _cache[key] = fn()
    return _cache[key]


def _same(got, want):
    assert torch.equal(got[0], want[0])
    assert torch.equal(got[1], want[1])


def _c_search(qf, gf, k, lab=(None,) * 4, bd=None, bi=None, ldb=1, base=0, prefiltered=True, ldq=None, ldg=None,
              Dn=None):
    """A direct call of reidmi_search_prefiltered_f32 (-> idx, dist, need, stats) or of
    reidmi_search_bounded_f32 (-> idx, dist)."""
    lib = _L()
    L = lib.load()
    Qn, Gn = qf.shape[0], gf.shape[0]
    Dn = qf.shape[1] if Dn is None else Dn
    ldq = qf.stride(0) if ldq is None else ldq
    ldg = gf.stride(0) if ldg is None else ldg
    dev = qf.device
    idx = torch.full((Qn, k), -7, device=dev, dtype=torch.int32)
    dist = torch.full((Qn, k), -5.0, device=dev, dtype=torch.float32)
    lab = tuple(None if a is None else torch.as_tensor(a, dtype=torch.int64).to(dev) for a in lab)
    if not prefiltered:
        nb = L.reidmi_search_workspace_bytes(Qn, Gn, Dn, k)
        ws = torch.empty(nb, device=dev, dtype=torch.uint8)
        lib.call("reidmi_search_bounded_f32", lib.ptr(qf), Qn, ldq, lib.ptr(gf), Gn, ldg, Dn, k,
                 *(lib.ptr(a) for a in lab), lib.ptr(bd), lib.ptr(bi), ldb, base, lib.ptr(idx), lib.ptr(dist), k,
                 lib.ptr(ws), nb, lib.stream())
        return idx, dist
    assert L.reidmi_search_prefilter_applies(Qn, Gn, Dn, k, S) == 1
    nb = L.reidmi_search_prefiltered_workspace_bytes(Qn, Gn, Dn, k, S)
    ws = torch.empty(nb, device=dev, dtype=torch.uint8)
    need = torch.full((Qn,), -1, device=dev, dtype=torch.int32)
    stats = torch.full((4,), -1, device=dev, dtype=torch.int32)
    lib.call("reidmi_search_prefiltered_f32", lib.ptr(qf), Qn, ldq, lib.ptr(gf), Gn, ldg, Dn, k,
             *(lib.ptr(a) for a in lab), lib.ptr(bd), lib.ptr(bi), ldb, base, lib.ptr(idx), lib.ptr(dist), k, S,
             lib.ptr(need), lib.ptr(stats), lib.ptr(ws), nb, lib.stream())
    return idx, dist, need, stats.tolist()


# ------------------------------------------------------------------ 1. edge shapes
@pytest.mark.parametrize("k", [1, 10, 128])
def test_edge_shapes_equal_the_exact_search(k):
    qf, gf = _base()[:2]
    want = _ref(("plain", k), lambda: _ev().search_device(qf, gf, k))
    idx, dist, st = _ev().search_device(qf, gf, k, prefilter=True, return_stats=True, _sample_stride=S)
    print("stats", k, st)
    assert st["applied"] is True and st["range_failed"] == 0
    assert st["need_rows"] == 0  # G <= 4096: a condition, not a measurement
    assert 0 < st["max_survivors"] <= G and st["rescored"] >= Q * k
    _same((idx, dist), want)


# ------------------------------------------------------------------ 2. labels, 9. determinism
def _skewed_labels():
    """All but 6 gallery rows are (pid 1, camera 0); half of the queries are too, and keep 6 < k items."""
    gp, gc = np.ones(G, np.int64), np.zeros(G, np.int64)
    keep = np.array([3, 256, 511, 512, 777, 1099])
    gp[keep], gc[keep] = [2, 2, 3, 1, 1, 4], [0, 1, 0, 1, 1, 1]
    qp, qc = np.ones(Q, np.int64), np.zeros(Q, np.int64)
    qp[1::2], qc[1::2] = 2, 1
    return qp, gp, qc, gc


def _label_cases():
    qp, gp, qc, gc = _base()[2:]
    return {"few_ids": (qp, qc, gp, gc), "skewed": tuple(_skewed_labels()[i] for i in (0, 2, 1, 3))}


@pytest.mark.parametrize("case", ["few_ids", "skewed"])
def test_labels_equal_the_exact_search_twice(case):
    qf, gf = _base()[:2]
    lab = _label_cases()[case]
    k = 10
    want = _ref(("lab", case), lambda: _ev().search_device(qf, gf, k, *lab))
    removed = (lab[0][:, None] == lab[2][None, :]) & (lab[1][:, None] == lab[3][None, :])
    assert (removed[:, ::S][:, :512].sum(1) >= 2).sum() >= Q // 2  # sample items are removed
    if case == "skewed":
        short = (~removed).sum(1) < k
        assert 0 < short.sum() < Q
        assert torch.equal(want[0].cpu()[torch.from_numpy(short)][:, 6:], torch.full((int(short.sum()), 4), -1,
                                                                                    dtype=torch.int32))
    runs = []
    for _ in range(2):
        idx, dist, st = _ev().search_device(qf, gf, k, *lab, prefilter=True, return_stats=True, _sample_stride=S)
        print("need rows", case, st["need_rows"], "of", Q, st)
        assert st["applied"] is True and st["need_rows"] < Q / 2
        _same((idx, dist), want)
        runs.append((idx, dist))
    _same(runs[0], runs[1])  # the survivors' order in their lists varies between runs; the output must not
    # the direct call: no row is left to the exact search at this size
    idx, dist, need, st = _c_search(qf, gf, k, lab)
    assert st[0] == 0 and int(need.sum()) == 0 and int(need.min()) == 0
    _same((idx, dist), want)


# ------------------------------------------------------------------ 3. ties
def test_equal_distances_come_out_in_index_order():
    qf, gf = _base()[:2]
    gf = gf.clone()
    gf[200:400] = gf[0:200]
    gf[800:1000] = gf[0:200]
    k = 10
    want = _ev().search_device(qf, gf, k)
    idx, dist, st = _ev().search_device(qf, gf, k, prefilter=True, return_stats=True, _sample_stride=S)
    assert st["applied"] is True and st["need_rows"] == 0
    _same((idx, dist), want)
    i, d = idx.cpu().numpy(), dist.cpu().numpy()
    tie = d[:, 1:] == d[:, :-1]
    assert tie.sum() >= Q  # the copies make ties in every row
    assert (i[:, 1:][tie] > i[:, :-1][tie]).all()


# ------------------------------------------------------------------ 4. bounds
def _bounds(k):
    qf, gf = _base()[:2]
    i50, d50 = _ref(("plain", 50), lambda: _ev().search_device(qf, gf, 50))
    bd = d50[:, 4].clone()  # each row's exact 5th distance
    bd[7], bd[64], bd[100], bd[129] = float("inf"), float("-inf"), float("nan"), float("inf")
    return bd, i50[:, 4].clone()


def test_radius_form_equals_the_bounded_search():
    qf, gf = _base()[:2]
    k = 10
    bd, _ = _bounds(k)
    want = _ev().search_device(qf, gf, k, max_dist=bd)
    got = _ev().search_device(qf, gf, k, max_dist=bd, prefilter=True, return_stats=True, _sample_stride=S)
    assert got[2]["applied"] is True and got[2]["need_rows"] == 0
    _same(got[:2], want)
    hits = (want[0] >= 0).sum(1).cpu()
    assert hits[0] == 5 and hits[7] == k and hits[64] == 0 and hits[100] == 0  # short, padded rows
    idx, dist, need, st = _c_search(qf, gf, k, bd=bd)
    assert st[0] == 0 and int(need.sum()) == 0
    _same((idx, dist), _c_search(qf, gf, k, bd=bd, prefiltered=False))


@pytest.mark.parametrize("labels", [False, True])
def test_key_form_with_an_index_base_equals_the_bounded_search(labels):
    qf, gf = _base()[:2]
    k, base = 10, 5000
    lab = _label_cases()["few_ids"] if labels else (None,) * 4
    bd, i5 = _bounds(k)
    # pitch 2: the bound sits in column 0 of [Q][2] arrays, as a carried list's column would
    bd2 = torch.zeros((Q, 2), device=qf.device, dtype=torch.float32)
    bi2 = torch.zeros((Q, 2), device=qf.device, dtype=torch.int32)
    bd2[:, 0] = bd
    bi2[:, 0] = i5 + base        # strict: the 5th item itself is out, ties before it are in
    bi2[1, 0] = INT_MAX          # every tie at the bound is in
    bi2[2, 0] = base             # no tie is in
    bi2[7, 0] = -1               # +inf / -1: a not-yet-full carried list admits everything
    want = _c_search(qf, gf, k, lab, bd2, bi2, 2, base, prefiltered=False)
    idx, dist, need, st = _c_search(qf, gf, k, lab, bd2, bi2, 2, base)
    assert st[0] == 0 and int(need.sum()) == 0 and st[3] == 0
    _same((idx, dist), want)
    if not labels:
        hits = (idx >= 0).sum(1).cpu()
        assert hits[0] == 4 and hits[1] == 5 and hits[2] == 4 and hits[7] == k and hits[64] == 0 and hits[100] == 0


# ------------------------------------------------------------------ 5. overflow fallback
def test_overflowing_rows_fall_back_to_the_exact_search():
    Qn, Gn, Dn, k = 64, 8192, 128, 10
    r = np.random.default_rng(3)
    v = r.standard_normal(Dn).astype(np.float32)
    gf = torch.from_numpy(v[None, :] + 1e-4 * r.standard_normal((Gn, Dn)).astype(np.float32)).cuda()
    qf = torch.from_numpy(v[None, :] + 1e-4 * r.standard_normal((Qn, Dn)).astype(np.float32)).cuda()
    want = _ev().search_device(qf, gf, k)
    idx, dist, st = _ev().search_device(qf, gf, k, prefilter=True, return_stats=True, _sample_stride=16)
    print("overflow stats", st)
    assert st["applied"] is True and st["need_rows"] == Qn and st["max_survivors"] > 4096 and st["range_failed"] == 0
    _same((idx, dist), want)


# ------------------------------------------------------------------ 6. range fallback
def test_a_feature_beyond_fp16_range_falls_back():
    qf, gf = _base()[:2]
    gf = gf.clone()
    gf[5, 7] = 1e6
    k = 10
    want = _ev().search_device(qf, gf, k)
    idx, dist, st = _ev().search_device(qf, gf, k, prefilter=True, return_stats=True, _sample_stride=S)
    assert st["applied"] is True and st["range_failed"] == 1 and st["need_rows"] == Q
    _same((idx, dist), want)
    need, stats = _c_search(qf, gf, k)[2:]
    assert stats[3] == 1 and stats[0] == Q and bool((need == 1).all())


# ------------------------------------------------------------------ 7. unaligned inputs
@pytest.mark.parametrize("pitch", [D + 6, D + 3])  # 136: 16-byte rows with D % 4 != 0; 133: odd, unaligned rows
def test_row_views_of_a_wider_buffer(pitch):
    qf, gf = _base()[:2]
    k = 10
    want = _ref(("plain", k), lambda: _ev().search_device(qf, gf, k))
    qb = torch.full((Q, pitch), 9.0, device=qf.device)
    gb = torch.full((G, pitch), -9.0, device=qf.device)
    qb[:, :D], gb[:, :D] = qf, gf
    idx, dist, need, st = _c_search(qb, gb, k, ldq=pitch, ldg=pitch, Dn=D)
    assert st[0] == 0 and int(need.sum()) == 0
    _same((idx, dist), want)
    # and through Python, which takes the views themselves
    _same(_ev().search_device(qb[:, :D], gb[:, :D], k, prefilter=True, _sample_stride=S), want)


# ------------------------------------------------------------------ 8. blocks
@pytest.mark.parametrize("carry", [True, False])
@pytest.mark.parametrize("cut", [(600, 500), (550, 550), (1000, 100)])
def test_blocks_equal_the_one_call_exact_search(cut, carry):
    qf, gf = _base()[:2]
    lab = _label_cases()["few_ids"]
    k = 10
    want = _ref(("lab", "few_ids"), lambda: _ev().search_device(qf, gf, k, *lab))
    ev = _ev()
    # (1000, 100): the second block is too small for the pre-filter and silently takes the exact search
    assert _L().load().reidmi_search_prefilter_applies(Q, 100, D, k, S) == 0
    acc = ev.SearchAccumulator(qf, k, lab[0], lab[1], carry_bound=carry, prefilter=True, _sample_stride=S)
    lo = 0
    for n in cut:
        acc.add(gf[lo:lo + n], lab[2][lo:lo + n], lab[3][lo:lo + n])
        lo += n
    _same(acc.result(), want)
