"""The fp16 pre-filter's bound itself, on the device: hi and the row width against the exact distance
for every pair, the survivor epilogue's lists entry by entry, and the outcomes on inputs whose fp16
rounding errors are sign-aligned (tests/prefilter_ref.py; tests/test_prefilter_ref.py shows on the
CPU that they reach the bound and that half the bound loses true neighbours on `planted`).

The outcome tests elsewhere (test_rank_prefilter_*, test_gpu_search_prefilter.py) run on data whose
rounding errors cancel: they use a fifth of the bound and would pass with a much narrower one."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import reidmi_boot  # noqa: E402

reidmi_boot.load()

import oracle  # noqa: E402
import prefilter_ref as pr  # noqa: E402
from multimodal_reid_amd import synthetic as syn  # noqa: E402

pytestmark = pytest.mark.gpu

_cache = {}


def _L():
    from multimodal_reid_amd import _lib
    return _lib


def _prepare(f):
    """sqn / nrm / x16 / nmax2 of device features f, as reranking.HipStages prepares them."""
    lib = _L()
    N, D = f.shape
    Np, Dp = (N + 255) // 256 * 256, (D + 63) // 64 * 64
    sqn = torch.empty(N, device=f.device)
    lib.call("reidmi_row_sqnorm_f32", lib.ptr(f), N, D, D, lib.ptr(sqn), lib.stream())
    nrm = torch.sqrt(sqn)
    x16 = torch.zeros((Np, Dp), dtype=torch.float16, device=f.device)
    ok = torch.ones(1, dtype=torch.int32, device=f.device)
    lib.call("reidmi_rr_feat16", lib.ptr(f), N, D, D, lib.ptr(x16), Np, Dp, lib.ptr(ok), lib.stream())
    assert int(ok.item()) == 1
    nmax2 = torch.empty(2, device=f.device)
    lib.call("reidmi_rr_norm_max", lib.ptr(sqn), lib.ptr(nrm), N, lib.ptr(nmax2), lib.stream())
    return sqn, nrm, x16, nmax2, Np, Dp


def _rank_rows_f16(f, K, stride, chunk_rows):
    """reidmi_rr_rank_rows_f16_ex over all rows -> (rank, rowmax, need, chunk, prepared)."""
    lib = _L()
    N, D = f.shape
    prep = _prepare(f)
    sqn, nrm, x16, nmax2, Np, Dp = prep
    R = torch.full((N, K), -1, dtype=torch.int32, device=f.device)
    rmax = torch.zeros(N, device=f.device)
    need = torch.full((N,), -1, dtype=torch.int32, device=f.device)
    chunk = torch.empty(chunk_rows * Np, device=f.device)
    lib.call("reidmi_rr_rank_rows_f16_ex", lib.ptr(f), N, D, D, lib.ptr(sqn), lib.ptr(nrm), lib.ptr(nmax2),
             lib.ptr(x16), Np, Dp, 0, N, K, lib.ptr(R), lib.ptr(rmax), lib.ptr(need), lib.ptr(chunk), chunk_rows,
             stride, lib.stream())
    return R.cpu().numpy(), rmax.cpu().numpy(), need.cpu().numpy(), chunk, prep


def _rank_rows_exact(f, K):
    """reidmi_rr_rank_rows over all rows -> (rank, rowmax)."""
    lib = _L()
    N, D = f.shape
    sqn = torch.empty(N, device=f.device)
    lib.call("reidmi_row_sqnorm_f32", lib.ptr(f), N, D, D, lib.ptr(sqn), lib.stream())
    R = torch.full((N, K), -1, dtype=torch.int32, device=f.device)
    rmax = torch.zeros(N, device=f.device)
    cr = 256
    chunk = torch.empty(cr * N, device=f.device)
    lib.call("reidmi_rr_rank_rows", lib.ptr(f), N, D, D, lib.ptr(sqn), 0, N, K, lib.ptr(R), lib.ptr(rmax),
             lib.ptr(chunk), cr, lib.stream())
    return R.cpu().numpy(), rmax.cpu().numpy()


def _dense_hi(f, K):
    """The dense form in one pass over all rows: the chunk then holds the epilogue's upper bounds
    hi [Np][Np] (rows < N written; rank_select1_kernel only reads them).  -> hi [N][Np] float32,
    sqn [N], nmax2 [2] (numpy, from the device), need [N]."""
    N = f.shape[0]
    Np = (N + 255) // 256 * 256
    assert int(_L().load().reidmi_rr_rank_rows_f16_pass_rows(N, Np, Np, K, 0)) == Np >= N  # one pass
    _, _, need, chunk, (sqn, _, _, nmax2, _, _) = _rank_rows_f16(f, K, 0, Np)
    hi = chunk.view(Np, Np)[:N].cpu().numpy()
    return hi, sqn.cpu().numpy(), nmax2.cpu().numpy(), need


# ---------------------------------------------------------------- a. dense bound, every pair
_A_CASES = {
    "down_128": (pr.aligned("down"), 300, 128), "down_130": (pr.aligned("down"), 300, 130),
    "down_256": (pr.aligned("down"), 300, 256), "down_1792": (pr.aligned("down"), 300, 1792),
    "up_128": (pr.aligned("up"), 300, 128), "up_130": (pr.aligned("up"), 300, 130),
    "mix_130_partial_tiles": (pr.aligned("mix"), 515, 130), "mix_256": (pr.aligned("mix"), 300, 256),
    "subnormal_128": (pr.subnormal, 300, 128), "subnormal_130": (pr.subnormal, 300, 130),
    "mixed_norm_128": (pr.mixed_norm, 300, 128), "mixed_norm_1792": (pr.mixed_norm, 300, 1792),
    "planted_128": (pr.planted(10), 300, 128),
}


@pytest.mark.parametrize("case", list(_A_CASES))
def test_dense_bound_holds_for_every_pair(gpu, case):
    """Every exact distance d_ij (the C oracle's fmaf chain, the distance kernel's bits) lies in
    [hi_ij - width_i, hi_ij], hi the EPI_RRHI epilogue's output and width_i prefilter_ref's float64
    restatement of rr_width from the device's squared norms: no tolerance (rr_width carries a 2^-10
    relative margin over 2 e).  Columns past N hold +inf.  On the aligned inputs the device uses as
    much of the bound as the float64 model says (within 0.05): it sees the model's worst case.
    `subnormal`: every fp16 operand is subnormal; d <= hi and d >= hi - width hold there only if the
    MFMA does not flush subnormal operands (the c_abs term's premise)."""
    build, N, D = _A_CASES[case]
    x = build(N, D, 11)
    hi, sqn, nmax2, _ = _dense_hi(torch.from_numpy(x).to(gpu), 11)
    d = oracle.distmat(x, x).astype(np.float64)
    s = sqn.astype(np.float64)
    n = np.sqrt(sqn).astype(np.float64)  # the fp32 square root the kernels hold
    e_ref = pr.e(s[:, None], s[None, :], n[:, None], n[None, :], D)
    w = pr.width(s, n, float(nmax2[0]), float(nmax2[1]), D)
    h = hi[:, :N].astype(np.float64)
    used = float((np.abs(h - e_ref - d) / e_ref).max())
    model = pr.reach(x)
    print(f"{case}: device max |hi - e - d| / e = {used:.4f}, model {model:.4f}; "
          f"min (hi - d) / e = {((h - d) / e_ref).min():.4f}, min (d - (hi - w)) / e = "
          f"{((d - (h - w[:, None])) / e_ref).min():.4f}")
    assert np.isfinite(h).all()
    assert (d <= h).all()
    assert (d >= h - w[:, None]).all()
    assert np.isposinf(hi[:, N:]).all() and hi.shape[1] > N
    if case.startswith(("down", "up", "mix")):
        assert abs(used - model) <= 0.05


# ---------------------------------------------------------------- b. survivor epilogue: bits and set
def _clustered(n, D, seed):
    qp, gp, _, _ = syn.labels(n // 10, n - n // 10, num_ids=max(8, n // 30), num_cams=6, seed=seed)
    qf, gf = syn.features(qp, gp, dim=D, seed=seed, noise=3.0)
    return oracle.l2norm(np.concatenate([qf, gf]))


def test_survivor_lists_are_the_stated_set_with_the_dense_bits(gpu):
    """The staged triangle calls (plan -> init -> sample -> survivors over all tiles) at N = 4352 (17
    tiles), D = 128, K = 51, on 4000 clustered unit rows followed by 352 aligned("mix") rows (their
    norms are 0.8; scaling by anything but a power of two would undo the alignment, and the nearest
    power is 2^0).  For every row m whose list did not overflow:
      * its columns are exactly {c < N : !(hi_max_m < hi[m][c] < lb_m)} (hi_max, lb from meta), each
        once, with hi the dense form's bounds;
      * each entry carries the bits of the dense hi[m][c], m the list's row: a pair reached through
        the transposed role (tile row c, tile column m) evaluates rr_hi with the roles swapped, that
        is with the list's row as rr_hi's row, so it is hi[m][c] and not hi[c][m];
      * d_mc <= hi_entry and d_mc >= hi_entry - w_m (w from wrow), d = evaluate.euclidean_distance;
      * no column >= N (the ragged last tile) appears.
    The diagonal pair (m, m) is in the stated set (hi_mm ~ e <= hi_max: an item is its own nearest
    neighbour and R2's lists hold it), so it must appear, once: it is not excluded."""
    from multimodal_reid_amd import evaluate
    lib = _L()
    N, D, K = 4352, 128, 51
    x = np.concatenate([_clustered(4000, D, 9), pr.aligned("mix")(352, D, 12)])
    f = torch.from_numpy(np.ascontiguousarray(x)).to(gpu)
    hi, _, _, _ = _dense_hi(f, K)
    hi = hi[:, :N]
    sqn, nrm, x16, nmax2, Np, Dp = _prepare(f)
    cc = 4096
    nt, cap, ns, sp = (ctypes.c_int64() for _ in range(4))
    lib.call("reidmi_rr_tri_plan", N, Np, cc, K, ctypes.byref(nt), ctypes.byref(cap), ctypes.byref(ns), ctypes.byref(sp))
    ntiles, cap, ns, sp = nt.value, cap.value, ns.value, sp.value
    assert ntiles == 17 * 18 // 2 and cap >= 1024 and ns == 256 and sp > 0
    meta = torch.zeros(Np * 4, device=gpu)
    wrow = torch.empty(N, device=gpu)
    cnt = torch.zeros(N, device=gpu, dtype=torch.int32)
    lst = torch.empty(N * cap * 2, device=gpu, dtype=torch.int32)
    sqn_s, nrm_s = torch.empty(ns, device=gpu), torch.empty(ns, device=gpu)
    tiles = torch.empty(ntiles, device=gpu, dtype=torch.int32)
    st = lib.stream()
    lib.call("reidmi_rr_tri_init", lib.ptr(sqn), lib.ptr(nrm), N, Np, ns, lib.ptr(meta), lib.ptr(sqn_s),
             lib.ptr(nrm_s), lib.ptr(tiles), st)
    lib.call("reidmi_rr_tri_sample", lib.ptr(x16), Np, Dp, lib.ptr(sqn), lib.ptr(nrm), lib.ptr(nmax2), N, D, K,
             lib.ptr(sqn_s), lib.ptr(nrm_s), ns, 0, N, lib.ptr(lst), sp, lib.ptr(meta), lib.ptr(wrow), lib.ptr(cnt),
             cap, st)
    lib.call("reidmi_rr_tri_survivors", lib.ptr(x16), Np, Dp, lib.ptr(sqn), lib.ptr(nrm), N, D, lib.ptr(meta),
             lib.ptr(tiles), 0, ntiles, lib.ptr(cnt), lib.ptr(lst), cap, st)
    cnt = cnt.cpu().numpy()
    ent = lst.view(N, cap, 2).cpu().numpy()
    m4 = meta.view(Np, 4)[:N].cpu().numpy()
    w = wrow.cpu().numpy().astype(np.float64)
    ok = cnt <= cap
    print(f"survivors: {ok.mean():.4f} of the rows within cap {cap}; list sizes min {cnt.min()} "
          f"median {int(np.median(cnt))} max {cnt.max()}")
    assert ok.mean() >= 0.9
    assert (cnt[ok] >= K).all()
    rows = np.nonzero(ok)[0]
    pos = np.arange(cap)[None, :] < cnt[rows, None]
    m = np.broadcast_to(rows[:, None], pos.shape)[pos]
    c = ent[rows, :, 0][pos].astype(np.int64)
    bits = ent[rows, :, 1][pos].view(np.uint32)
    assert (c >= 0).all() and (c < N).all()          # never a column of the ragged last tile
    flat = m * N + c
    assert len(np.unique(flat)) == len(flat)         # no column twice
    got = np.zeros((N, N), bool)
    got[m, c] = True
    hmax, lb = m4[:, 2:3], m4[:, 3:4]
    want = ~((hi > hmax) & (hi < lb))
    assert np.array_equal(got[rows], want[rows])
    assert got[rows, rows].all()                     # the diagonal pair: in the set, so in the list
    as_row = hi.view(np.uint32)[m, c] == bits
    as_col = hi.view(np.uint32)[c, m] == bits
    print(f"entries {len(bits)}: bits equal dense hi[m][c] {as_row.mean():.6f}, hi[c][m] {as_col.mean():.6f}")
    assert as_row.all()
    d = evaluate.euclidean_distance(f, f).astype(np.float64)[m, c]
    he = bits.view(np.float32).astype(np.float64)
    assert (d <= he).all()
    assert (d >= he - w[m]).all()


# ---------------------------------------------------------------- c. outcomes on the adversarial inputs
KP = 10  # planted(KP): KP A rows and 2 KP B rows per query


def _check_r2(f, K, stride, chunk_rows, must_decide=None):
    key = ("exact", f.data_ptr(), K)
    if key not in _cache:
        _cache[key] = _rank_rows_exact(f, K)
    Re, me = _cache[key]
    R, mx, need, _, _ = _rank_rows_f16(f, K, stride, chunk_rows)
    assert set(np.unique(need)) <= {0, 1}
    ok = need == 0
    print(f"stride {stride}, chunk rows {chunk_rows}: decides {ok.mean():.4f} of {len(ok)} rows")
    if must_decide is not None:
        assert ok[must_decide].all()
    assert np.array_equal(R[ok], Re[ok])
    assert np.array_equal(mx[ok].view(np.uint32), me[ok].view(np.uint32))
    return Re


def _r2_input(name, N, gpu):
    if ("r2", name, N) not in _cache:
        x = pr.planted(KP)(N, 128, 21) if name == "planted" else pr.aligned("mix")(N, 128, 22)
        _cache[("r2", name, N)] = (x, torch.from_numpy(x).to(gpu))
    return _cache[("r2", name, N)]


@pytest.mark.parametrize("name", ["planted", "mix"])
@pytest.mark.parametrize("form", ["dense", "rectangular", "triangle"])
def test_r2_forms_equal_the_exact_rows_on_adversarial_inputs(gpu, form, name):
    """reidmi_rr_rank_rows_f16_ex in the dense form (N = 1500) and the sampled rectangular and
    triangle forms (N = 4352; `planted` is padded with far rows) on `planted` and aligned("mix"):
    rank and rowmax equal reidmi_rr_rank_rows bit for bit on the rows with need == 0, and every
    planted query row is decided (need == 0) and ranks itself and its A rows first, where the fp16
    distances rank the B rows before them."""
    N = 1500 if form == "dense" else 4352
    Np = (N + 255) // 256 * 256
    K = KP + 1 if name == "planted" else 51
    stride, cr = {"dense": (0, 256), "rectangular": (16, 512), "triangle": (16, 4096)}[form]
    pass_rows = int(_L().load().reidmi_rr_rank_rows_f16_pass_rows(N, Np, cr, K, stride))
    assert pass_rows == {"dense": 256, "rectangular": 256, "triangle": N}[form]
    x, f = _r2_input(name, N, gpu)
    if name != "planted":
        _check_r2(f, K, stride, cr)
        return
    groups, q, A, B, far = pr.planted_layout(N, KP)
    Re = _check_r2(f, K, stride, cr, must_decide=q)
    for g in range(groups):
        assert set(Re[q[g]]) == {q[g], *A[g]}


def _search_case(gpu):
    """Q = 130 queries (32 planted, 98 clustered), G = 960 planted A / B rows + 1100 clustered rows
    (the planted rows first: the stride-2 sample of 1024 items holds half of every group's B rows),
    and labels under which every planted query loses 5 of its 20 B rows (same pid, same camera)."""
    if "search" not in _cache:
        from multimodal_reid_amd import evaluate
        groups = 32
        P = pr.planted(KP)(groups * (1 + 3 * KP), 128, 23)
        _, q, A, B, far = pr.planted_layout(len(P), KP)
        assert len(far) == 0 and len(q) == groups
        gal = np.sort(np.concatenate([A.ravel(), B.ravel()]))
        where = {int(r): i for i, r in enumerate(gal)}  # planted row -> gallery index
        qp, gp, qc, gc = syn.labels(130 - groups, 1100, num_ids=40, num_cams=4, seed=6)
        bq, bg = syn.features(qp, gp, dim=128, seed=6)
        base = evaluate.l2_normalize_device(torch.from_numpy(np.concatenate([bq, bg])).to(gpu))
        qf = torch.cat([torch.from_numpy(P[q]).to(gpu), base[:len(qp)]]).contiguous()
        gf = torch.cat([torch.from_numpy(P[gal]).to(gpu), base[len(qp):]]).contiguous()
        pq = np.concatenate([10000 + np.arange(groups), qp]).astype(np.int64)
        cq = np.concatenate([np.zeros(groups, np.int64), qc])
        pg = np.concatenate([10000 + (gal // (1 + 3 * KP)), gp]).astype(np.int64)
        cg = np.concatenate([np.ones(len(gal), np.int64), gc])
        for g in range(groups):
            for b in B[g, :5]:
                cg[where[int(b)]] = 0
        a_idx = np.array([[where[int(r)] for r in A[g]] for g in range(groups)])
        _cache["search"] = (qf, gf, (pq, cq, pg, cg), a_idx)
    return _cache["search"]


@pytest.mark.parametrize("mode", ["plain", "labels", "max_dist"])
def test_search_prefilter_equals_the_exact_search_on_planted(gpu, mode):
    """search_device(prefilter=True, _sample_stride=2) on `planted`: idx and dist torch.equal to the
    exact search and no row left to it (G = 2060 <= 4096: no list can overflow); with labels (the
    threshold comes from the admitted sample items only); and with max_dist = each row's exact K-th
    distance (the bounded form: T = min(U, bound)).  The planted queries' lists are their A rows."""
    from multimodal_reid_amd import evaluate
    qf, gf, lab, a_idx = _search_case(gpu)
    Q, G = qf.shape[0], gf.shape[0]
    assert Q == 130 and G == 2060
    kw = {}
    if mode == "max_dist":
        if "kth" not in _cache:
            _cache["kth"] = evaluate.search_device(qf, gf, KP)[1][:, KP - 1].clone()
        kw["max_dist"] = _cache["kth"]
    args = lab if mode == "labels" else ()
    want = evaluate.search_device(qf, gf, KP, *args, **kw)
    idx, dist, st = evaluate.search_device(qf, gf, KP, *args, prefilter=True, return_stats=True, _sample_stride=2,
                                           **kw)
    print("planted search", mode, st)
    assert st["applied"] is True and st["range_failed"] == 0 and st["need_rows"] == 0
    assert torch.equal(idx, want[0]) and torch.equal(dist, want[1])
    got = np.sort(want[0][:len(a_idx)].cpu().numpy(), axis=1)
    assert np.array_equal(got, np.sort(a_idx, axis=1))  # A rows carry camera 1: admitted under the labels too
