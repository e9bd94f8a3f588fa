"""reidmi_search_bounded_f32 (a per-query bound as the fused search's first threshold) and what is
built on it: search(max_dist=) and SearchAccumulator(carry_bound=, max_dist=).

Data as tests/test_gpu_search_blocks.py: Q = 130 (two query bands, the second ragged), G = 1000,
D = 36 (the pipelined mainloop) and D = 33 (the single-stage one), synthetic features and labels,
gallery rows duplicated so that bit-equal distances exist where a test needs them.

Oracle: euclidean_distance_device (the search's own bits), then on the host the label removal, the
bound's filter and a stable sort by (distance, index).  Indices are compared as integers, distances
as uint32 patterns.  Every direct call has its outputs pre-filled with sentinels, ldo > k and
ldb > 1, and the gaps are checked untouched."""
import numpy as np
import pytest
import torch

from multimodal_reid_amd import synthetic as syn

pytestmark = pytest.mark.gpu

Q, G = 130, 1000
T = (3, 70, 129)  # the queries that get copies of their pivot row (one per band half, the last row)
IDX_SENTINEL, DIST_SENTINEL = -77, -5.0
INT_MAX = 2 ** 31 - 1
SPLITS = {"one": (1000,), "ragged": (1, 127, 128, 300, 444), "empty": (500, 0, 500)}


def _ev():
    from multimodal_reid_amd import evaluate
    return evaluate


def _L():
    from multimodal_reid_amd import _lib
    return _lib


def _base_data(D):
    qp, gp, qc, gc = syn.labels(Q, G, num_ids=40, num_cams=6, seed=D)
    qf, gf = syn.features(qp, gp, dim=D, seed=D)
    gf = gf.copy()
    gf[0] = gf[1]
    for b in (128, 256, 500, 556):
        for i in range(8):
            gf[b + i] = gf[b - 1 - i]
    for i in range(7):
        gf[700 + i] = gf[650 + i]
    return qf, gf, qp, gp, qc, gc


def _removed(qp, gp, qc, gc):
    return (qp[:, None] == gp[None, :]) & (qc[:, None] == gc[None, :])


class Case:
    """A gallery, its distance matrix (the search's bits) and the stable ranking of every query's
    label-admissible items."""

    def __init__(self, qf, gf, qp, gp, qc, gc, labels):
        self.qf, self.gf, self.labels = qf, gf, labels
        self.lab = (qp, qc, gp, gc)  # the C ABI's order
        self.dm = _ev().euclidean_distance_device(qf, gf).cpu().numpy()
        assert np.isfinite(self.dm).all()
        self.rem = _removed(qp, gp, qc, gc) if labels else np.zeros((Q, G), bool)
        self.order = np.argsort(np.where(self.rem, np.inf, self.dm), axis=1, kind="stable")
        self.nadm = (~self.rem).sum(1)
        assert self.nadm.min() > 320
        self.sorted_d = np.take_along_axis(self.dm, self.order, 1)

    def oracle(self, k, bd=None, bi=None, base=0, lo=0, n=G):
        d = self.dm[:, lo:lo + n]
        adm = ~self.rem[:, lo:lo + n]
        if bd is not None:
            bd = np.asarray(bd, np.float32)[:, None]
            tie = True if bi is None else (base + np.arange(n, dtype=np.int64))[None, :] < np.asarray(bi, np.int64)[:, None]
            with np.errstate(invalid="ignore"):
                adm = adm & ((d < bd) | ((d == bd) & tie))
        o = np.argsort(np.where(adm, d, np.inf), axis=1, kind="stable")[:, :k]
        ok = np.take_along_axis(adm, o, 1)
        idx = np.where(ok, o, -1).astype(np.int32)
        dist = np.where(ok, np.take_along_axis(d, o, 1), np.float32(np.inf)).astype(np.float32)
        return idx, dist


_cache = {}


def _data(D):
    if ("data", D) not in _cache:
        _cache["data", D] = _base_data(D)
    return _cache["data", D]


def _plain(D, labels):
    """The blocks file's data."""
    key = ("plain", D, labels)
    if key not in _cache:
        _cache[key] = Case(*_data(D), labels)
    return _cache[key]


def _pivoted(D, labels, p):
    """The data with, for each query t of T, copies of the item at position p of t's ranking: one at
    a lower and one at a higher gallery index where rows are free, written over rows from the far
    end of every T query's ranking that are label-admissible for t.  A copy's distances are its
    source's, so the rankings are followed on the host; a copy made for one query can move another
    query's position p, hence the rounds."""
    key = ("pivot", D, labels, p)
    if key not in _cache:
        c0 = _plain(D, labels)
        qf, gf, qp, gp, qc, gc = _data(D)
        gf, dm, rem = gf.copy(), c0.dm.copy(), c0.rem
        tl, used = list(T), set()

        def orders():
            return np.argsort(np.where(rem[tl], np.inf, dm[tl]), axis=1, kind="stable")

        def ties(o, u):
            return int(((dm[tl[u]] == dm[tl[u], o[u][p]]) & ~rem[tl[u]]).sum())

        for _ in range(8):
            o = orders()
            todo = [u for u in range(len(tl)) if ties(o, u) < 2]
            if not todo:
                break
            for u in todo:
                o = orders()
                far_for_all = (np.argsort(o, axis=1) >= 400).all(0)  # moves no position below 400
                keep = used | {int(o[v][p]) for v in range(len(tl))}
                piv = int(o[u][p])
                far = [int(j) for j in o[u][400:c0.nadm[tl[u]]] if far_for_all[j] and int(j) not in keep]
                for r in [j for j in far if j < piv][:1] + [j for j in far if j > piv][:1]:
                    gf[r], dm[:, r] = gf[piv], dm[:, piv]
                    used.add(r)
        c = Case(qf, gf, qp, gp, qc, gc, labels)
        assert np.array_equal(c.dm.view(np.uint32), dm.view(np.uint32))  # a copy's distances are its source's bits
        o = orders()
        assert all(ties(o, u) >= 2 for u in range(len(tl))) and any(ties(o, u) >= 3 for u in range(len(tl)))
        _cache[key] = c
    return _cache[key]


def _dev(a, dtype):
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda", dtype)


def run(c, k, bd=None, bi=None, base=0, lo=0, n=G, ldb=2, opad=3, splits=None, cap=0, unbounded=False):
    """reidmi_search_bounded_f32 (or, with `splits`, the tools' _ex form; unbounded=True:
    reidmi_search_f32[_ex]) of gallery rows [lo, lo + n) -> (idx, dist[, stats])."""
    L = _L()
    D = c.qf.shape[1]
    qd, gd = _dev(c.qf, torch.float32), _dev(c.gf[lo:lo + n], torch.float32)
    ex = splits is not None
    if ex:
        nb = L.load_tools().reidmi_search_ex_workspace_bytes(Q, n, D, k, splits, cap)
    else:
        nb = L.load().reidmi_search_workspace_bytes(Q, n, D, k)
    assert nb > 0
    ws = torch.empty(nb, device="cuda", dtype=torch.uint8)
    ldo = k + opad
    oi = torch.full((Q, ldo), IDX_SENTINEL, device="cuda", dtype=torch.int32)
    od = torch.full((Q, ldo), DIST_SENTINEL, device="cuda", dtype=torch.float32)
    lab_t = [_dev(a[lo:lo + n] if i >= 2 else a, torch.int64) for i, a in enumerate(c.lab)] if c.labels else [None] * 4
    bdt = bit = None
    if bd is not None:
        bdt = torch.full((Q, ldb), -np.inf, device="cuda")  # a gap read as a bound would admit nothing
        bdt[:, 0] = _dev(np.asarray(bd, np.float32), torch.float32)
    if bi is not None:
        bit = torch.full((Q, ldb), -1, device="cuda", dtype=torch.int32)
        bit[:, 0] = _dev(np.asarray(bi, np.int32), torch.int32)
    st = torch.zeros(2, device="cuda", dtype=torch.int32) if ex else None
    head = [L.ptr(qd), Q, D, L.ptr(gd), n, D, D, k, *(L.ptr(t) for t in lab_t)]
    bound = [] if unbounded else [L.ptr(bdt), L.ptr(bit), ldb, base]
    tail = [L.ptr(oi), L.ptr(od), ldo, L.ptr(ws), nb]
    name = "reidmi_search_f32" if unbounded else "reidmi_search_bounded_f32"
    if ex:
        L.call_tools(name + "_ex", *head, *bound, *tail, splits, cap, L.ptr(st), L.stream())
    else:
        L.call(name, *head, *bound, *tail, L.stream())
    torch.cuda.synchronize()
    oin, odn = oi.cpu().numpy(), od.cpu().numpy()
    assert (oin[:, k:] == IDX_SENTINEL).all() and (odn[:, k:] == DIST_SENTINEL).all()
    res = [oin[:, :k].copy(), odn[:, :k].copy()]
    if ex:
        res.append(st.cpu().numpy())
    return res


def same(got, want):
    assert np.array_equal(got[0], want[0])
    assert np.array_equal(got[1].view(np.uint32), want[1].view(np.uint32))


def _below_min(c):
    return np.nextafter(c.sorted_d[:, 0], np.float32(-np.inf))


def radius_bound(c, m):
    """tau[i] = the exact distance of query i's m-th nearest admissible item; m = 0: below the row minimum."""
    return _below_min(c) if m == 0 else c.sorted_d[:, m - 1].copy()


def key_bound(c, p):
    """(d, index) of the item at position p of every query's ranking; for the queries of T the
    middle (or second) of the equal-distance copies that start there."""
    pos = np.full(Q, p)
    for t in T:
        if c.sorted_d[t, p + 1] == c.sorted_d[t, p]:
            pos[t] = p + 1
    r = np.arange(Q)
    return c.sorted_d[r, pos].copy(), c.order[r, pos].astype(np.int32), pos


KS = [1, 50, 128]
LAB = pytest.mark.parametrize("labels", [False, True], ids=["plain", "labels"])
DS = pytest.mark.parametrize("D", [36, 33])


# ------------------------------------------------------------------ 1. no bound
@LAB
@pytest.mark.parametrize("k", KS)
@DS
def test_no_bound_equals_search(gpu, D, k, labels):
    c = _plain(D, labels)
    want = _ev().search(c.qf, c.gf, k, *(c.lab if labels else ()))
    same(c.oracle(k), want)
    inf = np.full(Q, np.inf, np.float32)
    same(run(c, k, inf, None), want)
    same(run(c, k, inf, np.full(Q, -1, np.int32)), want)  # a not-yet-full carried list: +inf / -1
    same(run(c, k, None, None), want)


# ------------------------------------------------------------------ 2. radius form
@LAB
@pytest.mark.parametrize("which", ["k-1", "k", "k+5", "300", "below"])
@pytest.mark.parametrize("k", KS)
@DS
def test_radius(gpu, D, k, which, labels):
    m = {"k-1": k - 1, "k": k, "k+5": k + 5, "300": 300, "below": 0}[which]
    c = _pivoted(D, labels, max(m - 1, 0))
    tau = radius_bound(c, m)
    want = c.oracle(k, tau)
    hits = (want[0] >= 0).sum(1)
    if m == 0:
        assert (hits == 0).all()
    else:
        assert (hits >= min(k, m)).all()
        for t in T:  # every tie at tau is in: the copies of the m-th item count
            assert ((c.dm[t] == tau[t]) & ~c.rem[t]).sum() >= 2
        if m < k:
            assert any(hits[t] > m for t in T) and (hits < k).any()
    same(run(c, k, tau, None), want)


@LAB
@DS
def test_radius_nan_and_minus_inf_admit_nothing(gpu, D, labels):
    c = _plain(D, labels)
    tau = c.sorted_d[:, 60].copy()
    tau[0::3] = np.nan
    tau[1::3] = -np.inf
    got = run(c, 50, tau, None)
    same(got, c.oracle(50, tau))
    assert (got[0][0::3] == -1).all() and (got[0][1::3] == -1).all() and (got[0][2::3] >= 0).all()
    assert np.isposinf(got[1][0::3]).all()
    # the same bound values in the key form
    same(run(c, 50, tau, np.full(Q, 500, np.int32)), c.oracle(50, tau, np.full(Q, 500)))


# ------------------------------------------------------------------ 3. key form
@LAB
@pytest.mark.parametrize("which", ["0", "1", "k-1", "k", "300"])
@pytest.mark.parametrize("k", KS)
@DS
def test_key_bound(gpu, D, k, which, labels):
    m = {"0": 0, "1": 1, "k-1": k - 1, "k": k, "300": 300}[which]
    c = _pivoted(D, labels, m)
    bd, bi, pos = key_bound(c, m)
    want = c.oracle(k, bd, bi)
    # exactly the items before the bound in the ranking, the first k of them
    for i in range(Q):
        n = min(k, pos[i])
        assert np.array_equal(want[0][i, :n], c.order[i, :n]) and (want[0][i, n:] == -1).all()
    straddled = 0
    for t in T:  # copies a < b < c of one row, the bound is b: a is before it, b itself and c are not
        if pos[t] == m + 1 and c.sorted_d[t, m + 2] == bd[t]:
            straddled += 1
            a, cc = c.order[t, m], c.order[t, m + 2]
            assert a < bi[t] < cc and c.dm[t, a] == bd[t] == c.dm[t, cc]
            assert bi[t] not in want[0][t] and cc not in want[0][t] and (a in want[0][t]) == (m < k)
    assert straddled
    same(run(c, k, bd, bi), want)


# ------------------------------------------------------------------ 4. index_base
# no gallery index lies below a slice that starts at 0
@LAB
@pytest.mark.parametrize("lo,where", [(lo, w) for lo in (0, 1, 128, 500) for w in ("below", "inside", "beyond")
                                      if (lo, w) != (0, "below")])
@DS
def test_index_base(gpu, D, lo, where, labels):
    """The slice [lo, lo + n) searched with index_base = lo under bounds from the global ranking.
    For the queries of T the bound's item is a row below the slice, inside it or at / beyond its
    end, and copies of that row sit inside the slice (on both sides of an inside one)."""
    n, k, p = 300, 50, 30
    key = ("slice", D, labels, lo, where)
    if key not in _cache:
        c0 = _plain(D, labels)
        qf, gf, qp, gp, qc, gc = _data(D)
        gf = gf.copy()
        gp, gc = gp.copy(), gc.copy()
        rows = {}
        for u, t in enumerate(T):
            b = {"below": lo - 1 - u, "inside": lo + n // 2 + u, "beyond": lo + n + 7 * u}[where]
            if b < 0 or b >= G:
                continue
            src = gf[int(c0.order[t][p])].copy()
            mine = [b, lo + 3 + u, lo + n - 4 - u]  # the bound's row; copies near both ends of the slice
            for r in mine:
                gf[r] = src
                gp[r], gc[r] = -1 - u, 0  # admissible for every query
            rows[t] = mine
        assert rows
        _cache[key] = (Case(qf, gf, qp, gp, qc, gc, labels), rows)
    c, rows = _cache[key]
    r = np.arange(Q)
    bd, bi = c.sorted_d[r, p].copy(), c.order[r, p].astype(np.int32)
    for t, mine in rows.items():
        bd[t], bi[t] = c.dm[t, mine[0]], mine[0]
        assert c.dm[t, mine[1]] == bd[t] == c.dm[t, mine[2]]
    want = c.oracle(k, bd, bi, base=lo, lo=lo, n=n)
    for t, mine in rows.items():  # the copies inside the slice, as local indices
        a, b = mine[1] - lo, mine[2] - lo
        if where == "below":
            assert a not in want[0][t] and b not in want[0][t]
        elif where == "beyond":
            assert a in want[0][t] and b in want[0][t]
        else:
            assert a in want[0][t] and b not in want[0][t] and mine[0] - lo not in want[0][t]
    same(run(c, k, bd, bi, base=lo, lo=lo, n=n), want)
    if lo == 128:  # the same bounds in an index space that ends at 2^31 - 1
        far = INT_MAX - n
        bif = (bi.astype(np.int64) - lo + far).clip(-1, INT_MAX).astype(np.int32)
        same(c.oracle(k, bd, bif, base=far, lo=lo, n=n), want)  # the very same admissible sets
        same(run(c, k, bd, bif, base=far, lo=lo, n=n), want)


# ------------------------------------------------------------------ 5. splits and capacity
@pytest.mark.parametrize("form", ["radius", "key"])
@pytest.mark.parametrize("capsel", ["k+128", "default", "512"])
@pytest.mark.parametrize("S", [1, 3, 7])
@pytest.mark.parametrize("k", [50, 128])
@DS
def test_split_and_capacity_independence(gpu, D, k, S, capsel, form):
    cap = {"k+128": k + 128, "default": 0, "512": 512}[capsel]
    m = 300  # more than any capacity's slack: with S = 1 a bounded row compacts on its own candidates
    if form == "radius":
        c = _pivoted(D, True, m - 1)
        bd, bi = radius_bound(c, m), None
    else:
        c = _pivoted(D, True, m)
        bd, bi, _ = key_bound(c, m)
    want = c.oracle(k, bd, bi)
    assert (want[0] >= 0).all()
    idx, dist, st = run(c, k, bd, bi, splits=S, cap=cap)
    same((idx, dist), want)
    same(run(c, k, bd, bi), want)  # the product call: case 2 / case 3
    _, _, st0 = run(c, k, splits=S, cap=cap, unbounded=True)
    assert 0 < st[1] <= st0[1], (st, st0)
    # kept pairs are admissible pairs: never more than the bound admits
    nadm = sum(int((c.oracle(G, bd, bi)[0][i] >= 0).sum()) for i in range(Q))
    assert st[1] <= nadm
    # a bound that admits nothing: the filter runs before any append
    if form == "radius":
        none_d, none_i = _below_min(c), None
    else:
        none_d, none_i = c.sorted_d[:, 0].copy(), c.order[:, 0].astype(np.int32)
    idx, dist, st = run(c, k, none_d, none_i, splits=S, cap=cap)
    assert (idx == -1).all() and np.isposinf(dist).all() and st[1] == 0 and st[0] == 0, st


# ------------------------------------------------------------------ 6. accumulator, max_dist
def _blocks(c, order, sizes, host=False):
    gp, gc = c.lab[2][order], c.lab[3][order]
    gf = c.gf[order]
    out, lo = [], 0
    for n in sizes:
        f = torch.from_numpy(gf[lo:lo + n])
        f = f if host else f.cuda()
        out.append((f, gp[lo:lo + n], gc[lo:lo + n]) if c.labels else f)
        lo += n
    assert lo == G
    return out


def _search_all(c, order, k, **kw):
    lab = (c.lab[0], c.lab[1], c.lab[2][order], c.lab[3][order]) if c.labels else ()
    return _ev().search(c.qf, c.gf[order], k, *lab, **kw)


@LAB
@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("split", list(SPLITS))
@DS
def test_carry_bound_equals_search(gpu, D, split, k, labels):
    c = _plain(D, labels)
    ident = np.arange(G)
    want = _search_all(c, ident, k)
    same(c.oracle(k), want)
    ql = (c.lab[0], c.lab[1]) if labels else ()
    for cb in (True, False):
        same(_ev().search_blocks(c.qf, _blocks(c, ident, SPLITS[split]), k, *ql, carry_bound=cb), want)


@LAB
@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("direction", ["farthest_first", "nearest_first"])
def test_carry_bound_on_an_ordered_gallery(gpu, direction, k, labels):
    """The gallery sorted by its distance to query 0: farthest first, every block lowers that row's
    bound; nearest first, the blocks after the first hold nothing that can enter its list."""
    ev = _ev()
    c = _plain(36, labels)
    order = np.argsort(c.dm[0], kind="stable")
    if direction == "farthest_first":
        order = order[::-1].copy()
    want = _search_all(c, order, k)
    sizes = (200, 131, 128, 300, 241)
    ql = (c.lab[0], c.lab[1]) if labels else ()
    for cb in (True, False):
        acc = ev.SearchAccumulator(c.qf, k, *ql, carry_bound=cb)
        for b in _blocks(c, order, sizes):
            acc.add(*b) if labels else acc.add(b)
        idx, dist = acc.result()
        same((idx.cpu().numpy(), dist.cpu().numpy()), want)
        last_block_row0 = acc._idx[1][0].cpu().numpy()  # slot 1: the last block's own list
        if direction == "nearest_first" and cb:
            assert (last_block_row0 == -1).all()
        else:
            assert (last_block_row0 >= 0).all()


@LAB
def test_carry_bound_host_blocks(gpu, labels):
    c = _plain(33, labels)
    ident = np.arange(G)
    ql = (c.lab[0], c.lab[1]) if labels else ()
    got = _ev().search_blocks(c.qf, _blocks(c, ident, SPLITS["ragged"], host=True), 50, *ql, carry_bound=True)
    same(got, c.oracle(50))


def _mixed_radius(c):
    tau = c.sorted_d[:, 20].copy()  # short rows ...
    tau[1::2] = c.sorted_d[1::2, 300]  # ... and full ones
    tau[list(T)] = c.sorted_d[list(T), 20]
    tau[5] = np.nan
    tau[6] = -np.inf
    tau[7] = np.inf
    return tau


@LAB
@pytest.mark.parametrize("k", KS)
@DS
def test_max_dist(gpu, D, k, labels):
    ev = _ev()
    c = _pivoted(D, labels, 20)  # ties at the radius of the rows of T
    tau = _mixed_radius(c)
    want = c.oracle(k, tau)
    hits = (want[0] >= 0).sum(1)
    assert (hits[[5, 6]] == 0).all() and (hits[[7, 9, 11]] == k).all()
    if k > 30:
        assert ((hits > 20) & (hits < k)).any()
    lab = c.lab if labels else ()
    same(ev.search(c.qf, c.gf, k, *lab, max_dist=tau), want)
    same(ev.search(c.qf, c.gf, k, *lab, max_dist=torch.from_numpy(tau).cuda()), want)
    one = float(np.median(c.sorted_d[:, 40]))
    want1 = c.oracle(k, np.full(Q, one, np.float32))
    same(ev.search(c.qf, c.gf, k, *lab, max_dist=one), want1)
    ql = (c.lab[0], c.lab[1]) if labels else ()
    ident = np.arange(G)
    for cb in (True, False):
        for split in ("ragged", "empty"):
            got = ev.search_blocks(c.qf, _blocks(c, ident, SPLITS[split]), k, *ql, carry_bound=cb, max_dist=tau)
            same(got, want)
        same(ev.search_blocks(c.qf, _blocks(c, ident, SPLITS["ragged"]), k, *ql, carry_bound=cb, max_dist=one), want1)
