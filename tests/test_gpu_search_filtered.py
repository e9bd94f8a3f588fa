"""The filtered search (reidmi_search_filtered_f32, reidmi_search_prefiltered_filtered_f32) and what is
built on it: search(g_attrs=, q_filter=), SearchAccumulator(q_filter=), R1_mAP_eval.rank_lists.

Reference, from code the filtered search does not touch: euclidean_distance_device gives the
distances (the search's own bits), `admitted` below restates the table of include/reidmi.h on the
host, np.argsort(kind="stable") on the masked rows ranks by (distance, index), and the result is cut
at k and at the bound and padded with -1 / +inf.  idx is compared exactly, dist as int32 patterns.

Shapes: Q = 130 (two 128-row bands, the second ragged), G = 700 (ragged against 128-column tiles and
past one list capacity, so compactions run), D = 68 and 256, k = 1, 10, 128.  Gallery rows j and
j + 350 are identical, so every distance occurs twice in a row.

Conditions asserted on every case's inputs, so that none passes vacuously: between 5 % and 95 % of
all pairs admitted; a query with fewer than k admitted items (for k > 1: some, but fewer) and one
with none; a query whose unfiltered top-k holds a non-admitted item.  The valid and the group clause
alone cannot meet the second one (valid has no query side; `!=` admits nothing only against a
constant gallery column, which then admits everything for every other query): for those two cases
the first and third are asserted, and the all-clauses cases carry both clauses under all three."""
import ctypes

import numpy as np
import pytest
import torch

from multimodal_reid_amd import synthetic as syn

pytestmark = pytest.mark.gpu

Q, G = 130, 700
DS, KS = (68, 256), (1, 10, 128)
FIELDS = ["g_valid", "g_cam", "q_cam_mask", "g_time", "q_time_lo", "q_time_hi", "g_group", "q_group"]
I64_MIN, I64_MAX = -2 ** 63, 2 ** 63 - 1


def _ev():
    from multimodal_reid_amd import evaluate
    return evaluate


def _L():
    from multimodal_reid_amd import _lib
    return _lib


# ---------------------------------------------------------------- the host restatement
def admitted(nq, ng, lab=None, f=None):
    """[nq][ng] bool: include/reidmi.h's table.  lab = (qp, qc, gp, gc) or None; f: {field: array}."""
    f = f or {}
    a = np.ones((nq, ng), bool)
    if lab is not None:
        qp, qc, gp, gc = lab
        a &= ~((qp[:, None] == gp[None, :]) & (qc[:, None] == gc[None, :]))
    if "g_valid" in f:
        a &= (f["g_valid"] != 0)[None, :]
    if "g_cam" in f:
        c = f["g_cam"][None, :]
        bit = (f["q_cam_mask"].view(np.uint64)[:, None] >> (c & 63).astype(np.uint64)) & np.uint64(1)
        a &= (c >= 0) & (c < 64) & (bit != 0)
    if "g_time" in f:
        a &= (f["q_time_lo"][:, None] <= f["g_time"][None, :]) & (f["g_time"][None, :] <= f["q_time_hi"][:, None])
    if "g_group" in f:
        a &= f["g_group"][None, :] != f["q_group"][:, None]
    return a


def ranked(dm, adm, k, bd=None, bi=None, base=0):
    """The reference lists: dm's rows, non-admitted and out-of-bound entries removed, stable order."""
    adm = adm.copy()
    if bd is not None:
        bd = np.asarray(bd, np.float32)[:, None]
        tie = True if bi is None else (base + np.arange(dm.shape[1], dtype=np.int64))[None, :] < \
            np.asarray(bi, np.int64)[:, None]
        with np.errstate(invalid="ignore"):
            adm &= (dm < bd) | ((dm == bd) & tie)
    o = np.argsort(np.where(adm, dm, np.inf), axis=1, kind="stable")[:, :k]
    ok = np.take_along_axis(adm, o, 1)
    return (np.where(ok, o, -1).astype(np.int32),
            np.where(ok, np.take_along_axis(dm, o, 1), np.float32(np.inf)).astype(np.float32))


def _same(got, want):
    gi, gd = (t.cpu().numpy() if isinstance(t, torch.Tensor) else t for t in got)
    assert np.array_equal(gi, want[0])
    assert np.array_equal(gd.view(np.int32), want[1].view(np.int32))


# ---------------------------------------------------------------- data (deterministic)
_cache = {}


def _data(D, nq=Q, ng=G, ids=40, noise=4.0):
    key = ("data", D, nq, ng)
    if key not in _cache:
        qp, gp, qc, gc = syn.labels(nq, ng, num_ids=ids, num_cams=6, seed=D)
        qf, gf = syn.features(qp, gp, dim=D, seed=D, noise=noise)
        gf = gf.copy()
        if ng == G:
            gf[G // 2:] = gf[:G // 2]  # rows j and j + 350 are identical
        dm = _ev().euclidean_distance_device(qf, gf).cpu().numpy()
        assert np.isfinite(dm).all()
        _cache[key] = (qf, gf, (qp, qc, gp, gc), dm)
    return _cache[key]


def clauses(nq=Q, ng=G):
    """Every clause's two sides.  Of ten consecutive queries one has an empty camera mask, one the
    rare camera 7 alone (6 items), one a single ordinary camera, one cameras 7 and 63; one an empty
    time window, one a window of 9 ticks, one of 120; the others random masks and wide windows."""
    r = np.random.default_rng(20240607)
    f = {"g_valid": (r.random(ng) < 0.8).astype(np.uint8)}
    cam = r.integers(0, 7, ng)
    special = r.permutation(ng)[:16]
    cam[special[:6]], cam[special[6:]] = 7, 63
    f["g_cam"] = cam.astype(np.int64)
    f["g_time"] = r.integers(-500, 500, ng).astype(np.int64)
    f["g_group"] = r.integers(0, 8, ng).astype(np.int64)
    mask = np.zeros(nq, np.uint64)
    lo, hi = np.zeros(nq, np.int64), np.zeros(nq, np.int64)
    for i in range(nq):
        rnd = int(r.integers(0, 2 ** 62)) << 2 | int(r.integers(0, 4))  # 64 random bits
        m = i % 10
        mask[i] = (0, 1 << 7, 1 << (i // 10 % 7), 1 << 7 | 1 << 63)[m] if m < 4 else rnd | 0x15
        if m == 4:
            lo[i], hi[i] = 10, -10
        elif m == 5:
            lo[i] = int(r.integers(-400, 400))
            hi[i] = lo[i] + 8
        elif m == 6:
            lo[i] = int(r.integers(-400, 300))
            hi[i] = lo[i] + 120
        else:
            lo[i] = (I64_MIN, -10 ** 12, -450, -300)[i % 4]
            hi[i] = (I64_MAX, 250, 10 ** 12, 420)[i // 4 % 4]
    f["q_cam_mask"], f["q_time_lo"], f["q_time_hi"] = mask.view(np.int64), lo, hi
    f["q_group"] = r.integers(0, 10, nq).astype(np.int64)
    return f


def tie_clause():
    """g_time = j: even queries see the upper copies (j >= 350) only, odd ones the lower; of ten
    consecutive queries one has an empty window, one 6 items, one 100."""
    i = np.arange(Q, dtype=np.int64)
    lo, hi = np.where(i % 2 == 0, 350, 0), np.where(i % 2 == 0, 699, 349)
    lo, hi = np.where(i % 10 == 3, 5, lo), np.where(i % 10 == 3, 4, hi)
    lo, hi = np.where(i % 10 == 4, 350 + i, lo), np.where(i % 10 == 4, 355 + i, hi)
    lo, hi = np.where(i % 10 == 5, i, lo), np.where(i % 10 == 5, i + 99, hi)
    return {"g_time": np.arange(G, dtype=np.int64), "q_time_lo": lo.astype(np.int64), "q_time_hi": hi.astype(np.int64)}


SUBSETS = {"valid": ["g_valid"], "camera": ["g_cam", "q_cam_mask"], "time": ["g_time", "q_time_lo", "q_time_hi"],
           "group": ["g_group", "q_group"], "all": FIELDS}
NO_QUERY_SIDE_EMPTY = ("valid", "group")  # the module docstring's exception


def pick(f, name):
    return {n: f[n] for n in SUBSETS[name]}


def check_conditions(adm, dm, k, rows_condition=True):
    frac = adm.mean()
    assert 0.05 <= frac <= 0.95, frac
    n = adm.sum(1)
    if rows_condition:
        assert (n == 0).any() and (n < k).any()
        if k > 1:
            assert ((n > 0) & (n < k)).any()
    top = np.argsort(dm, axis=1, kind="stable")[:, :k]
    assert (~np.take_along_axis(adm, top, 1)).any()


def attrs_of(f):
    ev = _ev()
    return (ev.ItemAttrs(valid=f.get("g_valid"), camids=f.get("g_cam"), times=f.get("g_time"), groups=f.get("g_group")),
            ev.QueryFilter(cam_mask=f.get("q_cam_mask"),
                           time_range=np.stack([f["q_time_lo"], f["q_time_hi"]], 1) if "g_time" in f else None,
                           groups=f.get("q_group")))


def _dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def c_search(qf, gf, k, lab=None, f=None, order=None, bound=None, ex=None, null_struct=False):
    """reidmi_search_filtered_f32 (ex = (splits, cap): the tools variant), the struct's fields
    assigned in `order`.  bound = (bd, bi, ldb, base) of host arrays."""
    L = _L()
    q, g = _dev(qf), _dev(gf)
    nq, D = q.shape
    ng = g.shape[0]
    labs = [_dev(a) for a in lab] if lab is not None else [None] * 4
    keep = {n: _dev(a) for n, a in (f or {}).items()}
    s = L.structs("reidmi_filter.h")["reidmi_search_filter"]()
    for n in (order or list(keep)):
        setattr(s, n, keep[n].data_ptr())
    bd, bi, ldb, base = bound or (None, None, 1, 0)
    bd, bi = _dev(bd), _dev(bi)
    idx = torch.full((nq, k), -77, device="cuda", dtype=torch.int32)
    dist = torch.full((nq, k), -5.0, device="cuda", dtype=torch.float32)
    lib = L.load_tools() if ex else L.load()
    nb = lib.reidmi_search_ex_workspace_bytes(nq, ng, D, k, *ex) if ex else lib.reidmi_search_workspace_bytes(nq, ng, D, k)
    assert nb > 0
    ws = torch.empty(nb, device="cuda", dtype=torch.uint8)
    tail = (*ex, None) if ex else ()
    L.call("reidmi_search_filtered_f32" + ("_ex" if ex else ""), L.ptr(q), nq, D, L.ptr(g), ng, D, D, k,
           *(L.ptr(a) for a in labs), None if null_struct else ctypes.byref(s), L.ptr(bd), L.ptr(bi), ldb, base,
           L.ptr(idx), L.ptr(dist), k, L.ptr(ws), nb, *tail, L.stream(), tools=bool(ex))
    torch.cuda.synchronize()
    return idx, dist


# ---------------------------------------------------------------- each clause alone, all together
@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("D", DS)
@pytest.mark.parametrize("name", ["valid", "camera", "time", "group"])
def test_each_clause_alone(name, D, k):
    qf, gf, _, dm = _data(D)
    f = pick(clauses(), name)
    adm = admitted(Q, G, None, f)
    check_conditions(adm, dm, k, name not in NO_QUERY_SIDE_EMPTY)
    a, qfl = attrs_of(f)
    _same(_ev().search_device(qf, gf, k, g_attrs=a, q_filter=qfl), ranked(dm, adm, k))


@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("D", DS)
def test_all_clauses_with_the_label_rule_in_two_fill_orders(D, k):
    qf, gf, lab, dm = _data(D)
    f = clauses()
    adm = admitted(Q, G, lab, f)
    check_conditions(adm, dm, k)
    want = ranked(dm, adm, k)
    _same(c_search(qf, gf, k, lab, f, order=FIELDS), want)
    _same(c_search(qf, gf, k, lab, f, order=FIELDS[::-1]), want)
    a, qfl = attrs_of(f)
    qp, qc, gp, gc = lab
    _same(_ev().search(qf, gf, k, qp, qc, gp, gc, g_attrs=a, q_filter=qfl), want)
    # without the label rule the clauses stand alone
    _same(c_search(qf, gf, k, None, f), ranked(dm, admitted(Q, G, None, f), k))


@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("D", DS)
def test_all_admitting_filter_is_the_unfiltered_search(D, k):
    qf, gf, lab, dm = _data(D)
    f = {"g_valid": np.ones(G, np.uint8), "g_cam": clauses()["g_cam"], "q_cam_mask": np.full(Q, -1, np.int64),
         "g_time": clauses()["g_time"], "q_time_lo": np.full(Q, I64_MIN, np.int64),
         "q_time_hi": np.full(Q, I64_MAX, np.int64), "g_group": np.zeros(G, np.int64), "q_group": np.ones(Q, np.int64)}
    assert admitted(Q, G, None, f).all()
    a, qfl = attrs_of(f)
    ev = _ev()
    for labels in ((), (lab[0], lab[1], lab[2], lab[3])):
        plain = ev.search_device(qf, gf, k, *labels)
        _same(ev.search_device(qf, gf, k, *labels, g_attrs=a, q_filter=qfl), [t.cpu().numpy() for t in plain])
    plain = [t.cpu().numpy() for t in ev.search_device(qf, gf, k)]
    _same(c_search(qf, gf, k, None, {}), plain)            # every pointer NULL
    _same(c_search(qf, gf, k, null_struct=True), plain)    # flt == NULL
    _same(plain, ranked(dm, np.ones((Q, G), bool), k))


@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("D", DS)
def test_ties_the_filter_removes_one_copy(D, k):
    qf, gf, _, dm = _data(D)
    assert np.array_equal(dm[:, :G // 2].view(np.int32), dm[:, G // 2:].view(np.int32))
    f = tie_clause()
    adm = admitted(Q, G, None, f)
    check_conditions(adm, dm, k)
    assert adm[0, 350:].all() and not adm[0, :350].any() and adm[1, :350].all() and not adm[1, 350:].any()
    a, qfl = attrs_of(f)
    _same(_ev().search_device(qf, gf, k, g_attrs=a, q_filter=qfl), ranked(dm, adm, k))


# ---------------------------------------------------------------- forced ranges and capacities
@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("D", DS)
def test_forced_ranges_and_capacities(D, k):
    qf, gf, lab, dm = _data(D)
    f = clauses()
    want = ranked(dm, admitted(Q, G, lab, f), k)
    for S in (1, 3, 7):
        for cap in (k + 128, 512):
            _same(c_search(qf, gf, k, lab, f, ex=(S, cap)), want)
    f = pick(f, "time")  # one clause, no labels: the other filtered instantiation
    want = ranked(dm, admitted(Q, G, None, f), k)
    for S, cap in ((1, k + 128), (7, 512)):
        _same(c_search(qf, gf, k, None, f, ex=(S, cap)), want)


# ---------------------------------------------------------------- bounds under a filter
@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("D", DS)
def test_bounds_apply_to_admitted_items(D, k):
    qf, gf, lab, dm = _data(D)
    ev = _ev()
    f = clauses()
    adm = admitted(Q, G, lab, f)
    a, qfl = attrs_of(f)
    qp, qc, gp, gc = lab
    sd = np.sort(np.where(adm, dm, np.inf), axis=1)
    # a number: the median of the admitted distances; per query: the row's p-th admitted distance
    # itself (the inclusive form keeps it), +inf where the row has fewer
    tau = np.float32(np.median(dm[adm]))
    _same(ev.search_device(qf, gf, k, qp, qc, gp, gc, max_dist=float(tau), g_attrs=a, q_filter=qfl),
          ranked(dm, adm, k, np.full(Q, tau, np.float32)))
    p = np.arange(Q) % 23
    per = sd[np.arange(Q), p].astype(np.float32)
    got = ev.search_device(qf, gf, k, qp, qc, gp, gc, max_dist=per, g_attrs=a, q_filter=qfl)
    _same(got, ranked(dm, adm, k, per))
    full = np.isfinite(per)
    assert ((got[0].cpu().numpy() >= 0).sum(1)[full] >= np.minimum(k, p + 1)[full]).all()
    # the key form with an index base: (bd, bi) = the key of the row's p-th admitted item, the index
    # moved by -1 / 0 / +1, so that the item itself and its bit-equal copy fall on either side
    base = 1000
    order = np.argsort(np.where(adm, dm, np.inf), axis=1, kind="stable")
    bi = (base + order[np.arange(Q), p] + (np.arange(Q) % 3 - 1)).astype(np.int32)
    bd2 = np.zeros((Q, 2), np.float32)
    bi2 = np.zeros((Q, 2), np.int32)
    bd2[:, 0], bi2[:, 0] = per, bi
    _same(c_search(qf, gf, k, lab, f, bound=(bd2, bi2, 2, base)), ranked(dm, adm, k, per, bi, base))
    # a NaN radius admits nothing
    nan = per.copy()
    nan[::2] = np.nan
    got = ev.search_device(qf, gf, k, qp, qc, gp, gc, max_dist=nan, g_attrs=a, q_filter=qfl)
    _same(got, ranked(dm, adm, k, nan))
    assert (got[0].cpu().numpy()[::2] == -1).all()


# ---------------------------------------------------------------- blocks
@pytest.mark.parametrize("carry", [True, False])
@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("D", DS)
def test_blocks_equal_the_one_call_result(D, k, carry):
    qf, gf, lab, dm = _data(D)
    ev = _ev()
    f = clauses()
    f["g_valid"] = f["g_valid"].copy()
    f["g_valid"][300:451] = 0  # the middle block admits nothing
    adm = admitted(Q, G, lab, f)
    assert not adm[:, 300:451].any() and 0.05 <= adm.mean() <= 0.95
    a, qfl = attrs_of(f)
    qp, qc, gp, gc = lab
    want = ranked(dm, adm, k)
    one = ev.search_device(qf, gf, k, qp, qc, gp, gc, g_attrs=a, q_filter=qfl)
    _same(one, want)
    cuts = (0, 300, 451, G)
    blocks = [(gf[s:e], gp[s:e], gc[s:e], a[s:e]) for s, e in zip(cuts[:-1], cuts[1:])]
    _same(ev.search_blocks_device(qf, blocks, k, qp, qc, carry_bound=carry, q_filter=qfl), want)
    # without labels: (features, None, None, g_attrs)
    want = ranked(dm, admitted(Q, G, None, f), k)
    blocks = [(gf[s:e], None, None, a[s:e]) for s, e in zip(cuts[:-1], cuts[1:])]
    _same(ev.search_blocks(qf, blocks, k, carry_bound=carry, q_filter=qfl), want)


# ---------------------------------------------------------------- the pre-filter under a filter
def _prefilter_filter(ng, nq, frac):
    """frac 0.5: the valid clause at 50 %; frac 0.02: a time window per query that holds 2 % of the
    gallery (the time stamps are a permutation, so exactly G // 50 items)."""
    r = np.random.default_rng(ng)
    if frac == 0.5:
        return {"g_valid": (r.random(ng) < 0.5).astype(np.uint8)}
    t = r.permutation(ng).astype(np.int64)
    lo = r.integers(0, ng - ng // 50, nq).astype(np.int64)
    return {"g_time": t, "q_time_lo": lo, "q_time_hi": lo + ng // 50 - 1}


@pytest.mark.parametrize("frac", [0.5, 0.02])
@pytest.mark.parametrize("ng,k", [(4096, 10), (8192, 10), (8192, 128)])
def test_prefiltered_equals_the_exact_filtered_search(ng, k, frac):
    """G = 4096 / k = 10 and G = 8192 / k = 128 are the smallest sizes the pre-filter accepts.  At 2 %
    the 1/16 sample holds fewer than k admitted items, the threshold is +inf and every pair survives:
    past the survivor capacity (4096 per row) the rows overflow and fall back, which G = 8192 shows
    for both k.  At G = 4096 itself a list holds the whole gallery and cannot overflow, so there the
    same starved sample shows as max_survivors == G with no row left over."""
    D = 256
    assert _L().load().reidmi_search_prefilter_applies(Q, ng, D, k, 0) == 1
    qf, gf, lab, dm = _data(D, Q, ng, ids=200, noise=1.0)
    ev = _ev()
    f = _prefilter_filter(ng, Q, frac)
    adm = admitted(Q, ng, lab, f)
    assert abs(adm.mean() - frac) < 0.2 * frac
    a, qfl = attrs_of(f)
    qp, qc, gp, gc = lab
    exact = ev.search_device(qf, gf, k, qp, qc, gp, gc, g_attrs=a, q_filter=qfl)
    idx, dist, stats = ev.search_device(qf, gf, k, qp, qc, gp, gc, g_attrs=a, q_filter=qfl, prefilter=True,
                                        return_stats=True)
    print(f"G={ng} k={k} admitted={adm.mean():.3f} stats={stats}")
    assert stats["applied"] is True
    if frac == 0.02 and ng > 4096:
        assert stats["need_rows"] > 0  # the starved sample: the fallback path runs
    elif frac == 0.02:
        assert stats["need_rows"] == 0 and stats["max_survivors"] == ng
    _same((idx, dist), [t.cpu().numpy() for t in exact])
    _same((idx, dist), ranked(dm, adm, k))


# ---------------------------------------------------------------- R1_mAP_eval.rank_lists
@pytest.mark.parametrize("k", [10])
def test_rank_lists_cross_camera(k):
    D = 68
    qf, gf, lab, _ = _data(D)
    ev = _ev()
    qp, qc, gp, gc = lab
    m = ev.R1_mAP_eval(Q, feat_norm=True)
    m.reset()
    m.update((torch.from_numpy(np.concatenate([qf, gf])), np.concatenate([qp, gp]), np.concatenate([qc, gc])))
    f = {"g_cam": gc, "q_cam_mask": ev.cross_camera_mask(qc)}
    x = ev.l2_normalize_device(torch.from_numpy(np.concatenate([qf, gf])))
    dm = ev.euclidean_distance_device(x[:Q].contiguous(), x[Q:].contiguous()).cpu().numpy()
    adm = admitted(Q, G, None, f)
    assert np.array_equal(adm, qc[:, None] != gc[None, :]) and 0.05 <= adm.mean() <= 0.95
    got = m.rank_lists(k, remove_same_cam=False, g_attrs=ev.ItemAttrs(camids=gc),
                       q_filter=ev.QueryFilter(cam_mask=f["q_cam_mask"]))
    _same(got, ranked(dm, adm, k))
    got = m.rank_lists(k, remove_same_cam=True, g_attrs=ev.ItemAttrs(camids=gc),
                       q_filter=ev.QueryFilter(cam_mask=f["q_cam_mask"]))
    _same(got, ranked(dm, admitted(Q, G, lab, f), k))
