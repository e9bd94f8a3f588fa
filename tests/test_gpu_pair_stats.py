"""reidmi_pair_stats_f32 and evaluate.pair_stats*: the genuine / impostor distance histograms and the
nearest genuine / impostor item of every query, from the features.

Base data: Q = 200 query rows (two 128-row bands, the second ragged) against G = 300 gallery rows
(three column tiles, the last ragged), identity-clustered synthetic features, L2-normalised; labels
with junk and distractor pids, so removed pairs exist.  D = 36 runs the pipelined mainloop and
D = 33 the single-stage one.

Oracle: euclidean_distance_device(q, g) (the call's own distance bits), then on the host
np.searchsorted(edges, dm, side="left") under the class masks with np.bincount, and the nearest keys
by np.lexsort((index, dm)).  Counts and indices are compared as integers, distances as bits."""
import numpy as np
import pytest
import torch

from multimodal_reid_amd import synthetic as syn

pytestmark = pytest.mark.gpu

Q, G = 200, 300
_cache = {}


def _ev():
    from multimodal_reid_amd import evaluate
    return evaluate


def _err():
    from multimodal_reid_amd import _lib
    return _lib.ReidmiError


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _matrix(q, g):
    dm = _ev().euclidean_distance_device(q, g).cpu().numpy()
    assert np.isfinite(dm).all()  # the contract's precondition
    return dm


def _normalised(x):
    return _ev().l2_normalize_device(np.ascontiguousarray(x, dtype=np.float32)).cpu().numpy()


def _base(D):
    """(qf, gf, labels (qp, gp, qc, gc), dm), computed once and left unchanged."""
    if ("base", D) not in _cache:
        qp, gp, qc, gc = syn.labels(Q, G, num_ids=12, num_cams=6, seed=D, junk_frac=0.05)
        qf, gf = syn.features(qp, gp, dim=D, seed=D)
        qf, gf = _normalised(qf), _normalised(gf)
        dm = _matrix(qf, gf)
        for a in (qf, gf, dm):
            a.setflags(write=False)
        _cache[("base", D)] = (qf, gf, (qp, gp, qc, gc), dm)
    return _cache[("base", D)]


def _masks(qp, gp, qc=None, gc=None, self_pairs=False):
    """(genuine, impostor) masks [Q][G]: removed pairs are in neither."""
    same = np.asarray(qp)[:, None] == np.asarray(gp)[None, :]
    removed = np.zeros_like(same)
    if qc is not None:
        removed |= same & (np.asarray(qc)[:, None] == np.asarray(gc)[None, :])
    if self_pairs:
        removed |= np.eye(*same.shape, dtype=bool)
    return same & ~removed, ~same & ~removed


def _nearest_lexsort(dm, mask, index_base=0):
    dist = np.full(dm.shape[0], np.inf, np.float32)
    idx = np.full(dm.shape[0], -1, np.int32)
    for i in range(dm.shape[0]):
        cand = np.nonzero(mask[i])[0]
        if cand.size:
            j = cand[np.lexsort((cand, dm[i, cand]))[0]]
            dist[i], idx[i] = dm[i, j], index_base + j
    return dist, idx


def _nearest_argmin(dm, mask, index_base=0):
    """_nearest_lexsort without the per-row sort (argmin returns the first, i.e. lowest-index, minimum)."""
    d = np.where(mask, dm, np.inf)
    j = d.argmin(1)
    has = mask.any(1)
    rows = np.arange(dm.shape[0])
    return (np.where(has, dm[rows, j], np.inf).astype(np.float32),
            np.where(has, index_base + j, -1).astype(np.int32))


def _reference(dm, edges, pos, neg, index_base=0, nearest=_nearest_lexsort):
    bins = np.searchsorted(edges, dm, side="left")
    n = len(edges) + 1
    return (np.bincount(bins[pos], minlength=n).astype(np.int64), np.bincount(bins[neg], minlength=n).astype(np.int64),
            nearest(dm, pos, index_base), nearest(dm, neg, index_base))


def _assert_equal(got, want, edges=None):
    """got: a numpy PairStats; want: _reference's tuple."""
    hp, hn, npos, nneg = want
    assert got.hist_pos.dtype == np.int64 and got.hist_neg.dtype == np.int64
    assert got.near_pos[0].dtype == np.float32 and got.near_pos[1].dtype == np.int32
    assert np.array_equal(got.hist_pos, hp), (got.hist_pos, hp)
    assert np.array_equal(got.hist_neg, hn), (got.hist_neg, hn)
    for (gd, gi), (wd, wi) in ((got.near_pos, npos), (got.near_neg, nneg)):
        assert np.array_equal(gi, wi)
        assert np.array_equal(_bits(gd), _bits(wd))
    if edges is not None:
        assert np.array_equal(_bits(got.edges), _bits(edges))


def _same_stats(a, b):
    _assert_equal(a, (b.hist_pos, b.hist_neg, b.near_pos, b.near_neg), b.edges)


# --------------------------------------------------------------------- 1. main case
@pytest.mark.parametrize("D", [36, 33])
def test_main_default_edges(gpu, D):
    ev = _ev()
    qf, gf, (qp, gp, qc, gc), dm = _base(D)
    edges = ev.default_edges()
    pos, neg = _masks(qp, gp, qc, gc)
    assert pos.any() and neg.any() and (~pos & ~neg).any()  # all three classes occur
    want = _reference(dm, edges, pos, neg)
    got = ev.pair_stats(qf, gf, qp, gp, qc, gc)
    _assert_equal(got, want, edges)
    assert got.hist_pos.sum() == pos.sum() and got.hist_neg.sum() == neg.sum()
    assert (got.hist_neg > 0).sum() > 8  # the distances spread over many bins
    # the vectorised nearest of the large case is the same function
    for mask in (pos, neg):
        a, b = _nearest_lexsort(dm, mask), _nearest_argmin(dm, mask)
        assert np.array_equal(a[1], b[1]) and np.array_equal(_bits(a[0]), _bits(b[0]))
    # the device form holds the same arrays on the GPU
    dev = ev.pair_stats_device(qf, gf, qp, gp, qc, gc)
    assert dev.hist_pos.is_cuda and dev.near_neg[1].is_cuda
    _same_stats(dev.numpy(), got)


# --------------------------------------------- 2. edges that coincide with distances
@pytest.mark.parametrize("D", [36, 33])
def test_edges_on_distances(gpu, D):
    ev = _ev()
    qf, gf, (qp, gp, qc, gc), dm = _base(D)
    pos, neg = _masks(qp, gp, qc, gc)
    vals = np.unique(dm)
    rng = np.random.default_rng(D)

    def check(edges):
        edges = np.asarray(edges, np.float32)
        _assert_equal(ev.pair_stats(qf, gf, qp, gp, qc, gc, edges=edges), _reference(dm, edges, pos, neg), edges)

    # 255 edges that are entries of the matrix: an entry equal to an edge belongs below it
    e255 = np.sort(rng.choice(vals, 255, replace=False))
    assert (dm[..., None] == e255[:8]).any()
    check(e255)
    # a duplicated edge (an empty bin), one edge below and one above every distance
    e = np.sort(rng.choice(vals, 20, replace=False))
    e = np.concatenate([[np.nextafter(vals[0], np.float32(-np.inf))], e[:10], [e[10], e[10]], e[11:],
                        [np.nextafter(vals[-1], np.float32(np.inf))]]).astype(np.float32)
    ref = _reference(dm, e, pos, neg)
    assert ref[0][0] + ref[1][0] == 0 and ref[0][-1] + ref[1][-1] == 0 and ref[0][12] + ref[1][12] == 0
    check(e)
    # the smallest and the largest distance themselves as edges
    check([vals[0], vals[-1]])
    # one edge
    check([vals[len(vals) // 2]])
    check([-1.0])
    check([5.0])


# ------------------------------------------------------ 3. ties in the nearest keys
def test_ties_go_to_the_lower_index(gpu):
    ev = _ev()
    D = 36
    qf0, gf0, (qp, gp, qc, gc), _ = _base(D)
    qf, gf = qf0.copy(), gf0.copy()
    qp, gp, qc, gc = (a.copy() for a in (qp, gp, qc, gc))
    # duplicate rows across the band border of the queries and the tile borders of the gallery (as
    # tests/test_gpu_cluster.py's _dup): a copy's distances are its original's bit for bit
    for i in range(8):
        qf[128 + i] = qf[127 - i]
        qp[128 + i], qc[128 + i] = qp[127 - i], qc[127 - i]
    for b in (128, 256):
        for i in range(8):
            gf[b + i] = gf[b - 1 - i]
            gp[b + i], gc[b + i] = gp[b - 1 - i], gc[b - 1 - i]
    # a genuine and an impostor column that are bit-equal copies of the query's own row: both at the
    # query's smallest distance.  Query 5: genuine at 120, impostor at 130 (another tile); query 140
    # (the second band): impostor at 250, genuine at 260.
    other = int(gp[gp > 0].max()) + 1
    for qi, jg, ji in ((5, 120, 130), (140, 260, 250)):
        gf[jg] = gf[ji] = qf[qi]
        gp[jg], gc[jg] = qp[qi], qc[qi] + 1
        gp[ji], gc[ji] = other, qc[qi]
    # two impostor copies of query 20's row on either side of a tile border
    gf[127] = gf[128] = qf[20]
    gp[127] = gp[128] = other
    dm = _matrix(qf, gf)
    pos, neg = _masks(qp, gp, qc, gc)
    want = _reference(dm, ev.default_edges(), pos, neg)
    got = ev.pair_stats(qf, gf, qp, gp, qc, gc)
    _assert_equal(got, want)
    assert _bits(dm[20, 127]) == _bits(dm[20, 128]) and got.near_neg[1][20] == 127
    for qi, jg, ji in ((5, 120, 130), (140, 260, 250)):
        assert _bits(dm[qi, jg]) == _bits(dm[qi, ji])
        assert got.near_pos[1][qi] == jg and got.near_neg[1][qi] == ji
        assert _bits(got.near_pos[0][qi]) == _bits(got.near_neg[0][qi])
    # the copied query rows across the band border report what their originals report
    for i in range(8):
        for near in (got.near_pos, got.near_neg):
            assert near[1][128 + i] == near[1][127 - i] and _bits(near[0][128 + i]) == _bits(near[0][127 - i])
    # open_set_rates follows the key order: query 5 is identified at its distance (the genuine copy
    # has the lower index), query 140 never is (the impostor copy comes first)
    tau = float(max(dm[5, 120], dm[140, 260], 0.0)) + 1e-3

    def only(i):
        return ev.PairStats(got.edges, got.hist_pos, got.hist_neg, tuple(a[i:i + 1] for a in got.near_pos),
                            tuple(a[i:i + 1] for a in got.near_neg))

    assert ev.open_set_rates(only(5), [tau])[0][0] == 1.0
    assert ev.open_set_rates(only(140), [tau, 4.0])[0].tolist() == [0.0, 0.0]


# ------------------------------------------- 4. no cameras; queries without a genuine item
@pytest.mark.parametrize("D", [36, 33])
def test_without_cameras_and_unknown_queries(gpu, D):
    ev = _ev()
    qf, gf, (qp, gp, qc, gc), dm = _base(D)
    edges = ev.default_edges()
    # without cameras nothing is removed
    pos, neg = _masks(qp, gp)
    assert pos.sum() > _masks(qp, gp, qc, gc)[0].sum()
    _assert_equal(ev.pair_stats(qf, gf, qp, gp), _reference(dm, edges, pos, neg), edges)
    # query 3: every gallery item of its pid gets its camera (all removed); query 150 (second band):
    # a pid the gallery does not hold
    qp, gc = qp.copy(), gc.copy()
    gc[gp == qp[3]] = qc[3]
    qp[150] = int(gp.max()) + 7
    pos, neg = _masks(qp, gp, qc, gc)
    assert not pos[3].any() and not pos[150].any() and neg[150].all()
    got = ev.pair_stats(qf, gf, qp, gp, qc, gc)
    _assert_equal(got, _reference(dm, edges, pos, neg), edges)
    for i in (3, 150):
        assert got.near_pos[1][i] == -1 and np.isposinf(got.near_pos[0][i])
        assert got.near_neg[1][i] >= 0
    # both count as unknown: at a threshold above every distance they, and only the unknown, alarm
    unknown = got.near_pos[1] < 0
    dir_, far = ev.open_set_rates(got, [-1.0, 5.0])
    assert unknown[3] and unknown[150] and far.tolist() == [0.0, 1.0] and dir_[0] == 0.0
    first = (got.near_pos[0] < got.near_neg[0]) | ((got.near_pos[0] == got.near_neg[0]) &
                                                   (got.near_pos[1] < got.near_neg[1]))
    assert dir_[1] == (first & ~unknown).sum() / (~unknown).sum()


# ------------------------------------------------------------------ 5. exclude_self
@pytest.mark.parametrize("D", [36, 33])
@pytest.mark.parametrize("cams", [False, True])
def test_exclude_self(gpu, D, cams):
    ev = _ev()
    _, x, (_, p, _, c), _ = _base(D)
    dm = _matrix(x, x)
    assert np.array_equal(dm, dm.T)
    lab = (c, c) if cams else (None, None)
    pos, neg = _masks(p, p, *lab, self_pairs=True)
    edges = ev.default_edges()
    got = ev.pair_stats(x, x, p, p, *lab, exclude_self=True)
    _assert_equal(got, _reference(dm, edges, pos, neg), edges)
    assert (got.near_pos[1] != np.arange(G)).all() and (got.near_neg[1] != np.arange(G)).all()
    if not cams:
        # the symmetric matrix without its diagonal: every unordered pair twice
        assert (got.hist_pos % 2 == 0).all() and (got.hist_neg % 2 == 0).all()
        assert got.hist_pos.sum() + got.hist_neg.sum() == G * (G - 1)
        # with the diagonal: G more genuine pairs, all at the rounding of zero
        full = ev.pair_stats(x, x, p, p)
        assert full.hist_pos.sum() == got.hist_pos.sum() + G and np.array_equal(full.hist_neg, got.hist_neg)
    # in blocks the diagonal moves with index_base
    acc = ev.PairStatsAccumulator(x, p, lab[0], exclude_self=True)
    for lo, hi in ((0, 100), (100, 229), (229, 300)):
        acc.add(x[lo:hi], p[lo:hi], None if lab[1] is None else c[lo:hi])
    _same_stats(acc.result().numpy(), got)


# ------------------------------------------------------------------------ 6. blocks
@pytest.mark.parametrize("D", [36, 33])
def test_blocks_any_order_and_merge(gpu, D):
    ev = _ev()
    qf, gf, (qp, gp, qc, gc), dm = _base(D)
    one = ev.pair_stats(qf, gf, qp, gp, qc, gc)
    cuts = ((0, 100), (100, 229), (229, 300))
    for order in ((0, 1, 2), (2, 0, 1)):
        acc = ev.PairStatsAccumulator(qf, qp, qc, None)
        for n in order:
            lo, hi = cuts[n]
            acc.add(torch.from_numpy(gf[lo:hi].copy()), gp[lo:hi], gc[lo:hi], index_base=lo)
        _same_stats(acc.result().numpy(), one)
    blocks = [(gf[lo:hi], gp[lo:hi], gc[lo:hi]) for lo, hi in cuts]
    _same_stats(ev.pair_stats_blocks(qf, blocks, qp, qc), one)
    # two half-gallery results, as two ranks would hold them
    a = ev.pair_stats(qf, gf[:150], qp, gp[:150], qc, gc[:150])
    b = ev.pair_stats(qf, gf[150:], qp, gp[150:], qc, gc[150:], index_base=150)
    _same_stats(ev.merge_pair_stats(a, b), one)
    _same_stats(ev.merge_pair_stats(b, a), one)
    da = ev.pair_stats_device(qf, gf[:150], qp, gp[:150], qc, gc[:150])
    db = ev.pair_stats_device(qf, gf[150:], qp, gp[150:], qc, gc[150:], index_base=150)
    _same_stats(ev.merge_pair_stats(da, db).numpy(), one)
    with pytest.raises(_err()):
        ev.merge_pair_stats(a, ev.pair_stats(qf, gf[150:], qp, gp[150:], qc, gc[150:], edges=[1.0]))
    with pytest.raises(_err()):
        ev.merge_pair_stats(a, db)


def test_python_layer_refusals(gpu):
    ev, err = _ev(), _err()
    qf, gf, (qp, gp, qc, gc), _ = _base(36)
    for kw in (dict(edges=[1.0, 0.5]), dict(edges=np.zeros(256)), dict(edges=[float("nan")]),
               dict(exclude_self=1), dict(index_base=-1), dict(index_base=2 ** 31 - 200)):
        with pytest.raises(err):
            ev.pair_stats(qf, gf, qp, gp, qc, gc, **kw)
    with pytest.raises(err):
        ev.pair_stats(qf, gf, qp, gp, qc, None)  # one camera array without the other
    with pytest.raises(err):
        ev.pair_stats(qf, gf, qp[:-1], gp, qc, gc)
    with pytest.raises(err):
        ev.pair_stats(qf, gf[:, :20], qp, gp, qc, gc)
    with pytest.raises(err):
        ev.PairStatsAccumulator(qf, qp, qc).result()  # nothing added


# ------------------------------------------- 7. more than one tile per workgroup
def test_several_tiles_per_range(gpu):
    ev = _ev()
    Qb, Gb, D = 8200, 2100, 36
    # the planner of reidmi_pair_stats_f32 (reidmi_evf_count's): 1024 slots over the query bands
    bands, tiles = -(-Qb // 128), -(-Gb // 128)
    s0 = max(1, min(1024 // bands, tiles))
    per = -(-tiles // s0)
    assert bands == 65 and per >= 2
    qp, gp, qc, gc = syn.labels(Qb, Gb, num_ids=40, num_cams=6, seed=7, junk_frac=0.02)
    qf, gf = syn.features(qp, gp, dim=D, seed=7)
    qf, gf = _normalised(qf), _normalised(gf)
    dm = _matrix(qf, gf)
    edges = ev.default_edges()
    pos, neg = _masks(qp, gp, qc, gc)
    want = _reference(dm, edges, pos, neg, nearest=_nearest_argmin)
    _assert_equal(ev.pair_stats(qf, gf, qp, gp, qc, gc), want, edges)


# ----------------------------------------------------------------- 8. counter width
def test_counts_past_32_bits(gpu):
    ev = _ev()
    n = 65536
    x = torch.full((n, 4), 0.5, device=gpu, dtype=torch.float32)
    qp = torch.arange(n, device=gpu, dtype=torch.int64)
    got = ev.pair_stats_device(x, x.clone(), qp, qp + n, edges=[1.0]).numpy()
    assert got.hist_neg.tolist() == [2 ** 32, 0]
    assert got.hist_pos.tolist() == [0, 0]
    assert (got.near_neg[1] == 0).all() and (_bits(got.near_neg[0]) == 0).all()
    assert (got.near_pos[1] == -1).all() and np.isposinf(got.near_pos[0]).all()


# ------------------------------------------------- 9. the derived host functions
def _hand_built():
    ev = _ev()
    f32, i32 = np.float32, np.int32
    return ev.PairStats(np.array([1.0, 2.0, 3.0], f32), np.array([2, 1, 1, 0], np.int64), np.array([0, 1, 3, 4], np.int64),
                        (np.array([0.5, 1.5, np.inf, np.inf, 0.7, 1.0], f32), np.array([3, 5, -1, -1, 2, 4], i32)),
                        (np.array([0.9, 1.0, 0.4, 2.5, 0.7, 1.0], f32), np.array([1, 2, 7, 8, 9, 1], i32)))


def test_derived_rates(gpu):
    ev = _ev()
    s = _hand_built()
    far, tar = ev.verification_curve(s)
    assert far.dtype == np.float64 and far.tolist() == [0.0, 1 / 8, 4 / 8] and tar.tolist() == [2 / 4, 3 / 4, 1.0]
    assert ev.threshold_at_far(s, 1 / 8) == 2.0 and ev.tar_at_far(s, 1 / 8) == 0.75
    assert ev.threshold_at_far(s, 0.1) == 1.0 and ev.tar_at_far(s, 0.1) == 0.5
    assert ev.threshold_at_far(s, 1.0) == 3.0 and ev.tar_at_far(s, 1.0) == 1.0
    # FAR 0 / FRR 1 | 0 / .5 | .125 / .25 | .5 / 0 | 1 / 0: the crossing lies between the edges 2 and 3,
    # at s = (.25 - .125) / (.375 + .25) = .2 of the way: .125 + .2 * .375
    assert ev.equal_error_rate(s) == pytest.approx(0.2, abs=1e-15)
    # known: 0, 1, 4, 5.  0 is identified from .5 on; 1 never (the impostor is nearer); 4 ties at .7 and
    # the genuine index 2 < 9: identified from .7 on; 5 ties at 1.0 with the impostor index lower: never.
    # unknown: 2 alarms from .4 on, 3 from 2.5 on.
    dir_, alarm = ev.open_set_rates(s, [0.3, 0.5, 0.7, 2.0, 3.0])
    assert dir_.tolist() == [0.0, 1 / 4, 2 / 4, 2 / 4, 2 / 4]
    assert alarm.tolist() == [0.0, 1 / 2, 1 / 2, 1 / 2, 1.0]
    assert ev.open_set_rates(s, 0.5)[0].shape == ()
    # the first edge already accepts too many impostors
    t = ev.PairStats(s.edges, s.hist_pos, np.array([3, 1, 0, 0], np.int64), s.near_pos, s.near_neg)
    assert np.isnan(ev.threshold_at_far(t, 0.5)) and np.isnan(ev.tar_at_far(t, 0.5))
    assert ev.threshold_at_far(t, 0.75) == 1.0
    # empty classes give NaN, not an exception
    zero = np.zeros(4, np.int64)
    no_pos = ev.PairStats(s.edges, zero, s.hist_neg, (np.full(2, np.inf, np.float32), np.full(2, -1, np.int32)),
                          (np.array([0.5, 0.6], np.float32), np.array([0, 1], np.int32)))
    far, tar = ev.verification_curve(no_pos)
    assert not np.isnan(far).any() and np.isnan(tar).all()
    assert np.isnan(ev.equal_error_rate(no_pos)) and np.isnan(ev.tar_at_far(no_pos, 0.5))
    assert ev.threshold_at_far(no_pos, 0.5) == 3.0
    dir_, alarm = ev.open_set_rates(no_pos, [0.55])
    assert np.isnan(dir_[0]) and alarm[0] == 0.5
    no_neg = ev.PairStats(s.edges, s.hist_pos, zero, (np.array([0.5], np.float32), np.array([0], np.int32)),
                          (np.array([np.inf], np.float32), np.array([-1], np.int32)))
    assert np.isnan(ev.verification_curve(no_neg)[0]).all() and np.isnan(ev.threshold_at_far(no_neg, 0.5))
    dir_, alarm = ev.open_set_rates(no_neg, [0.4, 0.5])
    assert dir_.tolist() == [0.0, 1.0] and np.isnan(alarm).all()
    with pytest.raises(_err()):
        ev.threshold_at_far(s, 1.5)


# ------------------------------------------------------------ 10. R1_mAP_eval.pair_stats
def test_r1_map_eval_pair_stats(gpu):
    ev = _ev()
    D = 36
    qp, gp, qc, gc = syn.labels(Q, G, num_ids=12, num_cams=6, seed=3, junk_frac=0.05)
    qf, gf = syn.features(qp, gp, dim=D, seed=3)  # not normalised
    m = ev.R1_mAP_eval(Q)
    m.reset()
    feats, pids, cams = np.concatenate([qf, gf]), np.concatenate([qp, gp]), np.concatenate([qc, gc])
    for lo in range(0, Q + G, 128):
        m.update((torch.from_numpy(feats[lo:lo + 128]), pids[lo:lo + 128], cams[lo:lo + 128]))
    n = _normalised(feats)
    edges = np.linspace(0.0, 4.0, 50).astype(np.float32)
    _same_stats(m.pair_stats(edges), ev.pair_stats(n[:Q], n[Q:], qp, gp, qc, gc, edges=edges))
    _same_stats(m.pair_stats(), ev.pair_stats(n[:Q], n[Q:], qp, gp, qc, gc))
    # with query expansion the statistics are those of the expanded features
    mq = ev.R1_mAP_eval(Q, query_expansion=(3, 0))
    mq.reset()
    mq.update((torch.from_numpy(feats), pids, cams))
    xq = ev.expand_features(n[:Q], n[Q:], 3, 0)
    _same_stats(mq.pair_stats(edges), ev.pair_stats(xq, n[Q:], qp, gp, qc, gc, edges=edges))
    for kw in (dict(sharded=True), dict(reranking=True)):
        bad = ev.R1_mAP_eval(Q, **kw)
        bad.reset()
        bad.update((torch.from_numpy(feats), pids, cams))
        with pytest.raises(_err()):
            bad.pair_stats()
