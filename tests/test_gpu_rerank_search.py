"""Re-ranked rank lists (reidmi_rr_jaccard_topk_rows, reranking.re_ranking_search,
R1_mAP_eval(reranking=True).rank_lists) against np.argsort(final, kind="stable")[:, :k] of the
re-ranked matrix `final`: the CPU oracle's where N is small, else the project's own matrix route.
Every comparison is bit equality: indices as integers, distances as their uint32 patterns.  The
direct calls run on outputs prefilled with -2 / NaN inside a pitch of k + 3 and followed by a
sentinel tail, and on a workspace followed by a tail; pitch padding and tails must come back
untouched."""
import os
import socket
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import reidmi_boot  # noqa: E402

reidmi_boot.load()

import oracle  # noqa: E402
from multimodal_reid_amd import synthetic as syn  # noqa: E402

pytestmark = pytest.mark.gpu

JCH = 8192  # gallery columns per Jaccard workgroup (rerank.h)
TAIL, IDX_TAIL, DIST_TAIL = 64, -77, np.float32(-12345.5)
LAM = 0.3


def _rr():
    from multimodal_reid_amd import reranking
    return reranking


def _i64(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.int64)).cuda()


def reference(final, k, labels=None):
    """(idx, dist) of the stable argsort of `final`'s rows; with labels = (qp, qc, gp, gc) the
    same-pid-same-camera entries are masked out first and short rows end in -1 / +inf."""
    Q, G = final.shape
    if labels is None:
        idx = np.argsort(final, axis=1, kind="stable")[:, :k]
        return idx.astype(np.int32), np.take_along_axis(final, idx, 1)
    qp, qc, gp, gc = labels
    idx = np.full((Q, k), -1, np.int32)
    dist = np.full((Q, k), np.inf, np.float32)
    for i in range(Q):
        keep = np.flatnonzero(~((gp == qp[i]) & (gc == qc[i])))
        order = keep[np.argsort(final[i, keep], kind="stable")][:k]
        idx[i, :len(order)] = order
        dist[i, :len(order)] = final[i, order]
    return idx, dist


def same(got, ref):
    return np.array_equal(got[0], ref[0]) and np.array_equal(got[1].view(np.uint32), ref[1].view(np.uint32))


def run_lists(feats, Q, k1, k2, k, labels=None, chunk_bytes=None, with_dist=True):
    """The staged stages with the last one called directly (reidmi_rr_jaccard_topk_rows) on
    sentinel-filled buffers; returns (idx, dist, the number of query-row passes of that call)."""
    from multimodal_reid_amd import _lib
    rr = _rr()
    f = torch.from_numpy(np.ascontiguousarray(feats)).cuda()
    N, G = f.shape[0], f.shape[0] - Q
    box = {}

    class Checked(rr.HipStages):
        def jaccard_topk_rows(self, rmax, Vq, qlo, qhi, k, labels=None, with_dist=True):
            off, col, val = Vq
            coff, irow, ival = self._csc(Vq)
            bounds, bb, cr = self._jaccard_pass(qlo, qhi)
            box["passes"] = -(-(qhi - qlo) // cr)
            nb = int(_lib.load().reidmi_rr_jaccard_topk_workspace_bytes(cr, G, k))
            assert nb == cr * -(-G // JCH) * k * 8
            ws = torch.full((nb + TAIL,), 0xFF, device="cuda", dtype=torch.uint8)
            ws[nb:] = 0xA5
            rows, ldo = qhi - qlo, k + 3
            oi = torch.full((rows * ldo + TAIL,), -2, device="cuda", dtype=torch.int32)
            oi[rows * ldo:] = IDX_TAIL
            od = None
            if with_dist:
                od = torch.full((rows * ldo + TAIL,), float("nan"), device="cuda")
                od[rows * ldo:] = float(DIST_TAIL)
            lab = [_lib.ptr(t) for t in (labels or (None,) * 4)]
            chunk = torch.empty(cr * G, device="cuda")
            _lib.call("reidmi_rr_jaccard_topk_rows", _lib.ptr(self.feat), N, self.D, self.D, _lib.ptr(self.sqn),
                      _lib.ptr(rmax), Q, qlo, qhi, _lib.ptr(off), _lib.ptr(col), _lib.ptr(val), _lib.ptr(coff),
                      _lib.ptr(irow), _lib.ptr(ival), self.lam_h, self.lam_f, k, *lab, _lib.ptr(oi), _lib.ptr(od), ldo,
                      _lib.ptr(chunk), cr, _lib.ptr(bounds), bb, _lib.ptr(ws), nb, self.st)
            torch.cuda.synchronize()
            assert bool((ws[nb:] == 0xA5).all()), "wrote past the declared workspace"
            oin = oi.cpu().numpy()
            assert (oin[rows * ldo:] == IDX_TAIL).all()
            oin = oin[:rows * ldo].reshape(rows, ldo)
            assert (oin[:, k:] == -2).all()
            res = [oin[:, :k].copy(), None]
            if with_dist:
                odn = od.cpu().numpy()
                assert (odn[rows * ldo:] == DIST_TAIL).all()
                odn = odn[:rows * ldo].reshape(rows, ldo)
                assert np.isnan(odn[:, k:]).all()
                res[1] = odn[:, :k].copy()
            return res

    lab = None if labels is None else tuple(_i64(a) for a in labels)
    got = rr.staged_rerank(Checked(f, Q, k1, k2, LAM, chunk_bytes), N, Q, k, lab, with_dist)
    return got[0], got[1], box["passes"]


def matrix_route(feats, Q, k1, k2, chunk_bytes=None):
    f = torch.from_numpy(np.ascontiguousarray(feats)).cuda()
    return _rr().re_ranking_sharded(f[:Q], f[Q:], k1, k2, LAM, chunk_bytes=chunk_bytes).cpu().numpy()


# ------------------------------------------------------------------------- 1. one chunk
Q1, G1 = 100, 500


@pytest.fixture(scope="module")
def small():
    qp, gp, qc, gc = syn.labels(Q1, G1, num_ids=60, num_cams=6, seed=1, distractor_frac=0.1, junk_frac=0.04)
    qf, gf = syn.features(qp, gp, dim=64, seed=1, noise=1.0)
    feats = oracle.l2norm(np.concatenate([qf, gf]))
    finals = {}

    def final(k1, k2):
        if (k1, k2) not in finals:
            finals[(k1, k2)] = oracle.re_ranking(feats[:Q1], feats[Q1:], k1, k2, LAM)
        return finals[(k1, k2)]

    return feats, (qp, qc, gp, gc), final


@pytest.mark.parametrize("with_labels", [False, True])
@pytest.mark.parametrize("k", [1, 10, 128])
@pytest.mark.parametrize("k1,k2", [(50, 15), (20, 6), (20, 1)])
def test_one_chunk_vs_oracle(gpu, small, k1, k2, k, with_labels):
    feats, labels, final = small
    lab = labels if with_labels else None
    if with_labels:
        qp, qc, gp, gc = labels
        assert ((gp[None, :] == qp[:, None]) & (gc[None, :] == qc[:, None])).any()
    ref = reference(final(k1, k2), k, lab)
    idx, dist, _ = run_lists(feats, Q1, k1, k2, k, lab)
    assert same((idx, dist), ref)
    if k == 10:  # out_dist = NULL
        assert np.array_equal(run_lists(feats, Q1, k1, k2, k, lab, with_dist=False)[0], ref[0])


# ----------------------------------------------------------------------- 2. chunk edges
def _edge_feats(G, Q=48, ids=400, seed=7):
    """Gallery ids cycle with period `ids`, so every id has items on both sides of column 8192;
    the queries take the ids of the columns from 8192 on (the ragged chunk's 37 at G = 8229)."""
    gp = 1 + np.arange(G) % ids
    qp = gp[JCH + np.arange(Q) % min(37, G - JCH)]
    qf, gf = syn.features(qp, gp, dim=64, seed=seed, noise=0.35)
    return oracle.l2norm(np.concatenate([qf, gf]))


@pytest.mark.parametrize("G", [JCH + 37, 2 * JCH])
def test_chunk_edges(gpu, G):
    Q, k, k1, k2 = 48, 50, 20, 6
    feats = _edge_feats(G)
    N = Q + G
    final = matrix_route(feats, Q, k1, k2, chunk_bytes=4 * N * 20)  # the same chunk_bytes as the lists below
    ref = reference(final, k)
    both = ((ref[0] < JCH).any(1) & (ref[0] >= JCH).any(1)).sum()
    assert both >= Q // 2, both  # the lists span the chunk boundary
    if G == JCH + 37:
        assert G - JCH < k  # the ragged chunk's partial list is padded
        orc = oracle.re_ranking(feats[:Q], feats[Q:], k1, k2, LAM)
        assert np.array_equal(orc.view(np.uint32), final.view(np.uint32))
    idx, dist, passes = run_lists(feats, Q, k1, k2, k, chunk_bytes=4 * N * 20)
    assert passes == 3  # 20 + 20 + 8 query rows per pass
    assert same((idx, dist), ref)


# ------------------------------------------------------------------------------ 3. ties
def test_ties_across_chunks(gpu):
    """Every gallery row twice, at j and j + G/2 (different chunks): twins tie exactly where the
    Jaccard overlap is zero; the order inside a tie and the cut through one follow the index."""
    Q, H, k1, k2 = 16, JCH + 8, 20, 6
    gp = 1 + np.arange(H) % 1000
    qp = gp[:Q].copy()
    qf, gf = syn.features(qp, gp, dim=64, seed=3, noise=0.35)
    feats = oracle.l2norm(np.concatenate([qf, gf, gf]))
    G = 2 * H
    final = matrix_route(feats, Q, k1, k2)
    order = np.argsort(final, axis=1, kind="stable")[:, :129]
    vals = np.take_along_axis(final, order, 1)
    tied = vals[:, 1:] == vals[:, :-1]  # [:, p]: places p | p + 1 tie
    assert tied[:, :127].any()  # a tie group inside the top 128
    twins = (np.abs(order[:, 1:] - order[:, :-1]) == H) & tied
    assert twins[:, :127].any()  # ... of twins in different chunks
    cuts = np.flatnonzero(tied.any(0)) + 1  # k with a tie across places k-1 | k for some query
    cuts = cuts[cuts <= 128]
    assert len(cuts), "no k <= 128 cuts through a tie"
    for k in (128, int(cuts[-1])):
        idx, dist, _ = run_lists(feats, Q, k1, k2, k)
        assert same((idx, dist), reference(final, k)), k


# ---------------------------------------------------------------- 4. labels and padding
def test_labels_tiny_gallery_pads_short_rows(gpu):
    Q, G, k = 12, 8, 8
    r = np.random.default_rng(4)
    feats = oracle.l2norm(r.standard_normal((Q + G, 16)).astype(np.float32))
    gp = np.array([1, 1, 1, 2, 2, 3, 3, 0], np.int64)
    gc = np.array([0, 0, 1, 0, 1, 2, 2, 5], np.int64)
    qp = np.array([1, 1, 2, 3, 3, 4, 1, 2, 3, 1, 2, 4], np.int64)
    qc = np.array([0, 1, 0, 2, 0, 0, 2, 1, 2, 0, 3, 1], np.int64)
    final = oracle.re_ranking(feats[:Q], feats[Q:], 6, 3, LAM)
    ref = reference(final, k, (qp, qc, gp, gc))
    lost = (ref[0] < 0).sum(1)
    assert lost.max() == 2 and (lost == 0).any()  # some queries lose items, some none
    idx, dist, _ = run_lists(feats, Q, 6, 3, k, (qp, qc, gp, gc))
    assert same((idx, dist), ref)
    assert (idx[lost > 0, -1] == -1).all() and np.isposinf(dist[lost > 0, -1]).all()


# ------------------------------------------------------- 5. independence from chunking
def test_independent_of_chunk_bytes(gpu, small):
    feats, labels, final = small
    rr = _rr()
    N = Q1 + G1
    ref = reference(final(20, 6), 50, labels)
    one = rr.re_ranking_search(feats[:Q1], feats[Q1:], 50, 20, 6, LAM, *labels, chunk_bytes=4 * N * 4096)
    many = rr.re_ranking_search(feats[:Q1], feats[Q1:], 50, 20, 6, LAM, *labels, chunk_bytes=4 * N * 7)
    assert one[0].dtype == np.int32 and one[1].dtype == np.float32
    assert same(one, ref) and same(many, ref)
    idx, none = rr.re_ranking_search_device(torch.from_numpy(feats[:Q1]).cuda(), feats[Q1:], 50, 20, 6, LAM,
                                            with_dist=False)
    assert none is None and idx.is_cuda and np.array_equal(idx.cpu().numpy(), reference(final(20, 6), 50)[0])
    from multimodal_reid_amd import _lib
    with pytest.raises(_lib.ReidmiError, match=r"1 <= k <= min\(G, 128\)"):
        rr.re_ranking_search(feats[:Q1], feats[Q1:], 129, 20, 6, LAM)


# -------------------------------------------------------------------------- 6. evaluator
def test_evaluator_rank_lists(gpu):
    from multimodal_reid_amd import evaluate
    rr = _rr()
    qp, gp, qc, gc = syn.labels(Q1, G1, num_ids=60, num_cams=6, seed=1, distractor_frac=0.1, junk_frac=0.04)
    qf, gf = syn.features(qp, gp, dim=64, seed=1, noise=1.0)
    k = 10

    def evaluator(reranking):
        m = evaluate.R1_mAP_eval(Q1, max_rank=50, feat_norm=True, reranking=reranking)
        m.reset()
        m.update((torch.from_numpy(qf), qp, qc))
        m.update((torch.from_numpy(gf), gp, gc))
        return m

    m = evaluator(True)
    qn = evaluate.l2_normalize_device(torch.from_numpy(qf))
    gn = evaluate.l2_normalize_device(torch.from_numpy(gf))
    idx, dist = m.rank_lists(k)
    assert same((idx, dist), rr.re_ranking_search(qn, gn, k, 50, 15, 0.3, qp, qc, gp, gc))
    plain = m.rank_lists(k, remove_same_cam=False)
    assert same(plain, rr.re_ranking_search(qn, gn, k, 50, 15, 0.3))
    assert not np.array_equal(plain[0], idx)
    # rank-1 of compute(): the first kept item of every valid query
    cmc, _ = m.compute()
    removed = (gp[None, :] == qp[:, None]) & (gc[None, :] == qc[:, None])
    valid = ((gp[None, :] == qp[:, None]) & ~removed).any(1)
    hits = int((gp[idx[valid, 0]] == qp[valid]).sum())
    assert 0 < hits and valid.sum() > Q1 // 2
    assert (np.asarray([hits]).astype(np.float32) / float(valid.sum()))[0].view(np.uint32) == \
        np.float32(cmc[0]).view(np.uint32)
    # without re-ranking: the Euclidean lists, as before
    e = evaluator(False)
    assert same(e.rank_lists(k), evaluate.search(qn, gn, k, qp, qc, gp, gc))
    assert not np.array_equal(e.rank_lists(k)[0], idx)


# ------------------------------------------------------------- 7. two ranks on one GPU
Q7, G7 = 120, 900


def _feats7():
    qp, gp, qc, gc = syn.labels(Q7, G7, num_ids=400, num_cams=6, seed=5)
    qf, gf = syn.features(qp, gp, dim=256, seed=5, noise=3.0)
    return oracle.l2norm(np.concatenate([qf, gf])), (qp, qc, gp, gc)


def _worker(rank, world, port, out):
    import torch.distributed as dist
    from multimodal_reid_amd import reranking
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        torch.cuda.set_device(0)
        feats, labels = _feats7()
        out[rank] = reranking.re_ranking_search(feats[:Q7], feats[Q7:], 50, 50, 15, LAM, *labels, sharded=True,
                                                chunk_bytes=4 * (Q7 + G7) * 200)
    finally:
        dist.destroy_process_group()


def test_sharded_two_ranks_one_gpu(gpu):
    import torch.multiprocessing as mp
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    ctx = mp.get_context("spawn")
    mgr = ctx.Manager()
    out = mgr.dict()
    procs = [ctx.Process(target=_worker, args=(r, 2, port, out)) for r in range(2)]
    for p in procs:
        p.start()
    for p in procs:
        p.join(timeout=150)
    alive = [p.is_alive() for p in procs]
    for p in procs:
        if p.is_alive():
            p.kill()
            p.join()
    assert not any(alive), "a rank did not finish in time"
    assert [p.exitcode for p in procs] == [0, 0]
    feats, labels = _feats7()
    one = _rr().re_ranking_search(feats[:Q7], feats[Q7:], 50, 50, 15, LAM, *labels)
    assert (one[0] >= 0).all()
    for r in range(2):
        assert same(out[r], one), r
