"""The gallery-sharded search (evaluate.search_sharded, R1_mAP_eval(sharded=True).rank_lists) on one
GPU: 2 and 3 gloo ranks sharing cuda:0, each with its contiguous shard of the queries and of the
gallery, must return on every rank the one-process result over the whole split, bit for bit
(indices as integers, distances as their uint32 patterns):

* search_sharded with and without labels at k = 10 and k = 128 (Q = 130, G = 620, D = 256; at
  world 3 the gallery shards hold 206 or 207 rows), and at G = 5, k = 3, where at world 3 every
  shard (1, 2 and 2 rows) is smaller than k;
* R1_mAP_eval(num_query=local, sharded=True).rank_lists(10), Euclidean and re-ranked;
* R1_mAP_eval(sharded=False).rank_lists under the process group, on the last rank only: the
  one-process lists and no collective (the other ranks never call it: no hang);
* an nccl world of one process: search_sharded's collectives on the RCCL path.
(gloo moves the collectives' bytes through the host; RCCL refuses several ranks on one GPU.)"""
import os
import socket
import sys

import numpy as np
import pytest
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
import reidmi_boot  # noqa: E402  (the spawned workers re-import this module without conftest)

reidmi_boot.load()

from multimodal_reid_amd import synthetic as syn  # noqa: E402

pytestmark = pytest.mark.gpu

Q, G, D = 130, 620, 256
KS = (10, 128)


def _data():
    qp, gp, qc, gc = syn.labels(Q, G, num_ids=50, num_cams=6, seed=7, junk_frac=0.02)
    qf, gf = syn.features(qp, gp, dim=D, seed=7)
    return qf, gf, qp, gp, qc, gc


def _evaluator(qf, gf, qp, gp, qc, gc, **kw):
    from multimodal_reid_amd import evaluate
    ev = evaluate.R1_mAP_eval(num_query=len(qf), **kw)
    ev.reset()
    ev.update((torch.from_numpy(qf), qp, qc))
    ev.update((torch.from_numpy(gf), gp, gc))
    return ev


def _run(rank, world, sharded):
    """Everything under test on this rank's shards (sharded) or, world 1, on the whole split."""
    from multimodal_reid_amd import distributed as rd, evaluate
    qf, gf, qp, gp, qc, gc = _data()
    qlo, qhi = rd.shard(Q, rank, world)
    glo, ghi = rd.shard(G, rank, world)
    mine = (qf[qlo:qhi], gf[glo:ghi], qp[qlo:qhi], gp[glo:ghi], qc[qlo:qhi], gc[glo:ghi])
    q, g, sqp, sgp, sqc, sgc = mine
    find = evaluate.search_sharded if sharded else evaluate.search
    res = {}
    for k in KS:
        res["plain", k] = find(q, g, k)
        res["labels", k] = find(q, g, k, sqp, sqc, sgp, sgc)
    s5lo, s5hi = rd.shard(5, rank, world)  # a gallery of 5: shards of 1, 2 and 2 rows at world 3
    res["small"] = find(q, gf[s5lo:s5hi], 3)
    res["small labels"] = find(q, gf[s5lo:s5hi], 3, sqp, sqc, gp[s5lo:s5hi], gc[s5lo:s5hi])
    for rr in (False, True):
        res["eval", rr] = _evaluator(*mine, reranking=rr, sharded=sharded).rank_lists(10)
    if sharded and rank == world - 1:
        for rr in (False, True):
            res["unsharded", rr] = _evaluator(qf, gf, qp, gp, qc, gc, reranking=rr).rank_lists(10)
    return res


def _worker(rank, world, port, out):
    import torch.distributed as dist
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        torch.cuda.set_device(0)
        out[rank] = _run(rank, world, True)
    finally:
        dist.destroy_process_group()


def _nccl_worker(rank, port, out):
    import torch.distributed as dist
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    torch.cuda.set_device(0)
    dist.init_process_group("nccl", rank=0, world_size=1, device_id=torch.device("cuda", 0))
    try:
        from multimodal_reid_amd import evaluate
        assert dist.get_backend() == "nccl"
        qf, gf, qp, gp, qc, gc = _data()
        out["plain"] = evaluate.search_sharded(qf, gf, 10)
        out["labels"] = evaluate.search_sharded(qf, gf, 128, qp, qc, gp, gc)
        out["small"] = evaluate.search_sharded(qf, gf[:5], 3)
    finally:
        dist.destroy_process_group()


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _same(got, want, what):
    assert np.array_equal(got[0], want[0]), what
    assert np.array_equal(got[1].view(np.uint32), want[1].view(np.uint32)), what


@pytest.fixture(scope="module")
def single(gpu):
    return _run(0, 1, False)


def test_sharded_needs_a_process_group(gpu):
    from multimodal_reid_amd import evaluate
    from multimodal_reid_amd._lib import ReidmiError
    qf, gf, qp, gp, qc, gc = _data()
    with pytest.raises(ReidmiError, match="process group"):
        evaluate.search_sharded(qf, gf, 10)
    with pytest.raises(ReidmiError, match="process group"):
        _evaluator(qf, gf, qp, gp, qc, gc, sharded=True).rank_lists(10)


@pytest.mark.parametrize("world", [2, 3])
def test_sharded_search_equals_single_process(single, world):
    import torch.multiprocessing as mp
    mgr = mp.Manager()
    out = mgr.dict()
    mp.spawn(_worker, args=(world, _free_port(), out), nprocs=world, join=True)
    for r in range(world):
        for key, want in single.items():
            _same(out[r][key], want, (r, key))
    for rr in (False, True):
        _same(out[world - 1]["unsharded", rr], single["eval", rr], ("unsharded", rr))


def test_rccl_world1_search_sharded(single):
    import torch.multiprocessing as mp
    mgr = mp.Manager()
    out = mgr.dict()
    mp.spawn(_nccl_worker, args=(_free_port(), out), nprocs=1, join=True)
    _same(out["plain"], single["plain", 10], "plain")
    _same(out["labels"], single["labels", 128], "labels")
    _same(out["small"], single["small"], "small")
