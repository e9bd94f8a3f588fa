"""The gallery-sharded matrix-free scoring (evaluate.eval_features_sharded,
R1_mAP_eval(sharded=True, matrix_free=True).compute) on one GPU: 2 and 3 gloo ranks sharing
cuda:0, each with its contiguous shard of the queries and of the gallery, must return on every rank
the one-process result over the whole split, bit for bit (the CMC as float32 values, the mAP as
its uint64 pattern, the per-query records as integers / patterns):

* Q = 130, G = 620, D = 256 (at world 3 the gallery shards hold 206 or 207 rows);
* a gallery of 5 (shards of 1, 2 and 2 rows at world 3) whose last rows hold no match of any
  query: the last rank's shard contributes empty lists;
* an nccl world of one process: the collectives on the RCCL path.
Every worker runs under its own time limit (the process group's, and the parent's deadline for the
whole world); a rank that fails ends the others instead of leaving them in a collective.
(gloo moves the collectives' bytes through the host; RCCL refuses several ranks on one GPU.)"""
import datetime
import os
import socket
import sys
import time

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
WORKER_LIMIT = 120  # seconds: a collective that waits longer than this fails its rank


def _data():
    qp, gp, qc, gc = syn.labels(Q, G, num_ids=50, num_cams=6, seed=7, junk_frac=0.02)
    qf, gf = syn.features(qp, gp, dim=D, seed=7)
    return qf, gf, qp, gp, qc, gc


def _small():
    """A gallery of 5 in which only rows 0..2 carry query pids (rows 3, 4: a pid no query has)."""
    qf, gf, qp, gp, qc, gc = _data()
    gp5 = np.array([qp[0], qp[1], qp[0], -9, -9], np.int64)
    gc5 = np.array([qc[0] + 1, qc[1] + 1, qc[0], 0, 0], np.int64)
    return gf[:5], gp5, gc5


def _evaluator(qf, gf, qp, gp, qc, gc, **kw):
    from multimodal_reid_amd import evaluate
    ev = evaluate.R1_mAP_eval(num_query=len(qf), **kw)
    ev.reset()
    ev.update((torch.from_numpy(qf), qp, qc))
    ev.update((torch.from_numpy(gf), gp, gc))
    return ev


def _records(res):
    return [t.cpu().numpy() for t in res[0]] + [res[1]]


def _run(rank, world, sharded):
    """Everything under test on this rank's shards (sharded) or, world 1, on the whole split."""
    from multimodal_reid_amd import distributed as rd, evaluate
    qf, gf, qp, gp, qc, gc = _data()
    g5, gp5, gc5 = _small()
    qlo, qhi = rd.shard(Q, rank, world)
    glo, ghi = rd.shard(G, rank, world)
    slo, shi = rd.shard(5, rank, world)
    q, sqp, sqc = qf[qlo:qhi], qp[qlo:qhi], qc[qlo:qhi]
    res = {}
    if sharded:
        res["score"] = evaluate.eval_features_sharded(q, gf[glo:ghi], sqp, sqc, gp[glo:ghi], gc[glo:ghi])
        res["records"] = _records(evaluate.eval_features_sharded_device(q, gf[glo:ghi], sqp, sqc, gp[glo:ghi],
                                                                        gc[glo:ghi]))
        res["small"] = evaluate.eval_features_sharded(q, g5[slo:shi], sqp, sqc, gp5[slo:shi], gc5[slo:shi],
                                                      max_rank=3)
    else:
        res["score"] = evaluate.eval_func_features(qf, gf, qp, gp, qc, gc)
        res["records"] = _records((evaluate.eval_features_device(qf, gf, qp, gp, qc, gc), G))
        res["small"] = evaluate.eval_func_features(qf, g5, qp, gp5, qc, gc5, max_rank=3)
        res["matrix"] = evaluate.eval_func(evaluate.euclidean_distance(qf, gf), qp, gp, qc, gc)
    res["eval"] = _evaluator(q, gf[glo:ghi], sqp, gp[glo:ghi], sqc, gc[glo:ghi], sharded=sharded, feat_norm=False,
                             matrix_free=True).compute()
    return res


def _worker(rank, world, port, out):
    import torch.distributed as dist
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world, timeout=datetime.timedelta(seconds=WORKER_LIMIT))
    try:
        torch.cuda.set_device(0)
        out[rank] = _run(rank, world, True)
    finally:
        dist.destroy_process_group()


def _nccl_worker(rank, port, out):
    import torch.distributed as dist
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    torch.cuda.set_device(0)
    dist.init_process_group("nccl", rank=0, world_size=1, device_id=torch.device("cuda", 0),
                            timeout=datetime.timedelta(seconds=WORKER_LIMIT))
    try:
        assert dist.get_backend() == "nccl"
        out[0] = _run(0, 1, True)
    finally:
        dist.destroy_process_group()


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _spawn(fn, args, nprocs):
    """mp.spawn under a deadline: a rank that raises ends the others (ProcessContext.join), and a
    world still running at the deadline is ended and fails the test."""
    import torch.multiprocessing as mp
    ctx = mp.spawn(fn, args=args, nprocs=nprocs, join=False)
    deadline = time.monotonic() + WORKER_LIMIT + 30
    try:
        while not ctx.join(timeout=5):
            assert time.monotonic() < deadline, "the workers did not finish in time"
    finally:
        for p in ctx.processes:
            if p.is_alive():
                p.terminate()
        for p in ctx.processes:
            p.join(10)


def _same_score(got, want, what):
    assert got[0].dtype == want[0].dtype and np.array_equal(got[0], want[0]), what
    assert np.float64(got[1]).view(np.uint64) == np.float64(want[1]).view(np.uint64), what


def _check(got, single, what):
    for key in ("score", "small", "eval"):
        _same_score(got[key], single["score" if key == "eval" else key], (what, key))
    for a, b in zip(got["records"], single["records"]):
        a, b = np.asarray(a), np.asarray(b)
        assert a.dtype == b.dtype
        assert np.array_equal(a.view(np.uint64) if a.dtype == np.float64 else a,
                              b.view(np.uint64) if b.dtype == np.float64 else b), what


@pytest.fixture(scope="module")
def single(gpu):
    res = _run(0, 1, False)
    _same_score(res["score"], res["matrix"], "matrix-free against the matrix path")
    _same_score(res["eval"], res["matrix"], "R1_mAP_eval(matrix_free=True)")
    return res


def test_sharded_needs_a_process_group(gpu):
    from multimodal_reid_amd import evaluate
    from multimodal_reid_amd._lib import ReidmiError
    qf, gf, qp, gp, qc, gc = _data()
    with pytest.raises(ReidmiError, match="process group"):
        evaluate.eval_features_sharded(qf, gf, qp, qc, gp, gc)
    with pytest.raises(ReidmiError, match="process group"):
        _evaluator(qf, gf, qp, gp, qc, gc, sharded=True, matrix_free=True).compute()


@pytest.mark.parametrize("world", [2, 3])
def test_sharded_scoring_equals_single_process(single, world):
    import torch.multiprocessing as mp
    mgr = mp.Manager()
    out = mgr.dict()
    _spawn(_worker, (world, _free_port(), out), world)
    for r in range(world):
        _check(out[r], single, r)


def test_rccl_world1_scoring(single):
    import torch.multiprocessing as mp
    mgr = mp.Manager()
    out = mgr.dict()
    _spawn(_nccl_worker, (_free_port(), out), 1)
    _check(out[0], single, "nccl")
