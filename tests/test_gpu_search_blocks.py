"""Blocked search (evaluate.SearchAccumulator / search_blocks) against the one-call search on the
concatenated gallery, bit for bit: indices as integers, distances as their uint32 patterns, for
every way of cutting the gallery tried here.

Q = 130 (two query bands, the second ragged), G = 1000, D = 36 (the pipelined mainloop) and D = 33
(the single-stage one).  40 gallery rows are copies of other rows: their distances to a query are
equal bit for bit and only the global index orders them.  The copies sit on both sides of every
block boundary of the splits (1, 128, 256, 500, 556) and, a few, inside one block."""
import numpy as np
import pytest
import torch

from multimodal_reid_amd import synthetic as syn

pytestmark = pytest.mark.gpu

Q, G = 130, 1000
SPLITS = {"one": (1000,), "ragged": (1, 127, 128, 300, 444), "empty": (500, 0, 500), "rows": (1,) * 1000}


def _ev():
    from multimodal_reid_amd import evaluate
    return evaluate


def _data(D):
    qp, gp, qc, gc = syn.labels(Q, G, num_ids=40, num_cams=6, seed=D)
    qf, gf = syn.features(qp, gp, dim=D, seed=D)
    gf = gf.copy()
    gf[0] = gf[1]  # across the boundary at 1
    for b in (128, 256, 500, 556):  # across each boundary: row b + i is row b - 1 - i
        for i in range(8):
            gf[b + i] = gf[b - 1 - i]
    for i in range(7):  # inside a block of every split but the one-row blocks
        gf[700 + i] = gf[650 + i]
    return qf, gf, qp, gp, qc, gc


_cache = {}


def _case(D, k, labels):
    """The data of dimension D and the one-call search's (idx, dist) for it; computed once."""
    key = (D, k, labels)
    if key not in _cache:
        if D not in _cache:
            _cache[D] = _data(D)
        qf, gf, qp, gp, qc, gc = _cache[D]
        _cache[key] = _ev().search(qf, gf, k, *((qp, qc, gp, gc) if labels else ()))
    return _cache[D], _cache[key]


def _blocks(gf, gp, gc, sizes, labels, host=False):
    out, lo = [], 0
    for n in sizes:
        f = torch.from_numpy(gf[lo:lo + n])
        f = f if host else f.cuda()
        out.append((f, gp[lo:lo + n], gc[lo:lo + n]) if labels else f)
        lo += n
    assert lo == len(gf)
    return out


def _same(got, want):
    assert np.array_equal(got[0], want[0])
    assert np.array_equal(got[1].view(np.uint32), want[1].view(np.uint32))


@pytest.mark.parametrize("labels", [False, True], ids=["plain", "labels"])
@pytest.mark.parametrize("k", [1, 50, 128])
@pytest.mark.parametrize("split", list(SPLITS))
@pytest.mark.parametrize("D", [36, 33])
def test_search_blocks_equals_search(gpu, D, split, k, labels):
    (qf, gf, qp, gp, qc, gc), want = _case(D, k, labels)
    if k > 1:  # the copies are in the lists: rows with equal neighbouring distances exist
        assert ((want[1][:, 1:] == want[1][:, :-1]) & np.isfinite(want[1][:, 1:])).any()
    got = _ev().search_blocks(qf, _blocks(gf, gp, gc, SPLITS[split], labels), k, *((qp, qc) if labels else ()))
    assert got[0].dtype == np.int32 and got[0].shape == (Q, k)
    _same(got, want)


@pytest.mark.parametrize("labels", [False, True], ids=["plain", "labels"])
def test_search_blocks_without_distances(gpu, labels):
    (qf, gf, qp, gp, qc, gc), want = _case(36, 50, labels)
    idx, dist = _ev().search_blocks(qf, _blocks(gf, gp, gc, SPLITS["ragged"], labels), 50,
                                    *((qp, qc) if labels else ()), with_dist=False)
    assert dist is None and np.array_equal(idx, want[0])


def test_block_of_removed_items_only(gpu):
    """A block made only of items with one query's pid and camera: its list for that query is all
    padding, and the joined row still equals the one-call search."""
    ev = _ev()
    (qf, gf, qp, gp, qc, gc), _ = _case(36, 50, True)
    q0 = 5
    gp, gc = gp.copy(), gc.copy()
    gp[300:310], gc[300:310] = qp[q0], qc[q0]
    idx, _ = ev.search(qf, gf[300:310], 10, qp, qc, gp[300:310], gc[300:310])
    assert (idx[q0] == -1).all() and (idx[qp != qp[q0]] >= 0).all()
    want = ev.search(qf, gf, 50, qp, qc, gp, gc)
    _same(ev.search_blocks(qf, _blocks(gf, gp, gc, (300, 10, 690), True), 50, qp, qc), want)


@pytest.mark.parametrize("labels", [False, True], ids=["plain", "labels"])
def test_host_resident_blocks(gpu, labels):
    (qf, gf, qp, gp, qc, gc), want = _case(33, 50, labels)
    blocks = _blocks(gf, gp, gc, SPLITS["ragged"], labels, host=True)
    _same(_ev().search_blocks(qf, blocks, 50, *((qp, qc) if labels else ())), want)
    # numpy blocks as well
    blocks = [gf[:600], gf[600:]]
    _same(_ev().search_blocks(qf, blocks, 50), _case(33, 50, False)[1])


def test_accumulator_device_result_and_refusals(gpu):
    from multimodal_reid_amd._lib import ReidmiError
    ev = _ev()
    (qf, gf, qp, gp, qc, gc), want = _case(36, 50, False)
    acc = ev.SearchAccumulator(qf, 50)
    acc.add(gf[:49])
    with pytest.raises(ReidmiError, match="49 gallery items"):
        acc.result()  # fewer than k items so far
    acc.add(gf[49:49])  # an empty block is skipped
    acc.add(gf[49:])
    idx, dist = acc.result()
    assert idx.is_cuda and dist.is_cuda and acc.count == G
    _same((idx.cpu().numpy(), dist.cpu().numpy()), want)
    # labels on some blocks but not others, in both directions
    acc = ev.SearchAccumulator(qf, 50, qp, qc)
    acc.add(gf[:500], gp[:500], gc[:500])
    with pytest.raises(ReidmiError, match="labels"):
        acc.add(gf[500:])
    with pytest.raises(ReidmiError, match="label"):
        acc.add(gf[500:], gp[500:])
    acc = ev.SearchAccumulator(qf, 50)
    with pytest.raises(ReidmiError, match="labels"):
        acc.add(gf[:500], gp[:500], gc[:500])
    with pytest.raises(ReidmiError):
        ev.SearchAccumulator(qf, 129)
    with pytest.raises(ReidmiError, match="label"):
        ev.SearchAccumulator(qf, 50, qp)
