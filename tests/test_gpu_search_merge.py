"""reidmi_search_merge_f32 against a numpy restatement: the present entries of a row's S lists
concatenated, their indices moved by the lists' bases, ordered by np.lexsort((global index,
distance)), the first k kept, the rest -1 / +inf.  Index values and distance bits are compared.

Every case draws its distances from 8 values, so equal distances occur within a list and across
lists and only the global index orders them; row 0 has one list that is all padding, row 1 (and
the last row) fewer than k present entries in total, the other rows lists that are full or
partly padding.  Each case is run with the lists in ascending, descending and shuffled order of
their bases (the result must be the same), without out_dist, and in a padded layout (ldi > k_in,
ldo > k, list_stride > Q * ldi) whose gaps hold a sentinel that sorts first if it is ever read."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

VALUES = np.float32([0.0, 0.25, 0.5, 0.75, 1.0, 1.5, 2.0, 3.5])
SENT_I, SENT_D = 7777777, -5.0  # in the gaps of the inputs
KEEP_I, KEEP_D = -777, -9.0  # in the gaps of the outputs
SHAPES = [(1, 1), (50, 50), (128, 128), (10, 50), (128, 10)]


def _lists(S, Q, k_in, k, seed):
    """(idx int32 [S][Q][k_in], dist fp32 [S][Q][k_in], base int64 [S]): rows sorted by (distance,
    index) and ended by padding, as reidmi_search_f32 writes them over blocks of B[s] items."""
    r = np.random.default_rng(seed)
    B = r.integers(k_in, k_in + 40, S)
    base = np.concatenate([[0], np.cumsum(B)[:-1]]).astype(np.int64)
    idx = np.full((S, Q, k_in), -1, np.int32)
    dist = np.full((S, Q, k_in), np.inf, np.float32)
    for s in range(S):
        n = np.where(r.random(Q) < 0.5, k_in, r.integers(0, k_in + 1, Q))  # full, or partly padding
        few = r.integers(0, min(k_in, (k - 1) // S) + 1, 2)
        n[min(1, Q - 1)], n[Q - 1] = few  # fewer than k present entries in the whole row
        n[0] = 0 if s == 0 else n[0]  # row 0: list 0 is all padding
        loc = r.random((Q, B[s])).argsort(1)[:, :k_in]  # distinct per row
        code = r.integers(0, len(VALUES), (Q, k_in))
        order = (code * int(B[s]) + loc).argsort(1)
        loc, code = np.take_along_axis(loc, order, 1), np.take_along_axis(code, order, 1)
        present = np.arange(k_in)[None, :] < n[:, None]
        idx[s] = np.where(present, loc, -1)
        dist[s] = np.where(present, VALUES[code], np.inf)
    return idx, dist, base


def _reference(idx, dist, base, k):
    S, Q, _ = idx.shape
    oi = np.full((Q, k), -1, np.int32)
    od = np.full((Q, k), np.inf, np.float32)
    for i in range(Q):
        keep = idx[:, i] >= 0
        gi = (idx[:, i] + base[:, None])[keep]
        d = dist[:, i][keep]
        o = np.lexsort((gi, d))[:k]
        oi[i, :len(o)], od[i, :len(o)] = gi[o], d[o]
    return oi, od


def _merge(gpu, idx, dist, base, k, with_dist=True, pad=False):
    """The C call on device copies; pad: every pitch larger than it must be, the gaps filled."""
    from multimodal_reid_amd import _lib
    S, Q, k_in = idx.shape
    ldi, ldo = (k_in + 3, k + 5) if pad else (k_in, k)
    stride = Q * ldi + (7 if pad else 0)
    bi = np.full(S * stride, SENT_I, np.int32)
    bd = np.full(S * stride, SENT_D, np.float32)
    for s in range(S):
        bi[s * stride:s * stride + Q * ldi].reshape(Q, ldi)[:, :k_in] = idx[s]
        bd[s * stride:s * stride + Q * ldi].reshape(Q, ldi)[:, :k_in] = dist[s]
    ti, td = torch.from_numpy(bi).to(gpu), torch.from_numpy(bd).to(gpu)
    tb = torch.from_numpy(np.array(base, np.int64)).to(gpu) if base is not None else None
    oi = torch.full((Q, ldo), KEEP_I, dtype=torch.int32, device=gpu)
    od = torch.full((Q, ldo), KEEP_D, dtype=torch.float32, device=gpu) if with_dist else None
    _lib.call("reidmi_search_merge_f32", _lib.ptr(ti), _lib.ptr(td), S, Q, k_in, stride, ldi, _lib.ptr(tb), k,
              _lib.ptr(oi), _lib.ptr(od), ldo, _lib.stream())
    torch.cuda.synchronize()
    oi = oi.cpu().numpy()
    od = od.cpu().numpy() if with_dist else None
    assert (oi[:, k:] == KEEP_I).all() and (od is None or (od[:, k:] == KEEP_D).all()), "wrote beyond k"
    return oi[:, :k], (od[:, :k] if with_dist else None)


def _same(got, want):
    gi, gd = got
    wi, wd = want
    assert np.array_equal(gi, wi)
    assert gd is None or np.array_equal(gd.view(np.uint32), wd.view(np.uint32))


@pytest.mark.parametrize("k_in,k", SHAPES)
@pytest.mark.parametrize("Q", [1, 130])
@pytest.mark.parametrize("S", [1, 2, 3, 9])
def test_merge_equals_lexsort(gpu, S, Q, k_in, k):
    idx, dist, base = _lists(S, Q, k_in, k, seed=1000 * S + Q + k_in + k)
    want = _reference(idx, dist, base, k)
    assert (want[0][min(1, Q - 1)] < 0).any() and (want[0][Q - 1] < 0).any()  # the short rows are short
    assert not (idx[0, 0] >= 0).any()  # the all-padding list
    _same(_merge(gpu, idx, dist, base, k), want)
    # the lists in descending and in shuffled order of their bases: the same result
    for order in (np.arange(S)[::-1], np.random.default_rng(S).permutation(S)):
        _same(_merge(gpu, idx[order], dist[order], np.ascontiguousarray(base[order]), k), want)
    _same(_merge(gpu, idx, dist, base, k, with_dist=False), want)
    got = _merge(gpu, idx[::-1], dist[::-1], np.ascontiguousarray(base[::-1]), k, pad=True)
    assert not (got[0] == SENT_I).any() and not (got[1] == SENT_D).any()
    _same(got, want)


def test_merge_null_base_is_all_zero(gpu):
    """base = NULL: the lists' indices are global already (here: disjoint by construction)."""
    idx, dist, base = _lists(3, 130, 50, 50, seed=5)
    shifted = np.where(idx >= 0, idx + base[:, None, None].astype(np.int32), -1).astype(np.int32)
    _same(_merge(gpu, shifted, dist, None, 50), _reference(idx, dist, base, 50))


def test_merge_of_equal_distances_goes_by_global_index(gpu):
    """Every distance equal: the output is the k smallest global indices, whichever list they are in."""
    S, Q, k_in, k = 3, 2, 10, 25
    idx = np.tile(np.arange(k_in, dtype=np.int32), (S, Q, 1))
    dist = np.full((S, Q, k_in), 0.5, np.float32)
    base = np.int64([20, 0, 10])
    oi, od = _merge(gpu, idx, dist, base, k)
    assert np.array_equal(oi, np.tile(np.arange(k, dtype=np.int32), (Q, 1))) and (od == 0.5).all()
