"""Argument checks of reidmi_dbscan_jaccard and reidmi_rr_jaccard_self_rows through the C ABI: every
refusal returns before any HIP call (status REIDMI_EINVAL, a message, nothing launched), so these
run without a GPU, on pointers that are never dereferenced; and the workspace is a pure function:
the O(N) arrays plus N * (ceil(N / 8192) + 1) * 8 bytes of chunk bounds."""
import ctypes

import numpy as np
import pytest

EINVAL = 1
N = 300
PTR = ctypes.c_void_p(0x10000)  # non-null, 16-byte aligned, never touched
ODD = ctypes.c_void_p(0x10004)
BIG = 1 << 40
JCH = 8192


def _lib():
    from multimodal_reid_amd import _lib
    return _lib.load()


def _call(L, N=N, sparse=(PTR,) * 6, eps=0.6, min_samples=4, outs=(PTR,) * 4, ws=PTR, ws_bytes=BIG):
    """sparse = qoff, qcol, qval, coff, irow, ival; outs = labels, counts, core, n_clusters."""
    return L.reidmi_dbscan_jaccard(N, *sparse, eps, min_samples, *outs, ws, ws_bytes, None)


def _rows(L, N=N, lo=0, hi=N, sparse=(PTR,) * 6, out=PTR, ldo=None, bounds=PTR, bounds_bytes=BIG):
    return L.reidmi_rr_jaccard_self_rows(N, lo, hi, *sparse, out, N if ldo is None else ldo, bounds, bounds_bytes,
                                         None)


def _refused(rc, L, what):
    assert rc == EINVAL
    assert what in L.reidmi_last_error(), L.reidmi_last_error()


def test_exports_and_abi_version():
    from multimodal_reid_amd import _lib as binding
    L = _lib()
    d = binding.declarations()
    vp, i32, i64 = ctypes.c_void_p, ctypes.c_int, ctypes.c_int64
    assert d["reidmi_dbscan_jaccard_workspace_bytes"] == (i64, [i64])
    assert d["reidmi_dbscan_jaccard"] == (i32, [i64] + [vp] * 6 + [ctypes.c_float, i32] + [vp] * 5 + [i64, vp])
    assert d["reidmi_rr_jaccard_self_rows"] == (i32, [i64, i64, i64] + [vp] * 7 + [i64, vp, i64, vp])
    for name in ("reidmi_dbscan_jaccard", "reidmi_dbscan_jaccard_workspace_bytes", "reidmi_rr_jaccard_self_rows"):
        assert getattr(L, name).argtypes == d[name][1]
    assert L.reidmi_abi_version() >= 11


@pytest.mark.parametrize("n", [1, 300, JCH, JCH + 1, 100000, 1000000])
def test_workspace_is_the_linear_arrays_plus_the_chunk_bounds(n):
    L = _lib()
    bounds = n * (-(-n // JCH) + 1) * 8
    assert bounds == L.reidmi_rr_jaccard_bounds_bytes(n, n)
    got = L.reidmi_dbscan_jaccard_workspace_bytes(n)
    assert got == L.reidmi_dbscan_jaccard_workspace_bytes(n) and got % 8 == 0
    assert bounds + 12 * n <= got <= bounds + 13 * n + 64  # parent, border roots, numbers, block sums
    for bad in (0, -1, 1 << 31, 1 << 40):
        assert L.reidmi_dbscan_jaccard_workspace_bytes(bad) < 0, bad


def test_the_documented_sizes():
    L = _lib()
    assert 11e6 < L.reidmi_dbscan_jaccard_workspace_bytes(100000) - 12 * 100000 < 12e6
    assert 0.95e9 < L.reidmi_dbscan_jaccard_workspace_bytes(1000000) < 1.05e9


def test_refuses_bad_shapes():
    L = _lib()
    for n in (0, -1, 1 << 31):
        _refused(_call(L, N=n), L, b"bad shape")
    # the largest N the shape check admits: only the workspace is left to refuse
    _refused(_call(L, N=(1 << 31) - 1), L, b"workspace")


def test_refuses_bad_eps_and_min_samples():
    L = _lib()
    for eps in (-1e-30, -1.0, float("inf"), float("-inf"), float("nan")):
        _refused(_call(L, eps=eps), L, b"eps")
    # eps is compared in fp16: 0.9998 is the last value that rounds below 1
    assert float(np.float16(0.9997)) < 1 and float(np.float16(0.9998)) == 1
    for eps in (0.9998, 1.0, 1.5, 70000.0, 3e38):
        _refused(_call(L, eps=eps), L, b"less than 1 in fp16")
    for m in (0, -1):
        _refused(_call(L, min_samples=m), L, b"min_samples")
    # what is left passes the argument checks up to the workspace
    for eps in (0.0, 0.6, 0.9997):
        _refused(_call(L, eps=eps, ws_bytes=0), L, b"workspace")


def test_refuses_null_pointers_and_short_workspace():
    L = _lib()
    for n in range(6):
        _refused(_call(L, sparse=(PTR,) * n + (None,) + (PTR,) * (5 - n)), L, b"V_qe rows and their inverted index")
    for n in range(4):
        _refused(_call(L, outs=(PTR,) * n + (None,) + (PTR,) * (3 - n)), L, b"labels, counts, core and n_clusters")
    nb = L.reidmi_dbscan_jaccard_workspace_bytes(N)
    _refused(_call(L, ws_bytes=nb - 1), L, b"workspace")
    _refused(_call(L, ws=None, ws_bytes=nb), L, b"workspace")
    _refused(_call(L, ws=ODD, ws_bytes=nb), L, b"workspace")


def test_self_rows_refusals():
    L = _lib()
    for kw in (dict(N=0), dict(N=1 << 31), dict(lo=-1), dict(lo=5, hi=4), dict(hi=N + 1), dict(ldo=N - 1)):
        _refused(_rows(L, **kw), L, b"bad shape or row range")
    for n in range(6):
        _refused(_rows(L, sparse=(PTR,) * n + (None,) + (PTR,) * (5 - n)), L, b"inputs and out required")
    _refused(_rows(L, out=None), L, b"inputs and out required")
    nb = L.reidmi_rr_jaccard_bounds_bytes(N, N)
    _refused(_rows(L, bounds_bytes=nb - 1), L, b"bounds")
    _refused(_rows(L, bounds=None, bounds_bytes=nb), L, b"bounds")
    _refused(_rows(L, bounds=ODD, bounds_bytes=nb), L, b"bounds")
    assert _rows(L, lo=7, hi=7) == 0  # an empty row range: nothing to do, nothing launched
