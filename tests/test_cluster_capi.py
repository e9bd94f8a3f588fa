"""Argument checks of reidmi_dbscan_f32 through the C ABI: every refusal returns before any HIP call
(status REIDMI_EINVAL, a message, nothing launched), so these run without a GPU, on pointers that
are never dereferenced; and the workspace is a pure function that grows linearly in N."""
import ctypes

import pytest

EINVAL = 1
N, D = 300, 36
PTR = ctypes.c_void_p(0x10000)  # non-null, 16-byte aligned, never touched
ODD = ctypes.c_void_p(0x10004)
BIG = 1 << 40


def _lib():
    from multimodal_reid_amd import _lib
    return _lib.load()


def _call(L, x=PTR, N=N, D=D, ldx=None, eps=0.5, min_samples=4, outs=(PTR,) * 4, ws=PTR, ws_bytes=BIG):
    """outs = labels, counts, core, n_clusters."""
    return L.reidmi_dbscan_f32(x, N, D, D if ldx is None else ldx, eps, min_samples, *outs, ws, ws_bytes, None)


def _refused(rc, L, what):
    assert rc == EINVAL
    assert what in L.reidmi_last_error(), L.reidmi_last_error()


def test_exports_and_abi_version():
    from multimodal_reid_amd import _lib as binding
    L = _lib()
    d = binding.declarations()
    vp, i32, i64 = ctypes.c_void_p, ctypes.c_int, ctypes.c_int64
    assert d["reidmi_dbscan_workspace_bytes"] == (i64, [i64, i64])
    assert d["reidmi_dbscan_f32"] == (i32, [vp, i64, i64, i64, ctypes.c_float, i32, vp, vp, vp, vp, vp, i64, vp])
    assert L.reidmi_dbscan_f32 is not None and L.reidmi_dbscan_workspace_bytes is not None
    assert L.reidmi_abi_version() >= 10


@pytest.mark.parametrize("n", [1000, 1000000])
def test_workspace_is_linear_in_n(n):
    L = _lib()
    for d in (36, 1792):
        one, two = L.reidmi_dbscan_workspace_bytes(n, d), L.reidmi_dbscan_workspace_bytes(2 * n, d)
        assert one > 0 and one == L.reidmi_dbscan_workspace_bytes(n, d)
        assert two <= 2 * one + 4096
        assert one <= 20 * n + 4096  # norms, parent, border roots, numbers, block sums: nothing N x N
    for bad in ((0, D), (-1, D), (1 << 31, D), (N, 0), (N, -3)):
        assert L.reidmi_dbscan_workspace_bytes(*bad) < 0, bad


def test_refuses_bad_shapes_and_pitch():
    L = _lib()
    for kw in (dict(N=0), dict(N=-1), dict(N=1 << 31), dict(D=0), dict(D=-2)):
        _refused(_call(L, **kw), L, b"bad shape")
    _refused(_call(L, ldx=D - 1), L, b"pitch")
    # the largest N the shape check admits: only the workspace is left to refuse
    _refused(_call(L, N=(1 << 31) - 1, ws_bytes=1 << 20), L, b"workspace")


def test_refuses_bad_eps_and_min_samples():
    L = _lib()
    for eps in (-1e-30, -1.0, float("inf"), float("-inf"), float("nan")):
        _refused(_call(L, eps=eps), L, b"eps")
    for m in (0, -1):
        _refused(_call(L, min_samples=m), L, b"min_samples")


def test_refuses_null_pointers_and_short_workspace():
    L = _lib()
    _refused(_call(L, x=None), L, b"features")
    for n in range(4):
        _refused(_call(L, outs=(PTR,) * n + (None,) + (PTR,) * (3 - n)), L, b"labels, counts, core and n_clusters")
    nb = L.reidmi_dbscan_workspace_bytes(N, D)
    _refused(_call(L, ws_bytes=nb - 1), L, b"workspace")
    _refused(_call(L, ws=None, ws_bytes=nb), L, b"workspace")
    _refused(_call(L, ws=ODD, ws_bytes=nb), L, b"workspace")
