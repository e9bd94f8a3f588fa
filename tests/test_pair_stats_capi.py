"""Argument checks of reidmi_pair_stats_f32 through the C ABI: every refusal returns before any HIP
call (status REIDMI_EINVAL, a message, nothing launched), so these run without a GPU, on device
pointers that are never dereferenced.  The edges are a host array, so their checks run here on real
values.  The workspace is a pure function, linear in Q and independent of G beyond the norms."""
import ctypes

import numpy as np
import pytest

EINVAL = 1
Q, G, D = 200, 300, 36
PTR = ctypes.c_void_p(0x10000)  # non-null, 16-byte aligned, never touched
ODD = ctypes.c_void_p(0x10004)
BIG = 1 << 40
OUT_NAMES = b"hist_pos, hist_neg, near_pos_dist, near_pos_idx, near_neg_dist and near_neg_idx"


def _lib():
    from multimodal_reid_amd import _lib
    return _lib.load()


def _call(L, q=PTR, Q=Q, ldq=None, g=PTR, G=G, ldg=None, D=D, labels=(PTR,) * 4, edges=(0.5, 1.0), n_edges=None,
          index_base=0, self_base=-1, outs=(PTR,) * 6, ws=PTR, ws_bytes=BIG):
    """labels = q_pids, q_cams, g_pids, g_cams; outs = hist_pos, hist_neg, near_pos_dist, near_pos_idx,
    near_neg_dist, near_neg_idx.  edges: a sequence (a host fp32 array is made of it) or None."""
    e = None if edges is None else np.ascontiguousarray(edges, dtype=np.float32)
    ep = None if e is None else ctypes.c_void_p(e.ctypes.data)
    n = (0 if e is None else e.size) if n_edges is None else n_edges
    return L.reidmi_pair_stats_f32(q, Q, D if ldq is None else ldq, g, G, D if ldg is None else ldg, D, *labels, ep, n,
                                   index_base, self_base, *outs, ws, ws_bytes, None)


def _refused(rc, L, what):
    assert rc == EINVAL
    assert what in L.reidmi_last_error(), L.reidmi_last_error()


def test_exports_and_abi_version():
    from multimodal_reid_amd import _lib as binding
    L = _lib()
    d = binding.declarations()
    vp, i32, i64 = ctypes.c_void_p, ctypes.c_int, ctypes.c_int64
    assert d["reidmi_pair_stats_workspace_bytes"] == (i64, [i64, i64])
    assert d["reidmi_pair_stats_f32"] == (i32, [vp, i64, i64, vp, i64, i64, i64, vp, vp, vp, vp, vp, i32, i64, i64,
                                                vp, vp, vp, vp, vp, vp, vp, i64, vp])
    assert L.reidmi_pair_stats_f32 is not None and L.reidmi_pair_stats_workspace_bytes is not None
    assert L.reidmi_abi_version() >= 12


@pytest.mark.parametrize("q", [1000, 1000000])
def test_workspace_is_linear_in_q_and_holds_no_matrix(q):
    L = _lib()
    for g in (1, 5000, 1000000):
        one, two = L.reidmi_pair_stats_workspace_bytes(q, g), L.reidmi_pair_stats_workspace_bytes(2 * q, g)
        assert one > 0 and one == L.reidmi_pair_stats_workspace_bytes(q, g)
        assert two <= 2 * one + 64
        assert one <= 20 * q + 4 * g + 64  # the norms and two 8-byte keys per query: nothing Q x G
    # beyond the norms (4 bytes a row) the gallery size does not enter
    a, b = L.reidmi_pair_stats_workspace_bytes(q, 1000), L.reidmi_pair_stats_workspace_bytes(q, 2001000)
    assert b - a == 4 * 2000000
    assert L.reidmi_pair_stats_workspace_bytes(0, 5) >= 0
    for bad in ((-1, G), (Q, 0), (Q, -1), (1 << 31, G), (Q, 1 << 31)):
        assert L.reidmi_pair_stats_workspace_bytes(*bad) < 0, bad


def test_refuses_bad_shapes_and_pitches():
    L = _lib()
    for kw in (dict(Q=-1), dict(G=0), dict(G=-1), dict(D=0), dict(D=-2), dict(Q=1 << 31), dict(G=1 << 31)):
        _refused(_call(L, **kw), L, b"bad shape")
    _refused(_call(L, ldq=D - 1), L, b"pitches")
    _refused(_call(L, ldg=D - 1), L, b"pitches")
    # the largest shapes the check admits: only the workspace is left to refuse
    _refused(_call(L, Q=(1 << 31) - 1, G=(1 << 31) - 1, ws_bytes=1 << 20), L, b"workspace")


def test_refuses_bad_edges():
    L = _lib()
    for n in (0, -1, 256, 1000):
        _refused(_call(L, n_edges=n), L, b"n_edges")
    _refused(_call(L, edges=None, n_edges=2), L, b"edges")
    for bad in ((float("nan"),), (0.5, float("inf")), (float("-inf"), 1.0), (0.1, float("nan"), 0.3)):
        _refused(_call(L, edges=bad), L, b"finite")
    for bad in ((1.0, 0.5), (0.0, 0.5, 0.5, 0.25), tuple(np.linspace(4.0, 0.0, 255))):
        _refused(_call(L, edges=bad), L, b"non-decreasing")
    # accepted: equal neighbours, negative values, -0.0 next to +0.0, the full 255; the next check
    # (here the missing pids) is what then refuses
    for ok in ((0.5, 0.5), (-1.0, -0.0, 0.0, 2.0), (3.0,), tuple(np.linspace(0.0, 4.0, 255))):
        _refused(_call(L, edges=ok, labels=(None, PTR, PTR, PTR)), L, b"q_pids and g_pids")


def test_refuses_bad_labels_bases_and_pointers():
    L = _lib()
    _refused(_call(L, labels=(None, PTR, PTR, PTR)), L, b"q_pids and g_pids")
    _refused(_call(L, labels=(PTR, PTR, None, PTR)), L, b"q_pids and g_pids")
    _refused(_call(L, labels=(PTR, None, PTR, PTR)), L, b"both camera arrays or neither")
    _refused(_call(L, labels=(PTR, PTR, PTR, None)), L, b"both camera arrays or neither")
    _refused(_call(L, index_base=-1), L, b"index_base")
    _refused(_call(L, index_base=(1 << 31) - G), L, b"index_base")
    _refused(_call(L, self_base=-2), L, b"self_base")
    for n in range(6):
        _refused(_call(L, outs=(PTR,) * n + (None,) + (PTR,) * (5 - n)), L, OUT_NAMES)
    nb = L.reidmi_pair_stats_workspace_bytes(Q, G)
    _refused(_call(L, ws_bytes=nb - 1), L, b"workspace")
    _refused(_call(L, ws=None, ws_bytes=nb), L, b"workspace")
    _refused(_call(L, ws=ODD, ws_bytes=nb), L, b"workspace")
    _refused(_call(L, q=None), L, b"features")
    _refused(_call(L, g=None), L, b"features")
    # the last admitted base: index_base + G == 2^31 - 1; without cameras; then only the workspace refuses
    _refused(_call(L, index_base=(1 << 31) - 1 - G, labels=(PTR, None, PTR, None), self_base=7, ws_bytes=nb - 1), L,
             b"workspace")


def test_python_layer_checks_before_the_gpu():
    """The argument errors of the Python layer that need no device."""
    from multimodal_reid_amd import _lib as binding, evaluate as ev
    for bad in ([], np.zeros(256), [0.0, float("nan")], [1.0, 0.5], "x"):
        with pytest.raises(binding.ReidmiError):
            ev._edges("pair_stats", bad)
    e = ev.default_edges()
    assert e.dtype == np.float32 and e.size == 255 and e[-1] == 4.0 and (np.diff(e) > 0).all()
    assert np.array_equal(ev._edges("pair_stats", None), e)
    for kw in (dict(sharded=True), dict(reranking=True)):
        m = ev.R1_mAP_eval(4, **kw)
        m.reset()
        with pytest.raises(binding.ReidmiError):
            m.pair_stats()
