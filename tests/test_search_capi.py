"""Argument checks of reidmi_search_f32 through the C ABI: every refusal returns before any HIP
call (status REIDMI_EINVAL, a message, nothing launched), so these run without a GPU, on
pointers that are never dereferenced."""
import ctypes

import pytest

EINVAL = 1
Q, G, D = 300, 5000, 1280
PTR = ctypes.c_void_p(0x10000)  # non-null, 16-byte aligned, never touched


def _lib():
    from multimodal_reid_amd import _lib
    return _lib.load()


def _call(L, k, G=G, idx=PTR, dist=PTR, ws=PTR, ws_bytes=None, labels=(None,) * 4, ldo=None):
    if ws_bytes is None:
        ws_bytes = 1 << 40
    return L.reidmi_search_f32(PTR, Q, D, PTR, G, D, D, k, *labels, idx, dist, k if ldo is None else ldo, ws, ws_bytes,
                               None)


def test_search_workspace_has_no_q_by_g_term():
    L = _lib()
    for q, g, k in ((3368, 15913, 50), (11659, 82161, 50), (10000, 1000000, 10)):
        nb = L.reidmi_search_workspace_bytes(q, g, D, k)
        assert nb == L.reidmi_search_workspace_bytes(q, g, D, k)  # a pure function of the arguments
        # norms + at most 1024 (band, range) lists (or one per band) of 128 rows x 384 entries x 8 bytes
        bands = -(-q // 128)
        assert 4 * (q + g) <= nb <= 4 * (q + g) + 16 + max(1024, bands) * 128 * 384 * 8
    assert L.reidmi_search_workspace_bytes(10000, 1000000, D, 10) < 4 * 10000 * 1000000 // 100
    for bad in ((Q, G, D, 0), (Q, G, D, 129), (Q, 40, D, 41), (Q, 0, D, 1), (-1, G, D, 1), (Q, G, 0, 1)):
        assert L.reidmi_search_workspace_bytes(*bad) < 0, bad


# (Q, G, k) -> bytes, recorded from the library before the launch plan moved into distance.h
# (dm_walk_plan).  The value is the norms plus bands * S * 128 * cap * 8, so it pins S: no bands,
# one tile, ranges clamped by the tile count, both default capacities, more tiles than the 1024
# slots, more bands than slots.
WORKSPACE_BYTES = {
    (0, 100, 5): 400,
    (1, 1, 1): 262160,
    (1, 129, 10): 524816,
    (129, 300, 64): 1574592,
    (129, 129, 128): 1573904,
    (1000, 20000, 65): 248596512,
    (3368, 15913, 50): 226569552,
    (128, 131073, 10): 135004688,
    (200000, 5000, 10): 410551072,
}


def test_search_workspace_bytes_recorded_plan():
    L = _lib()
    got = {s: L.reidmi_search_workspace_bytes(s[0], s[1], D, s[2]) for s in WORKSPACE_BYTES}
    assert got == WORKSPACE_BYTES


@pytest.mark.parametrize("k,G_,what", [(0, G, b"1 <= k <= G"), (41, 40, b"1 <= k <= G"), (-3, G, b"1 <= k <= G")])
def test_search_refuses_k_out_of_range(k, G_, what):
    L = _lib()
    assert _call(L, k, G=G_, ldo=64) == EINVAL
    assert what in L.reidmi_last_error()


def test_search_refuses_k_above_128_and_names_the_route():
    L = _lib()
    assert _call(L, 129) == EINVAL
    msg = L.reidmi_last_error()
    assert b"reidmi_distmat_f32" in msg and b"reidmi_topk_rows_f32" in msg
    assert _call(L, 128, ws_bytes=0) == EINVAL and b"workspace" in L.reidmi_last_error()  # 128 itself is in range


def test_search_refuses_short_workspace():
    L = _lib()
    nb = L.reidmi_search_workspace_bytes(Q, G, D, 10)
    assert nb > 0
    assert _call(L, 10, ws_bytes=nb - 1) == EINVAL
    assert b"workspace" in L.reidmi_last_error()
    assert _call(L, 10, ws=None, ws_bytes=nb) == EINVAL
    assert _call(L, 10, ws=ctypes.c_void_p(0x10004), ws_bytes=nb) == EINVAL  # not 16-byte aligned


def test_search_refuses_null_outputs():
    L = _lib()
    assert _call(L, 10, idx=None) == EINVAL
    assert b"out_idx" in L.reidmi_last_error()
    assert _call(L, 10, ldo=9) == EINVAL  # rows of k entries do not fit the pitch


def test_search_refuses_partial_labels():
    L = _lib()
    for n in (1, 2, 3):
        assert _call(L, 10, labels=(PTR,) * n + (None,) * (4 - n)) == EINVAL
        assert b"label" in L.reidmi_last_error()


def test_search_ex_refuses_bad_splits_and_capacity():
    from multimodal_reid_amd import _lib
    T = _lib.load_tools()
    for splits, cap in ((-1, 0), (4097, 0), (0, 10 + 127), (0, 513)):
        assert T.reidmi_search_ex_workspace_bytes(Q, G, D, 10, splits, cap) < 0
        assert T.reidmi_search_f32_ex(PTR, Q, D, PTR, G, D, D, 10, None, None, None, None, PTR, PTR, 10, PTR, 1 << 40,
                                      splits, cap, None, None) == EINVAL
    assert T.reidmi_search_ex_workspace_bytes(Q, G, D, 10, 7, 138) == \
        (4 * (Q + G) + 15) // 16 * 16 + 3 * 7 * 128 * 138 * 8
