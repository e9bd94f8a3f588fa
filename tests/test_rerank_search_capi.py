"""Argument checks of reidmi_rr_jaccard_topk_rows (the re-ranked rank lists) through the C ABI:
every refusal returns before any HIP call (status REIDMI_EINVAL, a named message, nothing
launched), so these run without a GPU, on pointers that are never dereferenced."""
import ctypes
import os
import re

import pytest

from conftest import REPO

EINVAL = 1
Q, G, D = 300, 20000, 1280
N = Q + G
PTR = ctypes.c_void_p(0x10000)  # non-null, 16-byte aligned, never touched
BIG = 1 << 40
NAMES = ("reidmi_rr_jaccard_topk_rows", "reidmi_rr_jaccard_topk_workspace_bytes")


def _lib():
    from multimodal_reid_amd import _lib
    return _lib.load()


def _call(L, k, Q_=Q, N_=N, labels=(None,) * 4, idx=PTR, dist=PTR, ldo=None, chunk_rows=64, ws=PTR, ws_bytes=BIG,
          bounds=PTR, bounds_bytes=BIG):
    return L.reidmi_rr_jaccard_topk_rows(PTR, N_, D, D, PTR, PTR, Q_, 0, Q_, PTR, PTR, PTR, PTR, PTR, PTR, 0x3999, 0.3,
                                         k, *labels, idx, dist, max(k, 1) if ldo is None else ldo, PTR, chunk_rows,
                                         bounds, bounds_bytes, ws, ws_bytes, None)


def test_symbols_in_header_library_and_table():
    from multimodal_reid_amd import _lib
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(REPO, "include", "reidmi.h")).read(), flags=re.S)
    L = _lib.load()
    for name in NAMES:
        assert re.search(r"\b%s\s*\(" % name, txt), name
        assert name in _lib.declarations() and hasattr(L, name), name
    # reidmi_rr_jaccard_rows' 24, minus out, plus k, labels, lists, ws
    assert len(getattr(L, NAMES[0]).argtypes) == 32
    assert L.reidmi_abi_version() >= 5


def test_workspace_is_one_pass_of_partial_lists():
    L = _lib()
    wb = L.reidmi_rr_jaccard_topk_workspace_bytes
    assert wb(64, G, 50) == 64 * 3 * 50 * 8           # ceil(20000 / 8192) = 3 chunks
    assert wb(1, 8192, 128) == 128 * 8 and wb(1, 8193, 128) == 2 * 128 * 8
    assert wb(65535, 1000000, 128) == 65535 * 123 * 128 * 8  # rows per pass, never Q x G
    for bad in ((0, G, 10), (65536, G, 10), (64, 0, 1), (64, G, 0), (64, G, 129), (64, 40, 41), (-1, G, 10),
                (64, -5, 1), (64, 1 << 31, 10)):
        assert wb(*bad) == -1, bad


@pytest.mark.parametrize("k,N_", [(0, N), (-3, N), (41, Q + 40)])
def test_refuses_k_out_of_range(k, N_):
    L = _lib()
    assert _call(L, k, N_=N_, ldo=64) == EINVAL
    assert b"rr_jaccard_topk_rows" in L.reidmi_last_error() and b"1 <= k <= G" in L.reidmi_last_error()


def test_refuses_k_above_128_and_names_the_route():
    L = _lib()
    assert _call(L, 129) == EINVAL
    msg = L.reidmi_last_error()
    assert b"k > 128" in msg and b"reidmi_rr_jaccard_rows" in msg and b"reidmi_topk_rows_f32" in msg
    assert _call(L, 128, ws_bytes=0) == EINVAL and b"workspace" in L.reidmi_last_error()  # 128 itself is in range


def test_refuses_partial_labels():
    L = _lib()
    for n in (1, 2, 3):
        assert _call(L, 10, labels=(PTR,) * n + (None,) * (4 - n)) == EINVAL
        assert b"label" in L.reidmi_last_error()
        assert _call(L, 10, labels=(None,) * (4 - n) + (PTR,) * n) == EINVAL
        assert b"label" in L.reidmi_last_error()


def test_refuses_null_out_idx_and_short_pitch():
    L = _lib()
    assert _call(L, 10, idx=None) == EINVAL
    assert b"out_idx" in L.reidmi_last_error()
    assert _call(L, 10, ldo=9) == EINVAL and b"ldo" in L.reidmi_last_error()


def test_refuses_short_or_misaligned_workspace():
    L = _lib()
    nb = L.reidmi_rr_jaccard_topk_workspace_bytes(64, G, 10)
    assert nb > 0
    for kw in (dict(ws_bytes=nb - 1), dict(ws=None, ws_bytes=nb), dict(ws=ctypes.c_void_p(0x10004), ws_bytes=nb)):
        assert _call(L, 10, **kw) == EINVAL
        assert b"workspace" in L.reidmi_last_error() and b"reidmi_rr_jaccard_topk_workspace_bytes" in \
            L.reidmi_last_error()
    # the size follows chunk_rows, not the row range: 64 rows per pass need 64 rows of lists
    assert _call(L, 10, chunk_rows=65, ws_bytes=nb) == EINVAL and b"workspace" in L.reidmi_last_error()


@pytest.mark.parametrize("chunk_rows", [0, -1, 65536])
def test_refuses_chunk_rows_out_of_range(chunk_rows):
    L = _lib()
    assert _call(L, 10, chunk_rows=chunk_rows) == EINVAL
    assert b"chunk_rows" in L.reidmi_last_error()


def test_refuses_short_bounds_scratch():
    L = _lib()
    bb = L.reidmi_rr_jaccard_bounds_bytes(N, G)
    assert _call(L, 10, bounds_bytes=bb - 1) == EINVAL and b"bounds" in L.reidmi_last_error()
    assert _call(L, 10, bounds=None) == EINVAL and b"bounds" in L.reidmi_last_error()


def test_python_surface_names_what_it_refuses():
    """The refusals of the Python entry points that need no GPU: they come before any device work."""
    import numpy as np
    from multimodal_reid_amd import _lib, reranking
    f = np.zeros((4, 8), np.float32)
    with pytest.raises(_lib.ReidmiError, match="only_local / local_distmat"):
        reranking.re_ranking_search_device(f, f, 2, 20, 6, 0.3, local_distmat=np.zeros((8, 8), np.float32))
    with pytest.raises(_lib.ReidmiError, match="only_local / local_distmat"):
        reranking.re_ranking_search_device(f, f, 2, 20, 6, 0.3, only_local=True)
    with pytest.raises(_lib.ReidmiError, match="all four label arrays"):
        reranking.re_ranking_search_device(f, f, 2, 20, 6, 0.3, q_pids=np.zeros(4, np.int64))
    with pytest.raises(_lib.ReidmiError, match=r"1 <= k <= min\(G, 128\)"):
        reranking.check_topk(500, 129)
    with pytest.raises(_lib.ReidmiError, match=r"1 <= k <= min\(G, 128\)"):
        reranking.check_topk(40, 41)
    reranking.check_topk(500, 128)
