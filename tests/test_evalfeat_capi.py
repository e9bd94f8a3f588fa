"""Argument checks of the matrix-free scoring (reidmi_eval_feat_f32 and the reidmi_evf_* stages)
through the C ABI: every refusal returns before any HIP call (status REIDMI_EINVAL, a message,
nothing launched), so these run without a GPU, on pointers that are never dereferenced."""
import ctypes

import pytest

EINVAL = 1
Q, G, D, CAP = 300, 5000, 1280, 12
PTR = ctypes.c_void_p(0x10000)  # non-null, 16-byte aligned, never touched
ODD = ctypes.c_void_p(0x10004)  # not 16-byte (nor 8-byte) aligned
BIG = 1 << 40


def _lib():
    from multimodal_reid_amd import _lib
    return _lib.load()


def _one(L, Q=Q, G=G, D=D, ldq=None, ldg=None, q=PTR, g=PTR, labels=(PTR,) * 4, cap=CAP, outs=(PTR,) * 6,
         overflow=PTR, ws=PTR, ws_bytes=BIG):
    """reidmi_eval_feat_f32; outs = valid, first, last, npos, ap, nkept."""
    return L.reidmi_eval_feat_f32(q, Q, D if ldq is None else ldq, g, G, D if ldg is None else ldg, D, *labels, cap,
                                  *outs, overflow, ws, ws_bytes, None)


def _stage(L, name, Q=Q, G=G, D=D, ldq=None, ldg=None, q=PTR, g=PTR, labels=(PTR,) * 4, base=0, cap=CAP,
           state=None, ws=PTR, ws_bytes=BIG):
    """reidmi_evf_matches (state = pos, pos_cnt, junk_cnt, overflow) or reidmi_evf_count (state = pos,
    pos_cnt, hist)."""
    state = state or ((PTR,) * 4 if name == "matches" else (PTR,) * 3)
    return getattr(L, "reidmi_evf_" + name)(q, Q, D if ldq is None else ldq, g, G, D if ldg is None else ldg, D,
                                            *labels, base, cap, *state, ws, ws_bytes, None)


def _refused(rc, L, what):
    assert rc == EINVAL
    assert what in L.reidmi_last_error(), L.reidmi_last_error()


def test_abi_version_names_the_matrix_free_eval():
    assert _lib().reidmi_abi_version() >= 8


def test_workspace_is_a_pure_function_without_a_q_by_g_term():
    L = _lib()
    for q, g, d, cap in ((3368, 15913, 1280, 60), (11659, 82161, 1280, 100), (10000, 1000000, 1792, 64)):
        nb = L.reidmi_eval_feat_workspace_bytes(q, g, d, cap)
        assert nb == L.reidmi_eval_feat_workspace_bytes(q, g, d, cap)
        # norms + lists + histogram + counts, each rounded up to 16 bytes at the most
        need = 4 * (q + g) + q * cap * 8 + q * (cap + 1) * 4 + 8 * q
        assert need <= nb <= need + 64
    assert L.reidmi_eval_feat_workspace_bytes(10000, 1000000, 1792, 64) < 4 * 10000 * 1000000 // 100
    for bad in ((Q, G, D, 0), (Q, 0, D, CAP), (-1, G, D, CAP), (Q, G, 0, CAP), (Q, 1 << 31, D, CAP), (Q, G, D, -4)):
        assert L.reidmi_eval_feat_workspace_bytes(*bad) < 0, bad
    assert L.reidmi_evf_workspace_bytes(Q, G) == (4 * (Q + G) + 15) // 16 * 16
    assert L.reidmi_evf_workspace_bytes(Q, 0) < 0 and L.reidmi_evf_workspace_bytes(-1, G) < 0


def test_eval_feat_refuses_bad_shapes_capacity_and_pitches():
    L = _lib()
    for kw in (dict(G=0), dict(G=-5), dict(D=0), dict(Q=-1)):
        _refused(_one(L, **kw), L, b"bad shape")
    for cap in (0, -1):
        _refused(_one(L, cap=cap), L, b"cap >= 1")
    _refused(_one(L, ldq=D - 1), L, b"pitches")
    _refused(_one(L, ldg=D - 1), L, b"pitches")
    _refused(_one(L, G=1 << 31), L, b"2^31")


def test_eval_feat_refuses_missing_labels_and_null_pointers():
    L = _lib()
    for n in range(4):
        _refused(_one(L, labels=(PTR,) * n + (None,) + (PTR,) * (3 - n)), L, b"all four label arrays")
    _refused(_one(L, q=None), L, b"features")
    _refused(_one(L, g=None), L, b"features")
    for n in (0, 1, 4, 5):  # valid, first, ap, nkept; last (2) and npos (3) are nullable
        _refused(_one(L, outs=(PTR,) * n + (None,) + (PTR,) * (5 - n)), L, b"valid, first, ap, nkept")
    _refused(_one(L, overflow=None), L, b"overflow")
    nb = L.reidmi_eval_feat_workspace_bytes(Q, G, D, CAP)
    # with last and npos NULL only the workspace is left to refuse
    _refused(_one(L, outs=(PTR, PTR, None, None, PTR, PTR), ws_bytes=nb - 1), L, b"workspace")


def test_eval_feat_refuses_short_or_misaligned_workspace():
    L = _lib()
    nb = L.reidmi_eval_feat_workspace_bytes(Q, G, D, CAP)
    assert nb > 0
    _refused(_one(L, ws_bytes=nb - 1), L, b"workspace")
    _refused(_one(L, ws=None, ws_bytes=nb), L, b"workspace")
    _refused(_one(L, ws=ODD, ws_bytes=nb), L, b"workspace")


def test_eval_feat_with_no_query_is_a_no_op():
    assert _one(_lib(), Q=0) == 0  # nothing is launched: the pointers are never touched


@pytest.mark.parametrize("name", ["matches", "count"])
def test_block_stages_refuse(name):
    L = _lib()
    for kw in (dict(G=0), dict(D=0), dict(Q=-1)):
        _refused(_stage(L, name, **kw), L, b"bad shape")
    _refused(_stage(L, name, cap=0), L, b"cap >= 1")
    _refused(_stage(L, name, ldq=D - 1), L, b"pitches")
    _refused(_stage(L, name, ldg=D - 1), L, b"pitches")
    _refused(_stage(L, name, base=(1 << 31) - G), L, b"2^31")  # base + Gb == 2^31
    _refused(_stage(L, name, base=-1), L, b"2^31")
    for n in range(4):
        _refused(_stage(L, name, labels=(PTR,) * n + (None,) + (PTR,) * (3 - n)), L, b"all four label arrays")
    nb = L.reidmi_evf_workspace_bytes(Q, G)
    _refused(_stage(L, name, ws_bytes=nb - 1), L, b"workspace")
    _refused(_stage(L, name, ws=None), L, b"workspace")
    _refused(_stage(L, name, ws=ODD), L, b"workspace")
    ns = 4 if name == "matches" else 3
    for n in range(ns):
        _refused(_stage(L, name, state=(PTR,) * n + (None,) + (PTR,) * (ns - 1 - n)), L, b"required")
    _refused(_stage(L, name, state=(ODD,) + (PTR,) * (ns - 1)), L, b"8-byte aligned")
    _refused(_stage(L, name, q=None), L, b"features")
    assert _stage(L, name, Q=0) == 0
    assert _stage(L, name, base=(1 << 31) - G - 1, Q=0) == 0  # the last index is 2^31 - 1: in range


def test_append_sort_and_finish_refuse():
    L = _lib()
    _refused(L.reidmi_evf_append(PTR, PTR, PTR, PTR, Q, 0, PTR, None), L, b"cap >= 1")
    _refused(L.reidmi_evf_append(PTR, PTR, PTR, PTR, -1, CAP, PTR, None), L, b"bad Q")
    for n in range(5):
        a = [PTR] * 5
        a[n] = None
        _refused(L.reidmi_evf_append(a[0], a[1], a[2], a[3], Q, CAP, a[4], None), L, b"required")
    assert L.reidmi_evf_append(PTR, PTR, PTR, PTR, 0, CAP, PTR, None) == 0
    _refused(L.reidmi_evf_sort(PTR, PTR, Q, 0, None), L, b"cap >= 1")
    _refused(L.reidmi_evf_sort(None, PTR, Q, CAP, None), L, b"required")
    _refused(L.reidmi_evf_sort(PTR, None, Q, CAP, None), L, b"required")
    _refused(L.reidmi_evf_sort(PTR, PTR, -1, CAP, None), L, b"bad Q")
    assert L.reidmi_evf_sort(PTR, PTR, 0, CAP, None) == 0

    def finish(pos_cnt=PTR, hist=PTR, junk=PTR, Q=Q, cap=CAP, G=G, overflow=PTR, outs=(PTR,) * 6):
        valid, first, last, npos, ap, nkept = outs
        return L.reidmi_evf_finish(pos_cnt, hist, junk, Q, cap, G, overflow, valid, first, last, npos, ap, nkept, None)
    _refused(finish(cap=0), L, b"cap >= 1")
    _refused(finish(G=0), L, b"bad shape")
    _refused(finish(G=1 << 31), L, b"bad shape")
    _refused(finish(Q=-1), L, b"bad shape")
    for kw in (dict(pos_cnt=None), dict(hist=None), dict(junk=None), dict(overflow=None)):
        _refused(finish(**kw), L, b"required")
    for n in (0, 1, 4, 5):
        _refused(finish(outs=(PTR,) * n + (None,) + (PTR,) * (5 - n)), L, b"required")
    assert finish(Q=0, outs=(PTR, PTR, None, None, PTR, PTR)) == 0
