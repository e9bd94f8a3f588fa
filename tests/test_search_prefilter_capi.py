"""The pre-filtered search's C ABI without a GPU: the three symbols and their header-derived
bindings, reidmi_search_prefilter_applies' rule, the workspace size, and every refusal of
reidmi_search_prefiltered_f32 (each returns REIDMI_EINVAL with a message before any HIP call, so the
pointers here are never dereferenced)."""
import ctypes

import pytest

OK, EINVAL = 0, 1
Q, G, D = 130, 1100, 130
PTR = ctypes.c_void_p(0x10000)  # non-null, 16-byte aligned, never touched
NAME = "reidmi_search_prefiltered_f32"
APPLIES = "reidmi_search_prefilter_applies"
WS = "reidmi_search_prefiltered_workspace_bytes"


def _mod():
    from multimodal_reid_amd import _lib
    return _lib


def _call(L, Q=Q, G=G, D=D, k=10, labels=(None,) * 4, bd=None, bi=None, ldb=1, base=0, idx=PTR, ldo=None, S=2,
          need=PTR, stats=None, ws=PTR, ws_bytes=1 << 50):
    return getattr(L, NAME)(PTR, Q, D, PTR, G, D, D, k, *labels, bd, bi, ldb, base, idx, PTR, k if ldo is None else ldo,
                            S, need, stats, ws, ws_bytes, None)


def test_symbols_are_exported_and_bound_from_the_header():
    m = _mod()
    L = m.load()
    c, p, i64 = ctypes.c_int, ctypes.c_void_p, ctypes.c_int64
    decl = m.declarations()
    assert decl[APPLIES] == (c, [i64, i64, i64, c, c])
    assert decl[WS] == (i64, [i64, i64, i64, c, c])
    bounded = decl["reidmi_search_bounded_f32"][1]
    # every argument of the bounded search up to ldo, in its order, then this call's own
    assert decl[NAME] == (c, bounded[:19] + [c, p, p, p, i64, p])
    for name in (APPLIES, WS, NAME):
        fn = getattr(L, name)
        assert fn.restype is decl[name][0] and list(fn.argtypes) == decl[name][1]
    assert L.reidmi_abi_version() >= 13


def test_applies_follows_the_sampled_forms_rule():
    L = _mod().load()
    assert L.reidmi_search_prefilter_applies(130, 1100, 130, 10, 2) == 1
    assert L.reidmi_search_prefilter_applies(130, 1100, 130, 128, 16) == 0  # no whole sample tile
    assert L.reidmi_search_prefilter_applies(130, 1100, 64, 10, 2) == 0     # one K-step of the persistent tile
    assert L.reidmi_search_prefilter_applies(130, 600, 130, 128, 2) == 0    # a 256-item sample, below 4 k
    assert L.reidmi_search_prefilter_applies(130, 600, 130, 64, 2) == 1
    assert L.reidmi_search_prefilter_applies(130, 1100, 65, 10, 2) == 1     # D pads to 128
    # the default stride is 16: 4096 items are one 256-column sample tile
    assert L.reidmi_search_prefilter_applies(10, 4096, 128, 10, 0) == 1
    assert L.reidmi_search_prefilter_applies(10, 4095, 128, 10, 0) == 0
    assert L.reidmi_search_prefilter_applies(10, 4096, 128, 10, 16) == 1
    # shapes, k and strides that no call accepts
    for bad in ((-1, 1100, 130, 10, 2), (130, 0, 130, 10, 2), (130, 1100, 0, 10, 2), (130, 1100, 130, 0, 2),
                (130, 1100, 130, 129, 2), (130, 1100, 130, 10, 1), (130, 1100, 130, 10, -2)):
        assert L.reidmi_search_prefilter_applies(*bad) == 0, bad
    assert L.reidmi_search_prefilter_applies(0, 1100, 130, 10, 2) == 1


def test_workspace_is_aligned_positive_and_has_no_q_times_g_term():
    L = _mod().load()
    ws = L.reidmi_search_prefiltered_workspace_bytes
    for shape in ((130, 1100, 130, 10, 2), (0, 1100, 130, 10, 2), (3368, 15913, 1280, 128, 0),
                  (10000, 1000000, 1792, 10, 0)):
        nb = ws(*shape)
        assert nb > 0 and nb % 16 == 0, shape
    for bad in ((130, 1100, 64, 10, 2), (130, 1100, 130, 128, 16), (130, 600, 130, 128, 2), (130, 1100, 130, 0, 2),
                (130, 1100, 130, 10, 1), (-1, 1100, 130, 10, 2)):
        assert ws(*bad) < 0, bad
    small, big = ws(1000, 100000, 1280, 10, 0), ws(100000, 100000, 1280, 10, 0)
    assert small <= big < small + 100000 * 100000 * 4
    # what grows with Q alone: the fp16 copy (D padded to 64), norms, and at most one pass more of state
    assert big - small < 100000 * (1280 * 2 + 8) + (1 << 30) + (1 << 20)
    # the fp16 copies are in it
    assert ws(1000, 100000, 1280, 10, 0) > 2 * 1280 * (1000 + 100000)


def test_q_zero_is_a_no_op():
    L = _mod().load()
    assert _call(L, Q=0) == OK
    assert _call(L, Q=0, stats=PTR) == OK


def test_refuses_null_need():
    L = _mod().load()
    assert _call(L, need=None) == EINVAL and b"need" in L.reidmi_last_error()


@pytest.mark.parametrize("k", [0, 129])
def test_refuses_bad_k(k):
    L = _mod().load()
    assert _call(L, k=k, ldo=256) == EINVAL
    assert (b"1 <= k <= G" if k == 0 else b"k > 128") in L.reidmi_last_error()


def test_refuses_three_of_the_four_label_arrays():
    L = _mod().load()
    for n in (1, 2, 3):
        assert _call(L, labels=(PTR,) * n + (None,) * (4 - n)) == EINVAL and b"label" in L.reidmi_last_error()
    assert _call(L, labels=(PTR, PTR, PTR, None)) == EINVAL


def test_refuses_bound_idx_without_bound_dist():
    L = _mod().load()
    assert _call(L, bd=None, bi=PTR) == EINVAL and b"bound_idx needs bound_dist" in L.reidmi_last_error()
    assert _call(L, bd=PTR, bi=PTR, ldb=0) == EINVAL and b"ldb >= 1" in L.reidmi_last_error()
    assert _call(L, bd=PTR, bi=PTR, base=-1) == EINVAL and b"index_base" in L.reidmi_last_error()


def test_refuses_a_short_or_misaligned_workspace():
    L = _mod().load()
    nb = L.reidmi_search_prefiltered_workspace_bytes(Q, G, D, 10, 2)
    assert _call(L, ws_bytes=nb - 1) == EINVAL and b"workspace" in L.reidmi_last_error()
    assert _call(L, ws=ctypes.c_void_p(0x10004), ws_bytes=nb) == EINVAL and b"workspace" in L.reidmi_last_error()
    assert _call(L, ws=None, ws_bytes=nb) == EINVAL and b"workspace" in L.reidmi_last_error()


def test_refuses_sample_stride_one():
    L = _mod().load()
    for S in (1, -1):
        assert _call(L, S=S) == EINVAL and b"sample_stride" in L.reidmi_last_error()


def test_refuses_a_shape_the_prefilter_does_not_apply_to():
    L = _mod().load()
    for kw in (dict(D=64), dict(k=128, S=16, ldo=128), dict(G=600, k=128, ldo=128)):
        assert L.reidmi_search_prefilter_applies(kw.get("Q", Q), kw.get("G", G), kw.get("D", D), kw.get("k", 10),
                                                 kw.get("S", 2)) == 0
        assert _call(L, **kw) == EINVAL and b"does not apply" in L.reidmi_last_error()


def test_python_defaults_stay_off():
    import inspect
    from multimodal_reid_amd import evaluate as ev
    for fn in (ev.search, ev.search_device, ev.SearchAccumulator.__init__, ev.search_blocks, ev.search_blocks_device,
               ev.R1_mAP_eval.rank_lists):
        assert inspect.signature(fn).parameters["prefilter"].default is False, fn
    assert inspect.signature(ev.search_device).parameters["return_stats"].default is False
