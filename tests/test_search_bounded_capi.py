"""Argument checks of reidmi_search_bounded_f32 through the C ABI and of the Python layer on top of
it: every refusal returns before any HIP call (status REIDMI_EINVAL, a message, nothing launched),
so these run without a GPU, on pointers that are never dereferenced."""
import ctypes

import numpy as np
import pytest

EINVAL = 1
Q, G, D = 300, 5000, 1280
PTR = ctypes.c_void_p(0x10000)  # non-null, 16-byte aligned, never touched
NAME = "reidmi_search_bounded_f32"


def _mod():
    from multimodal_reid_amd import _lib
    return _lib


def _call(L, k=10, G=G, bd=PTR, bi=PTR, ldb=1, base=0, idx=PTR, ws=PTR, ws_bytes=1 << 40, labels=(None,) * 4,
          ldo=None, fn=NAME, extra=()):
    return getattr(L, fn)(PTR, Q, D, PTR, G, D, D, k, *labels, bd, bi, ldb, base, idx, PTR, k if ldo is None else ldo,
                          ws, ws_bytes, *extra, None)


def test_symbol_is_exported_and_bound_with_the_headers_types():
    m = _mod()
    L = m.load()
    restype, argtypes = m.declarations()[NAME]
    c, p, i64 = ctypes.c_int, ctypes.c_void_p, ctypes.c_int64
    assert restype is c
    assert argtypes == [p, i64, i64, p, i64, i64, i64, c, p, p, p, p, p, p, i64, i64, p, p, i64, p, i64, p]
    fn = getattr(L, NAME)
    assert fn.restype is restype and list(fn.argtypes) == argtypes
    assert L.reidmi_abi_version() >= 9
    # the forced-variant form is the tools library's alone
    assert NAME + "_ex" not in m.declarations() and not hasattr(L, NAME + "_ex")
    assert NAME + "_ex" in m.declarations(tools=True) and hasattr(m.load_tools(), NAME + "_ex")
    assert m.declarations(tools=True)[NAME + "_ex"][1] == argtypes[:-1] + [c, c, p, p]


def test_refuses_bound_idx_without_bound_dist():
    L = _mod().load()
    assert _call(L, bd=None, bi=PTR) == EINVAL
    assert b"bound_idx needs bound_dist" in L.reidmi_last_error()


def test_refuses_bad_ldb():
    L = _mod().load()
    for ldb in (0, -1):
        assert _call(L, ldb=ldb) == EINVAL
        assert b"ldb >= 1" in L.reidmi_last_error()
        assert _call(L, bd=None, bi=None, ldb=ldb) == EINVAL


def test_refuses_index_base_out_of_range():
    L = _mod().load()
    for base in (-1, 2 ** 31 - G, 2 ** 31, 2 ** 40):
        assert _call(L, base=base) == EINVAL, base
        assert b"index_base + G <= 2^31 - 1" in L.reidmi_last_error()
    # the largest base is in range: the next refusal is the workspace's
    assert _call(L, base=2 ** 31 - 1 - G, ws_bytes=0) == EINVAL and b"workspace" in L.reidmi_last_error()


@pytest.mark.parametrize("bound", ["none", "radius", "key"])
def test_refuses_what_the_unbounded_search_refuses(bound):
    L = _mod().load()
    kw = {"none": dict(bd=None, bi=None), "radius": dict(bi=None), "key": {}}[bound]
    for k, G_ in ((0, G), (41, 40), (-3, G)):
        assert _call(L, k=k, G=G_, ldo=64, **kw) == EINVAL and b"1 <= k <= G" in L.reidmi_last_error()
    assert _call(L, k=129, **kw) == EINVAL and b"reidmi_topk_rows_f32" in L.reidmi_last_error()
    nb = L.reidmi_search_workspace_bytes(Q, G, D, 10)
    assert _call(L, ws_bytes=nb - 1, **kw) == EINVAL and b"workspace" in L.reidmi_last_error()
    assert _call(L, ws=None, ws_bytes=nb, **kw) == EINVAL
    assert _call(L, ws=ctypes.c_void_p(0x10004), ws_bytes=nb, **kw) == EINVAL
    assert _call(L, idx=None, **kw) == EINVAL and b"out_idx" in L.reidmi_last_error()
    assert _call(L, ldo=9, **kw) == EINVAL
    for n in (1, 2, 3):
        assert _call(L, labels=(PTR,) * n + (None,) * (4 - n), **kw) == EINVAL and b"label" in L.reidmi_last_error()


def test_ex_form_refuses_the_same_and_bad_splits():
    T = _mod().load_tools()
    ex = dict(fn=NAME + "_ex")
    assert _call(T, bd=None, extra=(0, 0, None), **ex) == EINVAL and b"bound_idx needs" in T.reidmi_last_error()
    assert _call(T, ldb=0, extra=(0, 0, None), **ex) == EINVAL
    assert _call(T, base=-1, extra=(0, 0, None), **ex) == EINVAL
    for splits, cap in ((-1, 0), (4097, 0), (0, 10 + 127), (0, 513)):
        assert _call(T, extra=(splits, cap, None), **ex) == EINVAL and b"capacity" in T.reidmi_last_error()


def test_python_refuses_bad_max_dist_without_a_gpu():
    from multimodal_reid_amd import evaluate as ev
    Err = _mod().ReidmiError
    qf, gf = np.zeros((7, 8), np.float32), np.zeros((20, 8), np.float32)
    for bad in (np.zeros(6, np.float32), np.zeros((7, 1), np.float32), np.zeros((1, 7), np.float32), [1.0, 2.0]):
        with pytest.raises(Err, match="max_dist"):
            ev.search(qf, gf, 5, max_dist=bad)
        with pytest.raises(Err, match="max_dist"):
            ev.SearchAccumulator(qf, 5, max_dist=bad)
        with pytest.raises(Err, match="max_dist"):
            ev.search_blocks(qf, [gf], 5, max_dist=bad)
    with pytest.raises(Err, match="max_dist"):
        ev.search(qf, gf, 5, max_dist="near")
    for bad in (None, 1, "yes"):
        with pytest.raises(Err, match="carry_bound"):
            ev.SearchAccumulator(qf, 5, carry_bound=bad)


def test_python_signatures_keep_their_defaults():
    import inspect
    from multimodal_reid_amd import evaluate as ev
    for fn in (ev.search, ev.search_device):
        assert inspect.signature(fn).parameters["max_dist"].default is None
    for fn in (ev.SearchAccumulator.__init__, ev.search_blocks, ev.search_blocks_device):
        ps = inspect.signature(fn).parameters
        assert ps["max_dist"].default is None and isinstance(ps["carry_bound"].default, bool)
        assert ps["carry_bound"].default == ev.CARRY_BOUND_DEFAULT
