"""The filtered search's C ABI and the Python-side checks without a GPU: the symbols and their
header-derived bindings, the struct, every half-given clause refused by name (REIDMI_EINVAL before
any HIP call, so the pointers here are never dereferenced), and evaluate's checks of shapes, dtypes,
pairing and camera ids, which raise before anything touches the device (host arrays throughout)."""
import ctypes
import inspect

import numpy as np
import pytest

OK, EINVAL = 0, 1
Q, G, D = 130, 700, 68
PTR = ctypes.c_void_p(0x10000)  # non-null, 16-byte aligned, never touched
P = 0x10000
FILTERED = "reidmi_search_filtered_f32"
PRE = "reidmi_search_prefiltered_filtered_f32"
FIELDS = ["g_valid", "g_cam", "q_cam_mask", "g_time", "q_time_lo", "q_time_hi", "g_group", "q_group"]
# (clause name in the message, a half-given set of fields)
HALVES = [("camera mask", ("g_cam",)), ("camera mask", ("q_cam_mask",)),
          ("time window", ("g_time",)), ("time window", ("q_time_lo",)), ("time window", ("q_time_hi",)),
          ("time window", ("q_time_lo", "q_time_hi")), ("time window", ("g_time", "q_time_lo")),
          ("time window", ("g_time", "q_time_hi")),
          ("group", ("g_group",)), ("group", ("q_group",))]


def _mod():
    from multimodal_reid_amd import _lib
    return _lib


def _ev():
    from multimodal_reid_amd import evaluate
    return evaluate


def _flt(*names):
    s = _mod().structs("reidmi_filter.h")["reidmi_search_filter"]()
    for n in names:
        setattr(s, n, P)
    return s


def _exact(L, flt, k=10, tools=False):
    ref = None if flt is None else ctypes.byref(flt)
    tail = (0, 0, None) if tools else ()
    return getattr(L, FILTERED + ("_ex" if tools else ""))(PTR, Q, D, PTR, G, D, D, k, None, None, None, None, ref,
                                                           None, None, 1, 0, PTR, PTR, k, PTR, 1 << 50, *tail, None)


def _pre(L, flt, Gp=4096, Dp=256, k=10):
    ref = None if flt is None else ctypes.byref(flt)
    return getattr(L, PRE)(PTR, Q, Dp, PTR, Gp, Dp, Dp, k, None, None, None, None, ref, None, None, 1, 0, PTR, PTR, k,
                           0, PTR, None, PTR, 1 << 50, None)


def test_symbols_are_exported_and_bound_from_the_header():
    m = _mod()
    L = m.load()
    S = m.structs("reidmi_filter.h")["reidmi_search_filter"]
    assert [f for f, _ in S._fields_] == FIELDS
    assert all(t is ctypes.c_void_p for _, t in S._fields_) and ctypes.sizeof(S) == 64
    decl = m.declarations()
    bounded = decl["reidmi_search_bounded_f32"][1]
    pre = decl["reidmi_search_prefiltered_f32"][1]
    fp = ctypes.POINTER(S)
    # the unfiltered calls' arguments with the filter after the four label pointers
    assert decl[FILTERED] == (ctypes.c_int, bounded[:12] + [fp] + bounded[12:])
    assert decl[PRE] == (ctypes.c_int, pre[:12] + [fp] + pre[12:])
    for name in (FILTERED, PRE):
        fn = getattr(L, name)
        assert fn.restype is decl[name][0] and list(fn.argtypes) == decl[name][1]
    assert L.reidmi_abi_version() >= 14
    T = m.load_tools()
    tdecl = m.declarations(tools=True)
    c, p = ctypes.c_int, ctypes.c_void_p
    assert tdecl[FILTERED + "_ex"] == (c, decl[FILTERED][1][:-1] + [c, c, p, p])
    assert list(getattr(T, FILTERED + "_ex").argtypes) == tdecl[FILTERED + "_ex"][1]
    assert FILTERED + "_ex" not in decl


def test_struct_layout_matches_the_compiler(tmp_path):
    """reidmi_filter.h's struct (reidmi.h includes it) as the C++ compiler lays it out."""
    import shutil
    import subprocess
    from multimodal_reid_amd import build_lib
    if not shutil.which(build_lib.HIPCC):
        pytest.skip("hipcc not available")
    S = _mod().structs("reidmi_filter.h")["reidmi_search_filter"]
    assert "reidmi_search_filter" not in _mod().structs()  # reidmi.h's own are the model's
    lines = ["#include <cstddef>", "#include <cstdio>", '#include "reidmi.h"', "int main() {",
             '  std::printf("%zu\\n", sizeof(reidmi_search_filter));']
    lines += [f'  std::printf("%zu\\n", offsetof(reidmi_search_filter, {f}));' for f in FIELDS]
    src, exe = tmp_path / "layout.cpp", tmp_path / "layout"
    src.write_text("\n".join(lines + ["  return 0;", "}", ""]))
    subprocess.run([build_lib.HIPCC, "-x", "c++", "-std=c++17", f"-I{build_lib.INCLUDE}", str(src), "-o", str(exe)],
                   check=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()
    assert [int(x) for x in out] == [ctypes.sizeof(S)] + [getattr(S, f).offset for f in FIELDS]


def test_q_zero_and_absent_filters_pass_the_refusals():
    L = _mod().load()
    for flt in (None, _flt(), _flt(*FIELDS), _flt("g_valid")):
        assert getattr(L, FILTERED)(PTR, 0, D, PTR, G, D, D, 10, None, None, None, None,
                                    None if flt is None else ctypes.byref(flt), None, None, 1, 0, PTR, PTR, 10, PTR,
                                    1 << 50, None) == OK


@pytest.mark.parametrize("clause,given", HALVES, ids=["+".join(h[1]) for h in HALVES])
def test_every_half_given_clause_is_refused_by_name(clause, given):
    L, T = _mod().load(), _mod().load_tools()
    for lib, call in ((L, lambda f: _exact(L, f)), (L, lambda f: _pre(L, f)), (T, lambda f: _exact(T, f, tools=True))):
        assert call(_flt(*given)) == EINVAL
        msg = lib.reidmi_last_error()
        assert clause.encode() in msg and b"half given" in msg, msg
        # the other clauses, complete, do not hide it
        others = [f for f in FIELDS if clause == "camera mask" and "cam" not in f
                  or clause == "time window" and "time" not in f or clause == "group" and "group" not in f]
        assert call(_flt(*given, *others)) == EINVAL and clause.encode() in lib.reidmi_last_error()


def test_the_filtered_calls_keep_the_unfiltered_refusals():
    L = _mod().load()
    assert _exact(L, _flt("g_valid"), k=0) == EINVAL and b"1 <= k <= G" in L.reidmi_last_error()
    assert _exact(L, _flt("g_valid"), k=129) == EINVAL and b"k > 128" in L.reidmi_last_error()
    assert getattr(L, FILTERED)(PTR, Q, D, PTR, G, D, D, 10, PTR, None, None, None, None, None, None, 1, 0, PTR, PTR,
                                10, PTR, 1 << 50, None) == EINVAL and b"label" in L.reidmi_last_error()
    assert _pre(L, _flt("g_valid"), Gp=4095) == EINVAL and b"does not apply" in L.reidmi_last_error()


# ----------------------------------------------------------------- the Python-side checks
def _feat():
    return np.zeros((Q, D), np.float32), np.zeros((G, D), np.float32)


def _raises(match, g_attrs=None, q_filter=None, fn=None):
    ev = _ev()
    qf, gf = _feat()
    with pytest.raises(_mod().ReidmiError, match=match):
        (fn or ev.search_device)(qf, gf, 10, g_attrs=g_attrs, q_filter=q_filter)


def test_python_refuses_shapes_and_dtypes_before_any_device_call():
    ev = _ev()
    A, F = ev.ItemAttrs, ev.QueryFilter
    _raises(r"g_attrs\.valid must have shape \[700\]", A(valid=np.ones(G - 1, np.uint8)))
    _raises(r"g_attrs\.valid must have bool or uint8", A(valid=np.ones(G, np.int64)))
    _raises(r"g_attrs\.valid must", A(valid=np.ones(G, np.float32)))
    _raises(r"g_attrs\.camids must have shape", A(camids=np.zeros((G, 1), np.int64)), F(cam_mask=np.zeros(Q, np.int64)))
    _raises(r"g_attrs\.times must be an integer array", A(times=np.zeros(G, np.float64)), F(time_range=(0, 1)))
    _raises(r"g_attrs\.groups must have shape", A(groups=np.zeros(G + 1, np.int64)), F(groups=np.zeros(Q, np.int64)))
    _raises(r"q_filter\.cam_mask must have shape \[130\]", A(camids=np.zeros(G, np.int64)),
            F(cam_mask=np.zeros(Q + 1, np.int64)))
    _raises(r"q_filter\.cam_mask must be an integer array", A(camids=np.zeros(G, np.int64)),
            F(cam_mask=np.zeros(Q, np.float32)))
    _raises(r"time_range must be one \(lo, hi\) pair or have shape \[130, 2\]", A(times=np.zeros(G, np.int64)),
            F(time_range=np.zeros((Q, 3), np.int64)))
    _raises(r"time_range must hold integers", A(times=np.zeros(G, np.int64)), F(time_range=(0.5, 1.5)))
    _raises(r"q_filter\.groups must have shape", A(groups=np.zeros(G, np.int64)), F(groups=np.zeros(1, np.int64)))
    _raises(r"g_attrs must be an evaluate\.ItemAttrs", {"valid": np.ones(G, np.uint8)})
    _raises(r"q_filter must be an evaluate\.QueryFilter", A(groups=np.zeros(G, np.int64)), np.zeros(Q, np.int64))


def test_python_refuses_a_clause_with_one_side_only():
    ev = _ev()
    A, F = ev.ItemAttrs, ev.QueryFilter
    zg, zq = np.zeros(G, np.int64), np.zeros(Q, np.int64)
    _raises(r"camera mask clause has g_attrs\.camids but no q_filter\.cam_mask", A(camids=zg))
    _raises(r"camera mask clause has q_filter\.cam_mask but no g_attrs\.camids", None, F(cam_mask=zq))
    _raises(r"time window clause has g_attrs\.times but no q_filter\.time_range", A(times=zg), F(groups=zq))
    _raises(r"time window clause has q_filter\.time_range but no g_attrs\.times", A(valid=np.ones(G, bool)),
            F(time_range=(0, 5)))
    _raises(r"group clause has g_attrs\.groups but no q_filter\.groups", A(groups=zg))
    _raises(r"group clause has q_filter\.groups but no g_attrs\.groups", A(camids=zg), F(cam_mask=zq, groups=zq))
    _raises(r"group clause", None, F(groups=zq), fn=ev.search)


def test_python_refuses_camera_ids_outside_the_mask():
    ev = _ev()
    for bad in (64, -1):
        cams = np.zeros(G, np.int64)
        cams[G // 2] = bad
        _raises(r"camids must be in \[0, 64\)", ev.ItemAttrs(camids=cams), ev.QueryFilter(cam_mask=np.ones(Q, np.int64)))
    # without a mask the camera ids are not a clause at all: that is the missing-side refusal
    _raises(r"camera mask clause", ev.ItemAttrs(camids=np.full(G, 99, np.int64)))


def test_accumulator_checks_the_query_side_at_once_and_the_block_at_add():
    ev, E = _ev(), _mod().ReidmiError
    qf, gf = _feat()
    with pytest.raises(E, match=r"q_filter\.groups must have shape \[130\]"):
        ev.SearchAccumulator(qf, 10, q_filter=ev.QueryFilter(groups=np.zeros(3, np.int64)))
    with pytest.raises(E, match=r"q_filter must be an evaluate\.QueryFilter"):
        ev.SearchAccumulator(qf, 10, q_filter=(0, 1))


def test_mask_helpers():
    ev = _ev()
    assert int(ev.cam_mask([])) == 0 and int(ev.cam_mask([0, 3])) == 9
    assert ev.cam_mask([63]).dtype == np.int64 and int(ev.cam_mask([63])) == -2 ** 63
    assert int(ev.cam_mask(range(64))) == -1
    with pytest.raises(_mod().ReidmiError, match=r"\[0, 64\)"):
        ev.cam_mask([64])
    m = ev.cross_camera_mask(np.array([0, 5, 63]))
    assert m.dtype == np.int64 and m.tolist() == [-2, ~(1 << 5), 2 ** 63 - 1]
    with pytest.raises(_mod().ReidmiError, match=r"\[0, 64\)"):
        ev.cross_camera_mask(np.array([1, 64]))
    with pytest.raises(_mod().ReidmiError, match="integer"):
        ev.cross_camera_mask(np.array([1.0]))


def test_python_defaults_stay_off():
    ev = _ev()
    for fn in (ev.search, ev.search_device, ev.R1_mAP_eval.rank_lists):
        sig = inspect.signature(fn).parameters
        assert sig["g_attrs"].default is None and sig["q_filter"].default is None, fn
    for fn in (ev.SearchAccumulator.__init__, ev.search_blocks, ev.search_blocks_device):
        assert inspect.signature(fn).parameters["q_filter"].default is None, fn
    assert inspect.signature(ev.SearchAccumulator.add).parameters["g_attrs"].default is None


def test_item_attrs_slice_by_block():
    ev = _ev()
    a = ev.ItemAttrs(valid=np.arange(10) % 2 == 0, times=np.arange(10))
    b = a[3:7]
    assert b.valid.tolist() == [False, True, False, True] and b.times.tolist() == [3, 4, 5, 6]
    assert b.camids is None and b.groups is None
