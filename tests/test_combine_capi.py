"""Argument checks of reidmi_combine_rows_f32 through the C ABI: every refusal returns before any
HIP call (status REIDMI_EINVAL, a message, nothing launched), so these run without a GPU, on
pointers that are never dereferenced."""
import ctypes

import pytest

OK, EINVAL = 0, 1
PTR = ctypes.c_void_p(0x10000)  # non-null, never touched


def _lib():
    from multimodal_reid_amd import _lib
    return _lib.load()


def _call(L, src=PTR, n_src=97, d=64, ld_src=None, offsets=PTR, idx=PTR, w=None, rows=37, base=None, ld_base=0,
          base_w=1.0, mode=0, normalize=0, out=PTR, ldo=None, bad=None):
    return L.reidmi_combine_rows_f32(src, n_src, d, d if ld_src is None else ld_src, offsets, idx, w, rows, base,
                                     ld_base, base_w, mode, normalize, out, d if ldo is None else ldo, bad, None)


def test_abi_version_names_combine():
    assert _lib().reidmi_abi_version() >= 7


def test_binding_is_derived_from_the_header():
    from multimodal_reid_amd import _lib
    restype, argtypes = _lib.declarations()["reidmi_combine_rows_f32"]
    assert restype is ctypes.c_int
    i64, p, f, i = ctypes.c_int64, ctypes.c_void_p, ctypes.c_float, ctypes.c_int
    assert argtypes == [p, i64, i64, i64, p, p, p, i64, p, i64, f, i, i, p, i64, p, p]
    fn = _lib.load().reidmi_combine_rows_f32
    assert fn.restype is restype and list(fn.argtypes) == argtypes


@pytest.mark.parametrize("kw,what", [
    (dict(src=None), b"null"), (dict(offsets=None), b"null"), (dict(idx=None), b"null"), (dict(out=None), b"null"),
    (dict(d=0), b"d must be positive"), (dict(d=-3), b"d must be positive"),
    (dict(ld_src=63), b"ld_src"), (dict(ldo=63), b"ldo"),
    (dict(base=PTR, ld_base=63), b"ld_base"),
    (dict(mode=-1), b"mode"), (dict(mode=3), b"mode"),
    (dict(mode=2, w=PTR), b"max takes no weights"),
    (dict(n_src=1 << 31), b"2^31"), (dict(n_src=-1), b"n_src"),
    (dict(rows=-1), b"rows"),
])
def test_combine_refuses(kw, what):
    L = _lib()
    assert _call(L, **kw) == EINVAL
    assert what in L.reidmi_last_error()


def test_no_rows_is_a_no_op():
    # nothing is launched and nothing dereferenced: null pointers are fine without rows
    assert _call(_lib(), rows=0, src=None, offsets=None, idx=None, out=None) == OK
