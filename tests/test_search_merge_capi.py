"""Argument checks of reidmi_search_merge_f32 through the C ABI: every refusal returns before any
HIP call (status REIDMI_EINVAL, a message, nothing launched), so these run without a GPU, on
pointers that are never dereferenced."""
import ctypes

import pytest

EINVAL = 1
Q = 300
PTR = ctypes.c_void_p(0x10000)  # non-null, never touched


def _lib():
    from multimodal_reid_amd import _lib
    return _lib.load()


def _call(L, S=2, k_in=10, k=10, in_idx=PTR, in_dist=PTR, out_idx=PTR, out_dist=PTR, base=PTR, list_stride=None,
          ldi=None, ldo=None):
    ldi = k_in if ldi is None else ldi
    return L.reidmi_search_merge_f32(in_idx, in_dist, S, Q, k_in, Q * ldi if list_stride is None else list_stride,
                                     ldi, base, k, out_idx, out_dist, k if ldo is None else ldo, None)


def test_abi_version_names_the_merge():
    assert _lib().reidmi_abi_version() >= 6


@pytest.mark.parametrize("kw,what", [
    (dict(k=0), b"1 <= k <= 128"), (dict(k=129), b"1 <= k <= 128"),
    (dict(k_in=0), b"1 <= k_in <= 128"), (dict(k_in=129), b"1 <= k_in <= 128"),
    (dict(S=0), b"S >= 1"),
    (dict(ldi=9), b"ldi >= k_in"),
    (dict(ldo=9), b"ldo >= k"),
    (dict(list_stride=Q * 10 - 1), b"list_stride >= Q * ldi"),
    (dict(in_idx=None), b"in_idx"), (dict(in_dist=None), b"in_dist"), (dict(out_idx=None), b"out_idx"),
])
def test_merge_refuses(kw, what):
    L = _lib()
    assert _call(L, **kw) == EINVAL
    assert what in L.reidmi_last_error()


def test_merge_refuses_a_product_beyond_int32():
    L = _lib()
    assert _call(L, S=(1 << 31) // 128, k_in=128) == EINVAL
    assert b"2^31" in L.reidmi_last_error()
