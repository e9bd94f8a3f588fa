"""CPU-side checks of the drop-in boundary: libreidmi.so loads and exports every entry
point include/reidmi.h declares, each bound by _lib.py with the types the header states; the tools
library (include/reidmi_tools.h) adds exactly its forced-variant entry points, which the
product library does not export.  No compute calls (no GPU here)."""
import ctypes
import os
import re

import pytest

from conftest import REPO

HEADER = os.path.join(REPO, "include", "reidmi.h")
TOOLS_HEADER = os.path.join(REPO, "include", "reidmi_tools.h")
LIB = os.path.join(REPO, "multimodal-reid_amd", "libreidmi.so")
TOOLS_LIB = os.path.join(REPO, "multimodal-reid_amd", "libreidmi_tools.so")


def declared(header=HEADER):
    txt = open(header).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    return sorted(set(re.findall(r"\b(reidmi_\w+)\s*\(", txt)))


def test_header_declares_entry_points():
    names = declared()
    assert "reidmi_distmat_f32" in names and "reidmi_eval_rows" in names
    assert len(names) >= 6


def test_library_exports_every_declared_symbol():
    if not os.path.exists(LIB):
        pytest.skip("libreidmi.so not built (run __graft_entry__.build())")
    import torch  # noqa: F401  (load torch's HIP runtime first, as the product does)
    L = ctypes.CDLL(LIB)
    missing = [n for n in declared() if not hasattr(L, n)]
    assert not missing, missing
    L.reidmi_abi_version.restype = ctypes.c_int
    assert L.reidmi_abi_version() >= 1


def _assert_bound(L, decls):
    for name, (restype, argtypes) in decls.items():
        fn = getattr(L, name)
        assert fn.restype is restype, name
        assert list(fn.argtypes) == list(argtypes), name


def test_every_prototype_is_bound_with_the_parsed_types():
    """Every prototype of reidmi.h is typed on the loaded product library exactly as the header
    parses; the name set is cross-checked by this file's own regex."""
    from multimodal_reid_amd import _lib
    decls = _lib.declarations()
    assert set(decls) == set(declared()), set(decls) ^ set(declared())
    _assert_bound(_lib.load(), decls)


def test_tools_library_exports_variants_product_does_not():
    if not (os.path.exists(LIB) and os.path.exists(TOOLS_LIB)):
        pytest.skip("libraries not built (run __graft_entry__.build())")
    import torch  # noqa: F401
    from multimodal_reid_amd import _lib
    tools = declared(TOOLS_HEADER)
    decls = _lib.declarations(tools=True)
    assert set(tools) == set(decls) - set(_lib.declarations())
    _assert_bound(_lib.load_tools(), decls)
    assert not set(tools) & set(declared())
    P, T = ctypes.CDLL(LIB), ctypes.CDLL(TOOLS_LIB)
    assert not [n for n in tools if hasattr(P, n)], "the product library must not export the A/B variants"
    missing = [n for n in tools + declared() if not hasattr(T, n)]
    assert not missing, missing


@pytest.mark.parametrize("src,define", [("gemm.hip", "-DGEMM_VAR_NOSTORE=1"), ("gemm.hip", "-DGEMM_VAR_NOWAIT=1"),
                                        ("gemm.hip", "-DGEMM_VAR_NODMA=1"),
                                        ("distance.hip", "-DDM2_BK_=32"), ("search.hip", "-DDM2_BK_=32"),
                                        ("prefilter.hip", "-DRS_STATS")])
def test_variant_macros_refused_outside_tools_builds(src, define):
    """The A/B timing hooks (some compile kernels with wrong results by design) are an #error
    unless the tools define is set, so no variant can be built into libreidmi.so."""
    import shutil
    import subprocess
    from multimodal_reid_amd import build_lib as B
    if not shutil.which(B.HIPCC):
        pytest.skip("hipcc not available")
    base = [B.HIPCC, "-E", "-x", "hip", "--offload-arch=gfx950", "--cuda-device-only", f"-I{B.CSRC}",
            f"-I{B.INCLUDE}", os.path.join(B.CSRC, src), "-o", os.devnull]
    bad = subprocess.run(base + [define], capture_output=True, text=True)
    assert bad.returncode != 0 and "REIDMI_TOOLS" in bad.stderr
    ok = subprocess.run(base + [define, B.TOOLS_DEFINE], capture_output=True, text=True)
    assert ok.returncode == 0, ok.stderr[-2000:]


# the encoder's GEMM instances (EPI 0-6).  The re-rank pre-filter's EPI_RRHI / EPI_RRSV (7, 8)
# spill 20 bytes per lane in the tile prologue, where each reload is followed by the compiler's
# own vmcnt(0) (an over-wait: safe; their K-loops keep the plain vmcnt(6), no deferred stores)
_GEMM_ENCODER = tuple(f"gemm_persistent_kernelILi{e}E" for e in range(7))


@pytest.mark.parametrize("src,kernels", [("attention.hip", ("mhsa_kernel", "mhsa_pipe_kernel")),
                                         ("gemm.hip", _GEMM_ENCODER)])
def test_counted_wait_kernels_use_no_scratch(src, kernels):
    """The kernels whose `s_waitcnt vmcnt(N)` counts are derived from their own vector-memory
    instructions (attention's K/V^T rings, the GEMM's deferred epilogue stores) must not spill:
    a scratch load or store would enter the same counter and let a wait return early.
    Checked on the compiler's resource report of the product build flags."""
    import shutil
    import subprocess
    from multimodal_reid_amd import build_lib as B
    if not shutil.which(B.HIPCC):
        pytest.skip("hipcc not available")
    flags = [f for f in B.FLAGS if f not in ("-fPIC", "-fno-gpu-rdc")]
    r = subprocess.run([B.HIPCC, *flags, "--cuda-device-only", "-c", "-Rpass-analysis=kernel-resource-usage",
                        os.path.join(B.CSRC, src), "-o", os.devnull], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    name, seen = None, 0
    for line in r.stderr.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            name = m.group(1)
            continue
        m = re.search(r"ScratchSize \[bytes/lane\]: (\d+)", line)
        if m and name and any(k in name for k in kernels):
            seen += 1
            assert int(m.group(1)) == 0, f"{name} spills to scratch ({m.group(1)} bytes/lane)"
    assert seen >= 3, r.stderr[-2000:]


# ---- argument checks of the attention entry points: each returns before any HIP call, so they
# run here with null pointers and no GPU
def _tools():
    from multimodal_reid_amd import _lib
    return _lib.load_tools()


def _refused(T, rc):
    return rc != 0 and len(T.reidmi_last_error()) > 0


def test_attn_lpad_every_length():
    T = _tools()
    for L in range(1, 257):
        assert T.reidmi_attn_lpad(L) == 32 * -(-L // 32) + 4, L
    for L in (0, -1, 257):
        assert T.reidmi_attn_lpad(L) < 0, L


def test_attn_stride_rule_has_one_definition():
    """reidmi_attn_vt_stride is the rule for 1..1024, reidmi_attn_lpad the same rule cut at 256."""
    T = _tools()
    for L in range(1, 1025):
        assert T.reidmi_attn_vt_stride(L) == (L + 31) // 32 * 32 + 4, L
    for L in range(1, 257):
        assert T.reidmi_attn_lpad(L) == T.reidmi_attn_vt_stride(L), L
    assert T.reidmi_attn_lpad(0) == -1 and T.reidmi_attn_lpad(257) == -1
    assert T.reidmi_attn_vt_stride(0) == -1 and T.reidmi_attn_vt_stride(1025) == -1


@pytest.mark.parametrize("L", [0, 257])
@pytest.mark.parametrize("causal", [0, 1])
def test_mhsa_refuses_unsupported_lengths(L, causal):
    T = _tools()
    assert _refused(T, T.reidmi_mhsa_f16(None, None, None, None, 2, L, 3, causal, None))
    assert b"mhsa" in T.reidmi_last_error()


@pytest.mark.parametrize("L", [204, 213])
def test_mhsa_rr_refuses_lengths_outside_its_range(L):
    T = _tools()
    assert _refused(T, T.reidmi_mhsa_f16_rr(None, None, None, None, 2, L, 3, None))
    assert b"reidmi_mhsa_f16_rr" in T.reidmi_last_error()


@pytest.mark.parametrize("L,H,W,what", [(211, 8, 512, b"width"), (211, 12, 1024, b"width"), (211, 16, 768, b"width"),
                                        (0, 12, 768, b"<= L"), (225, 12, 768, b"<= L"), (225, 16, 1024, b"<= L")])
def test_cls_attn_nokv_refuses_unsupported_shapes(L, H, W, what):
    T = _tools()
    big = 1 << 40  # (the workspace is not what is refused)
    assert _refused(T, T.reidmi_cls_attn_nokv_f16(None, None, None, None, None, None, 4, L, H, W, None, big, None, None))
    assert what in T.reidmi_last_error(), T.reidmi_last_error()


def test_cls_attn_nokv_workspace_size_and_empty_batch():
    T = _tools()
    for W in (768, 1024):
        H = W // 64
        assert T.reidmi_cls_attn_nokv_f16(None, None, None, None, None, None, 0, 211, H, W, None, 0, None, None) == 0
        need = T.reidmi_cls_attn_nokv_ws_bytes(37, W)
        # u (fp16 hi, lo), the score constants, z and alpha of 37 images, each rounded up to 256 bytes
        assert need >= 37 * (2 * H * W * 2 + 32 * 4 + H * W * 4 + H * 4) and need % 256 == 0
        assert _refused(T, T.reidmi_cls_attn_nokv_f16(None, None, None, None, None, None, 37, 211, H, W, None,
                                                      need - 1, None, None))
        assert b"workspace" in T.reidmi_last_error()
