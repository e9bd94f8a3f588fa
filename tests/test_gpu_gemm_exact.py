"""The fp16 MFMA GEMM (csrc/gemm.hip, gemm_epilogue.h) against exact arithmetic, bit for bit.

The operands of tests/gemm_exact.py make every product and every partial sum exactly
representable in fp32, so the accumulator is the same in every summation order and the expected
output bits follow from an fp64 reference and one defined rounding, whatever the K-loop looks
like.  Each kernel is compared with that expectation, never only with another kernel:

  epi 0 / 5 / 6 (fp16, fp32, fp16 residual)   bit-equal; a mismatch names the first (m, n), the
                                               count and the residues of the wrong rows / columns
  epi 1 (QuickGELU)                            |got - ref| <= 0.5 ulp16(ref) + 2^-16 |ref|
                                               (gemm_exact.gelu_bound: derived, not measured)

through the product entry reidmi_gemm_f16 (automatic tiling) and the tools entry
reidmi_gemm_f16_tiled (tile 1 = 128x128, tile 2 = persistent 256x256 with 1 and 2 XCD groups).
A lives in a buffer whose rows from M on are NaN (the clamped source rows of a ragged tile), and
`out` between two sentinel guards that must come back untouched, as must the gaps between rows
when ldc > N.
"""
import functools

import numpy as np
import pytest
import torch

import gemm_exact as gx

pytestmark = pytest.mark.gpu

GUARD = 4096  # sentinel elements before and after `out` (a multiple of 8: 16-byte alignment kept)
FILL = -1234.0  # the sentinel, representable in fp16


def _lib():
    from multimodal_reid_amd import _lib
    return _lib


def _dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _a_with_nan_rows(A):
    """A in a buffer of round_up(M, 256) + 8 rows, NaN from row M on."""
    M, K = A.shape
    buf = np.full((gx.round_up(M, 256) + 8, K), np.nan, np.float16)
    buf[:M] = A
    return _dev(buf)


@functools.lru_cache(maxsize=2)
def _case(M, N, K):
    """Operands on the host and the device and the fp64 accumulator, shared by a shape's tests."""
    A, W, bias, x = gx.operands(M, N, K, seed=M * 7 + N * 3 + K, gain=gx.GAIN[K])
    return dict(A=A, W=W, bias=bias, x=x, acc=gx.accumulate(A, W), dA=_a_with_nan_rows(A), dW=_dev(W),
                dbias=_dev(bias))


def _run(c, epi, M, N, K, tile, ngroups, ldc=None, bias=True, dfold=(None, None)):
    """One GEMM into a guarded buffer.  Returns out[:, :N] on the host after checking that the
    guards and the gaps between rows still hold the sentinel.  tile None: the product entry."""
    L = _lib()
    ldc = ldc or N
    dt = torch.float32 if epi == 5 else torch.float16
    flat = torch.full((2 * GUARD + M * ldc,), FILL, dtype=dt, device="cuda")
    out = flat[GUARD:GUARD + M * ldc].view(M, ldc)
    if epi == 6:
        out[:, :N] = _dev(c["x"])
    args = (epi, L.ptr(c["dA"]), K, L.ptr(c["dW"]), K, M, N, K, L.ptr(c["dbias"] if bias else None), L.ptr(dfold[0]),
            L.ptr(dfold[1]), L.ptr(out), ldc)
    if tile is None:
        L.call("reidmi_gemm_f16", *args, L.stream())
    else:
        L.call_tools("reidmi_gemm_f16_tiled", *args, tile, ngroups, L.stream())
    torch.cuda.synchronize()
    host = flat.cpu().numpy()
    body = host[GUARD:GUARD + M * ldc].reshape(M, ldc)
    fill = np.asarray(FILL, host.dtype)
    assert (host[:GUARD] == fill).all() and (host[GUARD + M * ldc:] == fill).all(), "a write outside out"
    assert (body[:, N:] == fill).all(), "a write between the rows of out"
    return np.ascontiguousarray(body[:, :N])


def _tilings(N, K):
    """(tile, ngroups) of a shape: the product's own choice, the 128x128 tile, and the persistent
    tile with 1 and 2 XCD groups wherever it is admitted."""
    t = [(None, 0), (1, 0)]
    if N % 256 == 0 and K >= 128:
        t += [(2, 1), (2, 2)]
    return t


def _check(got, want, epi, where):
    if epi == 1:
        msg = gx.bound_report(got, want, gx.gelu_bound(want))
    else:
        msg = gx.mismatch_report(got, want)
    assert msg is None, f"{where}: {msg}"


def _name(epi, tile, ngroups, M, N, K):
    return f"epi {epi} tile {'auto' if tile is None else tile} ngroups {ngroups} (M, N, K) = ({M}, {N}, {K})"


def test_mfma_accumulates_exactly(gpu):
    """The one assumption no CPU check can confirm: v_mfma_f32_16x16x32_f16 accumulates without
    error when every product and partial sum is representable.  The smallest case (M = 1, N = 128,
    K = 64, fp32 output, the 128x128 tile); every other test of this file rests on it."""
    M, N, K = 1, 128, 64
    c = _case(M, N, K)
    got = _run(c, 5, M, N, K, 1, 0)
    want = gx.expected(5, c["acc"], c["bias"])
    print("max |got - expected|:", np.abs(got.astype(np.float64) - want).max())
    _check(got, want, 5, _name(5, 1, 0, M, N, K))


GRID_M = (1, 127, 128, 129, 255, 256, 257, 513)
GRID_NK = ((128, 64), (256, 128), (384, 192), (512, 256), (256, 704))


@pytest.mark.parametrize("M,N,K,epi", [(M, N, K, epi) for N, K in GRID_NK for M in GRID_M for epi in (0, 1, 5, 6)])
def test_edge_grid(gpu, M, N, K, epi):
    """Every epilogue at the tile edges: M around 128 and 256 and one row; M = 513 = two full
    256-row tiles and a ragged one in a launch (QuickGELU's unchecked full-tile stores beside the
    checked ones); N = 384 admits the 128x128 tile only; K = 128 is the persistent kernel's
    minimum of two K-steps; K = 704 > N = 256 takes the residual epilogue's second kernel copy."""
    c = _case(M, N, K)
    want = gx.expected(epi, c["acc"], c["bias"], c["x"])
    for tile, ngroups in _tilings(N, K):
        _check(_run(c, epi, M, N, K, tile, ngroups), want, epi, _name(epi, tile, ngroups, M, N, K))


@pytest.mark.parametrize("epi", [0, 1, 5, 6])
def test_row_pitch_beyond_n(gpu, epi):
    """ldc = N + 8: the same bits, and the 8 elements between rows keep the sentinel."""
    M, N, K = 257, 256, 128
    c = _case(M, N, K)
    want = gx.expected(epi, c["acc"], c["bias"], c["x"])
    for tile, ngroups in _tilings(N, K):
        _check(_run(c, epi, M, N, K, tile, ngroups, ldc=N + 8), want, epi, _name(epi, tile, ngroups, M, N, K))


@pytest.mark.parametrize("epi", [0, 5, 6])
def test_no_bias(gpu, epi):
    M, N, K = 129, 256, 128
    c = _case(M, N, K)
    want = gx.expected(epi, c["acc"], None, c["x"])
    for tile, ngroups in _tilings(N, K):
        _check(_run(c, epi, M, N, K, tile, ngroups, bias=False), want, epi, _name(epi, tile, ngroups, M, N, K))


@pytest.mark.parametrize("epi", [0, 1])
@pytest.mark.parametrize("M,N,K", [(129, 256, 128), (257, 512, 256), (300, 384, 192)])
def test_layernorm_fold(gpu, epi, M, N, K):
    """rstd_m * acc + (shift_m * colsum_n + bias_n) with power-of-two rstd: both FMAs exact.  The
    rowstat entries past M, which the kernels read, are NaN."""
    c = _case(M, N, K)
    rs, cs = gx.fold_operands(M, N, seed=M + N)
    want = gx.expected(epi, c["acc"], c["bias"], rowstat=rs, colsum=cs)
    dfold = (_dev(rs), _dev(cs))
    for tile, ngroups in _tilings(N, K):
        _check(_run(c, epi, M, N, K, tile, ngroups, dfold=dfold), want, epi, _name(epi, tile, ngroups, M, N, K))


@pytest.mark.parametrize("epi", [0, 6])
@pytest.mark.parametrize("M,N,K,walks", [(257 * 256 + 3, 256, 192, ((None, 0),)),
                                         (129 * 256 + 5, 512, 128, ((2, 1), (2, 2)))])
def test_more_tiles_than_workgroups(gpu, M, N, K, walks, epi):
    """More than 256 tiles: the persistent kernel walks several tiles per workgroup, the operand
    stage parity flipping across tiles when the K-step count is odd (K = 192) and at its minimum
    of two steps (K = 128, 1 and 2 XCD groups); every element against one fp64 matmul."""
    c = _case(M, N, K)
    want = gx.expected(epi, c["acc"], c["bias"], c["x"])
    for tile, ngroups in walks:
        _check(_run(c, epi, M, N, K, tile, ngroups), want, epi, _name(epi, tile, ngroups, M, N, K))


@pytest.mark.parametrize("M,W,K", [(129, 512, 512), (257, 768, 3072)])
def test_residual_partials(gpu, M, W, K):
    """reidmi_gemm_f16_resid_partials: the updated x bit-exact, and the 64-column sums of the
    written fp16 values (multiples of 2^-10 below 2^11: an exact fp32 sum) bit-exact.  The centred
    sums of squares stay with test_residual_partials_rowstats' tolerance."""
    L = _lib()
    c = _case(M, W, K)
    want = gx.expected(6, c["acc"], c["bias"], c["x"])
    sums = gx.assert_fp32_exact(want.astype(np.float64).reshape(M, W // 64, 64).sum(2), "sums").astype(np.float32)
    flat = torch.full((2 * GUARD + M * W,), FILL, dtype=torch.float16, device="cuda")
    out = flat[GUARD:GUARD + M * W].view(M, W)
    out.copy_(_dev(c["x"]))
    pst = torch.full((W // 64, M, 2), float("nan"), device="cuda")
    L.call("reidmi_gemm_f16_resid_partials", L.ptr(c["dA"]), K, L.ptr(c["dW"]), K, M, W, K, L.ptr(c["dbias"]),
           L.ptr(out), W, L.ptr(pst), L.stream())
    torch.cuda.synchronize()
    host = flat.cpu().numpy()
    fill = np.float16(FILL)
    assert (host[:GUARD] == fill).all() and (host[GUARD + M * W:] == fill).all(), "a write outside x"
    _check(host[GUARD:GUARD + M * W].reshape(M, W), want, 6, f"x, (M, W, K) = ({M}, {W}, {K})")
    p = pst.cpu().numpy()
    assert np.isfinite(p).all()
    _check(np.ascontiguousarray(p[..., 0].T), sums, 5, f"pstat sums [m][64-column block], (M, W, K) = ({M}, {W}, {K})")


@pytest.mark.parametrize("pad", [0, 3])
@pytest.mark.parametrize("Q,G,D", [(1, 1, 2), (37, 259, 70), (130, 129, 513), (257, 1001, 128)])
def test_distance_form(gpu, Q, G, D, pad):
    """reidmi_distmat_f16 (the fp32 epilogue's distance form, the fp16 copies, the fp32 norms) on
    fp16-representable q and g: (qq + gg) - 2 q.g is exact, so out[:, :G] has the fp64 result's
    bits.  D = 70 and 513 pad K with zero columns, G = 259 and 1001 pad the gallery rows; ldo = G
    and G + 3 between them take the scalar stores (ldo % 4 != 0) and the 16-byte ones; columns
    past G and both guards keep the sentinel."""
    L = _lib()
    q, g = gx.distance_operands(Q, G, D, seed=Q + G + D)
    want = gx.distance_expected(q, g)
    ldo = G + pad
    flat = torch.full((2 * GUARD + Q * ldo,), FILL, device="cuda")
    out = flat[GUARD:GUARD + Q * ldo].view(Q, ldo)
    ws = torch.empty(L.load().reidmi_distmat_f16_workspace_bytes(Q, G, D), device="cuda", dtype=torch.uint8)
    dq, dg = _dev(q), _dev(g)
    L.call("reidmi_distmat_f16", L.ptr(dq), Q, D, L.ptr(dg), G, D, D, L.ptr(out), ldo, L.ptr(ws), ws.numel(),
           L.stream())
    torch.cuda.synchronize()
    host = flat.cpu().numpy()
    body = host[GUARD:GUARD + Q * ldo].reshape(Q, ldo)
    fill = np.float32(FILL)
    assert (host[:GUARD] == fill).all() and (host[GUARD + Q * ldo:] == fill).all(), "a write outside out"
    assert (body[:, G:] == fill).all(), "a write past column G"
    _check(np.ascontiguousarray(body[:, :G]), want, 5, f"(Q, G, D) = ({Q}, {G}, {D}) ldo {ldo}")
