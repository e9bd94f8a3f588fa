"""Exact-arithmetic operands for the fp16 GEMM tests, and the bits the GEMM must produce from them.

Every operand lies on a dyadic grid coarse enough that each product, each partial sum in any
order of k and each epilogue intermediate is exactly representable in fp32.  The fp32
accumulator is then the same whatever the K-loop's summation order, and the expected output
follows from an fp64 evaluation and one defined rounding: a wrong element, a dropped or doubled
k-slice, a leaked padding row, a bias or colsum shifted by a column, a second rounding or a tie
rounded the wrong way is a bit mismatch at a named (m, n).

  A [M][K], W [N][K]   fp16, gain * i / 8 with integer |i| <= 8, gain a power of two
  bias [N]             fp32, multiples of 1/64, |b| <= 2
  x [M][N]             fp16 residual, multiples of 2^-10, |x| < 4 (even multiples from 2 up: fp16
                       holds 11 significant bits)
  rowstat [Mp][2]      fp32 (rstd, shift), rstd in {1/4, 1/2, 1, 2}, shift multiples of 1/8,
                       |shift| <= 2; Mp = round_up(M, 256), entries past M are NaN
  colsum [N]           fp32, multiples of 1/8, |s| <= 4

Products are multiples of q = gain^2 / 64 and at most gain^2, so every partial sum is a multiple
of q below K * 64 * q: 18 significant bits at K = 3072.  numpy only; no GPU.
"""
import numpy as np

# gain per K of the GPU grid (tests/test_gpu_gemm_exact.py), chosen so that at least 1 % of the
# fp16 outputs are inexact and at least 16 are exact ties (tests/test_gemm_exact_ref.py checks
# both): with quantum 1/64 an output is inexact in fp16 only from |v| >= 32, and |acc| has the
# standard deviation 0.375 gain^2 sqrt(K).  All magnitudes stay below 2^11.
GAIN = {64: 4, 128: 4, 192: 4, 256: 4, 512: 2, 704: 2, 3072: 1}


def round_up(v, m):
    return (v + m - 1) // m * m


def assert_fp32_exact(v, what):
    """Every element of the fp64 array is an fp32 number (24 significant bits, normal range)."""
    v = np.asarray(v, np.float64)
    ok = v.astype(np.float32).astype(np.float64) == v
    assert ok.all(), f"{what}: {int((~ok).sum())} values need more than 24 significant bits"
    return v


def _to_f16(v, what):
    h = np.asarray(v, np.float64).astype(np.float16)
    assert (h.astype(np.float64) == v).all(), f"{what}: not representable in fp16"
    return h


def operands(M, N, K, seed, gain):
    """(A, W, bias, x) on the exact grid (see the module text)."""
    assert gain in (1, 2, 4, 8) and K * 64 < 2 ** 24
    r = np.random.default_rng(seed)
    A = _to_f16(r.integers(-8, 9, (M, K)) * (gain / 8.0), "A")
    W = _to_f16(r.integers(-8, 9, (N, K)) * (gain / 8.0), "W")
    bias = (r.integers(-128, 129, N) / 64.0).astype(np.float32)
    xi = r.integers(-4095, 4096, (M, N))
    xi = np.where(np.abs(xi) >= 2048, np.sign(xi) * (np.abs(xi) & ~1), xi)
    x = _to_f16(xi / 1024.0, "x")
    return A, W, bias, x


def fold_operands(M, N, seed):
    """(rowstat [round_up(M, 256)][2] with NaN past M, colsum [N]) for the LayerNorm fold."""
    r = np.random.default_rng(seed)
    rs = np.full((round_up(M, 256), 2), np.nan, np.float32)
    rs[:M, 0] = r.choice(np.array([0.25, 0.5, 1.0, 2.0], np.float32), M)
    rs[:M, 1] = r.integers(-16, 17, M) / 8.0
    colsum = (r.integers(-32, 33, N) / 8.0).astype(np.float32)
    return rs, colsum


def accumulate(A, W, perm=None, dtype=np.float64):
    """A . W^T in `dtype`, optionally with the k axis permuted (the order-independence check)."""
    a, w = A.astype(dtype), W.astype(dtype)
    if perm is not None:
        a, w = np.ascontiguousarray(a[:, perm]), np.ascontiguousarray(w[:, perm])
    return a @ w.T + dtype(0)  # + 0: a zero sum is +0, as from a +0 accumulator


def fp16_rne(v):
    """One round-to-nearest-even of exact fp64 values to fp16 (numpy converts directly)."""
    return np.asarray(v, np.float64).astype(np.float16)


def expected(epi, acc, bias=None, x=None, rowstat=None, colsum=None):
    """What the GEMM must write for the fp64 accumulator `acc` (accumulate()):
    epi 0: fp16 bits of v;  5: fp32 bits of v;  6: fp16 bits of x + v (one rounding);
    epi 1: the fp64 value v * sigmoid(1.702 v), not rounded (for gelu_bound());
    v = acc + bias, or with the fold rstd_m * acc + (shift_m * colsum_n + bias_n)."""
    M = acc.shape[0]
    v = assert_fp32_exact(acc, "acc")
    if rowstat is not None:
        rstd = rowstat[:M, 0].astype(np.float64)[:, None]
        shift = rowstat[:M, 1].astype(np.float64)[:, None]
        t = assert_fp32_exact(shift * colsum.astype(np.float64)[None, :] + bias.astype(np.float64)[None, :], "fold term")
        v = assert_fp32_exact(rstd * v + t, "folded value")
    elif bias is not None:
        v = assert_fp32_exact(v + bias.astype(np.float64)[None, :], "acc + bias")
    assert np.abs(v).max(initial=0.0) < 2048.0, "value beyond 2^11"
    if epi == 0:
        return fp16_rne(v)
    if epi == 5:
        return v.astype(np.float32)
    if epi == 6:
        return fp16_rne(assert_fp32_exact(x.astype(np.float64) + v, "x + acc + bias"))
    if epi == 1:
        with np.errstate(over="ignore"):
            return v / (1.0 + np.exp(-1.702 * v))
    raise ValueError(epi)


def double_rounded_residual(acc, bias, x):
    """The wrong residual epilogue: acc + bias rounded to fp16 before x is added."""
    v = acc + bias.astype(np.float64)[None, :]
    return fp16_rne(fp16_rne(v).astype(np.float64) + x.astype(np.float64))


def fp16_inexact_and_ties(v):
    """(inexact, tie) masks of exact fp64 values under rounding to fp16."""
    v = np.asarray(v, np.float64)
    h = fp16_rne(v)
    hf = h.astype(np.float64)
    inexact = hf != v
    other = np.nextafter(h, np.where(v > hf, np.float16(np.inf), np.float16(-np.inf)).astype(np.float16))
    tie = inexact & (np.abs(v - hf) == np.abs(other.astype(np.float64) - v))
    return inexact, tie


def ulp16(ref):
    """Spacing of fp16 at |ref|, floored at the subnormal spacing 2^-24."""
    ref = np.asarray(ref, np.float64)
    _, e = np.frexp(np.abs(ref))  # |ref| = m 2^e, m in [0.5, 1)
    return np.ldexp(1.0, np.where(ref == 0, -14, np.maximum(e - 1, -14)) - 10)


def gelu_bound(ref):
    """|got - ref| allowed for the QuickGELU epilogue: the final fp16 rounding, 0.5 ulp16(ref),
    plus 2^-16 |ref| for the fp32 evaluation x / (1 + 2^(-1.702 log2(e) x)): the rounding of the
    exponent (|y| <= ~220 where the result is not yet 0) and exp2 / rcp at about 1 ulp each come to
    about 5e-6 relative; 2^-16 is three times that."""
    ref = np.asarray(ref, np.float64)
    return 0.5 * ulp16(ref) + 2.0 ** -16 * np.abs(ref)


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view({2: np.uint16, 4: np.uint32}[a.dtype.itemsize])


def _residues(idx, mod):
    r = np.unique(idx % mod)
    return f"all {mod} residues" if len(r) == mod else f"only residues {r.tolist()} mod {mod}"


def mismatch_report(got, want):
    """None when `got` has the bits of `want`; otherwise a message with the first (m, n), the
    number of mismatches and which residues modulo 16 and 64 the wrong rows and columns take
    (a lane group, a wave's 64 columns, a fragment)."""
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, (got.shape, want.shape, got.dtype, want.dtype)
    bad = _bits(got) != _bits(want)
    if not bad.any():
        return None
    rows, cols = np.nonzero(bad)
    m, n = int(rows[0]), int(cols[0])
    return (f"{len(rows)} of {bad.size} elements differ; first at (m, n) = ({m}, {n}): got {got[m, n]!r} "
            f"({int(_bits(got)[m, n]):#x}), expected {want[m, n]!r} ({int(_bits(want)[m, n]):#x}); "
            f"rows {int(rows.min())}..{int(rows.max())}: {_residues(rows, 16)}, {_residues(rows, 64)}; "
            f"columns {int(cols.min())}..{int(cols.max())}: {_residues(cols, 16)}, {_residues(cols, 64)}")


def bound_report(got, ref, bound):
    """None when |got - ref| <= bound everywhere; otherwise the worst element."""
    err = np.abs(np.asarray(got, np.float64) - ref)
    bad = ~(err <= bound)  # a NaN fails
    if not bad.any():
        return None
    ratio = np.where(bad, err / bound, 0.0)
    m, n = np.unravel_index(np.nanargmax(np.where(np.isnan(ratio), np.inf, ratio)), ratio.shape)
    return (f"{int(bad.sum())} of {bad.size} elements beyond the bound; worst at (m, n) = ({m}, {n}): got "
            f"{got[m, n]!r}, reference {ref[m, n]!r}, |err| {err[m, n]:.6g} = {err[m, n] / bound[m, n]:.3f} x bound")


def distance_operands(Q, G, D, seed):
    """q [Q][D], g [G][D] fp32 with entries i / 8, |i| <= 8: fp16-representable, so the fp16
    copies, the fp32 squared norms and (qq + gg) - 2 q.g are all exact."""
    r = np.random.default_rng(seed)
    q = (r.integers(-8, 9, (Q, D)) / 8.0).astype(np.float32)
    g = (r.integers(-8, 9, (G, D)) / 8.0).astype(np.float32)
    return q, g


def distance_expected(q, g):
    """fp32 bits of ||q_i||^2 + ||g_j||^2 - 2 q_i . g_j, evaluated in fp64 (each step exact in fp32)."""
    qd, gd = q.astype(np.float64), g.astype(np.float64)
    qq = assert_fp32_exact((qd * qd).sum(1), "qq")
    gg = assert_fp32_exact((gd * gd).sum(1), "gg")
    s = assert_fp32_exact(qq[:, None] + gg[None, :], "qq + gg")
    dot = assert_fp32_exact(qd @ gd.T + 0.0, "q.g")
    return assert_fp32_exact(s - 2.0 * dot, "distance").astype(np.float32)
