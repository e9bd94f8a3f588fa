"""The exact-arithmetic GEMM helper (tests/gemm_exact.py) on the CPU: its premise and its bite.

For every (K, gain) the GPU grid uses (gemm_exact.GAIN) the conditions the GPU tests rest on:
fp32 accumulation equals the fp64 result exactly in natural and in permuted k order (so the
K-loop's summation order cannot matter), at least 1 % of the fp16 outputs of the plain and the
residual epilogue are inexact and at least 16 are exact ties (so a wrong or a second rounding
shows).  These are conditions, not measurements."""
import numpy as np
import pytest

import gemm_exact as gx

M, N = 257, 256  # the sample per (K, gain): 65 792 outputs


@pytest.fixture(scope="module", params=sorted(gx.GAIN.items()), ids=lambda kg: f"K{kg[0]}-gain{kg[1]}")
def case(request):
    K, gain = request.param
    A, W, bias, x = gx.operands(M, N, K, seed=K, gain=gain)
    return K, A, W, bias, x, gx.accumulate(A, W)


def test_operands_lie_on_the_grid(case):
    K, A, W, bias, x, _ = case
    gain = gx.GAIN[K]
    for t, q, lim in ((A, gain / 8.0, gain), (W, gain / 8.0, gain), (bias, 1 / 64.0, 2), (x, 2.0 ** -10, 4)):
        v = t.astype(np.float64) / q
        assert (v == np.rint(v)).all() and np.abs(t.astype(np.float64)).max() <= lim
    assert A.dtype == W.dtype == x.dtype == np.float16 and bias.dtype == np.float32
    assert np.abs(x.astype(np.float64)).max() < 4
    assert len(np.unique(A.astype(np.float32))) == len(np.unique(W.astype(np.float32))) == 17  # every grid value


def test_fp32_accumulation_is_exact_in_any_order(case):
    K, A, W, bias, _, acc = case
    ref = acc + bias.astype(np.float64)
    perm = np.random.default_rng(K + 1).permutation(K)
    for p in (None, perm, perm[::-1]):
        got = gx.accumulate(A, W, p, np.float32) + bias
        assert got.dtype == np.float32 and np.array_equal(got.astype(np.float64), ref)
    # the strictest order: one k at a time, in fp32, permuted
    a, w = A[:64].astype(np.float32), W[:64].astype(np.float32)
    s = np.zeros((64, 64), np.float32)
    for k in perm:
        s += np.outer(a[:, k], w[:, k])
        assert s.dtype == np.float32
    assert np.array_equal(s.astype(np.float64), acc[:64, :64])


def test_outputs_exercise_the_rounding(case):
    K, A, W, bias, x, acc = case
    v = acc + bias.astype(np.float64)
    for name, val in (("epi 0", v), ("epi 6", x.astype(np.float64) + v)):
        inexact, tie = gx.fp16_inexact_and_ties(val)
        print(f"K {K} gain {gx.GAIN[K]} {name}: {inexact.mean():.2%} inexact, {int(tie.sum())} ties, "
              f"max |v| {np.abs(val).max():.1f}")
        assert inexact.mean() >= 0.01 and tie.sum() >= 16
        assert np.abs(val).max() < 2048
    # a residual epilogue that rounds acc + bias before adding x is told apart
    once = gx.expected(6, acc, bias, x)
    twice = gx.double_rounded_residual(acc, bias, x)
    assert (once != twice).mean() >= 0.01


def test_expected_epilogues(case):
    K, A, W, bias, x, acc = case
    v = acc + bias.astype(np.float64)
    e0, e5, e6, e1 = (gx.expected(e, acc, bias, x) for e in (0, 5, 6, 1))
    assert e0.dtype == np.float16 and e5.dtype == np.float32 and e6.dtype == np.float16 and e1.dtype == np.float64
    assert np.array_equal(e5.astype(np.float64), v)
    assert (np.abs(e0.astype(np.float64) - v) <= 0.5 * gx.ulp16(v)).all()
    assert np.allclose(e1, v * 0.5 * (1 + np.tanh(0.851 * v)), rtol=1e-12, atol=1e-13)
    assert np.array_equal(gx.expected(0, acc), gx.fp16_rne(acc))  # no bias
    rs, cs = gx.fold_operands(M, N, seed=K)
    assert rs.shape == (512, 2) and np.isnan(rs[M:]).all() and np.isfinite(rs[:M]).all()
    f5 = gx.expected(5, acc, bias, rowstat=rs, colsum=cs)
    ref = rs[:M, :1].astype(np.float64) * acc + rs[:M, 1:].astype(np.float64) * cs.astype(np.float64) + bias
    assert np.array_equal(f5.astype(np.float64), ref)
    # the fold's two FMAs in fp32 give the same bits
    t = rs[:M, 1:] * cs[None, :] + bias[None, :]
    got = rs[:M, :1] * acc.astype(np.float32) + t
    assert got.dtype == np.float32 and np.array_equal(got, f5)


def test_fp16_rounding_helpers():
    # ties to even at ulp 2 (2048..4096) and ulp 2^-5 (32..64); the subnormal floor
    v = np.array([2049.0, 2051.0, 2050.0, 32.0 + 1 / 64, 32.0 + 3 / 64, 33.0 + 1 / 128, -2049.0])
    assert gx.fp16_rne(v).astype(np.float64).tolist() == [2048.0, 2052.0, 2050.0, 32.0, 32.0 + 1 / 16, 33.0, -2048.0]
    inexact, tie = gx.fp16_inexact_and_ties(v)
    assert inexact.tolist() == [True, True, False, True, True, True, True]
    assert tie.tolist() == [True, True, False, True, True, False, True]
    assert gx.ulp16(np.array([0.0, 2.0 ** -30, 2.0 ** -14, 1.0, 1.999, 2.0, -1500.0])).tolist() == \
        [2.0 ** -24, 2.0 ** -24, 2.0 ** -24, 2.0 ** -10, 2.0 ** -10, 2.0 ** -9, 1.0]
    assert gx.gelu_bound(np.array([1.0]))[0] == 2.0 ** -11 + 2.0 ** -16


def test_reports_name_the_element():
    want = np.zeros((128, 128), np.float16)
    assert gx.mismatch_report(want.copy(), want) is None
    got = want.copy()
    got[5::16, 64:128] = 1  # one lane of each row group, the second wave's columns
    msg = gx.mismatch_report(got, want)
    assert "(m, n) = (5, 64)" in msg and "512 of 16384" in msg
    assert "only residues [5] mod 16" in msg and "columns 64..127: all 16 residues" in msg
    assert gx.mismatch_report(np.array([[-0.0]], np.float32), np.array([[0.0]], np.float32)) is not None
    ref = np.ones((4, 4))
    assert gx.bound_report(ref.astype(np.float16), ref, gx.gelu_bound(ref)) is None
    bad = ref.astype(np.float16)
    bad[2, 3] = 1.002
    assert "(m, n) = (2, 3)" in gx.bound_report(bad, ref, gx.gelu_bound(ref))
    bad[1, 1] = np.nan
    assert "2 of 16" in gx.bound_report(bad, ref, gx.gelu_bound(ref))


def test_distance_expectation():
    q, g = gx.distance_operands(37, 259, 70, seed=3)
    d = gx.distance_expected(q, g)
    assert d.dtype == np.float32 and d.shape == (37, 259) and (d >= 0).all()
    assert np.array_equal(q.astype(np.float16).astype(np.float32), q)
    brute = ((q[:, None, :].astype(np.float64) - g[None, :, :]) ** 2).sum(2)
    assert np.array_equal(d.astype(np.float64), brute)
    # fp32 evaluation in the kernel's form gives the same bits
    qq, gg = (q * q).sum(1), (g * g).sum(1)
    assert np.array_equal((qq[:, None] + gg[None, :]) - np.float32(2) * (q @ g.T), d)
