"""The fp16 pre-filter's pair bound in plain numpy (float64), and inputs that reach it.

The re-rank's R2 pre-filter and the pre-filtered search discard pairs on the strength of
    |d~_ij - d_ij| <= e_ij,
d~ the distance from the fp16 MFMA product, d the exact fp32 chain distance, e the error model
written above rank_select1_kernel (csrc/prefilter.hip).  This module restates that model from its
documentation (it calls nothing in the library) and builds deterministic inputs whose fp16 rounding
errors all have one sign, so that |d~ - d| comes close to e; on random data the errors cancel and
|d~ - d| / e stays below 0.2 (tests/test_prefilter_ref.py shows both).

Model:   consts, e, width, model_dtilde, model_exact, model_bounds, model_candidates, reach.
Inputs:  aligned, subnormal, mixed_norm, planted (+ planted_layout), random_unit; each
         (N, D, seed) -> float32 [N][D].
"""
import numpy as np

# fp16: 10 mantissa bits.  A value 2^k (1 + 2^-11 (1 - 2^-7)) lies just below the midpoint of the grid
# points 2^k and 2^k (1 + 2^-10) and rounds DOWN by almost half an ulp, at the mantissa (1.0) where
# half an ulp is the largest relative error (2^-11); with (1 + 2^-7) it lies just above and rounds UP.
# Both factors are exact in fp32 (18 fractional bits).
_DOWN = 1.0 + 2.0 ** -11 * (1.0 - 2.0 ** -7)
_UP = 1.0 + 2.0 ** -11 * (1.0 + 2.0 ** -7)


# ------------------------------------------------------------------------------ the model
def consts(D):
    """(c_rel, c_abs, c_d) as documented above rank_select1_kernel: fp16 operand rounding 2^-11
    relative + 2^-25 absolute per element, both accumulation chains, the final fma."""
    c_rel = 2.0 * (2.0 ** -10 + 2.0 ** -22 + 2.02 * D * 2.0 ** -24) + 2.02 * 2.0 ** -23
    c_abs = 2.01 * 2.0 ** -25 * np.sqrt(float(D))
    c_d = D * 2.0 ** -49
    return c_rel, c_abs, c_d


def e(s_i, s_j, n_i, n_j, D):
    """The pair error: 1.01 (c_rel n_i n_j + 2^-23 (s_i + s_j) + c_abs (n_i + n_j) + D 2^-49)."""
    c_rel, c_abs, c_d = consts(D)
    s_i, s_j, n_i, n_j = (np.asarray(a, np.float64) for a in (s_i, s_j, n_i, n_j))
    return 1.01 * (c_rel * n_i * n_j + 2.0 ** -23 * (s_i + s_j) + c_abs * (n_i + n_j) + c_d)


def width(s_i, n_i, n_max, s_max, D, scale=1.0):
    """rr_width's formula: the row's bound width from the largest norm and squared norm over the
    items, 2 e (1 + 2^-10) + 2^-20 (s_i + s_max + e) with e = e(s_i, s_max, n_i, n_max).
    scale multiplies e (a deliberately wrong bound, for the tests of the inputs' bite)."""
    s_i = np.asarray(s_i, np.float64)
    em = scale * e(s_i, s_max, n_i, n_max, D)
    return 2.0 * em * (1.0 + 2.0 ** -10) + 2.0 ** -20 * (s_i + float(s_max) + em)


def _sq(f):
    f = np.asarray(f, np.float64)
    return (f * f).sum(1)


def model_dtilde(f, g=None):
    """d~ of the rows of f against the rows of g (default f): the dot products of the fp16-rounded
    rows accumulated in float64, and the squared norms of the unrounded rows."""
    g = f if g is None else g
    a = np.asarray(f, np.float32).astype(np.float16).astype(np.float64)
    b = np.asarray(g, np.float32).astype(np.float16).astype(np.float64)
    return _sq(f)[:, None] + _sq(g)[None, :] - 2.0 * (a @ b.T)


def model_exact(f, g=None):
    """The distances of the unrounded rows in float64."""
    g = f if g is None else g
    a, b = np.asarray(f, np.float64), np.asarray(g, np.float64)
    return _sq(f)[:, None] + _sq(g)[None, :] - 2.0 * (a @ b.T)


def pair_e(f, g=None):
    """e of every pair (rows of f, rows of g) from float64 norms."""
    g = f if g is None else g
    sf, sg = _sq(f), _sq(g)
    return e(sf[:, None], sg[None, :], np.sqrt(sf)[:, None], np.sqrt(sg)[None, :], np.shape(f)[1])


def reach(f):
    """max over all pairs of |d~ - d| / e: how much of the bound the input uses (1: all of it)."""
    return float((np.abs(model_dtilde(f) - model_exact(f)) / pair_e(f)).max())


def model_bounds(f, g=None, scale=1.0):
    """(hi [N][M], w [N]) of the model: hi = d~ + scale e, w = width(..., scale) against g's largest
    norms, as the selection kernels hold them (lo = hi - w)."""
    g = f if g is None else g
    sf, sg = _sq(f), _sq(g)
    hi = model_dtilde(f, g) + scale * pair_e(f, g)
    w = width(sf, np.sqrt(sf), np.sqrt(sg.max()), sg.max(), np.shape(f)[1], scale)
    return hi, w


def model_candidates(hi, w, K):
    """Per row the candidate set {j : hi_j - w <= thr(K-th smallest hi)} as a boolean [N][M], with
    rank_select1_kernel's thr(tau) = tau + |tau| 2^-21 + 1e-37."""
    hi = np.asarray(hi, np.float64)
    tau = np.partition(hi, K - 1, axis=1)[:, K - 1]
    thr = tau + np.abs(tau) * 2.0 ** -21 + 1e-37
    return hi - np.asarray(w, np.float64)[:, None] <= thr[:, None]


# ------------------------------------------------------------------------------ the inputs
def random_unit(N, D, seed):
    """Random L2-normalised rows: the data the outcome tests use; rounding errors cancel."""
    x = np.random.default_rng(seed).standard_normal((N, D))
    return (x / np.linalg.norm(x, axis=1, keepdims=True)).astype(np.float32)


def aligned(mode):
    """Builder of rows whose every element rounds the same way in fp16 by almost half an ulp:
    row_sign 2^k _DOWN ("down"), _UP ("up"), or the first half of the rows down and the second
    half up ("mix"); k uniform in -6..-3 per element."""
    assert mode in ("down", "up", "mix")

    def build(N, D, seed):
        r = np.random.default_rng(seed)
        k = r.integers(-6, -2, size=(N, D))
        sign = r.choice([-1.0, 1.0], size=(N, 1))
        fac = np.full((N, 1), _DOWN if mode != "up" else _UP)
        if mode == "mix":
            fac[N // 2:] = _UP
        x = (sign * fac * 2.0 ** k).astype(np.float32)
        assert np.array_equal(x.astype(np.float64), sign * fac * 2.0 ** k)  # exact in fp32
        return x

    return build


def subnormal(N, D, seed):
    """|x| = (m + 1/2 - 2^-7) 2^-24, m in 128..383: inside 2^-17 [1, 3), every element an fp16
    subnormal (spacing 2^-24) that rounds down by almost 2^-25, the absolute error the c_abs term
    allows per element.  Row signs are random, so dot products of both signs occur: an MFMA that
    flushed subnormal operands would give d~ = s_i + s_j, off by 2 |dot| >> e in both directions."""
    r = np.random.default_rng(seed)
    m = r.integers(128, 384, size=(N, D)).astype(np.float64)
    sign = r.choice([-1.0, 1.0], size=(N, 1))
    v = sign * (m + 0.5 - 2.0 ** -7) * 2.0 ** -24
    x = v.astype(np.float32)
    assert np.array_equal(x.astype(np.float64), v)
    h = np.abs(x.astype(np.float16).astype(np.float64))
    assert (h > 0).all() and (h < 2.0 ** -14).all() and np.array_equal(h, m * 2.0 ** -24)
    return x


def mixed_norm(N, D, seed):
    """aligned("down") rows, row r scaled by 2^m, m uniform in -5..5: norms spread over 2^10, so
    the n_i n_j term of e is far below the row width's n_i n_max for most pairs."""
    x = aligned("down")(N, D, seed)
    m = np.random.default_rng(seed + 1000).integers(-5, 6, size=(N, 1))
    return (x * 2.0 ** m).astype(np.float32)


def _hadamard(n):
    h = np.ones((1, 1))
    while h.shape[0] < n:
        h = np.block([[h, h], [h, -h]])
    return h


def planted_layout(N, K, D=128):
    """Row indices of planted(K)(N, D, .): (groups, q [groups], A [groups][K], B [groups][2K],
    far [rest]).  Group g is rows g (1 + 3K) .. : its query, its K A rows, its 2K B rows."""
    per = 1 + 3 * K
    groups = min(D // 2, N // per)
    base = np.arange(groups)[:, None] * per
    q = base[:, 0].copy()
    A = base + 1 + np.arange(K)[None, :]
    B = base + 1 + K + np.arange(2 * K)[None, :]
    return groups, q, A, B, np.arange(groups * per, N)


def planted(K):
    """Builder of an input on which the fp16 ranking inverts the true one, at D = 128 (halves S1 =
    dims 0..63, S2 = 64..127), 2K <= 64.  Group g has a sign pattern h_g (a row of the 64 x 64
    Hadamard matrix, the same on both halves; patterns of different groups are orthogonal) and
      query  q   = h_g 2^-4 (_DOWN on S1, _UP on S2)          |q|^2 = 1/2, equal mass on both halves
      A_a        = h_g 2^-3 _DOWN on S1, 0 on S2              |A| = 1,  q.A = 1/2,  d = 1/2
      B_b        = h_g 2^-3 _UP on S2, 0 on S1                |B| = 1,  q.B = 1/2,  d = 1/2
    Perturbations by whole fp16 ulps (the rounding direction and size stay): A_a has element a moved
    one ulp (2^-13) away from q's, d_A = 1/2 + 2^-16 (1 + o(1)); B_b has element 64 + b moved 8
    ulps, d_B = 1/2 + 8 2^-16: every A row is truly nearer than every B row by 7 2^-16 ~ 1.07e-4.
    fp16 rounds q and A down on S1 (the product shrinks by 2^-10, d~_A ~ d_A + 2^-9 q.A) and q and B
    up on S2 (d~_B ~ d_B - 2^-9 q.B): d~_B < d~_A by ~ 2^-9 - 1.07e-4 ~ 1.85e-3, while e ~ 1.45e-3
    covers each error.  Rows of other groups are at d = 3/2 (A, B) or 1 (queries); the remaining
    rows are random unit rows (d ~ 3/2 +- 0.4), so the candidate lists stay short.  No norm exceeds
    1 = |A|: the row width (from n_max) is then 2 e of the planted pairs, not more, which a halved
    bound needs to lose them (2^-8 n_q (cos n_A - 0.52 n_max) > 1.07e-4 with cos = 2^-1/2)."""
    assert 1 <= K <= 32

    def build(N, D, seed):
        assert D == 128
        groups, q, A, B, far = planted_layout(N, K, D)
        assert groups >= 1
        h = _hadamard(64)
        x = np.zeros((N, D))
        ulp = 2.0 ** -13  # fp16 spacing in [2^-3, 2^-2)
        for g in range(groups):
            x[q[g], :64] = h[g] * 2.0 ** -4 * _DOWN
            x[q[g], 64:] = h[g] * 2.0 ** -4 * _UP
            for a in range(K):
                x[A[g, a], :64] = h[g] * 2.0 ** -3 * _DOWN
                x[A[g, a], a] += h[g, a] * ulp
            for b in range(2 * K):
                x[B[g, b], 64:] = h[g] * 2.0 ** -3 * _UP
                x[B[g, b], 64 + b] += h[g, b] * 8 * ulp
        if len(far):
            r = random_unit(len(far), D, seed).astype(np.float64)
            x[far] = (r * (1.0 - 2.0 ** -12)).astype(np.float32)  # norms below |A|
        out = x.astype(np.float32)
        assert np.array_equal(out[:groups * (1 + 3 * K)].astype(np.float64), x[:groups * (1 + 3 * K)])
        return out

    return build
