"""tests/prefilter_ref.py on the CPU: the adversarial inputs have teeth.

Conditions on the inputs, checked with the float64 model alone (no kernel runs here): the aligned
inputs use almost all of the pair bound e, random rows a fifth of it; the bound holds in the model
for every builder; `planted` is decided correctly by the documented bound and wrongly by half of it.
tests/test_gpu_prefilter_bound.py rests on these."""
import numpy as np
import pytest

import prefilter_ref as pr

N = 300


def _reach(name, f):
    v = pr.reach(f)
    print(f"reach {name}: max |d~ - d| / e = {v:.4f}")
    return v


@pytest.mark.parametrize("D,floor", [(128, 0.9), (256, 0.9), (1792, 0.75)])
def test_aligned_rows_reach_the_bound(D, floor):
    """Measured at N = 300: 0.965 / 0.950 / 0.803 (the diagonal pairs: cos = 1)."""
    v = _reach(f"aligned(down) D={D}", pr.aligned("down")(N, D, 1))
    assert floor <= v <= 1.0


@pytest.mark.parametrize("D", [128, 1792])
def test_random_rows_stay_far_below_the_bound(D):
    """Documents the gap the outcome tests leave; not a claim about the kernel."""
    assert _reach(f"random unit rows D={D}", pr.random_unit(N, D, 2)) <= 0.25


@pytest.mark.parametrize("name,build,D", [
    ("aligned(up)", pr.aligned("up"), 128), ("aligned(up)", pr.aligned("up"), 130),
    ("aligned(mix)", pr.aligned("mix"), 130), ("aligned(mix)", pr.aligned("mix"), 256),
    ("aligned(down)", pr.aligned("down"), 130), ("subnormal", pr.subnormal, 128), ("subnormal", pr.subnormal, 130),
    ("mixed_norm", pr.mixed_norm, 128), ("mixed_norm", pr.mixed_norm, 1792), ("planted(10)", pr.planted(10), 128)])
def test_the_bound_holds_in_the_model_for_every_builder(name, build, D):
    f = build(N, D, 3)
    assert f.dtype == np.float32 and f.shape == (N, D)
    assert np.array_equal(f, build(N, D, 3))  # deterministic
    v = _reach(f"{name} D={D}", f)
    assert v <= 1.0
    if name != "planted(10)":
        assert v >= 0.5  # every adversarial input uses at least half of the bound


def test_aligned_elements_round_as_stated():
    for mode, way in (("down", -1), ("up", 1)):
        f = pr.aligned(mode)(64, 130, 4).astype(np.float64)
        h = f.astype(np.float32).astype(np.float16).astype(np.float64)
        rel = (h - f) / f  # (the sign of f cancels)
        assert (np.sign(rel) == way).all()
        assert (np.abs(rel) > 2.0 ** -11 * 0.98).all() and (np.abs(rel) < 2.0 ** -11).all()
    f = pr.aligned("mix")(64, 128, 4).astype(np.float64)
    h = f.astype(np.float32).astype(np.float16).astype(np.float64)
    assert ((h - f) / f < 0)[:32].all() and ((h - f) / f > 0)[32:].all()


K = 10


def _planted_sets(scale):
    f = pr.planted(K)(N, 128, 5)
    groups, q, A, B, far = pr.planted_layout(N, K)
    d = pr.model_exact(f)
    hi, w = pr.model_bounds(f, scale=scale)
    cand = pr.model_candidates(hi, w, K + 1)  # all-pairs form: the row itself is its nearest item
    top = np.argsort(d, axis=1, kind="stable")[:, :K + 1]
    return f, groups, q, A, B, d, hi, cand, top


def test_planted_is_what_it_says():
    f, groups, q, A, B, d, hi, cand, top = _planted_sets(1.0)
    nrm = np.sqrt((f.astype(np.float64) ** 2).sum(1))
    assert groups == N // (1 + 3 * K) >= 8
    far = pr.planted_layout(N, K)[4]
    assert nrm.max() == nrm[B].max() < 1.001 and nrm[far].max() < 1.0  # no row widens the planted rows' bound
    dt = pr.model_dtilde(f)
    for g in range(groups):
        dA, dB = d[q[g], A[g]], d[q[g], B[g]]
        assert 0.9e-4 < dB.min() - dA.max() < 1.2e-4           # every A truly nearer than every B
        assert dt[q[g], B[g]].max() < dt[q[g], A[g]].min()     # the fp16 ranking inverts them
        assert set(top[q[g]]) == {q[g], *A[g]}
        rest = np.setdiff1d(np.arange(N), np.r_[q[g], A[g], B[g]])
        assert d[q[g], rest].min() > 0.9                       # everything else is far


def test_planted_is_decided_by_the_documented_bound():
    f, groups, q, A, B, d, hi, cand, top = _planted_sets(1.0)
    assert (d <= hi).all()
    rows = np.arange(N)[:, None]
    assert cand[rows, top].all()                # every row's true top-K is among its candidates
    assert cand[q].sum(1).max() < 256           # short lists: the rows are decided, not sent on
    print("planted: candidates per query row", cand[q].sum(1).min(), "..", cand[q].sum(1).max())


def test_planted_defeats_a_halved_bound():
    f, groups, q, A, B, d, hi, cand, top = _planted_sets(0.5)
    lost = np.array([(~cand[i, top[i]]).sum() for i in q])
    print("planted, e x 0.5: true top-K items lost per query row", lost)
    assert (lost >= 1).sum() >= (len(q) + 1) // 2
