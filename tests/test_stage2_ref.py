"""tests/stage2_ref.py, the long-double restatement of stage 2 that referees the GPU shape
tests, checked on the CPU: against the oracle, the committed golden arrays and published
polars values, and its error bounds against what f64 arithmetic can deliver."""
import numpy as np
import pytest
from numpy.lib.stride_tricks import sliding_window_view

import stage2_cases
import stage2_ref
from parity import compare


def _small_panel(seed):
    """[60][12]: ABSENT runs, NULLs, NaN, +-inf, a constant column, a stock listed late and
    a stock present every 9th day."""
    val, state = stage2_cases.panel(1, 60, 12, seed, absent=0.08)
    val, state = val[0], state[0]
    state[10:25, 1] = 0
    state[:40, 2] = 0
    state[:, 4] = 0
    state[::9, 4] = 2
    val[30, 7], state[30, 7] = -np.inf, 2
    val[31, 8], val[33, 8] = np.inf, -np.inf
    state[31:34, 8] = 2
    val[12, 9], state[12, 9] = np.nan, 2
    val[13:20, 9], state[13:20, 9] = 7.0, 2  # a constant window right after a NaN
    state[12, 10] = 1
    val[13:20, 10], state[13:20, 10] = -3.5, 2  # ... and right after a NULL
    return val, state


@pytest.mark.parametrize("N", [1, 2, 5, 20, 61])
def test_ref_agrees_with_oracle(N):
    import mff_oracle as O
    bad = []
    for seed in (1, 2):
        val, state = _small_panel(seed)
        ref = stage2_ref.rolling_all(val, state, N)
        for meth in stage2_ref.METHODS:
            ov, os_ = O.oracle_stage2(val, state, N, meth)
            rv, rs, rb = ref[meth]
            assert np.array_equal(rs, os_), (N, meth)
            assert (rv[rs != 2] == 0).all() and (rb[rs != 2] == 0).all()
            bad += compare(rv, rs, ov, os_, f"N{N}/{meth}", atol=1e-9)
            # constant and non-finite windows: exact, bound 0
            exact = (rs == 2) & (rb == 0)
            assert np.array_equal(rv[exact], ov[exact], equal_nan=True), (N, meth)
            if meth != "o" and N <= 20:
                assert exact.any()
            if N > 60:  # longer than the panel: no window at all
                assert meth == "o" or not (rs == 2).any()
    assert not bad, "\n".join(bad[:20])


def test_ref_shapes_and_method_names():
    val, state = stage2_cases.panel(2, 30, 5, 3)
    v3, s3, b3 = stage2_ref.rolling(val, state, 4, "z")
    v2, s2, b2 = stage2_ref.rolling(val[1], state[1], 4, "z")
    assert v3.shape == val.shape and v3.dtype == np.float64 and s3.dtype == np.uint8
    assert np.array_equal(v3[1], v2, equal_nan=True) and np.array_equal(s3[1], s2) and np.array_equal(b3[1], b2)
    assert not np.array_equal(v3[0], v3[1], equal_nan=True)
    with pytest.raises(ValueError):
        stage2_ref.rolling(val, state, 4, "mean")


def test_ref_agrees_with_golden():
    from golden.make_golden import STAGE23_FACTORS, load
    import mff_oracle as O
    _, z = load("panel_ragged.npz")
    bad = []
    for nm in STAGE23_FACTORS:
        i = O.ORACLE_NAMES.index(nm)
        ref = stage2_ref.rolling_all(z["val"][i], z["state"][i], 3)
        for meth in stage2_ref.METHODS:
            rv, rs, _ = ref[meth]
            bad += compare(rv, rs, z[f"s2_{nm}_{meth}_val"], z[f"s2_{nm}_{meth}_state"], f"{nm}/{meth}", atol=1e-12)
    assert not bad, "\n".join(bad[:20])


def test_ref_matches_polars_rendered_rolling_var():
    """pl.Series([1.0, 3.0, 1.0, 4.0]).rolling_var(window_size=2, min_samples=1) = [null, 2.0,
    2.0, 4.5] (ddof 1): the ddof-0 std over 2 days is null, then sqrt(var / 2)."""
    val = np.array([1.0, 3.0, 1.0, 4.0]).reshape(4, 1)
    rv, rs, rb = stage2_ref.rolling(val, np.full((4, 1), 2, np.uint8), 2, "std")
    assert rs[:, 0].tolist() == [1, 2, 2, 2]
    assert np.allclose(rv[1:, 0], np.sqrt(np.array([2.0, 2.0, 4.5]) / 2), rtol=1e-14, atol=0)
    assert (rb[1:, 0] > 0).all() and (rb[1:, 0] < 1e-13).all()


def test_fraction_fallback_agrees_with_longdouble(monkeypatch):
    """The exact-rational path (hosts whose long double is f64) gives the long-double path's
    values to a rounding, far inside the bound, and the same states and bounds."""
    val, state = _small_panel(5)
    a = stage2_ref.rolling_all(val, state, 5)
    monkeypatch.setattr(stage2_ref, "LONGDOUBLE_OK", False)
    b = stage2_ref.rolling_all(val, state, 5)
    for meth in ("m", "z", "std"):
        bad, ratio = stage2_ref.check(b[meth][0], b[meth][1], a[meth], meth)
        assert not bad and ratio < 0.02, (meth, ratio, bad)
        assert np.allclose(a[meth][2], b[meth][2], rtol=1e-12, atol=0)


def _f64_forms(W):
    """Two f64 computations of finite windows W [M][N], both shifted by a window member:
    the one-pass form of the register kernel's window_stats (shift by the oldest value,
    terms summed oldest to newest, var = (sum d^2 - sum d * mean_d) / N) and a two-pass."""
    N = W.shape[1]
    x0 = W[:, 0]
    s1, s2 = np.zeros(len(W)), np.zeros(len(W))
    for k in range(N):
        dk = W[:, k] - x0
        s1 = s1 + dk
        s2 = s2 + dk * dk
    m1 = s1 * (1.0 / N)
    mean = x0 + m1
    with np.errstate(all="ignore"):
        sd = np.sqrt((s2 - s1 * m1) * (1.0 / N))
        yield "one-pass", mean, sd, (W[:, -1] - mean) / sd
        y = W - x0[:, None]
        my = y.sum(axis=1) / N
        sd2 = np.sqrt(((y - my[:, None]) ** 2).sum(axis=1) / N)
        yield "two-pass", x0 + my, sd2, (W[:, -1] - (x0 + my)) / sd2


@pytest.mark.parametrize("N", [2, 3, 5, 20, 64, 65, 120, 250])
def test_bound_is_not_tighter_than_f64_allows(N):
    """f64 computations of the shifted forms stay inside ``bound`` against the long-double
    reference, on the data the GPU tests use (scales 1e-3 / 1 / 1e5, ties, the trend
    column, the 1e15 outlier entering and leaving)."""
    val, state = stage2_cases.panel(1, 320, 40, 11 * N, absent=0.03, null=0.2 / N, nan=0.1 / N)
    val, state = val[0], state[0]
    ref = stage2_ref.rolling_all(val, state, N)
    worst = {}
    n_checked = 0
    for s in range(val.shape[1]):
        idx = np.flatnonzero(state[:, s] != 0)
        x = np.where(state[idx, s] == 1, 0.0, val[idx, s])
        if idx.size < N:
            continue
        W = sliding_window_view(x, N)
        d = idx[N - 1:]
        gen = ref["m"][2][d, s] > 0  # finite, non-constant, no NULL
        assert np.isfinite(W[gen]).all()
        n_checked += int(gen.sum())
        for form, mean, sd, z in _f64_forms(W[gen]):
            for meth, got in (("m", mean), ("std", sd), ("z", z)):
                rv, _, rb = ref[meth]
                ratio = np.abs(got - rv[d[gen], s]) / rb[d[gen], s]
                worst[form, meth] = max(worst.get((form, meth), 0.0), float(ratio.max(initial=0.0)))
    print(f"N={N}: {n_checked} windows, worst |f64 - ref| / bound:",
          ", ".join(f"{k[0]} {k[1]} {v:.3f}" for k, v in sorted(worst.items())))
    assert n_checked > 1000
    assert all(v <= 1.0 for v in worst.values()), worst
