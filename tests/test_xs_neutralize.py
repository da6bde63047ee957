"""The numpy restatement of mff_xs_neutralize (tests/xs_neutralize_ref.py) against an
independent formulation -- numpy.linalg.lstsq on the explicit dummy + covariate design
matrix, then ddof-1 standardisation -- and against hand-made segments that pin the
degrees-of-freedom rule, the mad == 0 rule, even / odd medians and the output states.
The last tests pin the C ABI's argument checks and the binding (no device work)."""
import numpy as np
import pytest

import xs_neutralize_ref as ref
from xs_neutralize_ref import ABSENT, NULL, VALUE

ATOL = 1e-9  # parity.py's floor for O(1) statistics; the two f64 formulations differ by ~6e-12


def _lstsq_formulation(x, g, z, winsor_k):
    """Winsorise (sorted order statistics), regress on [dummies | z], standardise."""
    n = x.size
    xs = np.sort(x)
    med = xs[n // 2] if n % 2 else 0.5 * (xs[n // 2 - 1] + xs[n // 2])
    ds = np.sort(np.abs(x - med))
    mad = ds[n // 2] if n % 2 else 0.5 * (ds[n // 2 - 1] + ds[n // 2])
    if winsor_k > 0 and mad > 0:
        x = np.clip(x, med - winsor_k * 1.4826 * mad, med + winsor_k * 1.4826 * mad)
    ids = np.unique(g)
    X = np.zeros((n, ids.size + 1))
    X[np.arange(n), np.searchsorted(ids, g)] = 1.0
    X[:, -1] = z
    coef, *_ = np.linalg.lstsq(X, x, rcond=None)
    e = x - X @ coef
    return (e - e.mean()) / e.std(ddof=1)


@pytest.mark.parametrize("n", [64, 257, 1000, 5000, 8192])
def test_restatement_matches_least_squares(n):
    rng = np.random.default_rng(100 + n)
    G = 31
    g = rng.integers(0, G, n).astype(np.int32)
    z = rng.normal(23.0, 1.5, n)                      # ln market cap
    x = rng.standard_t(3, n) + 0.3 * (z - 23.0) + 0.1 * g   # heavy tails, size and industry bets
    st = np.full(n, VALUE, np.uint8)
    ov, os_ = ref.segment(x, st, g, G, z, st, winsor_k=3.0, standardize=True)
    assert (os_ == VALUE).all()
    want = _lstsq_formulation(x, g, z, 3.0)
    err = float(np.abs(ov - want).max())
    print(f"n={n}: restatement vs lstsq max abs diff {err:.3e}")
    assert err <= ATOL


def test_degrees_of_freedom_rule():
    st = np.full(4, VALUE, np.uint8)
    x = np.array([1.0, 2.0, 4.0, 8.0])
    # every stock alone in its industry: n - k = 0 -> all NULL, by counting
    ov, os_ = ref.segment(x, st, np.arange(4, dtype=np.int32), 4, winsor_k=0, standardize=False)
    assert (os_ == NULL).all() and (ov == 0).all()
    # one pair: n - k = 1 -> values (the pair's demeaned halves, the singles 0)
    ov, os_ = ref.segment(x, st, np.array([0, 0, 1, 2], np.int32), 3, winsor_k=0, standardize=False)
    assert (os_ == VALUE).all()
    np.testing.assert_allclose(ov, [-0.5, 0.5, 0.0, 0.0])
    # the covariate costs one more: the same segment is NULL with it
    z = np.array([1.0, 2.0, 3.0, 5.0])
    ov, os_ = ref.segment(x, st, np.array([0, 0, 1, 2], np.int32), 3, z, st, winsor_k=0, standardize=False)
    assert (os_ == NULL).all()
    # no industries: k = 1 (intercept); one stock is NULL, and so are two with standardize
    # (n - k = 0 -> NULL ... n = 2, k = 1 -> fine)
    ov, os_ = ref.segment(x[:1], st[:1], winsor_k=0, standardize=False)
    assert os_[0] == NULL
    ov, os_ = ref.segment(x[:2], st[:2], winsor_k=0, standardize=True)
    assert (os_ == VALUE).all()
    np.testing.assert_allclose(ov, [-np.sqrt(0.5), np.sqrt(0.5)])


def test_mad_zero_means_no_clipping():
    x = np.array([1.0] * 6 + [2.0, 50.0, -7.0])   # more than half tied: mad == 0
    st = np.full(x.size, VALUE, np.uint8)
    ov, os_ = ref.segment(x, st, winsor_k=3.0, standardize=False)
    np.testing.assert_allclose(ov, x - x.mean())


def test_even_and_odd_medians():
    st5, st6 = np.full(5, VALUE, np.uint8), np.full(6, VALUE, np.uint8)
    # odd: med 3, |x - med| = 2 1 0 1 97 -> mad 1; 100 clipped to 3 + 3 * 1.4826
    got = ref.winsorize(np.array([1.0, 2.0, 3.0, 4.0, 100.0]), 3.0)
    np.testing.assert_allclose(got, [1, 2, 3, 4, 3 + 3 * 1.4826])
    # even: med 3.5, deviations .5 .5 1.5 1.5 2.5 96.5 -> mad 1.5
    got = ref.winsorize(np.array([1.0, 2.0, 3.0, 4.0, 5.0, 100.0]), 3.0)
    np.testing.assert_allclose(got, [1, 2, 3, 4, 5, 3.5 + 3 * 1.4826 * 1.5])
    # values exactly on the bounds stay
    b = 3 + 3 * 1.4826
    got = ref.winsorize(np.array([1.0, 2.0, 3.0, 4.0, b]), 3.0)
    assert got[-1] == b
    ov, _ = ref.segment(np.array([1.0, 2.0, 3.0, 4.0, 100.0]), st5, winsor_k=3.0, standardize=False)
    np.testing.assert_allclose(ov + np.mean([1, 2, 3, 4, b]), [1, 2, 3, 4, b])
    ov, _ = ref.segment(np.array([1.0, 2.0, 3.0, 4.0, 5.0, 100.0]), st6, winsor_k=0.0, standardize=False)
    np.testing.assert_allclose(ov, np.array([1.0, 2, 3, 4, 5, 100]) - 115 / 6)


def test_output_states():
    x = np.array([0.5, np.nan, np.inf, -np.inf, 1.5, 2.5, 9.0, 3.0, 4.0, 7.0])
    st = np.array([VALUE, VALUE, VALUE, VALUE, NULL, ABSENT, VALUE, VALUE, VALUE, VALUE], np.uint8)
    g = np.array([0, 0, 0, 0, 0, 0, -1, 0, 0, 0], np.int32)   # stock 6: no industry
    z = np.array([1.0, 1, 1, 1, 1, 1, 1, np.nan, 2.0, 3.0])   # stock 7: non-finite size
    zst = np.full(10, VALUE, np.uint8)
    zst[8] = NULL                                             # stock 8: null size
    ov, os_ = ref.segment(x, st, g, 1, z, zst, winsor_k=0, standardize=False)
    assert os_.tolist() == [NULL, VALUE, VALUE, VALUE, NULL, ABSENT, NULL, NULL, NULL, NULL]
    # (U = {0, 9}: n - k = 2 - 2 = 0 -> NULL)
    assert np.isnan(ov[1]) and ov[2] == np.inf and ov[3] == -np.inf and (ov[[0, 4, 5, 6, 7, 8, 9]] == 0).all()
    ov, os_ = ref.segment(x, st, g, 1, winsor_k=0, standardize=False)
    assert os_.tolist() == [VALUE, VALUE, VALUE, VALUE, NULL, ABSENT, NULL, VALUE, VALUE, VALUE]
    np.testing.assert_allclose(ov[[0, 7, 8, 9]], np.array([0.5, 3, 4, 7]) - 14.5 / 4)
    # an id >= G is "none"
    ov, os_ = ref.segment(x, st, np.where(g == 0, 5, g), 5, winsor_k=0, standardize=False)
    assert os_.tolist() == [NULL, VALUE, VALUE, VALUE, NULL, ABSENT, NULL, NULL, NULL, NULL]


def test_c_abi_argument_checks():
    from mff import _lib
    lib = _lib.load()
    assert lib.mff_xs_neutralize_max_stocks() == 8192
    assert lib.mff_xs_neutralize_max_groups() == 256
    assert lib.mff_xs_neutralize_workspace_bytes(0, 100) == 0
    assert lib.mff_xs_neutralize_workspace_bytes(3, 100) >= 3 * (100 * 10 + 258 * 2)
    call = lambda rows, D, S, grp, G, size, sst: lib.mff_xs_neutralize(
        None, None, rows, D, S, grp, G, size, sst, 3.0, 1, None, None, None, None)
    fake = 256  # a non-NULL pointer value: the checks return before any dereference or launch
    for args, word in (((1, 1, 8193, None, 0, None, None), b"S=8193"),
                       ((1, 1, 10, fake, 257, None, None), b"G=257"),
                       ((1, 1, 10, fake, 0, None, None), b"G=0"),
                       ((-1, 1, 10, None, 0, None, None), b"rows=-1"),
                       ((1, -1, 10, None, 0, None, None), b"D=-1"),
                       ((1, 1, -1, None, 0, None, None), b"S=-1"),
                       ((1, 1, 10, None, 0, fake, None), b"size_state")):
        rc = call(*args)
        assert rc < 0 and word in lib.mff_last_error(), (args, lib.mff_last_error())
        with pytest.raises(_lib.MffError):
            _lib.check(rc, "mff_xs_neutralize")
    assert call(0, 5, 10, None, 0, None, None) == 0  # nothing to do


def test_factor_neutralize_rejects_bad_arguments():
    import datetime as dt

    from mff import frames
    from mff.factor import Factor
    codes = ["a", "b", "c"]
    dates = [dt.date(2024, 1, 2)]
    f = Factor("f", frames.to_long(np.ones((1, 3)), np.full((1, 3), VALUE, np.uint8), codes, dates, "f"))
    import pandas as pd
    with pytest.raises(ValueError, match="size must be"):
        f.neutralize(size="mc")
    with pytest.raises(ValueError, match="winsor"):
        f.neutralize(size=None, winsor="3")
    with pytest.raises(ValueError, match="industry must be a frame"):
        f.neutralize(industry=pd.DataFrame({"code": codes, "sector": [1, 2, 3]}), size=None)
    with pytest.raises(ValueError, match="one row per code"):
        f.neutralize(industry=pd.DataFrame({"code": ["a", "a"], "industry": [1, 2]}), size=None)
    with pytest.raises(ValueError, match="distinct labels"):
        f.neutralize(industry=pd.DataFrame({"code": [str(i) for i in range(300)], "industry": range(300)}),
                     size=None)
