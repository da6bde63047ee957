"""The numpy restatement of the pairwise factor correlation (tests/xs_corr_ref.py) pinned
against numpy / pandas and hand-made cases (no GPU)."""
import numpy as np
import pytest

import xs_corr_ref as ref
from xs_corr_ref import ABSENT, NULL, VALUE

pd = pytest.importorskip("pandas")


def _full(rng, F, D, S):
    return rng.standard_t(3, (F, D, S)), np.full((F, D, S), VALUE, np.uint8)


def test_full_coverage_equals_corrcoef():
    rng = np.random.default_rng(1)
    x, st = _full(rng, 7, 3, 211)
    x[1] = 0.7 * x[0] + 0.3 * x[1]
    x[2] = -x[3]
    c, n = ref.corr(x, st)
    assert (n == 211).all()
    for d in range(3):
        np.testing.assert_allclose(c[d], np.corrcoef(x[:, d]), rtol=0, atol=1e-13)
        assert (np.diag(c[d]) == 1.0).all() and np.array_equal(c[d], c[d].T)
    assert c[0, 2, 3] == pytest.approx(-1.0, abs=1e-15) and abs(c[0, 2, 3]) <= 1.0


@pytest.mark.parametrize("min_pairs", [2, 40])
def test_masks_and_nan_equal_pandas(min_pairs):
    rng = np.random.default_rng(2)
    F, D, S = 6, 3, 120
    x, st = _full(rng, F, D, S)
    st[rng.random((F, D, S)) < 0.25] = NULL
    st[rng.random((F, D, S)) < 0.15] = ABSENT
    st[5, :, 40:] = ABSENT                     # a thin row: pair sets below min_pairs = 40
    x[rng.random((F, D, S)) < 0.05] = np.nan
    x[0, 0, 3], x[1, 0, 4] = np.inf, -np.inf
    c, n = ref.corr(x, st, min_pairs=min_pairs)
    for d in range(D):
        v = np.where(ref.usable(x[:, d], st[:, d]), x[:, d], np.nan)
        want = pd.DataFrame(v.T).corr(min_periods=min_pairs).to_numpy()
        assert np.array_equal(np.isnan(c[d]), np.isnan(want))
        np.testing.assert_allclose(c[d], want, rtol=0, atol=1e-13)
        ok = ~np.isnan(v)
        assert np.array_equal(n[d], ok.astype(np.int32) @ ok.astype(np.int32).T)
    if min_pairs == 40:
        assert np.isnan(c[:, 5, 0]).any()


def test_full_coverage_spearman_equals_pandas():
    rng = np.random.default_rng(3)
    x, st = _full(rng, 5, 2, 150)
    x = np.round(x, 1)                          # ties
    c, _ = ref.corr(x, st, method="spearman")
    for d in range(2):
        want = pd.DataFrame(x[:, d].T).corr(method="spearman").to_numpy()
        np.testing.assert_allclose(c[d], want, rtol=0, atol=1e-13)


def test_average_ranks_with_and_without_scipy():
    v = np.array([3.0, 1.0, 3.0, 2.0, 3.0, -1.0, 2.0])
    want = np.array([6.0, 2.0, 6.0, 3.5, 6.0, 1.0, 3.5])
    np.testing.assert_array_equal(ref._rank_average(v), want)
    np.testing.assert_array_equal(ref._rank_average_numpy(v), want)


def test_hand_made_cases():
    S = 8
    x = np.zeros((5, 1, S))
    st = np.full((5, 1, S), ABSENT, np.uint8)
    x[0, 0] = [1, 2, 4, 8, 16, 32, 64, 128]
    st[0, 0] = VALUE
    x[1, 0, :2] = [5.0, 3.0]                    # with row 0: n = 2, decreasing -> -1 exactly
    st[1, 0, :2] = VALUE
    x[2, 0, 7] = 9.0                            # n = 1 with row 0 (and with itself)
    st[2, 0, 7] = VALUE
    x[3, 0] = [7, 7, 7, 1, 2, 3, 4, 5]          # constant on the pair set with row 4, not as a row
    st[3, 0] = VALUE
    x[4, 0, :3] = [1.0, -2.0, 0.5]
    st[4, 0, :3] = VALUE
    c, n = ref.corr(x, st)
    assert n[0, 0, 1] == 2 and c[0, 0, 1] == -1.0 and c[0, 1, 0] == -1.0
    x2 = x.copy()
    x2[1, 0, :2] = [3.0, 5.0]
    assert ref.corr(x2, st)[0][0, 0, 1] == 1.0
    assert n[0, 0, 2] == 1 and np.isnan(c[0, 0, 2]) and n[0, 2, 2] == 1 and np.isnan(c[0, 2, 2])
    assert n[0, 3, 4] == 3 and np.isnan(c[0, 3, 4]) and c[0, 3, 3] == 1.0 and c[0, 4, 4] == 1.0
    assert np.isfinite(c[0, 0, 3])
    assert n[0, 1, 2] == 0 and np.isnan(c[0, 1, 2])
    # a row that is all ABSENT
    st[2] = ABSENT
    c, n = ref.corr(x, st)
    assert (n[0, 2] == 0).all() and (n[0, :, 2] == 0).all() and np.isnan(c[0, 2]).all()
    m, days = ref.corr_mean(c)
    assert days[0, 1] == 1 and m[0, 1] == -1.0 and days[2, 2] == 0 and np.isnan(m[2, 2])


def test_mean_skips_nan_days():
    c = np.array([[[1.0, 0.5], [0.5, 1.0]], [[1.0, np.nan], [np.nan, np.nan]], [[1.0, -0.25], [-0.25, 1.0]]])
    m, days = ref.corr_mean(c)
    assert days.tolist() == [[3, 2], [2, 2]]
    np.testing.assert_array_equal(m, [[1.0, 0.125], [0.125, 1.0]])


def test_arguments():
    x, st = _full(np.random.default_rng(0), 2, 1, 5)
    with pytest.raises(ValueError):
        ref.corr(x, st, method="kendall")
    with pytest.raises(ValueError):
        ref.corr(x, st, min_pairs=1)
