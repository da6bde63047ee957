"""tests/xs_reg_ref.py (the numpy restatement of the per-day cross-sectional regression,
include/mff.h mff_xs_reg_*) pinned on the CPU against an independent second route (explicit
within-industry weighted demeaning + numpy.linalg.solve), numpy.polyfit for K = 1 without
industries, and hand-made days.  The binding of the C entry points is checked too, so this
file fails without the feature."""
import numpy as np
import pytest

import xs_reg_ref as ref
from xs_reg_ref import ABSENT, NULL, VALUE

TOL = dict(rtol=1e-9, atol=1e-9)


def _day(seed, n, K, G=None, weights=True):
    rng = np.random.default_rng(seed)
    X = 0.5 * rng.standard_normal((n, 1)) + rng.standard_normal((n, K))
    gid = rng.integers(0, G, n) if G else np.zeros(n, np.int64)
    y = X @ rng.standard_normal(K) + (rng.standard_normal(G)[gid] if G else 0.3) + 0.5 * rng.standard_normal(n)
    wt = np.sqrt(np.exp(rng.normal(3.0, 1.0, n))) if weights else np.ones(n)
    return X, y, wt, gid


def _second_route(X, y, wt, gid):
    """Frisch-Waugh by hand: demean inside industries, solve the K x K normal equations."""
    Xt, yt = X.copy(), y.copy()
    for g in np.unique(gid):
        m = gid == g
        W = wt[m].sum()
        Xt[m] -= (wt[m, None] * X[m]).sum(axis=0) / W
        yt[m] -= (wt[m] * y[m]).sum() / W
    M = Xt.T @ (wt[:, None] * Xt)
    b = Xt.T @ (wt * yt)
    beta = np.linalg.solve(M, b)
    e = yt - Xt @ beta
    rss = (wt * e * e).sum()
    dof = len(y) - X.shape[1] - len(np.unique(gid))
    se = np.sqrt(rss / dof * np.diag(np.linalg.inv(M)))
    ybar = (wt * y).sum() / wt.sum()
    return beta, beta / se, 1.0 - rss / (wt * (y - ybar) ** 2).sum(), e


def test_library_binds_the_regression_entry_points():
    from mff import _lib
    for name in ("mff_xs_reg_max_factors", "mff_xs_reg_max_groups", "mff_xs_reg_workspace_bytes", "mff_xs_reg_groups",
                 "mff_xs_reg_gram", "mff_xs_reg_solve", "mff_xs_reg_residual", "mff_xs_reg_mean"):
        assert name in _lib.SIGNATURES
    import mff
    assert "factor_returns" in mff.__all__


@pytest.mark.parametrize("K,G,weights", [(1, None, False), (3, None, True), (4, 3, True), (9, 31, True), (2, 5, False)])
def test_restatement_matches_second_route(K, G, weights):
    X, y, wt, gid = _day(10 + K, 400, K, G, weights)
    r = ref.regress_day(X, y, wt, gid)
    beta, t, r2, e = _second_route(X, y, wt, gid)
    assert r["status"] == 0 and r["dof"] == 400 - K - len(np.unique(gid)) and r["cond"] < 1e3
    np.testing.assert_allclose(r["beta"], beta, **TOL)
    np.testing.assert_allclose(r["t"], t, **TOL)
    np.testing.assert_allclose(r["r2"], r2, **TOL)
    np.testing.assert_allclose(r["resid"], e, **TOL)


def test_single_factor_is_polyfit():
    X, y, wt, gid = _day(3, 200, 1, None, True)
    r = ref.regress_day(X, y, wt, gid)
    coef, cov = np.polyfit(X[:, 0], y, 1, w=np.sqrt(wt), cov="unscaled")
    resid = y - np.polyval(coef, X[:, 0])
    sigma2 = (wt * resid ** 2).sum() / (200 - 2)
    np.testing.assert_allclose(r["beta"][0], coef[0], **TOL)
    np.testing.assert_allclose(r["t"][0], coef[0] / np.sqrt(sigma2 * cov[0, 0]), **TOL)
    np.testing.assert_allclose(r["resid"], resid, **TOL)


def _dense(X, y, wt=None, gid=None):
    """One day [n][K] -> the dense single-day inputs of ref.regress."""
    n, K = X.shape
    x = X.T[:, None, :].copy()
    xs = np.full((K, 1, n), VALUE, np.uint8)
    a = dict(x=x, xs=xs, y=y[None].copy(), ys=np.full((1, n), VALUE, np.uint8))
    a["w"] = None if wt is None else wt[None].copy()
    a["ws"] = None if wt is None else np.full((1, n), VALUE, np.uint8)
    a["group"] = None if gid is None else gid[None].astype(np.int32)
    a["G"] = None if gid is None else int(gid.max()) + 1
    return a


def _reg(a, **kw):
    return ref.regress(a["x"], a["xs"], a["y"], a["ys"], a["w"], a["ws"], a["group"], a["G"], **kw)


def test_two_stocks_per_industry():
    """Within-industry differences only: beta = sum w' dx dy / sum w' dx^2, w' = w1 w2 / (w1 + w2)."""
    rng = np.random.default_rng(1)
    G = 6
    gid = np.repeat(np.arange(G), 2)
    X = rng.standard_normal((2 * G, 1))
    y = rng.standard_normal(2 * G)
    wt = rng.uniform(0.5, 2.0, 2 * G)
    r = _reg(_dense(X, y, wt, gid))
    dx, dy = X[0::2, 0] - X[1::2, 0], y[0::2] - y[1::2]
    wp = wt[0::2] * wt[1::2] / (wt[0::2] + wt[1::2])
    assert r["status"][0] == 0 and r["dof"][0] == 2 * G - 1 - G and r["n"][0] == 2 * G
    np.testing.assert_allclose(r["beta"][0, 0], (wp * dx * dy).sum() / (wp * dx * dx).sum(), **TOL)


def test_singular_days():
    X, y, wt, gid = _day(5, 90, 3, 3)
    dup = X.copy()
    dup[:, 2] = dup[:, 0]
    r = _reg(_dense(dup, y, wt, gid))
    assert r["status"][0] == 2 and np.isnan(r["beta"]).all() and np.isnan(r["t"]).all() and np.isnan(r["r2"]).all()
    assert r["min_pivot"][0] < 1e-12 and (r["resid_state"] == NULL).all() and r["n"][0] == 90
    comb = X.copy()
    comb[:, 2] = comb[:, 0] + comb[:, 1]
    assert _reg(_dense(comb, y, wt, gid))["status"][0] == 2
    const = X.copy()
    const[:, 1] = 1.5 * gid + 0.25
    r = _reg(_dense(const, y, wt, gid))
    assert r["status"][0] == 2 and np.isnan(r["min_pivot"][0])     # caught by the constant rule, before the Cholesky
    assert _reg(_dense(X, y, wt, gid))["status"][0] == 0


def test_degrees_of_freedom_and_min_obs():
    X, y, wt, gid = _day(6, 40, 2, 3)
    gid[:6] = [0, 1, 2, 0, 1, 2]
    for n, dof, status in ((5, 0, 1), (6, 1, 0), (40, 35, 0)):
        r = _reg(_dense(X[:n], y[:n], wt[:n], gid[:n]))
        assert r["n"][0] == n and r["dof"][0] == dof and r["status"][0] == status
        assert np.isnan(r["beta"]).all() == (status == 1)
    assert _reg(_dense(X, y, wt, gid), min_obs=40)["status"][0] == 0
    assert _reg(_dense(X, y, wt, gid), min_obs=41)["status"][0] == 1
    # without industries the intercept takes one degree of freedom
    r = _reg(_dense(X[:3], y[:3]))
    assert r["dof"][0] == 0 and r["status"][0] == 1
    assert _reg(_dense(X[:4], y[:4]))["status"][0] == 0


def test_empty_set_and_bad_weights():
    X, y, wt, gid = _day(8, 30, 2, 2)
    a = _dense(X, y, wt, gid)
    a["ys"][:] = NULL
    r = _reg(a)
    assert r["n"][0] == 0 and r["status"][0] == 1 and r["dof"][0] == -2 and (r["resid_state"] == NULL).all()
    a = _dense(X, y, wt, gid)
    a["ys"][0, 3] = ABSENT
    a["w"][0, :3] = (0.0, -2.0, np.nan)
    a["ws"][0, 4] = NULL
    a["x"][1, 0, 5] = np.inf
    a["group"][0, 6] = -1
    r = _reg(a)
    assert r["n"][0] == 30 - 7 and r["status"][0] == 0
    assert r["resid_state"][0, :8].tolist() == [NULL, NULL, NULL, ABSENT, NULL, NULL, NULL, VALUE]
    keep = np.ones(30, bool)
    keep[:7] = False
    alone = ref.regress_day(X[keep], y[keep], wt[keep], gid[keep])
    np.testing.assert_allclose(r["beta"][0], alone["beta"], **TOL)


def test_constant_regressand_and_aggregate():
    X, y, wt, gid = _day(9, 50, 2, None)
    r = _reg(_dense(X, np.full(50, 0.5), wt))
    assert r["status"][0] == 0 and (r["beta"] == 0).all() and np.isnan(r["t"]).all() and np.isnan(r["r2"]).all()
    days = [_reg(_dense(*_day(20 + i, 60, 2, 3))) for i in range(4)]
    res = {k: np.concatenate([d[k] for d in days]) for k in ("beta", "t", "r2", "n", "status")}
    res["status"][2] = 2
    agg, overall = ref.aggregate(res)
    b = res["beta"][[0, 1, 3]]
    assert (agg[:, 0] == 3).all()
    np.testing.assert_allclose(agg[:, 1], b.mean(axis=0))
    np.testing.assert_allclose(agg[:, 3], b.mean(axis=0) / (b.std(axis=0, ddof=1) / np.sqrt(3)))
    np.testing.assert_allclose(agg[:, 4], np.abs(res["t"][[0, 1, 3]]).mean(axis=0))
    np.testing.assert_allclose(overall, [res["r2"][[0, 1, 3]].mean(), 60.0])
