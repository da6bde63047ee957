"""tests/xs_combine_ref.py (the numpy restatement of the composite factor, include/mff.h
mff_xs_comb_*) pinned on the CPU against independent second routes (numpy.corrcoef, pandas
Spearman, pandas shift + rolling mean / std, numpy.linalg.solve, a direct per-stock loop),
closed forms and hand-made days.  The binding of the C entry points and their argument checks
are tested too, so this file fails without the feature."""
import numpy as np
import pytest

import xs_combine_ref as ref
from xs_combine_ref import ABSENT, NULL, VALUE

pd = pytest.importorskip("pandas")

TOL = dict(rtol=1e-11, atol=1e-11)
ENTRY_POINTS = ("mff_xs_comb_moments", "mff_xs_comb_finalize", "mff_xs_comb_weights", "mff_xs_comb_apply")
H, W, M = 2, 8, 4


def test_library_binds_the_combine_entry_points():
    from mff import _lib
    for name in ENTRY_POINTS:
        assert name in _lib.SIGNATURES
    lib = _lib.load()
    for name in ENTRY_POINTS:
        assert hasattr(lib, name)
    import mff
    from mff import engine
    from mff.factor import Factor, combine
    assert "combine" in mff.__all__ and mff.combine is combine and callable(Factor.combine_with)
    assert engine.COMBINE_METHODS == ref.METHODS == ("equal", "ic", "icir", "max_icir")
    assert engine.COMBINE_IC == ref.IC_KINDS
    assert engine.CombineResult._fields == ("val", "state", "weights", "ic", "n_pairs", "count", "status")


def test_c_abi_argument_checks():
    """Bad arguments return a negative code before anything touches a device."""
    from mff import _lib
    lib = _lib.load()
    fake = 4096  # never dereferenced: every call fails its checks first
    mom = lambda K=2, D=1, S=8, Ky=1, y=fake: lib.mff_xs_comb_moments(fake, fake, K, D, S, y, y, Ky, fake, None)
    fin = lambda R=1, K=2, D=1, mo=0: lib.mff_xs_comb_finalize(fake, R, K, D, mo, fake, fake, fake, None)
    wts = lambda K=2, D=1, me=2, h=1, w=5, m=2, sh=0.5: lib.mff_xs_comb_weights(fake, K, D, me, h, w, m, sh, fake, fake,
                                                                                 fake, None)
    app = lambda K=2, D=1, S=8, mf=1: lib.mff_xs_comb_apply(fake, fake, K, D, S, fake, fake, fake, mf, fake, fake, None)
    for call, kw, word in ((mom, dict(K=0), b"K=0"), (mom, dict(K=65), b"K=65"), (mom, dict(D=-1), b"D=-1"),
                           (mom, dict(S=-1), b"S=-1"), (mom, dict(Ky=3, K=4), b"Ky=3"), (mom, dict(Ky=0), b"Ky=0"),
                           (mom, dict(Ky=1, y=None), b"Ky=1"),
                           (fin, dict(R=0), b"R=0"), (fin, dict(K=65), b"K=65"), (fin, dict(D=-1), b"D=-1"),
                           (fin, dict(mo=-1), b"min_obs=-1"),
                           (wts, dict(K=0), b"K=0"), (wts, dict(K=65), b"K=65"), (wts, dict(D=-1), b"D=-1"),
                           (wts, dict(me=4), b"method=4"), (wts, dict(me=-1), b"method=-1"),
                           (wts, dict(h=0), b"future_days=0"), (wts, dict(w=0), b"window=0"),
                           (wts, dict(m=0), b"min_periods=0"), (wts, dict(sh=1.5), b"shrink=1.5"),
                           (wts, dict(sh=-0.25), b"shrink=-0.25"), (wts, dict(sh=float("nan")), b"shrink="),
                           (app, dict(K=0), b"K=0"), (app, dict(K=65), b"K=65"), (app, dict(S=-1), b"S=-1"),
                           (app, dict(mf=0), b"min_factors=0"), (app, dict(mf=3), b"min_factors=3")):
        rc = call(**kw)
        assert rc < 0 and word in lib.mff_last_error(), (kw, lib.mff_last_error())
        with pytest.raises(_lib.MffError):
            _lib.check(rc, "mff_xs_comb")
    # nothing to do
    assert mom(D=0) == 0 and fin(D=0) == 0 and wts(D=0) == 0 and app(D=0) == 0 and app(S=0) == 0


@pytest.fixture(scope="module")
def panel():
    return ref.make_panel(3, 5, 30, 120, h=H)


@pytest.fixture(scope="module")
def clean():
    return ref.make_panel(4, 4, 30, 90, h=H, holes=False)


def test_ic_is_numpy_corrcoef_and_pandas_spearman(panel):
    x, xs, y, ys = panel
    K, D, S = x.shape
    ic, n = ref.ic_series(x, xs, y, ys, "pearson")
    ric, rn = ref.ic_series(x, xs, y, ys, "rank")
    assert np.array_equal(n, rn) and np.isnan(ic[:, D - H:]).all() and (n[:, D - H:] == 0).all()
    for k in range(K):
        for d in range(D - H):
            p = (xs[k, d] == VALUE) & ~np.isnan(x[k, d]) & (ys[d] == VALUE)
            assert n[k, d] == p.sum() and np.isfinite(x[k, d][p]).all()
            np.testing.assert_allclose(ic[k, d], np.corrcoef(x[k, d][p], y[d][p])[0, 1], **TOL)
            sp = pd.Series(x[k, d][p]).corr(pd.Series(y[d][p]), method="spearman")
            np.testing.assert_allclose(ric[k, d], sp, **TOL)
    assert 0.02 < np.nanmean(ic) < 0.3                      # the planted IC is there
    # a non-finite value inside the pair set: the Pearson IC of that date is NaN, the rank IC is not
    q = x.copy()
    p = np.nonzero((xs[1, 3] == VALUE) & (ys[3] == VALUE) & np.isfinite(x[1, 3]))[0][0]
    q[1, 3, p] = np.inf
    ic2, n2 = ref.ic_series(q, xs, y, ys, "pearson")
    assert np.isnan(ic2[1, 3]) and n2[1, 3] == n[1, 3] and np.isfinite(ref.ic_series(q, xs, y, ys, "rank")[0][1, 3])
    # min_obs
    big = int(n[:, :D - H].max())
    assert np.isnan(ref.ic_series(x, xs, y, ys, min_obs=big + 1)[0]).all()
    assert np.isfinite(ref.ic_series(x, xs, y, ys, min_obs=big)[0]).any()


def test_zscore_moments(panel):
    x, xs, _, _ = panel
    zm = ref.zscore_moments(x, xs)
    for k in range(x.shape[0]):
        for d in range(x.shape[1]):
            v = x[k, d][(xs[k, d] == VALUE) & np.isfinite(x[k, d])]
            np.testing.assert_allclose(zm[k, d], [len(v), v.mean(), v.std(ddof=1)], **TOL)
    assert ref.shifted_moments(np.full(7, 0.1)) == (7, 0.1, 0.0)   # a constant: M2 exactly 0
    assert np.isnan(ref.zscore_moments(x[:, :, :1], xs[:, :, :1])[..., 2]).all()


@pytest.mark.parametrize("h,w,m", [(H, W, M), (1, 1, 1), (3, 50, 2), (5, 6, 6)])
def test_ic_and_icir_weights_are_pandas_rolling(panel, h, w, m):
    x, xs, y, ys = panel
    ic, _ = ref.ic_series(x, xs, y, ys)
    ic[2, :10] = np.nan                                      # a factor whose coverage starts later
    ic[0, 14] = np.nan
    K, D = ic.shape
    roll = pd.DataFrame(ic.T).shift(h).rolling(w, min_periods=m)
    mean, std = roll.mean().to_numpy(), roll.std().to_numpy()
    cnt = pd.DataFrame(ic.T).shift(h).notna().astype(float).rolling(w, min_periods=1).sum().to_numpy()
    for method, raw in (("ic", mean), ("icir", np.where(cnt >= 2, mean / std, np.nan))):
        wts, count, status, _ = ref.weights(ic, method, h, w, m)
        raw = np.where(np.isfinite(raw), raw, 0.0)
        assert np.array_equal(count, cnt.astype(np.int32))
        for d in range(D):
            tot = np.abs(raw[d]).sum()
            if tot == 0.0:
                assert status[d] == 1 and np.isnan(wts[d]).all()
            else:
                assert status[d] == 0
                np.testing.assert_allclose(wts[d], raw[d] / tot, rtol=1e-9, atol=1e-12)
                np.testing.assert_allclose(np.abs(wts[d]).sum(), 1.0, **TOL)
        assert (status[:h] == 1).all()
        if method == "ic" or w >= 2:                          # (icir on a window of one date has no std)
            assert (status[h + m - 1:D - H] == 0).all()      # (y ends H dates early)
        else:
            assert (status == 1).all()


@pytest.mark.parametrize("shrink", [0.0, 0.3, 0.5, 1.0])
def test_max_icir_is_numpy_solve_on_the_listwise_window(panel, shrink):
    x, xs, y, ys = panel
    ic, _ = ref.ic_series(x, xs, y, ys)
    ic[2, :10] = np.nan
    K, D = ic.shape
    h, w, m = 2, 12, 4
    wts, count, status, cond = ref.weights(ic, "max_icir", h, w, m, shrink)
    seen = set()
    for d in range(D):
        win = ic[:, max(0, d - h - w + 1):d - h + 1] if d >= h else ic[:, :0]
        L = win[:, np.isfinite(win).all(axis=0)]
        c = L.shape[1]
        assert (count[d] == c).all()
        need = max(m, 2, K + 1 if shrink == 0 else 0)
        if c < need:
            assert status[d] == 1 and np.isnan(wts[d]).all()
            continue
        cov = np.cov(L, ddof=1)
        cov_s = (1 - shrink) * cov + shrink * np.diag(np.diag(cov))
        raw = np.linalg.solve(cov_s, L.mean(axis=1))
        assert status[d] == 0 and cond[d] < 1e3
        np.testing.assert_allclose(wts[d], raw / np.abs(raw).sum(), rtol=1e-9, atol=1e-12)
        seen.add(c)
    assert (status[:10 + h + m - 1] == 1).all() and status[-1] == 0 and len(seen) >= 2
    if shrink == 1.0:                                         # a diagonal covariance: mean / variance
        d = D - 1
        win = ic[:, d - h - w + 1:d - h + 1]
        raw = win.mean(axis=1) / win.var(axis=1, ddof=1)
        np.testing.assert_allclose(wts[d], raw / np.abs(raw).sum(), rtol=1e-9, atol=1e-12)


@pytest.mark.parametrize("method", ref.METHODS)
@pytest.mark.parametrize("min_factors", [1, 3])
def test_composite_is_the_per_stock_loop(panel, method, min_factors):
    x, xs, y, ys = panel
    K, D, S = x.shape
    r = ref.combine(x, xs, y, ys, method, H, W, M, min_factors=min_factors)
    assert (r["status"][H + M - 1:] == 0).all() and (r["status"][:H] == (0 if method == "equal" else 1)).all()
    nvalue = 0
    for d in range(D):
        for s in range(S):
            num = den = 0.0
            cnt = 0
            for k in range(K):
                v = x[k, d][(xs[k, d] == VALUE) & np.isfinite(x[k, d])]
                if xs[k, d, s] != VALUE or not np.isfinite(x[k, d, s]) or len(v) < 2 or not v.std(ddof=1) > 0:
                    continue
                wk = r["weights"][d, k]
                if r["status"][d] != 0 or wk == 0.0:
                    continue
                num += wk * (x[k, d, s] - v.mean()) / v.std(ddof=1)
                den += abs(wk)
                cnt += 1
            if r["status"][d] == 0 and cnt >= min_factors:
                assert r["state"][d, s] == VALUE
                np.testing.assert_allclose(r["val"][d, s], num / den, rtol=1e-10, atol=1e-10)
                nvalue += 1
            else:
                assert r["val"][d, s] == 0.0
                assert r["state"][d, s] == (ABSENT if (xs[:, d, s] == ABSENT).all() else NULL)
    assert nvalue > 0.5 * D * S


def test_closed_forms(clean):
    x, xs, y, ys = clean
    K, D, S = x.shape
    z = (x - x.mean(axis=2, keepdims=True)) / x.std(axis=2, ddof=1, keepdims=True)
    r = ref.combine(x, xs, None, None, "equal")
    assert (r["status"] == 0).all() and (r["state"] == VALUE).all() and (r["count"] == 0).all()
    assert np.isnan(r["ic"]).all() and (r["weights"] == 1.0 / K).all()
    np.testing.assert_allclose(r["val"], z.mean(axis=0), **TOL)
    for method in ("ic", "icir", "max_icir"):                 # K = 1: sign(w) z
        for sign in (1.0, -1.0):
            r = ref.combine(sign * x[:1], xs[:1], y, ys, method, H, W, M)
            ok = r["status"] == 0
            assert ok[H + M - 1:].all() and not ok[:H + M - 1].any()
            assert (np.abs(r["weights"][ok]) == 1.0).all()
            np.testing.assert_allclose(r["val"][ok], (r["weights"][ok] * sign) * z[0][ok], **TOL)
            assert (r["state"][ok] == VALUE).all() and (r["state"][~ok] == NULL).all() and (r["val"][~ok] == 0).all()
    # a stock missing one factor still gets a composite, renormalised over the others
    q = xs.copy()
    q[1, :, 5] = NULL
    r = ref.combine(x, q, None, None, "equal")
    zq = ref.zscore_moments(x, q)
    want = np.mean([(x[k, :, 5] - zq[k, :, 1]) / zq[k, :, 2] for k in (0, 2, 3)], axis=0)
    np.testing.assert_allclose(r["val"][:, 5], want, **TOL)
    assert (ref.combine(x, q, None, None, "equal", min_factors=K)["state"][:, 5] == NULL).all()


def test_hand_made_days(clean):
    x, xs, y, ys = clean
    K, D, S = x.shape
    ic, _ = ref.ic_series(x, xs, y, ys)
    for method in ("ic", "icir", "max_icir"):
        _, count, status, _ = ref.weights(ic, method, H, W, M)
        assert (status[:H + M - 1] == 1).all() and (status[H + M - 1:] == 0).all()   # d < h, then exactly m dates
        assert (count[:H] == 0).all() and (count[H + M - 1] == M).all() and (count[-1] == W).all()
        assert (ref.weights(ic, method, D, W, M)[2] == 1).all()                       # h >= D
        assert (ref.weights(ic, method, H, W, W + 1)[2] == 1).all()                   # m > W
        assert (ref.weights(ic, method, H, 1, 1)[2][H:] == (0 if method == "ic" else 1)).all()   # W = 1: no std
        assert (ref.weights(ic, method, H, 5 * D, M)[1][-1] == D - H).all()           # W > D: every date with an IC
    # a constant factor: no z-score, no IC, weight 0 (ic / icir), no listwise date (max_icir)
    c = x.copy()
    c[1] = 2.5
    for method, stat in (("ic", 0), ("icir", 0), ("max_icir", 1)):
        r = ref.combine(c, xs, y, ys, method, H, W, M)
        assert (r["zmom"][1, :, 2] == 0.0).all() and np.isnan(r["ic"][1]).all()
        assert (r["status"][H + M - 1:] == stat).all()
        if stat == 0:
            assert (r["weights"][H + M - 1:, 1] == 0.0).all() and (r["state"][H + M - 1:] == VALUE).all()
    r = ref.combine(c, xs, None, None, "equal")               # equal: the constant factor has no z
    assert (r["state"] == VALUE).all()
    np.testing.assert_allclose(r["val"], ref.combine(c[[0, 2, 3]], xs[[0, 2, 3]], None, None, "equal")["val"], **TOL)
    # a constant IC series: icir weight 0; max_icir degenerate
    k_ic = ic.copy()
    k_ic[0] = 0.05
    assert (ref.weights(k_ic, "icir", H, W, M)[0][H + M - 1:, 0] == 0.0).all()
    assert (ref.weights(k_ic, "max_icir", H, W, M)[2][H + M - 1:] == 2).all()
    # a duplicated factor: singular without shrinkage, fine with it
    dup = x.copy()
    dup[3] = dup[0]
    ic_d, _ = ref.ic_series(dup, xs, y, ys)
    s0 = ref.weights(ic_d, "max_icir", H, 12, K + 1, 0.0)[2]
    s5 = ref.weights(ic_d, "max_icir", H, 12, K + 1, 0.5)
    assert (s0[H + K:] == 2).all() and (s0[:H + K] == 1).all()
    assert (s5[2][H + K:] == 0).all()
    np.testing.assert_allclose(s5[0][H + K:, 0], s5[0][H + K:, 3], **TOL)   # the twins share their weight
    # all-ABSENT day and stock
    a = xs.copy()
    a[:, 7] = ABSENT
    a[:, :, 11] = ABSENT
    r = ref.combine(x, a, y, ys, "icir", H, W, M)
    assert (r["state"][7] == ABSENT).all() and (r["state"][:, 11] == ABSENT).all() and (r["val"][7] == 0).all()
    assert (r["n_pairs"][:, 7] == 0).all() and np.isnan(r["ic"][:, 7]).all() and r["status"][7] == 0
    assert (r["status"][H + M - 1:] == 0).all()
