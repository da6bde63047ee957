"""Plain numpy restatement of the per-day multi-factor cross-sectional regression
(include/mff.h, mff_xs_reg_*), one day at a time: numpy.linalg.lstsq on the
explicit sqrt(w)-scaled design [dummies of the non-empty industries | X], the classical
covariance, t, r2, dof, the residual, the two status rules and the time aggregate.  It
shares no code with the engine."""
import numpy as np

ABSENT, NULL, VALUE = 0, 1, 2
CONST_REL = 1e-20
PIVOT_MIN = 1e-10
AGG_COLUMNS = ("days", "mean", "std", "t_fm", "mean_abs_t", "share_abs_t_gt_2")


def usable(x, xs, y, ys, w=None, ws=None, group=None, G=None):
    """The listwise usable set [D][S]."""
    with np.errstate(invalid="ignore"):
        u = ((xs == VALUE) & np.isfinite(x)).all(axis=0) & (ys == VALUE) & np.isfinite(y)
        if w is not None:
            u &= (ws == VALUE) & np.isfinite(w) & (w > 0)
        if group is not None:
            u &= (group >= 0) & (group < G)
    return u


def _demean(v, wt, gid):
    """v minus its weighted mean inside each industry (v: [n] or [n][k])."""
    out = np.array(v, dtype=np.float64, copy=True)
    for g in np.unique(gid):
        m = gid == g
        out[m] -= np.average(out[m], axis=0, weights=wt[m])
    return out


def _cholesky_pivots(A):
    """Pivots of the unpivoted Cholesky of A, stopping at the first one <= PIVOT_MIN."""
    A = A.copy()
    k_ = A.shape[0]
    piv = []
    for k in range(k_):
        p = A[k, k]
        piv.append(p)
        if not p > PIVOT_MIN:
            break
        col = A[k + 1:, k] / np.sqrt(p)
        A[k + 1:, k + 1:] -= np.outer(col, col)
    return np.array(piv)


def regress_day(X, y, wt, gid, min_obs=0):
    """One day on its usable set: X [n][K], y [n], wt [n] > 0, gid [n] industry labels.
    Returns dict(beta, t, r2, n, dof, status, resid, cond, min_pivot)."""
    n, K = X.shape
    nan = np.full(K, np.nan)
    labels = np.unique(gid)
    dof = n - K - len(labels)
    out = dict(beta=nan, t=nan.copy(), r2=np.nan, n=n, dof=dof, status=1, resid=np.zeros(n), cond=np.nan,
               min_pivot=np.nan)
    if n < max(min_obs, 1) or dof < 1:
        return out
    Xt, yt = _demean(X, wt, gid), _demean(y, wt, gid)
    M = (Xt * wt[:, None]).T @ Xt
    raw = (wt[:, None] * X * X).sum(axis=0)
    if (np.diag(M) <= CONST_REL * raw).any():
        out["status"] = 2
        return out
    sc = 1.0 / np.sqrt(np.diag(M))
    Ms = M * sc[:, None] * sc[None, :]
    piv = _cholesky_pivots(Ms)
    out["min_pivot"] = float(piv.min())
    if not piv[-1] > PIVOT_MIN:
        out["status"] = 2
        return out
    out["cond"] = float(np.linalg.cond(Ms))
    # the explicit design: dummies of the non-empty industries, then the exposures
    Z = np.concatenate([(gid[:, None] == labels[None, :]).astype(np.float64), X], axis=1)
    sw = np.sqrt(wt)
    Zw, yw = Z * sw[:, None], y * sw
    rawy = float((wt * y * y).sum())
    T = float((wt * yt * yt).sum())
    ybar = np.average(y, weights=wt)
    den = float((wt * (y - ybar) ** 2).sum())
    if T <= CONST_REL * rawy:      # the regressand is constant within industries: an exact fit
        out.update(status=0, beta=np.zeros(K), r2=(1.0 if den > CONST_REL * rawy else np.nan))
        return out
    coef = np.linalg.lstsq(Zw, yw, rcond=None)[0]
    resid = y - Z @ coef
    rss = float((wt * resid * resid).sum())
    # classical covariance sigma^2 (Z^T W Z)^-1 from the QR factor: (R^T R)^-1 = R^-1 R^-T
    rinv = np.linalg.inv(np.linalg.qr(Zw, mode="r"))
    se = np.sqrt(rss / dof * (rinv * rinv).sum(axis=1)[len(labels):])
    beta = coef[len(labels):]
    with np.errstate(divide="ignore", invalid="ignore"):
        t = np.where(se == 0, np.nan, beta / se)
    out.update(status=0, beta=beta, t=t, resid=resid, r2=(1.0 - rss / den if den > CONST_REL * rawy else np.nan))
    return out


def regress(x, xs, y, ys, w=None, ws=None, group=None, G=None, min_obs=0):
    """x [K][D][S] + states, y [D][S] + state, optional w / ws and group [D][S] (ids in
    [0, G)).  Returns dict of beta [D][K], t [D][K], r2 [D], n, dof, status (int32 [D]),
    resid_val / resid_state [D][S], cond [D] (of the unit-diagonal Gram, NaN off status 0)."""
    K, D, S = x.shape
    if group is not None and G is None:
        G = int(group.max()) + 1
    u = usable(x, xs, y, ys, w, ws, group, G)
    res = dict(beta=np.full((D, K), np.nan), t=np.full((D, K), np.nan), r2=np.full(D, np.nan),
               n=np.zeros(D, np.int32), dof=np.zeros(D, np.int32), status=np.zeros(D, np.int32),
               resid_val=np.zeros((D, S)), resid_state=np.where(ys == VALUE, NULL, ys).astype(np.uint8),
               cond=np.full(D, np.nan), min_pivot=np.full(D, np.nan))
    for d in range(D):
        m = u[d]
        n = int(m.sum())
        gid = group[d][m] if group is not None else np.zeros(n, np.int64)
        wt = w[d][m].astype(np.float64) if w is not None else np.ones(n)
        g_ne = len(np.unique(gid)) if group is not None else 1
        res["n"][d], res["dof"][d] = n, n - K - g_ne
        if n == 0:
            res["status"][d] = 1
            continue
        r = regress_day(x[:, d][:, m].T.astype(np.float64), y[d][m].astype(np.float64), wt, gid, min_obs)
        assert r["dof"] == res["dof"][d]
        for k in ("beta", "t", "r2", "status", "cond", "min_pivot"):
            res[k][d] = r[k]
        if r["status"] == 0:
            res["resid_val"][d][m] = r["resid"]
            res["resid_state"][d][m] = VALUE
    return res


def aggregate(res):
    """The Fama-MacBeth time aggregate: (agg [K][6] in AGG_COLUMNS order, overall [2] = (mean
    r2, mean n)) over the status-0 days."""
    ok = res["status"] == 0
    beta, t = res["beta"][ok], res["t"][ok]
    K = res["beta"].shape[1]
    agg = np.full((K, 6), np.nan)
    days = int(ok.sum())
    for j in range(K):
        b = beta[:, j]
        agg[j, 0] = days
        if days:
            agg[j, 1] = b.mean()
        if days > 1:
            agg[j, 2] = b.std(ddof=1)
            if agg[j, 2] != 0:
                agg[j, 3] = agg[j, 1] / (agg[j, 2] / np.sqrt(days))
        a = np.abs(t[:, j][~np.isnan(t[:, j])])
        if len(a):
            agg[j, 4] = a.mean()
            agg[j, 5] = (a > 2).mean()
    r2 = res["r2"][ok]
    r2 = r2[~np.isnan(r2)]
    overall = np.array([r2.mean() if len(r2) else np.nan, res["n"][ok].mean() if days else np.nan])
    return agg, overall
