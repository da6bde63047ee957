"""Plain numpy restatement of the composite factor (include/mff.h, mff_xs_comb_*; DESIGN.md
§13), one (factor, date) and one date at a time: the z-score moments, the per-date IC (Pearson,
or on the average ranks of the pair set), the trailing-window weights (equal / ic / icir /
max_icir with the unit-diagonal Cholesky and its pivot rule) and the per-stock renormalised
weighted sum of z-scores.  It shares no code with the engine."""
import numpy as np

ABSENT, NULL, VALUE = 0, 1, 2
METHODS = ("equal", "ic", "icir", "max_icir")
IC_KINDS = ("pearson", "rank")
PIV_MIN = 1e-10


def make_panel(seed, K, D, S, h=2, holes=True):
    """Test panel: K exposure rows = 0.5 common + sqrt(0.75) own noise (mutual correlation 0.25)
    and a forward return y with a planted IC that differs by factor and wanders by date.  The
    last h dates of y are NULL (the horizon has not closed).  With ``holes`` and S >= 16 every
    day holds, spread over DIFFERENT factor rows: an ABSENT run, NULLs, NaN, +inf, -inf, -0.0 and
    +0.0; y is NULL at the stocks that got an inf, so the infinity tests the z-score set without
    turning the day's Pearson IC into NaN; y has NULL / ABSENT entries of its own.
    Returns x, xs [K][D][S], y, ys [D][S]."""
    rng = np.random.default_rng(seed)
    common = rng.standard_normal((D, S))
    own = rng.standard_normal((K, D, S))
    x = 0.5 * common[None] + np.sqrt(0.75) * own
    load = (0.05 + 0.1 * rng.random(K))[:, None] * (1.0 + 0.8 * rng.standard_normal((K, D)))
    y = 0.02 * ((load[:, :, None] * own).sum(axis=0) / np.sqrt(K) + rng.standard_normal((D, S)))
    xs = np.full((K, D, S), VALUE, np.uint8)
    ys = np.full((D, S), VALUE, np.uint8)
    ys[max(D - h, 0):] = NULL
    if holes and S >= 16:
        for d in range(D):
            hit = rng.permutation(S)[:max(8, S // 10)]
            kinds = ("absent", "null", np.nan, np.inf, -np.inf, -0.0, 0.0, "ynull", "yabsent")
            for i, s in enumerate(hit):
                r = int(rng.integers(0, K))
                kind = kinds[i % len(kinds)]
                if kind == "absent":
                    xs[r, d, s:s + max(1, S // (20 * (K + 1)))] = ABSENT
                elif kind == "null":
                    xs[r, d, s] = NULL
                elif kind == "ynull":
                    ys[d, s] = NULL
                elif kind == "yabsent":
                    ys[d, s] = ABSENT
                else:
                    x[r, d, s] = kind
                    if np.isinf(kind):
                        ys[d, s] = NULL
    y = np.where(ys == VALUE, y, 0.0)
    return x, xs, y, ys


def shifted_moments(v):
    """(n, mean, M2) of a 1-d array, shifted by its first entry: a constant array gives M2 = 0
    exactly."""
    n = len(v)
    if n == 0:
        return 0, 0.0, 0.0
    mean = v[0] + float((v - v[0]).sum()) / n
    return n, mean, float(((v - mean) ** 2).sum())


def zscore_moments(x, xs):
    """zmom [K][D][3] = (n, mean, std ddof = 1) over the stocks whose x is VALUE and finite; std
    NaN when n < 2."""
    K, D, _ = x.shape
    out = np.zeros((K, D, 3))
    for k in range(K):
        for d in range(D):
            m = (xs[k, d] == VALUE) & np.isfinite(x[k, d])
            n, mean, M2 = shifted_moments(x[k, d][m])
            out[k, d] = (n, mean, np.sqrt(M2 / (n - 1)) if n >= 2 else np.nan)
    return out


def pair_set(xv, xs, ys):
    """The rule of mff_ic_pairs: x VALUE and not NaN, y VALUE."""
    return (xs == VALUE) & ~np.isnan(xv) & (ys == VALUE)


def pearson(px, py, min_obs=0):
    """Cxy / sqrt(Cxx Cyy) over the pairs; NaN with fewer than max(2, min_obs) pairs, a zero
    denominator or a non-finite value among the pairs."""
    n = len(px)
    if n < max(2, min_obs) or not (np.isfinite(px).all() and np.isfinite(py).all()):
        return np.nan
    _, _, cxx = shifted_moments(px)
    _, _, cyy = shifted_moments(py)
    mx = px[0] + (px - px[0]).sum() / n
    my = py[0] + (py - py[0]).sum() / n
    cxy = float(((px - mx) * (py - my)).sum())
    den = np.sqrt(cxx * cyy)
    return np.nan if den == 0.0 else cxy / den


def average_rank(v):
    """1-based average ranks (ties share the mean of their positions)."""
    _, inv, cnt = np.unique(v, return_inverse=True, return_counts=True)
    last = np.cumsum(cnt)                                  # the last position of each tie group
    return (last - 0.5 * (cnt - 1))[inv]


def ic_series(x, xs, y, ys, kind="pearson", min_obs=0):
    """ic [K][D], n_pairs int32 [K][D] of x [K][D][S] against y [D][S].  'rank': both sides
    replaced by their average ranks over the pair set (y entries that are NaN get no rank and
    leave the moment set, the x ranks are kept: the route of engine.ic_series)."""
    assert kind in IC_KINDS
    K, D, _ = x.shape
    ic = np.full((K, D), np.nan)
    npairs = np.zeros((K, D), np.int32)
    for k in range(K):
        for d in range(D):
            p = pair_set(x[k, d], xs[k, d], ys[d])
            npairs[k, d] = int(p.sum())
            px, py = x[k, d][p], y[d][p]
            if kind == "rank" and len(px):
                px = average_rank(px)
                keep = ~np.isnan(py)
                px, py = px[keep], average_rank(py[keep])
            ic[k, d] = pearson(px, py, min_obs)
    return ic, npairs


def cholesky_solve(C, b):
    """Unpivoted Cholesky of C (unit diagonal) and C u = b; None when a pivot is <= PIV_MIN (the
    rule of mff_xs_orth_solve / mff_xs_reg_solve)."""
    K = len(b)
    L = np.zeros((K, K))
    A = C.copy()
    for j in range(K):
        piv = A[j, j]
        if not piv > PIV_MIN:
            return None
        L[j, j] = np.sqrt(piv)
        L[j + 1:, j] = A[j + 1:, j] / L[j, j]
        for i in range(j + 1, K):
            A[i, j + 1:i + 1] -= L[i, j] * L[j + 1:i + 1, j]
    u = b.astype(np.float64).copy()
    for j in range(K):
        u[j] /= L[j, j]
        u[j + 1:] -= L[j + 1:, j] * u[j]
    for j in range(K - 1, -1, -1):
        u[j] /= L[j, j]
        u[:j] -= L[j, :j] * u[j]
    return u


def weights_day(ic, d, method, h, W, m, shrink=0.5):
    """(w [K], count [K], status, cond) of date index d from ic [K][D]."""
    K = ic.shape[0]
    nan = np.full(K, np.nan)
    count = np.zeros(K, np.int32)
    cond = np.nan
    hi = d - h
    lo = max(0, hi - W + 1)
    win = ic[:, lo:hi + 1] if hi >= 0 else ic[:, :0]      # E(d)
    raw = np.zeros(K)
    if method == "equal":
        raw[:] = 1.0
    elif method in ("ic", "icir"):
        any_ok = False
        for k in range(K):
            v = win[k][np.isfinite(win[k])]
            c, mean, M2 = shifted_moments(v)
            count[k] = c
            if method == "ic":
                ok = c >= m
                val = mean
            else:
                sd = np.sqrt(M2 / (c - 1)) if c >= 2 else np.nan
                ok = c >= max(m, 2) and np.isfinite(sd) and sd > 0.0
                val = mean / sd if ok else 0.0
            if ok:
                raw[k] = val
                any_ok = True
        if not any_ok:
            return nan, count, 1, cond
    else:
        L = win[:, np.isfinite(win).all(axis=0)]           # the listwise dates
        c = L.shape[1]
        count[:] = c
        need = max(m, 2)
        if shrink == 0:
            need = max(need, K + 1)
        if c < need:
            return nan, count, 1, cond
        mom = [shifted_moments(L[k]) for k in range(K)]
        mu = np.array([q[1] for q in mom])
        dev = L - mu[:, None]
        M = dev @ dev.T
        dg = np.diag(M).copy()
        if not (dg > 0.0).all():
            return nan, count, 2, cond
        C = (1.0 - shrink) * (M / np.sqrt(np.outer(dg, dg)))
        np.fill_diagonal(C, 1.0)
        sig = np.sqrt(dg / (c - 1))
        u = cholesky_solve(C, mu / sig)
        if u is None:
            return nan, count, 2, cond
        cond = float(np.linalg.cond(C))
        raw = u / sig
    norm = np.abs(raw).sum()
    if not (norm > 0.0 and np.isfinite(norm)):
        return nan, count, 2, cond
    return raw / norm, count, 0, cond


def weights(ic, method, h, W, m, shrink=0.5, D=None):
    """weights [D][K], count int32 [D][K], status int32 [D], cond [D] (max_icir: the condition
    number of the scaled, shrunk covariance of the date; NaN elsewhere)."""
    assert method in METHODS
    if ic is None:
        ic = np.full((0, D), np.nan)
    K, D = ic.shape
    w = np.full((D, K), np.nan)
    count = np.zeros((D, K), np.int32)
    status = np.zeros(D, np.int32)
    cond = np.full(D, np.nan)
    for d in range(D):
        w[d], count[d], status[d], cond[d] = weights_day(ic, d, method, h, W, m, shrink)
    return w, count, status, cond


def composite(x, xs, zmom, w, status, min_factors=1):
    """val [D][S], state u8 [D][S]."""
    K, D, S = x.shape
    val = np.zeros((D, S))
    state = np.where((xs != ABSENT).any(axis=0), NULL, ABSENT).astype(np.uint8)
    for d in range(D):
        if status[d] != 0:
            continue
        num, den, cnt = np.zeros(S), np.zeros(S), np.zeros(S, np.int64)
        for k in range(K):
            n, mean, sd = zmom[k, d]
            if not (n >= 2 and sd > 0.0 and w[d, k] != 0.0):
                continue
            p = (xs[k, d] == VALUE) & np.isfinite(x[k, d])
            z = (np.where(p, x[k, d], mean) - mean) / sd
            num += np.where(p, w[d, k] * z, 0.0)
            den += np.where(p, abs(w[d, k]), 0.0)
            cnt += p
        ok = cnt >= min_factors
        val[d][ok] = num[ok] / den[ok]
        state[d][ok] = VALUE
    return val, state


def combine(x, xs, y=None, ys=None, method="icir", future_days=5, window=60, min_periods=20, ic="pearson",
            shrink=0.5, min_obs=0, min_factors=1):
    """x [K][D][S] + states, y [D][S] + states (None for 'equal': every IC NaN).  Returns dict of
    val / state [D][S], weights [D][K], ic [K][D], n_pairs [K][D], count [D][K], status [D],
    cond [D], zmom [K][D][3]."""
    assert method in METHODS and ic in IC_KINDS
    K, D, S = x.shape
    zmom = zscore_moments(x, xs)
    if y is None:
        assert method == "equal"
        ics, npairs = np.full((K, D), np.nan), np.zeros((K, D), np.int32)
    else:
        ics, npairs = ic_series(x, xs, y, ys, ic, min_obs)
    w, count, status, cond = weights(ics, method, future_days, window, min_periods, shrink)
    val, state = composite(x, xs, zmom, w, status, min_factors)
    return dict(val=val, state=state, weights=w, ic=ics, n_pairs=npairs, count=count, status=status, cond=cond,
                zmom=zmom)
