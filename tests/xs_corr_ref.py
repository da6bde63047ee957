"""numpy restatement of the pairwise factor correlation (mff_xs_corr_*, include/mff.h):
an explicit loop over days and pairs i <= j, two-pass on the pair set.

Usable entry: state VALUE and x finite.  Pair set P_ij(d): stocks usable in both rows.
corr_ij(d): Pearson over P_ij(d) with both means taken over it; NaN when n_ij < min_pairs or
a side is constant on the pair set by the constant rule (y = x - c_i, c_i = the row's mean
over its usable set that day; constant when Q - (sum y)^2 / n <= 1e-12 * Q, Q = sum y^2 over
the pair set).  Diagonal exactly 1.0 where defined, symmetric, clamped to [-1, 1].
Spearman: each row replaced per day by its average ranks over its own usable set, then the
same (the ranks are not recomputed inside a pair set)."""
import numpy as np

ABSENT, NULL, VALUE = 0, 1, 2
CONST_REL = 1e-12


def usable(x, st):
    return (np.asarray(st) == VALUE) & np.isfinite(x)


def _rank_average_numpy(v):
    order = np.argsort(v, kind="stable")
    sv = v[order]
    r = np.empty(len(v))
    i = 0
    while i < len(v):
        j = i
        while j + 1 < len(v) and sv[j + 1] == sv[i]:
            j += 1
        r[order[i:j + 1]] = 0.5 * (i + j) + 1.0
        i = j + 1
    return r


def _rank_average(v):
    try:
        from scipy.stats import rankdata
    except ImportError:
        return _rank_average_numpy(v)
    return rankdata(v, method="average")


def ranks(x, st):
    """Rows -> per-day average ranks over each row's own usable set (state VALUE there, NULL
    elsewhere unless ABSENT)."""
    x = np.asarray(x, dtype=np.float64)
    st = np.asarray(st)
    u = usable(x, st)
    out = np.zeros_like(x)
    ost = np.where(st == ABSENT, ABSENT, NULL).astype(np.uint8)
    for r in range(x.shape[0]):
        for d in range(x.shape[1]):
            m = u[r, d]
            if m.any():
                out[r, d, m] = _rank_average(x[r, d, m])
    ost[u] = VALUE
    return out, ost


def centres(x, st):
    """[rows][D]: each row's mean over its usable set of the day (0 when it has none)."""
    u = usable(x, st)
    n = u.sum(-1)
    s = np.where(u, x, 0.0).sum(-1)
    return np.where(n > 0, s / np.maximum(n, 1), 0.0)


def corr(x, st, min_pairs=2, method="pearson"):
    """(corr float64 [D][F][F], n int32 [D][F][F])."""
    if method not in ("pearson", "spearman"):
        raise ValueError(method)
    if min_pairs < 2:
        raise ValueError(min_pairs)
    x = np.asarray(x, dtype=np.float64)
    st = np.asarray(st)
    if method == "spearman":
        x, st = ranks(x, st)
    F, D, S = x.shape
    u = usable(x, st)
    c = centres(x, st)
    out = np.full((D, F, F), np.nan)
    nn = np.zeros((D, F, F), dtype=np.int32)
    with np.errstate(all="ignore"):
        for d in range(D):
            for i in range(F):
                for j in range(i, F):
                    p = u[i, d] & u[j, d]
                    n = int(p.sum())
                    nn[d, i, j] = nn[d, j, i] = n
                    if n < min_pairs:
                        continue
                    xi, xj = x[i, d, p], x[j, d, p]
                    const = False
                    for xv, cv in ((xi, c[i, d]), (xj, c[j, d])):
                        y = xv - cv
                        q = float(np.sum(y * y))
                        const |= q - float(np.sum(y)) ** 2 / n <= CONST_REL * q
                    if const:
                        continue
                    if i == j:
                        out[d, i, i] = 1.0
                        continue
                    a, b = xi - xi.mean(), xj - xj.mean()
                    r = float(a @ b) / np.sqrt(float(a @ a) * float(b @ b))
                    out[d, i, j] = out[d, j, i] = min(1.0, max(-1.0, r)) if r == r else np.nan
    return out, nn


def corr_mean(corr_d):
    """(mean [F][F] over the days where corr is not NaN, summed in day order; days int32)."""
    corr_d = np.asarray(corr_d, dtype=np.float64)
    D, F, _ = corr_d.shape
    s = np.zeros((F, F))
    days = np.zeros((F, F), dtype=np.int32)
    for d in range(D):
        ok = ~np.isnan(corr_d[d])
        s[ok] += corr_d[d][ok]
        days += ok
    with np.errstate(all="ignore"):
        mean = np.where(days > 0, s / np.maximum(days, 1), np.nan)
    return mean, days
