"""Plain numpy restatement of the per-day factor orthogonalisation (include/mff.h,
mff_xs_orth_*), one day at a time: the listwise usable set, centring, the
correlation matrix, numpy.linalg.eigh (symmetric) / numpy.linalg.cholesky (Gram-Schmidt), the
transform, the outputs and their states, eig, keep, cond and the status rules.  It shares no
code with the engine."""
import numpy as np

ABSENT, NULL, VALUE = 0, 1, 2
CONST_REL = 1e-20
EIG_MIN = 1e-10
METHODS = ("symmetric", "schmidt")


def usable(x, xs):
    """The listwise usable set [D][S]."""
    with np.errstate(invalid="ignore"):
        return ((xs == VALUE) & np.isfinite(x)).all(axis=0)


def orth_day(X, method="symmetric", min_obs=0):
    """One day on its usable set: X [n][K].  Returns dict(status, T [K][K], eig [K], keep [K],
    cond, out [n][K])."""
    n, K = X.shape
    nan = np.full(K, np.nan)
    out = dict(status=1, T=np.full((K, K), np.nan), eig=nan, keep=nan.copy(), cond=np.nan, out=np.zeros((n, K)))
    if n < max(min_obs, K + 1):
        return out
    c = X - X.mean(axis=0)
    M = c.T @ c
    dg = np.diag(M).copy()
    if (dg <= CONST_REL * (X * X).sum(axis=0)).any():
        out["status"] = 2
        return out
    R = M / np.sqrt(np.outer(dg, dg))
    R = 0.5 * (R + R.T)
    np.fill_diagonal(R, 1.0)
    lam, V = np.linalg.eigh(R)
    if not lam[0] > EIG_MIN:
        out["status"] = 2
        return out
    if method == "symmetric":
        T = (V / np.sqrt(lam)) @ V.T
        keep = (V * V) @ np.sqrt(lam)
    else:
        L = np.linalg.cholesky(R)
        T = np.linalg.inv(L).T
        T[np.tril_indices(K, -1)] = 0.0
        keep = np.diag(L).copy()
    z = c / np.sqrt(dg / (n - 1))
    out.update(status=0, T=T, eig=lam, keep=keep, cond=float(lam[-1] / lam[0]), out=z @ T)
    return out


def orthogonalize(x, xs, method="symmetric", min_obs=0):
    """x [K][D][S] + states.  Returns dict of val / state [K][D][S], T [D][K][K], eig / keep
    [D][K], cond [D], n / status int32 [D]."""
    assert method in METHODS
    K, D, S = x.shape
    u = usable(x, xs)
    res = dict(val=np.zeros((K, D, S)), state=np.where(xs == VALUE, NULL, xs).astype(np.uint8),
               T=np.full((D, K, K), np.nan), eig=np.full((D, K), np.nan), keep=np.full((D, K), np.nan),
               cond=np.full(D, np.nan), n=np.zeros(D, np.int32), status=np.ones(D, np.int32))
    for d in range(D):
        m = u[d]
        res["n"][d] = int(m.sum())
        r = orth_day(x[:, d][:, m].T.astype(np.float64), method, min_obs)
        res["status"][d] = r["status"]
        for k in ("T", "eig", "keep", "cond"):
            res[k][d] = r[k]
        if r["status"] == 0:
            res["val"][:, d][:, m] = r["out"].T
            res["state"][:, d][:, m] = VALUE
    return res
