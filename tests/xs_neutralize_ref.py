"""numpy restatement of mff_xs_neutralize (include/mff.h): per-day MAD winsorisation,
industry / size neutralisation by within-industry demeaning, ddof-1 standardisation.
The checker of tests/test_gpu_neutralize.py; tests/test_xs_neutralize.py pins it against
an explicit least-squares formulation and hand-made segments."""
import numpy as np

ABSENT, NULL, VALUE = 0, 1, 2


def usable(x, state, g=None, G=None, z=None, z_state=None):
    """The usable set U of one segment (bool [S])."""
    u = (state == VALUE) & np.isfinite(x)
    if g is not None:
        u &= (g >= 0) & (g < G)
    if z is not None:
        u &= (z_state == VALUE) & np.isfinite(z)
    return u


def winsorize(xu, winsor_k):
    """Step 1 on the usable values."""
    if winsor_k <= 0 or xu.size == 0:
        return xu
    med = np.median(xu)
    mad = np.median(np.abs(xu - med))
    if not mad > 0:
        return xu
    w = (winsor_k * 1.4826) * mad
    return np.minimum(np.maximum(xu, med - w), med + w)


def segment(x, state, g=None, G=None, z=None, z_state=None, winsor_k=3.0, standardize=True):
    """One segment (one factor row on one day) -> (out_val, out_state) [S]."""
    x = np.asarray(x, dtype=np.float64)
    state = np.asarray(state)
    S = x.size
    ov = np.zeros(S)
    os_ = state.astype(np.uint8).copy()
    passes = (state == VALUE) & ~np.isfinite(x)
    ov[passes] = x[passes]
    u = usable(x, state, g, G, z, z_state)
    os_[(state == VALUE) & np.isfinite(x) & ~u] = NULL
    n = int(u.sum())
    if n == 0:
        return ov, os_
    xu = winsorize(x[u].copy(), winsor_k)
    gu = np.asarray(g)[u] if g is not None else np.zeros(n, dtype=np.int64)
    zu = np.asarray(z, dtype=np.float64)[u] if z is not None else None
    k = len(np.unique(gu)) + (1 if z is not None else 0)
    if n - k < 1 or (standardize and n < 2):
        os_[u] = NULL
        return ov, os_
    xt = xu.copy()
    zt = zu.copy() if zu is not None else None
    for gi in np.unique(gu):
        m = gu == gi
        xt[m] -= xu[m].mean()
        if zt is not None:
            zt[m] -= zu[m].mean()
    e = xt
    if zt is not None:
        szz = float((zt * zt).sum())
        beta = float((xt * zt).sum()) / szz if szz > 0 else 0.0
        e = xt - beta * zt
    if standardize:
        with np.errstate(invalid="ignore", divide="ignore"):
            e = (e - e.mean()) / np.sqrt(((e - e.mean()) ** 2).sum() / (n - 1))
    ov[u] = e
    return ov, os_


def neutralize(val, state, group=None, G=None, size=None, size_state=None, winsor_k=3.0, standardize=True):
    """[rows][D][S] exposures, [D][S] side inputs -> (out_val, out_state) [rows][D][S]."""
    val = np.asarray(val, dtype=np.float64)
    state = np.asarray(state)
    rows, D, S = val.shape
    ov = np.zeros_like(val)
    os_ = np.zeros(val.shape, dtype=np.uint8)
    for r in range(rows):
        for d in range(D):
            ov[r, d], os_[r, d] = segment(
                val[r, d], state[r, d], None if group is None else group[d], G,
                None if size is None else size[d], None if size is None else size_state[d],
                winsor_k, standardize)
    return ov, os_
