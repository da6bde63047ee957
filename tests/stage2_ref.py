"""Vectorised high-precision restatement of stage 2, the N-day rolling mean / z / std of
``cal_final_exposure(N, method, mode='days')`` (include/mff.h, mff_stage2),
with a per-entry error bound for an f64 implementation.  It shares no code with the engine
or with oracle/mff_oracle.py (which is one Python loop per window and plain f64).

Operation.  Per (row, stock) the non-ABSENT days are compacted in date order and windows of
the last N of them are taken.  The output on a present day is NULL for the first N - 1
present days and for a window holding a NULL; ABSENT days give state 0, value 0; 'o' passes
value and state through (a NULL's value is 0).  std is ddof = 0, z = (x - mean) / std with x
the window's newest value.  A window whose values are finite and identical gives mean
exactly the value, std exactly 0.0 and z NaN (rule C6); a window holding NaN or both
infinities gives mean NaN, std NaN; one sign of infinity gives mean +-inf, std NaN; z is NaN
in all three.

Arithmetic.  Finite windows are computed two-pass in np.longdouble (64-bit mantissa on
x86-64) after subtracting the window's oldest value, which is a member of the window:
y = x - x[0], mean = x[0] + sum(y) / N, var = sum((y - mean_y)^2) / N.  With the shift every
long-double operation has an error relative to the window's range R and not to its level,
so the reference's own error is about N * 2^-64 * R, 2^11 times below one f64 rounding of a
term.  Where np.longdouble is no wider than f64 the sums are exact fractions.Fraction.
Results are rounded to f64 once, at the end.

Bounds.  ``bound`` is the admissible |f64 implementation - reference| per entry, for finite
non-constant windows.  u = 2^-53, R = max - min and A = max |x| of the window, sd the
reference std:

  mean  2 u A + 2 N u R
        An f64 implementation that shifts by a member c of the window forms N terms
        x - c, each with |x - c| <= R and a rounding error <= u R; it sums N of them,
        the partial sums bounded by N R, which adds <= (N - 1) u N R before the division
        by N, i.e. <= N u R on the mean; together < 2 N u R.  The final c + m is one add
        at the level of the data, error <= u A, and the reference's own rounding to f64
        is another u A.
  std   8 N^1.5 u R
        The variance of N shifted terms, each squared term <= R^2 and computed with a
        relative error of a few u, summed over N: error <= 4 N u R^2 (per term: 2 u from
        the rounding of x - c entering squared, 1 u from the square or its fma, and the
        partial sums <= N R^2 give N u R^2 / N per add, with the mean correction the
        same again).  A non-constant window has two values R apart, so its variance is
        at least R^2 / (2 N), sd >= R / sqrt(2 N).  d(sd) = d(var) / (2 sd)
        <= 4 N u R^2 sqrt(2 N) / (2 R) = 2 sqrt(2) N^1.5 u R < 8 N^1.5 u R; the factor
        2 sqrt(2) left over covers the final square root and the rounding of the
        reference.
  z     (bound_mean + |z| bound_std) / sd + 4 u |z|
        First-order propagation of the two errors through (x - mean) / sd, plus the
        roundings of the subtraction, the division and the reference.

Constant windows and windows holding a non-finite value have bound 0: the result must match
exactly (NaN matching NaN, infinities by sign).  tests/test_stage2_ref.py checks on the CPU
that f64 computations of the shifted form stay inside these bounds, i.e. that they are not
tighter than f64 allows.  A constant here may be widened only with a derivation written
above and only if such an f64 computation on the CPU exceeds it against this reference --
never because a GPU kernel does.
"""
from fractions import Fraction
import math

import numpy as np
from numpy.lib.stride_tricks import sliding_window_view

ABSENT, NULL, VALUE = 0, 1, 2
METHODS = ("o", "m", "z", "std")
U = 2.0 ** -53
# x86-64: 63 explicit fraction bits.  Elsewhere (long double == double) the sums are Fractions.
LONGDOUBLE_OK = np.finfo(np.longdouble).nmant >= 63


def bounds(N, R, A, sd, z):
    """(bound_mean, bound_std, bound_z) from the formulas of the module docstring (f64 arrays)."""
    bm = 2.0 * U * A + 2.0 * N * U * R
    bs = 8.0 * N ** 1.5 * U * R
    with np.errstate(all="ignore"):
        bz = (bm + np.abs(z) * bs) / sd + 4.0 * U * np.abs(z)
    return bm, bs, bz


def _finite_longdouble(W):
    """Shifted two-pass over finite windows W [M][N] (f64): f64 (mean, sd, z)."""
    N = W.shape[1]
    L = W.astype(np.longdouble)
    y = L - L[:, :1]
    my = y.sum(axis=1) / N
    dev = y - my[:, None]
    sd = np.sqrt((dev * dev).sum(axis=1) / N)
    with np.errstate(all="ignore"):
        z = dev[:, -1] / sd
    return (L[:, 0] + my).astype(np.float64), sd.astype(np.float64), z.astype(np.float64)


def _finite_fraction(W):
    """The same with exact rational sums (hosts whose long double is f64)."""
    M, N = W.shape
    mean, sd, z = np.empty(M), np.empty(M), np.empty(M)
    for i in range(M):
        x = [Fraction(float(t)) for t in W[i]]
        m = sum(x) / N
        var = sum((t - m) ** 2 for t in x) / N
        mean[i] = float(m)
        # sqrt to ~2^-100 relative: integer square root of the scaled fraction
        sc = 1 << 200
        root = Fraction(math.isqrt(var.numerator * sc * sc // var.denominator), sc) if var > 0 else Fraction(0)
        sd[i] = float(root)
        z[i] = float((x[-1] - m) / root) if root > 0 else np.nan
    return mean, sd, z


def column_stats(x, isnull, N):
    """One stock's present days: x [K] f64 (0 where null), isnull [K] bool.  Returns dict of
    [K] arrays: ok (False: the output is NULL), mean, std, z, and bound_m / bound_std / bound_z."""
    K = x.shape[0]
    out = {k: np.zeros(K) for k in ("mean", "std", "z", "bound_m", "bound_std", "bound_z")}
    out["ok"] = np.zeros(K, bool)
    if K < N:
        return out
    W = sliding_window_view(x, N)                      # [K - N + 1][N], window k ends on row k + N - 1
    ok = ~sliding_window_view(isnull, N).any(axis=1)
    M = W.shape[0]
    mean, sd, z = np.full(M, np.nan), np.full(M, np.nan), np.full(M, np.nan)
    bm, bs, bz = np.zeros(M), np.zeros(M), np.zeros(M)
    nan = np.isnan(W).any(axis=1)
    pinf = (W == np.inf).any(axis=1)
    ninf = (W == -np.inf).any(axis=1)
    fin = ~(nan | pinf | ninf)
    mean[pinf & ~ninf & ~nan] = np.inf
    mean[ninf & ~pinf & ~nan] = -np.inf
    const = fin & (W == W[:, :1]).all(axis=1)
    mean[const] = W[const, 0]
    sd[const] = 0.0
    gen = fin & ~const & ok
    if gen.any():
        Wg = W[gen]
        mean[gen], sd[gen], z[gen] = (_finite_longdouble if LONGDOUBLE_OK else _finite_fraction)(Wg)
        R = Wg.max(axis=1) - Wg.min(axis=1)
        A = np.abs(Wg).max(axis=1)
        bm[gen], bs[gen], bz[gen] = bounds(N, R, A, sd[gen], z[gen])
    sl = slice(N - 1, K)
    out["ok"][sl] = ok
    for k, a in (("mean", mean), ("std", sd), ("z", z), ("bound_m", bm), ("bound_std", bs), ("bound_z", bz)):
        out[k][sl] = np.where(ok, a, 0.0)
    return out


def rolling_all(val, state, N):
    """Every method at once (one pass over the windows): {method: (val, state, bound)}."""
    val, state = np.asarray(val, np.float64), np.asarray(state, np.uint8)
    if val.ndim == 2:
        r = rolling_all(val[None], state[None], N)
        return {m: tuple(a[0] for a in t) for m, t in r.items()}
    assert val.shape == state.shape and val.ndim == 3 and N >= 1
    rows, D, S = val.shape
    res = {m: (np.zeros_like(val), np.zeros_like(state), np.zeros_like(val)) for m in METHODS}
    keys = {"m": ("mean", "bound_m"), "z": ("z", "bound_z"), "std": ("std", "bound_std")}
    for r in range(rows):
        for s in range(S):
            idx = np.flatnonzero(state[r, :, s] != ABSENT)
            if idx.size == 0:
                continue
            isnull = state[r, idx, s] == NULL
            x = np.where(isnull, 0.0, val[r, idx, s])
            res["o"][0][r, idx, s] = x
            res["o"][1][r, idx, s] = state[r, idx, s]
            c = column_stats(x, isnull, N)
            for m, (kv, kb) in keys.items():
                res[m][0][r, idx, s] = c[kv]
                res[m][1][r, idx, s] = np.where(c["ok"], VALUE, NULL)
                res[m][2][r, idx, s] = c[kb]
    return res


def rolling(val, state, N, method):
    """Stage 2 on [rows][D][S] or [D][S]: (val, state, bound), f64 / uint8 / f64."""
    if method not in METHODS:
        raise ValueError("Unknown method")
    return rolling_all(val, state, N)[method]


def check(gv, gs, ref, name):
    """Compare an implementation's (gv, gs) with ref = (val, state, bound).  Returns
    (mismatch descriptions, worst |error| / bound over the entries with bound > 0)."""
    rv, rs, rb = ref
    gv, gs = np.asarray(gv), np.asarray(gs)
    bad = []
    st = gs != rs
    if st.any():
        i = tuple(np.argwhere(st)[0])
        bad.append(f"{name}: {int(st.sum())} state mismatches, first at {i}: got {gs[i]} ref {rs[i]}")
    m = ~st
    nn = m & (np.isnan(gv) != np.isnan(rv))
    if nn.any():
        i = tuple(np.argwhere(nn)[0])
        bad.append(f"{name}: {int(nn.sum())} NaN mismatches, first at {i}: got {gv[i]!r} ref {rv[i]!r}")
    f = m & ~np.isnan(gv) & ~np.isnan(rv)
    with np.errstate(invalid="ignore"):
        err = np.where(f & (gv != rv), np.abs(gv - rv), 0.0)  # equal infinities: 0, unequal: inf / nan
    err = np.where(np.isnan(err), np.inf, err)
    over = err > rb
    if over.any():
        with np.errstate(all="ignore"):
            ex = np.where(over, np.where(rb > 0, err / rb, np.inf), 0.0)
        i = tuple(np.unravel_index(np.argmax(ex), ex.shape))
        bad.append(f"{name}: {int(over.sum())} entries past the bound, worst at {i}: got {gv[i]!r} "
                   f"ref {rv[i]!r} err {err[i]:.3e} bound {rb[i]:.3e}")
    pos = rb > 0
    ratio = float((err[pos] / rb[pos]).max()) if pos.any() else 0.0
    return bad, ratio
