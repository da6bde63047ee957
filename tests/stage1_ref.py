"""Vectorised high-precision restatement of the 23 stage-1 factors of the cancelling families
(MOMR, MOMV, MOMH, CORR, OLS; csrc/mff_stage1s.hip) on the minute grid, with a
per-entry error bound for an f64 implementation of the documented algorithm.  It shares no
code with the engine or with oracle/mff_oracle.py (one Python loop per stock-day, two-pass
f64).  Input: open / high / low / close / volume planes [D][S][240] (fp32 prices, integral
volumes) and ``present`` [D][S][240]; no nulls, no off-grid rows (the row set is out of
scope).  Output of :func:`reference`: ``({name: (val, state, bound)}, {name: undecided})``,
f64 / uint8 / f64 / bool arrays [D][S].

Operations (CM:<line> of the reference's cal_* as restated in mff/catalog.py; rules S1-S12 and
C3 of DESIGN.md §4).  Rows = the present bars of a stock-day in time order, n of them; a
stock-day with n = 0 is ABSENT in every factor.
  r = close / open - 1 per row (CM:518-687).
    vol_return1min   std(r), ddof 1 (S1): NULL when n < 2.
    vol_upVol/downVol  std of the rows with r > 0 / r < 0 (S11), fill_null(0): exactly 0 when
                     the subset has fewer than 2 members or is constant (C3).
    vol_upRatio/downRatio  that value / std(r): NULL when n < 2, 0/0 = NaN when r is constant.
    shape_skew, shape_kurt  biased m3 / m2^1.5 and Fisher m4 / m2^2 - 3 (S2): n = 1 NaN,
                     constant NaN, n = 2 skew exactly 0.  shape_skratio = skew / kurt.
  vol_volume1min     std(volume), ddof 1.   share = volume / sum(volume):
    shape_skewVol, shape_kurtVol, shape_skratioVol  the same moments of the shares (a zero
                     volume sum makes the shares NaN and so the moments).
  vol_range1min      std(high / low), ddof 1.
  Pearson (S3: NaN when fewer than two pairs or a side is constant, C3), pct = pct_change in
  row order (S4, first row null):
    corr_pv (close, volume); corr_pvd (close_k, volume_k-1); corr_pvl (close_k, volume_k+1);
    corr_prv (pct close_k, volume_k); over the rows with volume != 0 re-grouped (CM:855, 924;
    ABSENT when there is none): corr_prvr (pct close, pct volume), corr_pvr (close, pct volume).
  OLS (CM:93-376): x = low, y = high; window t = the rows with minute in (t-50, t] (S12), kept
  when it has 50 rows (all 50 minutes present); ddof-0 var_x, var_y, cov, means mx, my; no
  window -> ABSENT.  beta = cov / var_x when var_x != 0, otherwise my / mx.  Over the windows
  with var_x var_y != 0: mmt_ols_corr_square_mean = mean cov^2 / (var_x var_y),
  mmt_ols_corr_mean = mean cov / sqrt(var_x var_y), csm = mean cov**0.5 / (var_x var_y)
  (cov < 0: NaN); none -> fill_null(0), csm null.  mmt_ols_beta_mean = mean beta;
  sd_b = std(beta) ddof 1 (null with one window, exactly 0 for identical betas);
  mmt_ols_beta_zscore_last = (beta_last - mean) / sd_b when sd_b > 0, otherwise the mean;
  mmt_ols_qrs = csm (beta_last - mean) / sd_b when sd_b != 0 and csm is not null, otherwise 0.

Arithmetic.  Every set is shifted by its first member and computed two-pass in np.longdouble
(64-bit mantissa on x86-64): y = x - x_first, mean_y, dev = y - mean_y, m_k = sum dev^k / n.
The quotients (close / open, high / low, pct_change, the shares) are formed in long double
too, i.e. the reference does NOT round them to f64; the definition's own rounding is part of
the bound (Q below).  The reference's own error is about n 2^-64 R^k on m_k, 2^11 below one
f64 rounding of a term.  Where np.longdouble is no wider than f64 (LONGDOUBLE_OK false), or
with ``exact=True``, all sums are fractions.Fraction in object arrays and only the final
roots are floating point.  Results are rounded to f64 once, at the end.

Bounds.  ``bound`` is the admissible |f64 implementation - reference| of a finite entry.
u = 2^-53.  ur = 2^-47 is what mff_fmath.h documents for a "refined" reciprocal or rsqrt
(one Newton step: 2.1e-15 and 4.2e-15 relative; 2^-47 = 7.1e-15), which the documented
algorithm uses for its roots and for 1 / m2, 1 / (vx vy); it is the header's figure, not a
measured one.  For a set of n members: R = max - min, ad_k = mean |dev|^k, all from the
reference.
  Q   A quotient of fp32 operands formed in f64 carries a rounding of the quotient: the
      definition (polars) rounds it once (u |q|) and the documented residual-corrected
      quotient is within about one ulp (2 u |q|): eq = 4 u max|q| absolute per member (one
      u spare for q - shift).  Raw closes and volumes are exact in f64 (eq = 0) and so are
      their differences from the shift.
  M   Shifted one-pass sums S_k = sum y^k, |y| <= R: each term carries <= (k + 1) u R^k of
      rounding, the n partial sums <= n R^k add <= n u n R^k, so a_k = S_k / n is off by
      <= (n + k + 2) u R^k.  m2 = a2 - mu^2 (mu <= R, two factors each off by n u R):
      <= 3 n u R^2 + ..; m3 = a3 - 3 mu a2 + 2 mu^3: (1 + 3 * 2 + 2 * 3) n = 13 n;
      m4 = a4 - 4 mu a3 + 6 mu^2 a2 - 3 mu^4: (1 + 8 + 18 + 12) n = 39 n.  Rounded up for the
      (k + 2) terms: E2 = 4 n u R^2, E3 = 16 n u R^3, E4 = 48 n u R^4.  A member error e_i,
      |e_i| <= eq, moves m_k to first order by (k / n) sum (dev^(k-1) - m_(k-1)) e_i, so
      dm2 = E2 + 2 eq ad_1, dm3 = E3 + 6 eq m2, dm4 = E4 + 4 eq (ad_3 + |m3|).
  std   sd = sqrt(n / (n - 1) m2): d = n / (n - 1) dm2 / (2 sd) + (ur + 2 u) sd
  skew  d = dm3 / m2^1.5 + 1.5 |skew| dm2 / m2 + (2 ur + 4 u) |skew|
  kurt  d = dm4 / m2^2 + 2 (kurt + 3) dm2 / m2 + (2 ur + 4 u) (kurt + 3) + 3 u
  First order holds while g = dm2 / m2 is small: every d is divided by 1 - 4 g, and is
  infinite (no claim) from g >= 1/8 on.  Ratios a / b (up / down ratios, skew / kurt):
  d = (d_a + |a / b| d_b) / (|b| - d_b) + 4 u |a / b|, infinite when |b| <= d_b: the bound of
  shape_skratio* grows with 1 / |kurt|.
  Pearson over n pairs, vx = sum devx^2 / n, vy, cov likewise, corr = cov / sqrt(vx vy).  The
  sums of pv / pvd / pvl / prv are shared and shifted by the day's first row, which a subset
  may not hold, and a subset's sums are the day's sums minus one row's term, so Rx, Ry are
  the ranges over all rows of the day (for prvr / pvr: over the non-zero-volume rows).
      dvx = 4 n u Rx^2 + 2 eqx adx_1, dvy alike, dcov = 4 n u Rx Ry + 2 (eqx ady_1 + eqy adx_1)
      d = dcov / sqrt(vx vy) + |corr| / 2 (dvx / vx + dvy / vy) + (ur + 4 u) |corr| + 2 u
  with the same 1 - 4 g guard, g = max(dvx / vx, dvy / vy).
  OLS.  Set H slides its second-order sums over the day, shifted by the first row's low /
  high: a bar is added on entry and subtracted 50 bars later.  At window t,
  e_t rows have entered, so each sum has seen <= 2 e_t additions of terms <= Dx^2 (Dx = max
  |low - low_first| over the rows so far, Dy alike), each rounding <= u times a partial sum
  <= 50 Dx^2; after the division by 50: <= 2 e_t u Dx^2, and the terms' own roundings and
  the mean correction fma(-Sx / 50, Sx, Sxx) (Sx is exact: fp32 differences summed in f64)
  add the same again:  Evx = 4 (e_t + 2) u Dx^2, Evy alike, Ecov = 4 (e_t + 2) u Dx Dy.
  Per window with vx vy != 0 (c = cov):
      beta = c / vx            d = Ecov / vx + |beta| Evx / vx + 4 ur |beta|
      c^2 / (vx vy)            d = 2 |c| Ecov / (vx vy) + t (Evx / vx + Evy / vy) + 4 ur t
      c / sqrt(vx vy)          d = Ecov / sqrt(vx vy) + |t| / 2 (Evx / vx + Evy / vy) + 2 ur |t|
      sqrt(c) / (vx vy)        d = t (Ecov / (2 c) + Evx / vx + Evy / vy) + (2^-24 + 4 ur) t
  (1 / (vx vy) is the square of one refined rsqrt: 2 ur, doubled for the products.)  The 2^-24
  is the hardware v_sqrt_f64's documented 2^29 ulp, which the kernel uses on purpose for
  sqrt(cov) only (every term of that mean is >= 0, §3); no other root gets it.  The fallback
  beta my / mx of a window with var_x = 0 has d = 8 u |beta| (two exact sums, two divisions by
  50, one quotient).  A mean over W windows: mean of the d plus W u max |term|.
  sd_b: |sd(b + e) - sd(b)| <= sqrt(W / (W - 1)) max |e|, plus its own shifted sums:
      d_sd = sqrt(W / (W - 1)) max d_beta + W / (W - 1) 4 W u Rb^2 / (2 sd_b) + (ur + 2 u) sd_b
  z = (beta_last - mean) / sd_b: d = (d_last + d_mean + |z| d_sd) / (sd_b - d_sd) + 4 u |z|;
  qrs = csm z: d = d_csm |z| + |csm| d_z + 4 u |qrs|.
  Constant sets and windows have bound 0: exact zeros, NaN by rule, states exact.

Undecided entries (only states are compared): a window whose cov sign is open (|cov| <= Ecov,
with var_x var_y != 0: the NaN of cov**0.5) -> mmt_ols_qrs; a non-constant window with
vx <= 8 Evx or vy <= 8 Evy (var_x var_y != 0, and beta's branch) -> all five OLS factors; betas
that differ by no more than 2 max d_beta (beta_std != 0) -> qrs and beta_zscore_last.  A
return's sign is never open for fp32 operands: close != open implies |c / o - 1| >= 2^-24.

tests/test_stage1_ref.py checks on the CPU that two f64 computations (the two-pass oracle and
a one-pass shifted / sliding restatement of the kernels' algorithm) stay inside these bounds
and that five wrong variants do not.  A constant here may be widened only with a derivation
written above and only if one of those two CPU computations exceeds it against this
reference -- never because a GPU kernel does.
"""
from fractions import Fraction

import numpy as np
from numpy.lib.stride_tricks import sliding_window_view

ABSENT, NULL, VALUE = 0, 1, 2
U = 2.0 ** -53
UR = 2.0 ** -47
HWSQRT = 2.0 ** -24
T = 240
LONGDOUBLE_OK = np.finfo(np.longdouble).nmant >= 63
LD = np.longdouble

MOMR = ["vol_return1min", "vol_upVol", "vol_upRatio", "vol_downVol", "vol_downRatio",
        "shape_skew", "shape_kurt", "shape_skratio"]
MOMV = ["vol_volume1min", "shape_skewVol", "shape_kurtVol", "shape_skratioVol"]
MOMH = ["vol_range1min"]
CORR = ["corr_prv", "corr_prvr", "corr_pv", "corr_pvd", "corr_pvl", "corr_pvr"]
OLS = ["mmt_ols_qrs", "mmt_ols_corr_square_mean", "mmt_ols_corr_mean", "mmt_ols_beta_mean",
       "mmt_ols_beta_zscore_last"]
NAMES = MOMR + MOMV + MOMH + CORR + OLS
_FRAC = np.frompyfunc(lambda v: Fraction(float(v)), 1, 1)


def _lift(a, exact):
    """f64-exact input -> the working number type (long double, or Fractions in an object array)."""
    a = np.asarray(a, np.float64)
    return _FRAC(a) if exact else a.astype(LD)


def _f(a):
    """Working type -> long double for the final formulas (Fractions through f64: one rounding)."""
    return a.astype(np.float64).astype(LD) if a.dtype == object else a


def _zero(a):
    return Fraction(0) if a.dtype == object else LD(0)


def _sum(a):
    """Sum over the last axis (object arrays: Python's exact sum)."""
    return a.sum(axis=-1)


def _div(a, b, m):
    """a / b where m, 0 elsewhere (no division outside the mask)."""
    one = Fraction(1) if a.dtype == object or getattr(b, "dtype", None) == object else LD(1)
    return np.where(m, a, _zero(a)) / np.where(m, b, one)


def _guard(d, g):
    with np.errstate(all="ignore"):
        return np.where(g < 0.125, d / (1.0 - 4.0 * g), np.inf)


def _ratio(a, da, b, db):
    """a / b with first-order bound; f64 in, (value, bound) out."""
    with np.errstate(all="ignore"):
        q = a / b
        d = np.where(np.abs(b) > db, (da + np.abs(q) * db) / (np.abs(b) - db) + 4 * U * np.abs(q), np.inf)
    return q, np.where(np.isfinite(q), d, 0.0)


def moments(X, M, eq):
    """Shifted two-pass moments of the members M of X ([N][K] working type, bool); eq [N] f64 is
    the per-member input error (Q).  Returns a dict of f64 [N] arrays (long double inside)."""
    N = X.shape[0]
    n = M.sum(axis=1)
    z = _zero(X)
    first = X[np.arange(N), M.argmax(axis=1)]
    y = np.where(M, X - first[:, None], z)
    nn = np.maximum(n, 1)
    mean = _sum(y) / nn
    dev = np.where(M, y - mean[:, None], z)
    d2 = dev * dev
    m2, m3, m4 = _sum(d2) / nn, _sum(d2 * dev) / nn, _sum(d2 * d2) / nn
    ad = np.abs(dev)
    ad1, ad3 = _f(_sum(ad) / nn), _f(_sum(ad * d2) / nn)
    yf = _f(y).astype(np.float64)
    R = np.where(M, yf, -np.inf).max(axis=1) - np.where(M, yf, np.inf).min(axis=1)
    R = np.where(n > 0, R, 0.0)
    const = (m2 == z) & (n > 0)          # exact: every member equals the first
    m2, m3, m4 = _f(m2), _f(m3), _f(m4)
    nf = n.astype(np.float64)
    with np.errstate(all="ignore"):
        dm2 = 4 * nf * U * R ** 2 + 2 * eq * ad1
        dm3 = 16 * nf * U * R ** 3 + 6 * eq * m2
        dm4 = 48 * nf * U * R ** 4 + 4 * eq * (ad3 + np.abs(m3))
        g = (dm2 / m2).astype(np.float64)
        sd = np.sqrt(m2 * nn / np.maximum(n - 1, 1))
        dsd = _guard(nf / np.maximum(nf - 1, 1) * dm2 / (2 * sd) + (UR + 2 * U) * sd, g)
        sk = m3 / m2 ** LD(1.5)
        dsk = _guard(dm3 / m2 ** LD(1.5) + 1.5 * np.abs(sk) * dm2 / m2 + (2 * UR + 4 * U) * np.abs(sk), g)
        ku = m4 / (m2 * m2) - 3
        dku = _guard(dm4 / (m2 * m2) + 2 * (ku + 3) * dm2 / m2 + (2 * UR + 4 * U) * (ku + 3) + 3 * U, g)
    gen = (n >= 2) & ~const
    f64 = lambda a, fill: np.where(gen, a, fill).astype(np.float64)
    sk, dsk = np.where(n == 2, 0.0, sk), np.where(n == 2, 0.0, dsk)
    return {"n": n, "const": const, "gen": gen, "sd": f64(sd, 0.0), "dsd": f64(dsd, 0.0),
            "skew": f64(sk, np.nan), "dskew": f64(dsk, 0.0), "kurt": f64(ku, np.nan), "dkurt": f64(dku, 0.0)}


def pearson(X, Y, P, eqx, eqy, Rx, Ry):
    """Pearson over the pairs P of (X, Y); Rx, Ry [N] f64 the ranges the sums are relative to.
    Returns (val, bound) f64 [N] (NaN, 0 for fewer than two pairs or a constant side)."""
    N = X.shape[0]
    n = P.sum(axis=1)
    nn = np.maximum(n, 1)
    z = _zero(X)
    i0 = P.argmax(axis=1)
    dx = np.where(P, X - X[np.arange(N), i0][:, None], z)
    dy = np.where(P, Y - Y[np.arange(N), i0][:, None], z)
    ex = np.where(P, dx - (_sum(dx) / nn)[:, None], z)
    ey = np.where(P, dy - (_sum(dy) / nn)[:, None], z)
    vx, vy, cov = _sum(ex * ex) / nn, _sum(ey * ey) / nn, _sum(ex * ey) / nn
    ok = (n >= 2) & (vx != z) & (vy != z)
    adx, ady = _f(_sum(np.abs(ex)) / nn), _f(_sum(np.abs(ey)) / nn)
    vx, vy, cov = _f(vx), _f(vy), _f(cov)
    nf = n.astype(np.float64)
    with np.errstate(all="ignore"):
        dvx = 4 * nf * U * Rx ** 2 + 2 * eqx * adx
        dvy = 4 * nf * U * Ry ** 2 + 2 * eqy * ady
        dcov = 4 * nf * U * Rx * Ry + 2 * (eqx * ady + eqy * adx)
        root = np.sqrt(vx * vy)
        c = cov / root
        g = np.maximum(dvx / vx, dvy / vy).astype(np.float64)
        d = _guard(dcov / root + np.abs(c) / 2 * (dvx / vx + dvy / vy) + (UR + 4 * U) * np.abs(c) + 2 * U, g)
    return np.where(ok, c, np.nan).astype(np.float64), np.where(ok, d, 0.0).astype(np.float64)


def _compact(M, *arrays):
    """Members first, in time order: (member mask [N][K], arrays reordered)."""
    order = np.argsort(~M, axis=1, kind="stable")
    n = M.sum(axis=1)
    return (np.arange(M.shape[1])[None, :] < n[:, None],) + tuple(np.take_along_axis(a, order, axis=1) for a in arrays)


def _range(X, M):
    x = _f(X).astype(np.float64)
    r = np.where(M, x, -np.inf).max(axis=1) - np.where(M, x, np.inf).min(axis=1)
    return np.where(M.any(axis=1), r, 0.0)


def _absmax(X, M):
    return np.where(M, np.abs(_f(X).astype(np.float64)), 0.0).max(axis=1)


def _pct(X, Mc):
    """pct_change of compacted rows: (values, mask of rows 1..n-1)."""
    P = Mc.copy()
    P[:, 0] = False
    prev = np.concatenate([X[:, :1], X[:, :-1]], axis=1)
    return _div(X - prev, prev, P), P


def _ols(lo, hi, M):
    """Per stock-day OLS factors.  Returns {name: (val, state, bound, undecided)} [N]."""
    N = lo.shape[0]
    Wn = T - 49
    ok = sliding_window_view(M, 50, axis=1).all(axis=2)                  # [N][191], window ends at 49 + j
    x = sliding_window_view(lo, 50, axis=1)
    y = sliding_window_view(hi, 50, axis=1)
    z = _zero(lo)
    okb = ok[:, :, None]
    dx = np.where(okb, x - x[:, :, :1], z)
    dy = np.where(okb, y - y[:, :, :1], z)
    sx, sy = _sum(dx) / 50, _sum(dy) / 50
    ex, ey = dx - sx[:, :, None], dy - sy[:, :, None]
    vx, vy, cv = _sum(ex * ex) / 50, _sum(ey * ey) / 50, _sum(ex * ey) / 50
    cx, cy = ok & (vx == z), ok & (vy == z)
    mx, my = _f(x[:, :, 0] + sx), _f(y[:, :, 0] + sy)
    vx, vy, cv = _f(vx), _f(vy), _f(cv)
    # the day's shifted ranges over the rows entered so far
    first = M.argmax(axis=1)
    lof, hif = _f(lo).astype(np.float64), _f(hi).astype(np.float64)
    Dx = np.maximum.accumulate(np.where(M, np.abs(lof - lof[np.arange(N), first][:, None]), 0.0), axis=1)[:, 49:]
    Dy = np.maximum.accumulate(np.where(M, np.abs(hif - hif[np.arange(N), first][:, None]), 0.0), axis=1)[:, 49:]
    et = np.cumsum(M, axis=1)[:, 49:].astype(np.float64)
    Evx, Evy, Ecv = 4 * (et + 2) * U * Dx ** 2, 4 * (et + 2) * U * Dy ** 2, 4 * (et + 2) * U * Dx * Dy
    reg = ok & ~cx & ~cy                                                  # var_x var_y != 0
    fb = ok & cx                                                          # beta = my / mx
    und_var = (ok & ~cx & (vx <= 8 * Evx)) | (ok & ~cy & (vy <= 8 * Evy))
    with np.errstate(all="ignore"):
        prod = vx * vy
        rx, ry = Evx / vx, Evy / vy
        cov0 = np.where(cy, 0.0, cv)                                      # constant high: cov exactly 0
        beta = np.where(fb, my / mx, cov0 / vx)
        dbeta = np.where(fb, 8 * U * np.abs(beta),
                         np.where(cy, 0.0, Ecv / vx + np.abs(beta) * rx + 4 * UR * np.abs(beta)))
        cs = cv * cv / prod
        dcs = 2 * np.abs(cv) * Ecv / prod + cs * (rx + ry) + 4 * UR * cs
        cr = cv / np.sqrt(prod)
        dcr = Ecv / np.sqrt(prod) + np.abs(cr) / 2 * (rx + ry) + 2 * UR * np.abs(cr)
        q = np.sqrt(cv) / prod                                            # NaN for cov < 0
        dq = q * (Ecv / (2 * cv) + rx + ry) + (HWSQRT + 4 * UR) * q
    und_cov = reg & (np.abs(cv) <= Ecv)
    out = {}
    W = ok.sum(axis=1)
    Wq = reg.sum(axis=1)
    have = W > 0
    Wf, Wqf = np.maximum(W, 1).astype(np.float64), np.maximum(Wq, 1).astype(np.float64)

    def mean_of(v, d, m, cnt):
        with np.errstate(all="ignore"):
            val = np.where(m, v, 0).sum(axis=1) / cnt
            nanrow = (m & np.isnan(v)).any(axis=1)
            bnd = np.where(m, d, 0).sum(axis=1) / cnt + cnt * U * np.where(m, np.abs(v), 0).max(axis=1)
        return np.where(nanrow, np.nan, val), np.where(nanrow, 0.0, bnd)

    state = np.where(have, VALUE, ABSENT).astype(np.uint8)
    und_all = und_var.any(axis=1)
    for nm, v, d in (("mmt_ols_corr_square_mean", cs, dcs), ("mmt_ols_corr_mean", cr, dcr)):
        val, bnd = mean_of(v, d, reg, Wqf)
        val, bnd = np.where(Wq > 0, val, 0.0), np.where(Wq > 0, bnd, 0.0)
        out[nm] = (val, bnd, und_all)
    csm, dcsm = mean_of(q, dq, reg, Wqf)
    bm, dbm = mean_of(beta, dbeta, ok, Wf)
    out["mmt_ols_beta_mean"] = (bm, dbm, und_all)
    # std of the betas, shifted by the first one
    j0 = ok.argmax(axis=1)
    b0 = beta[np.arange(N), j0]
    db = np.where(ok, beta - b0[:, None], 0)
    spread = np.where(ok, db, -np.inf).max(axis=1) - np.where(ok, db, np.inf).min(axis=1)
    spread = np.where(have, spread, 0).astype(np.float64)
    emax = np.where(ok, dbeta, 0.0).max(axis=1).astype(np.float64)
    mb = db.sum(axis=1) / Wf
    with np.errstate(all="ignore"):
        sdb = np.sqrt(np.where(ok, (db - mb[:, None]) ** 2, 0).sum(axis=1) / np.maximum(W - 1, 1))
        dsd = (np.sqrt(Wf / np.maximum(Wf - 1, 1)) * emax
               + Wf / np.maximum(Wf - 1, 1) * 4 * Wf * U * spread ** 2 / (2 * sdb) + (UR + 2 * U) * sdb)
        j1 = Wn - 1 - ok[:, ::-1].argmax(axis=1)
        bl, dbl = beta[np.arange(N), j1], dbeta[np.arange(N), j1]
        zz = (bl - bm) / sdb
        dz = np.where(sdb > dsd, (dbl + dbm + np.abs(zz) * dsd) / (sdb - dsd) + 4 * U * np.abs(zz), np.inf)
    has_sd = (W >= 2) & (spread > 0)
    und_sd = (W >= 2) & (spread > 0) & (spread <= 2 * emax)
    zval = np.where(has_sd, zz, bm)
    zbnd = np.where(has_sd, dz, dbm)
    out["mmt_ols_beta_zscore_last"] = (zval, zbnd, und_all | und_sd)
    with np.errstate(all="ignore"):
        qrs = csm * zz
        dqrs = dcsm * np.abs(zz) + np.abs(csm) * dz + 4 * U * np.abs(qrs)
    use = has_sd & (Wq > 0)
    qv = np.where(use, qrs, 0.0)
    qb = np.where(use & np.isfinite(qrs), dqrs, 0.0)
    out["mmt_ols_qrs"] = (qv, qb, und_all | und_sd | und_cov.any(axis=1))
    res = {}
    for nm, (v, b, un) in out.items():
        v = np.where(have, v, 0.0).astype(np.float64)
        b = np.where(have & ~np.isnan(v), b, 0.0).astype(np.float64)
        res[nm] = (v, state.copy(), b, un & have)
    return res


def reference(open_, high, low, close, volume, present, exact=False):
    """The 23 factors of the planes [D][S][240] (or [S][240]).  Returns
    ({name: (val f64, state u8, bound f64)}, {name: undecided bool}), arrays [D][S]."""
    present = np.asarray(present, bool)
    shape = present.shape[:-1]
    assert present.shape[-1] == T
    exact = exact or not LONGDOUBLE_OK
    M = present.reshape(-1, T)
    N = M.shape[0]
    clean = lambda a, fill: np.where(M, np.asarray(a, np.float64).reshape(-1, T), fill)
    o, h, lo, c = (_lift(clean(a, 1.0), exact) for a in (open_, high, low, close))
    v = _lift(clean(volume, 0.0), exact)
    n = M.sum(axis=1)
    z = _zero(o)
    out = {}
    st_val = np.where(n > 0, VALUE, ABSENT).astype(np.uint8)
    st_std = np.where(n > 1, VALUE, np.where(n > 0, NULL, ABSENT)).astype(np.uint8)

    def put(nm, val, st, bnd, und=None):
        val = np.where(st == VALUE, val, 0.0).astype(np.float64)
        with np.errstate(invalid="ignore"):
            bnd = np.where((st == VALUE) & ~np.isnan(val), bnd, 0.0).astype(np.float64)
        out[nm] = (val, st, bnd, np.zeros(N, bool) if und is None else und)

    # ---- MOMR
    q = _div(c, o, M)
    r = np.where(M, q - 1, z)
    eq = 4 * U * _absmax(q, M)
    mr = moments(r, M, eq)
    put("vol_return1min", mr["sd"], st_std, mr["dsd"])
    put("shape_skew", mr["skew"], st_val, mr["dskew"])
    put("shape_kurt", mr["kurt"], st_val, mr["dkurt"])
    put("shape_skratio", *_ins(_ratio(mr["skew"], mr["dskew"], mr["kurt"], mr["dkurt"]), st_val))
    for nm, sel in (("up", M & (r > z)), ("down", M & (r < z))):
        ms = moments(r, sel, eq)
        put(f"vol_{nm}Vol", ms["sd"], st_val, ms["dsd"])
        with np.errstate(all="ignore"):
            ratio, dr = _ratio(ms["sd"], ms["dsd"], mr["sd"], mr["dsd"])
        put(f"vol_{nm}Ratio", ratio, st_std, dr)
    # ---- MOMV
    mv = moments(v, M, np.zeros(N))
    put("vol_volume1min", mv["sd"], st_std, mv["dsd"])
    tot = _sum(np.where(M, v, z))
    pos = tot > z
    share = _div(v, np.where(pos, tot, z + 1)[:, None], M)
    ms = moments(share, M, 4 * U * _absmax(share, M))
    nanv = lambda a: np.where(pos, a, np.nan)
    put("shape_skewVol", nanv(ms["skew"]), st_val, ms["dskew"])
    put("shape_kurtVol", nanv(ms["kurt"]), st_val, ms["dkurt"])
    put("shape_skratioVol", *_ins(_ratio(nanv(ms["skew"]), ms["dskew"], nanv(ms["kurt"]), ms["dkurt"]), st_val))
    # ---- MOMH
    hl = _div(h, lo, M)
    mh = moments(hl, M, 4 * U * _absmax(hl, M))
    put("vol_range1min", mh["sd"], st_std, mh["dsd"])
    # ---- CORR
    Mc, cc, vc = _compact(M, c, v)
    Rc, Rv = _range(cc, Mc), _range(vc, Mc)
    z0 = np.zeros(N)
    put("corr_pv", *_ins(pearson(cc, vc, Mc, z0, z0, Rc, Rv), st_val))
    P1 = Mc.copy()
    P1[:, 0] = False
    vprev = np.concatenate([vc[:, :1], vc[:, :-1]], axis=1)
    cprev = np.concatenate([cc[:, :1], cc[:, :-1]], axis=1)
    put("corr_pvd", *_ins(pearson(cc, vprev, P1, z0, z0, Rc, Rv), st_val))
    put("corr_pvl", *_ins(pearson(cprev, vc, P1, z0, z0, Rc, Rv), st_val))
    pc, P = _pct(cc, Mc)
    eqp = 4 * U * _absmax(pc, P)
    put("corr_prv", *_ins(pearson(pc, vc, P, eqp, z0, _range(pc, P), Rv), st_val))
    Z = M & (v != z)
    Zc, cz, vz = _compact(Z, c, v)
    st_z = np.where(Z.any(axis=1), VALUE, ABSENT).astype(np.uint8)
    pcz, PZ = _pct(cz, Zc)
    pvz, _ = _pct(vz, Zc)
    eqc, eqv = 4 * U * _absmax(pcz, PZ), 4 * U * _absmax(pvz, PZ)
    put("corr_prvr", *_ins(pearson(pcz, pvz, PZ, eqc, eqv, _range(pcz, PZ), _range(pvz, PZ)), st_z))
    put("corr_pvr", *_ins(pearson(cz, pvz, PZ, z0, eqv, _range(cz, Zc), _range(pvz, PZ)), st_z))
    # ---- OLS
    for nm, (val, st, bnd, und) in _ols(lo, h, M).items():
        out[nm] = (val, st, bnd, und)
    res = {nm: tuple(a.reshape(shape) for a in out[nm][:3]) for nm in NAMES}
    und = {nm: out[nm][3].reshape(shape) for nm in NAMES}
    return res, und


def _ins(vb, st):
    """(val, bound) -> (val, state, bound) argument order of put()."""
    return vb[0], st, vb[1]


def counts(open_, close, present):
    """(n, n_up, n_down, n_flat) per stock-day from exact comparisons of the fp32 planes."""
    M = np.asarray(present, bool)
    o, c = np.asarray(open_, np.float64), np.asarray(close, np.float64)
    with np.errstate(invalid="ignore"):
        return M.sum(-1), (M & (c > o)).sum(-1), (M & (c < o)).sum(-1), (M & (c == o)).sum(-1)


def check(gv, gs, ref, name, undecided=None):
    """Compare an implementation's (gv, gs) with ref = (val, state, bound).  States exact
    everywhere; values (NaN pattern, infinities by sign, finite inside the bound) outside the
    undecided entries.  Returns (mismatch descriptions, worst |error| / bound over the
    compared entries with a finite bound > 0)."""
    rv, rs, rb = ref
    gv, gs = np.asarray(gv, np.float64), np.asarray(gs)
    bad = []
    st = gs != rs
    if st.any():
        i = tuple(np.argwhere(st)[0])
        bad.append(f"{name}: {int(st.sum())} state mismatches, first at {i}: got {gs[i]} ref {rs[i]}")
    m = ~st if undecided is None else ~st & ~undecided
    nn = m & (np.isnan(gv) != np.isnan(rv))
    if nn.any():
        i = tuple(np.argwhere(nn)[0])
        bad.append(f"{name}: {int(nn.sum())} NaN mismatches, first at {i}: got {gv[i]!r} ref {rv[i]!r}")
    f = m & ~np.isnan(gv) & ~np.isnan(rv)
    with np.errstate(invalid="ignore"):
        err = np.where(f & (gv != rv), np.abs(gv - rv), 0.0)
    err = np.where(np.isnan(err), np.inf, err)
    over = err > rb
    if over.any():
        with np.errstate(all="ignore"):
            ex = np.where(over, np.where(rb > 0, err / rb, np.inf), 0.0)
        i = tuple(np.unravel_index(np.argmax(ex), ex.shape))
        bad.append(f"{name}: {int(over.sum())} entries past the bound, worst at {i}: got {gv[i]!r} "
                   f"ref {rv[i]!r} err {err[i]:.3e} bound {rb[i]:.3e}")
    pos = f & (rb > 0) & np.isfinite(rb)
    ratio = float((err[pos] / rb[pos]).max()) if pos.any() else 0.0
    return bad, ratio
