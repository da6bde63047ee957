"""Plain numpy restatement of the daily group portfolios (the definition on the mff_pf_*
declarations of include/mff.h).  Loops over the dates, vectorised over the
stocks; shares no code with mff/.  Sums over the stocks are numpy's (pairwise) sums: the
order of the kernels is theirs, the tests bound the difference.

States: 0 = ABSENT, 1 = NULL, 2 = VALUE."""
from typing import NamedTuple, Optional

import numpy as np

ABSENT, NULLV, VALUE = 0, 1, 2


class Signal(NamedTuple):
    m: np.ndarray     # int64 [P][S]: membership, -1 = none
    u: np.ndarray     # f64 [P][S]: raw weight (0 where m = -1)
    cend: np.ndarray  # f64 [P][S]: growth over the period (1 when not held)
    c: np.ndarray     # f64 [D][S]: growth from the period's first date to d


class Portfolios(NamedTuple):
    ret: np.ndarray     # f64 [D][G]
    count: np.ndarray   # int64 [P][G]
    traded: np.ndarray  # f64 [P][G]
    V: np.ndarray       # f64 [D][G]
    U: np.ndarray       # f64 [P][G]
    A: np.ndarray       # f64 [D][G]
    union: np.ndarray   # int64 [P][G]: stocks in m(p) = g or m(p-1) = g
    sig: Signal


def period_bounds(period_of, P):
    period_of = np.asarray(period_of)
    lo = np.searchsorted(period_of, np.arange(P), side="left")
    hi = np.searchsorted(period_of, np.arange(P), side="right")
    return lo, hi


def signal(group, x_state, pct, pct_state, period_of, P, w=None, w_state=None) -> Signal:
    """One factor: group int [D][S], x_state [D][S]."""
    D, S = x_state.shape
    lo, hi = period_bounds(period_of, P)
    m = np.full((P, S), -1, np.int64)
    u = np.zeros((P, S))
    cend = np.ones((P, S))
    c = np.ones((D, S))
    g_prev = np.full(S, -1, np.int64)
    u_prev = np.zeros(S)
    has_prev = np.zeros(S, bool)
    for p in range(P):
        held = np.zeros(S, bool)
        prod = np.ones(S)
        g_last = np.full(S, -1, np.int64)
        u_last = np.ones(S)
        for d in range(lo[p], hi[p]):
            row = x_state[d] != ABSENT
            held |= row
            mul = row & (pct_state[d] == VALUE)
            with np.errstate(all="ignore"):
                prod = np.where(mul, prod * (pct[d] + 1.0), prod)
            c[d] = prod
            g_last = np.where(row, group[d], g_last)
            if w is not None:
                with np.errstate(all="ignore"):
                    ok = (w_state[d] == VALUE) & np.isfinite(w[d]) & (w[d] > 0)
                u_last = np.where(row, np.where(ok, w[d], 0.0), u_last)
        mem = held & has_prev
        m[p] = np.where(mem, g_prev, -1)
        u[p] = np.where(m[p] >= 0, u_prev, 0.0)
        cend[p] = np.where(held, prod, 1.0)
        g_prev = np.where(held, g_last, g_prev)
        u_prev = np.where(held, u_last, u_prev)
        has_prev |= held
    return Signal(m, u, cend, c)


def portfolios(group, x_state, pct, pct_state, period_of, P, G, w=None, w_state=None) -> Portfolios:
    """One factor's G portfolios."""
    D, S = x_state.shape
    lo, hi = period_bounds(period_of, P)
    sig = signal(group, x_state, pct, pct_state, period_of, P, w, w_state)
    ret = np.zeros((D, G))
    V = np.ones((D, G))
    A = np.zeros((D, G))
    U = np.zeros((P, G))
    count = np.zeros((P, G), np.int64)
    traded = np.zeros((P, G))
    union = np.zeros((P, G), np.int64)
    with np.errstate(all="ignore"):
        for p in range(P):
            for g in range(G):
                sel = sig.m[p] == g
                count[p, g] = sel.sum()
                U[p, g] = sig.u[p][sel].sum()
                vprev = 1.0
                for d in range(lo[p], hi[p]):
                    A[d, g] = (sig.u[p][sel] * sig.c[d][sel]).sum()
                    V[d, g] = A[d, g] / U[p, g] if U[p, g] > 0 else 1.0
                    ret[d, g] = V[d, g] / vprev - 1.0
                    vprev = V[d, g]
                if p >= 1:
                    t = np.where(sel, sig.u[p] / U[p, g], 0.0) if U[p, g] > 0 else np.zeros(S)
                    selb = sig.m[p - 1] == g
                    a_end = A[hi[p - 1] - 1, g]
                    b = (np.where(selb, sig.u[p - 1] * sig.cend[p - 1] / a_end, 0.0)
                         if U[p - 1, g] > 0 else np.zeros(S))
                    traded[p, g] = np.abs(t - b).sum()
                    union[p, g] = (sel | selb).sum()
    return Portfolios(ret, count, traded, V, U, A, union, sig)


# ------------------------------------------------------------------ host statistics
def net_series(ret, traded, period_of, cost):
    """ret [D], traded [P] -> ret_net [D]: the cost of a rebalance is charged on the period's
    first date."""
    period_of = np.asarray(period_of)
    first = np.r_[True, period_of[1:] != period_of[:-1]]
    charge = np.where(first, cost * traded[period_of], 0.0)
    return (1.0 + ret) * (1.0 - charge) - 1.0


def summary(ret_net, annual_days=252):
    """days, total_return, annual_return, annual_vol, sharpe, max_drawdown of a daily series."""
    n = len(ret_net)
    nav = np.cumprod(1.0 + ret_net)
    out = {"days": n}
    if n == 0:
        out.update(total_return=np.nan, annual_return=np.nan, annual_vol=np.nan, sharpe=np.nan,
                   max_drawdown=np.nan)
        return out
    out["total_return"] = nav[-1] - 1.0
    out["annual_return"] = nav[-1] ** (annual_days / n) - 1.0
    sd = np.std(ret_net, ddof=1) if n >= 2 else np.nan
    out["annual_vol"] = sd * np.sqrt(annual_days)
    out["sharpe"] = (np.mean(ret_net) / sd * np.sqrt(annual_days)) if n >= 2 and sd > 0 else np.nan
    peak = np.maximum.accumulate(np.r_[1.0, nav])[1:]
    out["max_drawdown"] = float(np.max(1.0 - nav / peak))
    return out
