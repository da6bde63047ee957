"""tests/pf_ref.py (the numpy restatement of the daily group portfolios, include/mff.h
mff_pf_*) pinned on the CPU: against exact dyadic arithmetic on a hand-built case, and against
oracle_group_test per period.  The host statistics of mff.factor.portfolio_statistics, the
Python-side argument errors, the binding of the C entry points and their argument checks are
tested too, so this file fails without the feature."""
import numpy as np
import pytest

import mff_oracle as O
import pf_ref as ref
from pf_ref import ABSENT, NULLV, VALUE

pd = pytest.importorskip("pandas")

ENTRY_POINTS = ("mff_pf_signal", "mff_pf_sums", "mff_pf_finalize", "mff_pf_traded", "mff_pf_traded_finalize")


def test_library_binds_the_portfolio_entry_points():
    from mff import _lib
    for name in ENTRY_POINTS:
        assert name in _lib.SIGNATURES
    lib = _lib.load()
    for name in ENTRY_POINTS:
        assert hasattr(lib, name)
    import mff
    from mff import engine
    from mff.factor import Factor, portfolio_tests
    assert "portfolio_tests" in mff.__all__ and mff.portfolio_tests is portfolio_tests
    assert callable(Factor.portfolio_test)
    assert engine.PortfolioResult._fields == ("ret", "count", "traded")
    assert (ABSENT, NULLV, VALUE) == (engine.ABSENT, engine.NULL, engine.VALUE) == (O.ABSENT, O.NULLV, O.VALUE)


def test_c_abi_argument_checks():
    """Bad arguments return a negative code before anything touches a device."""
    from mff import _lib
    lib = _lib.load()
    fake = 4096  # never dereferenced: every call fails its checks first
    sig = lambda K=2, D=4, S=8, P=2, w=fake, ws=fake: lib.mff_pf_signal(fake, fake, fake, fake, w, ws, fake, K, D, S, P,
                                                                         fake, fake, fake, None)
    sums = lambda K=2, D=4, S=8, P=2, G=5: lib.mff_pf_sums(fake, fake, fake, fake, fake, fake, K, D, S, P, G, fake,
                                                           fake, None)
    fin = lambda R=1, K=2, D=4, P=2, G=5: lib.mff_pf_finalize(fake, fake, fake, R, K, D, P, G, fake, fake, fake, None)
    trd = lambda K=2, P=2, S=8, G=5: lib.mff_pf_traded(fake, fake, fake, fake, K, P, S, G, fake, None)
    tfin = lambda R=1, K=2, P=2, G=5: lib.mff_pf_traded_finalize(fake, R, K, P, G, fake, None)
    for call, kw, word in ((sig, dict(K=0), b"K=0"), (sig, dict(D=-1), b"D=-1"), (sig, dict(S=-1), b"S=-1"),
                           (sig, dict(P=0), b"P=0"), (sig, dict(P=5), b"P=5"), (sig, dict(P=-1), b"P=-1"),
                           (sig, dict(ws=None), b"weight_state"), (sig, dict(w=None), b"weight_state"),
                           (sums, dict(K=0), b"K=0"), (sums, dict(K=65536), b"K=65536"), (sums, dict(D=-1), b"D=-1"),
                           (sums, dict(S=-1), b"S=-1"), (sums, dict(P=0), b"P=0"), (sums, dict(G=0), b"G=0"),
                           (sums, dict(G=64), b"G=64"),
                           (fin, dict(R=0), b"R=0"), (fin, dict(K=0), b"K=0"), (fin, dict(D=-1), b"D=-1"),
                           (fin, dict(P=0), b"P=0"), (fin, dict(G=64), b"G=64"), (fin, dict(G=0), b"G=0"),
                           (trd, dict(K=0), b"K=0"), (trd, dict(P=-1), b"P=-1"), (trd, dict(S=-1), b"S=-1"),
                           (trd, dict(G=64), b"G=64"),
                           (tfin, dict(R=0), b"R=0"), (tfin, dict(K=0), b"K=0"), (tfin, dict(P=-1), b"P=-1"),
                           (tfin, dict(G=0), b"G=0")):
        rc = call(**kw)
        assert rc < 0 and word in lib.mff_last_error(), (kw, lib.mff_last_error())
        with pytest.raises(_lib.MffError):
            _lib.check(rc, "mff_pf")
    # nothing to do
    assert sig(D=0, P=0) == 0 and sums(D=0, P=0) == 0 and fin(D=0, P=0) == 0 and trd(P=0) == 0 and tfin(P=0) == 0
    assert sig(S=0) == 0 and sums(S=0) == 0 and trd(S=0) == 0


# --------------------------------------------------------------------------- the hand-built case
def _hand():
    """4 stocks, 5 dates in periods [0, 0, 1, 2, 2], G = 2, equal weights, dyadic pct.
    s0: group 0 then 1.  s1: group 1 throughout; its pct on date 2 is null.  s2: group 0 in period
    0, ABSENT in the whole of period 1 (so in period 2 it is held on its period-0 signal).
    s3: the last row of period 0 is a null exposure (group -1: no membership in period 1), group 0
    in period 1."""
    period_of = np.array([0, 0, 1, 2, 2])
    xs = np.full((5, 4), VALUE, np.uint8)
    xs[2, 2] = ABSENT
    xs[1, 3] = NULLV
    group = np.array([[0, 1, 0, 1],
                      [0, 1, 0, -1],
                      [1, 1, -1, 0],
                      [0, 0, 0, 0],
                      [1, 0, 1, 0]])
    pct = np.array([[-0.5, 0.25, 0.5, 0.0],
                    [0.5, 0.25, -0.5, 0.25],
                    [0.5, 0.25, 0.25, 0.25],
                    [0.5, 0.0, 0.5, 0.0],
                    [0.5, 0.5, 0.0, 0.0]])
    ps = np.full((5, 4), VALUE, np.uint8)
    ps[2, 1] = NULLV   # a null pct on a row: the growth of s1 stays 1 over period 1
    ps[2, 2] = ABSENT
    return group, xs, pct, ps, period_of


def test_reference_on_the_hand_case_is_exact():
    group, xs, pct, ps, period_of = _hand()
    r = ref.portfolios(group, xs, pct, ps, period_of, 3, 2)
    assert r.sig.m.tolist() == [[-1, -1, -1, -1], [0, 1, -1, -1], [1, 1, 0, 0]]
    assert r.sig.cend.tolist() == [[0.75, 1.5625, 0.75, 1.25], [1.5, 1.0, 1.0, 1.25], [2.25, 1.5, 1.5, 1.0]]
    assert r.sig.u.tolist() == [[0, 0, 0, 0], [1, 1, 0, 0], [1, 1, 1, 1]]
    assert r.count.tolist() == [[0, 0], [1, 1], [2, 2]]
    assert r.U.tolist() == [[0, 0], [1, 1], [2, 2]]
    assert r.V.tolist() == [[1, 1], [1, 1], [1.5, 1.0], [1.25, 1.25], [1.25, 1.875]]
    assert r.ret.tolist() == [[0, 0], [0, 0], [0.5, 0.0], [0.25, 0.25], [0.0, 0.5]]
    # period 1: both portfolios built from cash.  period 2, group 0: s0 (all of it) sold, s2 and s3
    # bought: 1 + 0.5 + 0.5; group 1: s1 from all to half, s0 bought: 0.5 + 0.5
    assert r.traded.tolist() == [[0, 0], [1, 1], [2, 1]]
    assert r.union.tolist() == [[0, 0], [1, 1], [3, 2]]


def test_weighted_reference_on_the_hand_case_is_exact():
    """Weights of the signal rows: period 2, group 1 holds s0 (weight 3 on date 2) and s1 (weight 1):
    V = (3 c0 + c1) / 4; group 0 holds s2 (a null weight on its period-0 signal row: u = 0, still a
    member) and s3 (weight 2)."""
    group, xs, pct, ps, period_of = _hand()
    w = np.array([[1.0, 1, 1, 1], [1, 1, 5, 1], [3, 1, 1, 2], [1, 1, 1, 1], [1, 1, 1, 1]])
    wst = np.full((5, 4), VALUE, np.uint8)
    wst[1, 2] = NULLV
    r = ref.portfolios(group, xs, pct, ps, period_of, 3, 2, w, wst)
    assert r.sig.u.tolist() == [[0, 0, 0, 0], [1, 1, 0, 0], [3, 1, 0, 2]]
    assert r.count.tolist() == [[0, 0], [1, 1], [2, 2]]
    assert r.U.tolist() == [[0, 0], [1, 1], [2, 4]]
    # group 0 is s3 alone (c = 1, 1); group 1: (3 * 1.5 + 1) / 4 = 1.375, (3 * 2.25 + 1.5) / 4 = 2.0625
    assert r.V.tolist() == [[1, 1], [1, 1], [1.5, 1.0], [1.0, 1.375], [1.0, 2.0625]]
    assert r.ret[3:].tolist() == [[0.0, 0.375], [0.0, 0.5]]
    # group 0: s0 sold (1), s3 bought (1), s2 a member of weight 0; group 1: s0 to 0.75, s1 from 1 to 0.25
    assert r.traded.tolist() == [[0, 0], [1, 1], [2, 1.5]]


def test_statistics_on_the_hand_case_are_exact():
    from mff.factor import PORTFOLIO_SUMMARY, portfolio_statistics
    group, xs, pct, ps, period_of = _hand()
    r = ref.portfolios(group, xs, pct, ps, period_of, 3, 2)
    st = portfolio_statistics(r.ret, r.count, r.traded, period_of, cost=0.0, annual_days=9)
    assert st["names"] == ["group_1", "group_2", "long_short"] and (st["d0"], st["p0"]) == (2, 1)
    assert st["ret"].tolist() == [[0.5, 0.25, 0.0], [0.0, 0.25, 0.5], [-0.5, 0.0, 0.5]]
    assert np.array_equal(st["ret_net"], st["ret"])
    assert st["nav"].tolist() == [[1.5, 1.875, 1.875], [1.0, 1.25, 1.875], [0.5, 0.5, 0.75]]
    assert st["traded"].tolist() == [[1, 2], [1, 1], [2, 3]]
    exp = {"group_1": (3, 0.875, 5.591796875, 0.75, 3.0, 0.0, 0.75, 0.0),
           "group_2": (3, 0.875, 5.591796875, 0.75, 3.0, 0.0, 0.5, 0.0),
           "long_short": (3, -0.25, -0.578125, 1.5, 0.0, 0.5, 1.25, 0.0)}
    for nm, s in zip(st["names"], st["summary"]):
        assert tuple(s[c] for c in PORTFOLIO_SUMMARY) == exp[nm], nm
    # a quarter per unit traded, charged on the first date of each period
    sc = portfolio_statistics(r.ret, r.count, r.traded, period_of, cost=0.25, annual_days=9)
    assert np.array_equal(sc["ret"], st["ret"]) and np.array_equal(sc["traded"], st["traded"])
    assert sc["ret_net"].tolist() == [[0.125, -0.375, 0.0], [-0.25, -0.0625, 0.5], [-1.0, -0.75, 0.5]]
    assert sc["nav"].tolist() == [[1.125, 0.703125, 0.703125], [0.75, 0.703125, 1.0546875], [0.0, 0.0, 0.0]]
    assert [s["total_cost"] for s in sc["summary"]] == [0.75, 0.5, 1.25]
    assert [s["mean_turnover"] for s in sc["summary"]] == [0.75, 0.5, 1.25]
    # group_1 falls from its peak 1.125 to 0.703125; group_2 from the starting 1 to 0.703125
    assert [s["max_drawdown"] for s in sc["summary"]] == [0.375, 0.296875, 1.0]
    for s, t in zip(sc["summary"], sc["ret_net"]):
        assert s == {**s, **ref.summary(t, 9)}  # the reference's formulas on the same series


def test_statistics_on_a_hand_series():
    """One group, four dates in two periods: drawdown against the running maximum that starts at
    1, Sharpe, annualisation; days < 2 and a constant series have no Sharpe."""
    from mff.factor import portfolio_statistics
    ret = np.array([[-0.5], [1.0], [0.5], [-0.5]])    # nav 0.5, 1, 1.5, 0.75
    st = portfolio_statistics(ret, np.array([[3], [3]]), np.array([[0.0], [0.5]]), [0, 0, 1, 1], 0.0, 8)
    s = st["summary"][0]
    assert st["names"] == ["group_1"] and st["nav"].tolist() == [[0.5, 1.0, 1.5, 0.75]]
    assert s["days"] == 4 and s["total_return"] == -0.25 and s["annual_return"] == 0.75 ** 2 - 1
    assert s["max_drawdown"] == 0.5 and s["mean_turnover"] == 0.125
    sd = np.std(ret[:, 0], ddof=1)
    assert s["annual_vol"] == sd * np.sqrt(8) and s["sharpe"] == 0.125 / sd * np.sqrt(8)
    # an arithmetic progression has std = its step: everything exact
    ap = portfolio_statistics(np.array([[0.0], [0.25], [0.5]]), np.array([[1]]), np.zeros((1, 1)), [0, 0, 0], 0.0, 4)
    assert ap["summary"][0]["annual_vol"] == 0.5 and ap["summary"][0]["sharpe"] == 2.0
    one = portfolio_statistics(np.array([[0.25]]), np.array([[1]]), np.zeros((1, 1)), [0], 0.0, 252)["summary"][0]
    assert one["days"] == 1 and np.isnan(one["sharpe"]) and np.isnan(one["annual_vol"]) and one["max_drawdown"] == 0.0
    flat = portfolio_statistics(np.full((3, 1), 0.5), np.array([[1]]), np.zeros((1, 1)), [0, 0, 0], 0.0, 252)
    assert np.isnan(flat["summary"][0]["sharpe"]) and flat["summary"][0]["annual_vol"] == 0.0
    # nothing present: an empty window
    none = portfolio_statistics(np.zeros((3, 2)), np.zeros((2, 2), int), np.zeros((2, 2)), [0, 0, 1], 0.0, 252)
    assert (none["d0"], none["p0"]) == (3, 2) and none["ret"].shape == (3, 0)
    assert all(s["days"] == 0 and np.isnan(s["total_return"]) for s in none["summary"])
    # the window opens with the first period holding a stock; a cell without stocks returns 0
    late = portfolio_statistics(np.array([[9.0, 9.0], [0.0, 0.5], [0.0, 0.0]]), np.array([[0, 0], [0, 2], [1, 1]]),
                                np.array([[0.0, 0], [0, 1], [1, 0]]), [0, 1, 2], 0.5, 252)
    assert (late["d0"], late["p0"]) == (1, 1) and late["ret"].tolist() == [[0.0, 0.0], [0.5, 0.0], [0.5, 0.0]]
    assert late["ret_net"].tolist() == [[0.0, -0.5], [0.5 * 1.5 - 1 + 0.0, 0.0], [0.0, -0.5]]
    assert late["present"].tolist() == [[False, True], [True, True], [True, True]]


# --------------------------------------------------------------------------- against the oracle
def _panel(seed, D, S):
    rng = np.random.default_rng(seed)
    pct = rng.normal(0, 0.02, (D, S))
    ps = np.full((D, S), VALUE, np.uint8)
    ps[5:9, 3] = ABSENT
    ps[7:25, 7] = ABSENT      # absent for two whole weeks
    ps[rng.random((D, S)) < 0.02] = NULLV
    x = np.round(rng.normal(size=(D, S)), 1)
    xs = ps.copy()
    x[rng.random((D, S)) < 0.03] = np.nan
    xs[(rng.random((D, S)) < 0.03) & (ps != ABSENT)] = NULLV
    w = rng.uniform(1, 5, (D, S))
    wst = ps.copy()
    wst[(rng.random((D, S)) < 0.05) & (ps != ABSENT)] = NULLV
    return pct, ps, x, xs, w, wst


@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("G", [1, 3, 5])
def test_reference_compounds_to_the_oracle_group_test(G, weighted):
    """(1 + ret) compounded over a period, minus 1, is oracle_group_test's number of that period
    (equal-weighted: the mean of the members' returns; weighted: sum w r / sum w), and the
    present cells are the cells with members."""
    D, S = 40, 37
    pct, ps, x, xs, w, wst = _panel(5 + G, D, S)
    period_of = np.arange(D) // 7
    P = int(period_of[-1]) + 1
    wa = (w, wst) if weighted else (None, None)
    oret, opres = O.oracle_group_test(x, xs, pct, ps, period_of, P, G, *wa)
    group = np.stack([O.oracle_qcut(x[d], (xs[d] == VALUE) & ~np.isnan(x[d]), G) for d in range(D)])
    r = ref.portfolios(group, xs, pct, ps, period_of, P, G, *wa)
    assert np.array_equal(r.count > 0, opres == 1) and opres.sum() >= P * G // 2
    comp = np.stack([np.prod(1.0 + r.ret[period_of == p], axis=0) - 1.0 for p in range(P)])
    np.testing.assert_allclose(comp, oret, rtol=0, atol=1e-13)
    assert (r.traded[0] == 0).all() and (r.traded >= 0).all() and (r.traded <= 2 + 1e-12).all()
    # the stock that skipped two weeks comes back on its older signal
    assert (r.sig.m[1:3, 7] == -1).all() and r.sig.m[3, 7] == group[6, 7] and (r.sig.cend[1:3, 7] == 1.0).all()


# --------------------------------------------------------------------------- Python-side errors
def test_python_argument_errors():
    import datetime as dt

    from mff import frames
    from mff.factor import Factor, portfolio_tests
    codes = ["000001.SZ", "000002.SZ"]
    dates = [dt.date(2024, 1, 1) + dt.timedelta(days=i) for i in range(3)]
    ex = frames.to_long(np.ones((3, 2)), np.full((3, 2), VALUE, np.uint8), codes, dates, "f")
    pv = frames.to_long(np.zeros((3, 2)), np.full((3, 2), VALUE, np.uint8), codes, dates, "pct_change")
    f = Factor("f", ex)
    for kw, word in ((dict(weight_param="size"), "weight_param"), (dict(group_num=0), "group_num"),
                     (dict(group_num=64), "group_num"), (dict(group_num=2.5), "group_num"),
                     (dict(cost=1.0), "cost"), (dict(cost=-0.1), "cost"), (dict(cost="x"), "cost"),
                     (dict(annual_days=0), "annual_days"), (dict(weight_param="tmc"), "tmc"),
                     (dict(frequency="daily"), "frequency")):
        with pytest.raises(ValueError, match=word):
            portfolio_tests([f], pv_data=pv, **kw)
    with pytest.raises(ValueError, match="at least one"):
        portfolio_tests([], pv_data=pv)
    with pytest.raises(ValueError, match="duplicate"):
        portfolio_tests([f, f], pv_data=pv)
    with pytest.raises(ValueError, match="pct_change"):
        portfolio_tests([f], pv_data=pv.drop(columns="pct_change"))
    with pytest.raises(ValueError, match="cost"):
        f.portfolio_test(cost=2, pv_data=pv, plot_out=False)


def test_engine_argument_errors():
    torch = pytest.importorskip("torch")
    from mff import engine
    z = lambda *s, dt=torch.float64: torch.zeros(s, dtype=dt)
    xv, xs, pv, ps = z(2, 4, 3), z(2, 4, 3, dt=torch.uint8), z(4, 3), z(4, 3, dt=torch.uint8)
    per = torch.zeros(4, dtype=torch.int32)
    for args, kw, word in (((xv[0], xs[0], pv, ps, per, 1), {}, r"\[K\]\[D\]\[S\]"),
                           ((xv, xs, pv[:3], ps[:3], per, 1), {}, "pct_val"),
                           ((xv, xs, pv, ps, per[:3], 1), {}, "period_of"),
                           ((xv, xs, pv, ps, per, 1), dict(group_num=0), "group_num"),
                           ((xv, xs, pv, ps, per, 1), dict(group_num=64), "group_num"),
                           ((xv, xs, pv, ps, per, 1), dict(w_val=pv), "go together"),
                           ((xv, xs, pv, ps, per, 1), dict(w_val=pv[:2], w_state=ps[:2]), "w_val")):
        with pytest.raises(ValueError, match=word):
            engine.group_portfolios(*args, **kw)
