"""tests/stage1_ref.py, the long-double restatement of the 23 cancelling stage-1 factors that
referees tests/test_gpu_stage1_bounds.py, checked on the CPU: against published polars
values, the known-answer frames, exact rational arithmetic and the oracle; its error bounds
against what f64 arithmetic delivers (two f64 implementations inside every bound) and against
five wrong variants written here in numpy (each outside a bound on every factor it touches).
No kernel is touched.  Run with -s for the mutant table (which of them tests/parity.py's C5
tolerance would have caught)."""
import numpy as np
import pytest
from numpy.lib.stride_tricks import sliding_window_view

import stage1_cases
import stage1_ref as R
from parity import compare

ABSENT, NULL, VALUE = 0, 1, 2
T = 240
FIELDS = ("open", "high", "low", "close", "volume")


def _ref(p, **kw):
    return R.reference(*(p[k] for k in FIELDS), p["present"], **kw)


@pytest.fixture(scope="module")
def panel():
    return stage1_cases.panel()


@pytest.fixture(scope="module")
def ref(panel):
    return _ref(panel)


@pytest.fixture(scope="module")
def oracle(panel):
    import mff_oracle as O
    ov, os_ = O.oracle_stage1(panel, R.NAMES)
    return {nm: (ov[i], os_[i]) for i, nm in enumerate(R.NAMES)}


# ------------------------------------------------------------------ the panel
def test_panel_contract_and_classes(panel):
    from mff import engine
    engine.validate_host_panel(panel)
    D, S = stage1_cases.D, stage1_cases.S
    assert (D, S) == (2, 161) and panel["present"].shape == (D, S, T)
    for k in FIELDS[:4]:
        assert panel[k].dtype == np.float32
        x = panel[k][panel["present"]].astype(np.float64)
        assert np.array_equal(np.float32(np.round(x, 2)), panel[k][panel["present"]])  # on the tick
    specs = [stage1_cases.spec(sd) for sd in range(D * S)]
    n = panel["present"].reshape(-1, T).sum(axis=1)
    # stock-days 0..63: all present or suspended (two of them): the full-wave walk
    assert set(n[:64]) == {0, T} and (n[:64] == 0).sum() == 2
    dense = {(a, "p") for a, b, c in specs[:64] if c == "full"} | {(b, "v") for a, b, c in specs[:64] if c == "full"}
    ragged = ({(a, "p") for a, b, c in specs[64:] if c not in ("full", "suspended")}
              | {(b, "v") for a, b, c in specs[64:] if c not in ("full", "suspended")})
    every = {(a, "p") for a in stage1_cases.PRICE} | {(b, "v") for b in stage1_cases.VOLUME}
    assert dense == every and ragged == every
    # every ragged wave of the pair kernel (64 stock-days from 64 on) mixes full and holed days
    for w in range(1, 5):
        kinds = {c for a, b, c in specs[64 * w:64 * w + 64]}
        assert "full" in kinds and len(kinds) > 8
    assert {c for a, b, c in specs} == set(stage1_cases.PRESENCE)
    v = panel["volume"][panel["present"]]
    assert (v == 2.0 ** 32 - 2).any() and ((v > 2 ** 24) & (v % 2 == 1)).any() and (v == 0).any()


# ------------------------------------------------------------------ the reference is right
def _planes(rows, S):
    """rows: (stock, minute, o, h, l, c, v) -> [S][240] planes + present."""
    p = {k: np.full((S, T), np.nan) for k in FIELDS}
    p["present"] = np.zeros((S, T), bool)
    for s, m, *x in rows:
        for k, val in zip(FIELDS, x):
            p[k][s, m] = val
        p["present"][s, m] = True
    return p


def test_polars_published_skew_kurt():
    """polars' skew / kurtosis of [1, 1, 2, 10, 100] (narwhals docstrings), as
    volumes (the shares are scale-free) and as 1-minute returns (open 1, close 1 + x)."""
    x = [1, 1, 2, 10, 100]
    p = _planes([(0, 10 * i, 1.0, 200.0, 1.0, 1.0 + a, float(a)) for i, a in enumerate(x)], 1)
    out, und = _ref(p)
    for nm, want in (("shape_skewVol", 1.4724267269058975), ("shape_kurtVol", 0.2106571340718002),
                     ("shape_skew", 1.4724267269058975), ("shape_kurt", 0.2106571340718002)):
        v, s, b = out[nm]
        # the published digits carry polars' own f64 rounding of m4 / m2^2 at 3.21: a few u there
        assert s[0] == VALUE and abs(v[0] - want) <= 2e-15, (nm, v[0])
        assert 0 < b[0] < 1e-11
    assert out["shape_skratio"][0][0] == pytest.approx(1.4724267269058975 / 0.2106571340718002, rel=1e-15)


def _frame_to_planes(df):
    import mff_oracle as O
    codes = [g[0] for g in df.groups]
    rows = []
    for i, (code, s, e) in enumerate(df.groups):
        for k in range(s, e):
            rows.append((i, int(O._minute_in_trade(df.time[k:k + 1])[0]), df.open[k], df.high[k], df.low[k],
                         df.close[k], df.volume[k]))
    return codes, _planes(rows, len(codes))


def _vs_oracle_frame(df):
    import mff_oracle as O
    codes, p = _frame_to_planes(df)
    out, und = _ref(p)
    for nm in R.NAMES:
        res = O.ORACLE_FUNCS[nm](df)
        v, s, b = out[nm]
        for i, code in enumerate(codes):
            if code not in res:
                assert s[i] == ABSENT, (nm, code)
            elif res[code] is None:
                assert s[i] == NULL, (nm, code)
            else:
                assert s[i] == VALUE, (nm, code)
                assert (np.isnan(v[i]) and np.isnan(res[code])) or abs(v[i] - res[code]) <= 1e-12 * abs(v[i]) + b[i], \
                    (nm, code, v[i], res[code])
    return codes, out


def test_known_answer_frames():
    """The hand frames of tests/test_oracle_kat.py: the oracle's values and the answers
    asserted there, for the 23 factors."""
    import mff_oracle as O
    from test_oracle_kat import frame
    codes, out = _vs_oracle_frame(frame())
    A, B = codes.index("A"), codes.index("B")
    val = lambda nm, i: out[nm][0][i]
    assert val("vol_volume1min", A) == pytest.approx(float(np.std([100, 300, 0, 200], ddof=1)), rel=1e-15)
    assert out["vol_volume1min"][1][B] == NULL
    assert np.isnan(val("shape_skew", B)) and np.isnan(val("shape_skewVol", B)) and np.isnan(val("corr_pv", B))
    assert val("corr_pv", A) == pytest.approx(
        float(np.corrcoef([10.1, 10.2, 10.3, 10.4], [100, 300, 0, 200])[0, 1]), rel=1e-12)
    assert val("corr_pvr", A) == pytest.approx(-1.0, rel=1e-14)
    assert out["corr_pvr"][1][B] == ABSENT and out["corr_prvr"][1][B] == ABSENT
    # one full 50-minute window with a perfect linear high ~ low relation; 49 bars: no window
    m = np.arange(100, 150)
    lo = 10.0 + 0.01 * (m - 100)
    hi = 2.0 * lo + 1.0
    df = O.DayFrame(np.array(["X"] * 50), 0, O.minute_to_time(m), lo, hi, lo, lo, np.ones(50))
    codes, out = _vs_oracle_frame(df)
    assert out["mmt_ols_beta_mean"][0][0] == pytest.approx(2.0, rel=1e-9)
    assert out["mmt_ols_corr_mean"][0][0] == pytest.approx(1.0, rel=1e-9)
    assert out["mmt_ols_corr_square_mean"][0][0] == pytest.approx(1.0, rel=1e-9)
    assert out["mmt_ols_qrs"][0][0] == 0.0 and out["mmt_ols_qrs"][2][0] == 0.0
    assert out["mmt_ols_beta_zscore_last"][0][0] == pytest.approx(2.0, rel=1e-9)
    df2 = O.DayFrame(np.array(["X"] * 49), 0, O.minute_to_time(m[:49]), lo[:49], hi[:49], lo[:49], lo[:49],
                     np.ones(49))
    codes, out = _vs_oracle_frame(df2)
    assert all(out[nm][1][0] == ABSENT for nm in R.OLS)


def test_long_double_matches_exact_fractions():
    """Small dyadic stock-days (prices on a 1/64 grid, small volumes): the long-double path
    against exact rational sums (the fallback of hosts whose long double is f64)."""
    if not R.LONGDOUBLE_OK:
        pytest.skip("long double is f64 here: the reference already is the Fraction path")
    rng = np.random.default_rng(5)
    S = 4
    p = {k: np.full((S, T), np.nan) for k in FIELDS}
    p["present"] = np.zeros((S, T), bool)
    for s in range(S):
        m = np.zeros(T, bool)
        m[30:30 + (60, 55, 2, 1)[s]] = True
        if s == 1:
            m[40] = False
        c = 640 + np.cumsum(rng.integers(-3, 4, T))
        o = np.concatenate([[640], c[:-1]])
        p["open"][s], p["close"][s] = o / 64.0, c / 64.0
        p["high"][s] = (np.maximum(o, c) + rng.integers(0, 3, T)) / 64.0
        p["low"][s] = (np.minimum(o, c) - rng.integers(0, 3, T)) / 64.0
        p["volume"][s] = rng.integers(0, 9, T).astype(np.float64)
        p["present"][s] = m
    a, ua = _ref(p)
    b, ub = _ref(p, exact=True)
    for nm in R.NAMES:
        assert np.array_equal(a[nm][1], b[nm][1]), nm
        assert np.array_equal(ua[nm], ub[nm]), nm
        assert np.array_equal(np.isnan(a[nm][0]), np.isnan(b[nm][0])), nm
        x, y = np.nan_to_num(a[nm][0]), np.nan_to_num(b[nm][0])
        # two roundings of differently rounded intermediates: a few u, far inside the bound
        assert (np.abs(x - y) <= 8 * R.U * np.abs(y) + a[nm][2] / 64).all(), (nm, x, y)
        assert np.allclose(a[nm][2], b[nm][2], rtol=1e-9, atol=0), nm
    assert (a["mmt_ols_beta_mean"][1] == [VALUE, ABSENT, ABSENT, ABSENT]).all()


def test_ref_agrees_with_oracle_under_c5(panel, ref, oracle):
    """Sanity at the old tolerance: the same states and NaN pattern as the oracle on every
    entry and C5-close values, except where the oracle's own two-pass f64 loses the up / down
    subsets of the tiny-range days (measured below against the derived bound instead)."""
    out, und = ref
    for nm in R.NAMES:
        ov, os_ = oracle[nm]
        assert np.array_equal(out[nm][1], os_), nm
        if nm not in ("vol_upRatio", "vol_downRatio", "vol_upVol", "vol_downVol"):
            bad = compare(np.where(und[nm], ov, out[nm][0]), out[nm][1], ov, os_, nm)
            assert not bad, bad


# ------------------------------------------------------------------ f64 implementations and mutants
def _seqsum(a, dt):
    """One-pass running sum over the last axis with the accumulator in dtype dt."""
    return np.cumsum(a.astype(dt), axis=-1, dtype=dt)[..., -1].astype(np.float64)


def _first(X, M):
    return X[np.arange(X.shape[0]), M.argmax(axis=1)]


def _quot(a, b, m, qt):
    """a / b where m (1 elsewhere) with the quotient formed in dtype qt."""
    with np.errstate(all="ignore"):
        return np.where(m, (a.astype(qt) / np.where(m, b, 1.0).astype(qt)).astype(np.float64), 1.0)


def kernel_f64(p, shift=True, acc=np.float64, quot=np.float64, ols="slide", root=0.0):
    """A plain numpy restatement of the serial kernels' documented algorithm (DESIGN.md §3,
    mff_stats.h): sets shifted by their first member, one-pass raw power sums, the central
    moments from them, Pearson from shifted sums, OLS window sums slid over the day (added on
    entry, subtracted 50 bars later) shifted by the first bar's low / high.  The keyword
    arguments turn it into the mutants M1-M5: shift=False (M1: unshifted sums), acc=float32
    (M2: sums accumulated in f32), quot=float32 (M3: quotients formed in f32), ols="prefix"
    (M4: window sums as differences of unshifted f64 prefix sums), root=2^-24 (M5: that
    relative error on the root of every std and Pearson).  Returns {name: (val, state)}."""
    M = p["present"].reshape(-1, T)
    N = M.shape[0]
    g = lambda k, fill: np.where(M, p[k].reshape(-1, T).astype(np.float64), fill)
    o, h, lo, c, v = g("open", 1.0), g("high", 1.0), g("low", 1.0), g("close", 1.0), g("volume", 0.0)
    n = M.sum(axis=1)
    out = {}
    st_val = np.where(n > 0, VALUE, ABSENT).astype(np.uint8)
    st_std = np.where(n > 1, VALUE, np.where(n > 0, NULL, ABSENT)).astype(np.uint8)
    rt = 1.0 + root

    def put(nm, val, st):
        out[nm] = (np.where(st == VALUE, val, 0.0), st)

    def raw(X, S):
        cnt = S.sum(axis=1)
        x0 = _first(X, S) if shift else np.zeros(N)
        y = np.where(S, X - x0[:, None], 0.0)
        f = _first(X, S)[:, None]
        const = (np.where(S, X, f) == f).all(axis=1)      # C3, decided on the values (exact)
        return cnt, [_seqsum(y ** k, acc) for k in (1, 2, 3, 4)], const

    def std1(cnt, s, const):
        with np.errstate(all="ignore"):
            var = (s[1] - s[0] * s[0] / cnt) / (cnt - 1)
            return np.where(cnt >= 2, np.where(const, 0.0, np.sqrt(var) * rt), 0.0)

    def skku(cnt, s, const):
        with np.errstate(all="ignore"):
            inv = 1.0 / cnt
            mu, a2, a3, a4 = s[0] * inv, s[1] * inv, s[2] * inv, s[3] * inv
            m2 = a2 - mu * mu
            m3 = a3 - 3 * mu * a2 + 2 * mu ** 3
            m4 = a4 - 4 * mu * a3 + 6 * mu * mu * a2 - 3 * mu ** 4
            sk = np.where(cnt == 2, 0.0, m3 / m2 ** 1.5)
            ku = m4 / (m2 * m2) - 3.0
            bad = (cnt < 1) | const | np.isnan(m2) | (m2 == 0)
            return np.where(bad, np.nan, sk), np.where(bad, np.nan, ku)

    # MOMR
    r = np.where(M, _quot(c, o, M, quot) - 1.0, 0.0)
    cnt, s, const = raw(r, M)
    sd = std1(cnt, s, const)
    put("vol_return1min", sd, st_std)
    sk, ku = skku(cnt, s, const)
    put("shape_skew", sk, st_val)
    put("shape_kurt", ku, st_val)
    with np.errstate(all="ignore"):
        put("shape_skratio", sk / ku, st_val)
        for nm, sel in (("up", M & (r > 0)), ("down", M & (r < 0))):
            sub = std1(*raw(r, sel))
            put(f"vol_{nm}Vol", sub, st_val)
            put(f"vol_{nm}Ratio", sub / sd, st_std)
    # MOMV (the moments of the shares are those of the volumes: scale-free)
    cnt, s, const = raw(v, M)
    put("vol_volume1min", std1(cnt, s, const), st_std)
    sk, ku = skku(cnt, s, const)
    zero = np.where(M, v, 0.0).sum(axis=1) == 0
    sk, ku = np.where(zero, np.nan, sk), np.where(zero, np.nan, ku)
    put("shape_skewVol", sk, st_val)
    put("shape_kurtVol", ku, st_val)
    with np.errstate(all="ignore"):
        put("shape_skratioVol", sk / ku, st_val)
    # MOMH
    put("vol_range1min", std1(*raw(_quot(h, lo, M, quot), M)), st_std)

    # CORR
    def pear(X, Y, P, x0, y0):
        cnt = P.sum(axis=1)
        if not shift:
            x0, y0 = np.zeros(N), np.zeros(N)
        dx, dy = np.where(P, X - x0[:, None], 0.0), np.where(P, Y - y0[:, None], 0.0)
        sx, sy, sxx, syy, sxy = (_seqsum(t, acc) for t in (dx, dy, dx * dx, dy * dy, dx * dy))
        cx = (np.where(P, X, _first(X, P)[:, None]) == _first(X, P)[:, None]).all(axis=1)
        cy = (np.where(P, Y, _first(Y, P)[:, None]) == _first(Y, P)[:, None]).all(axis=1)
        with np.errstate(all="ignore"):
            inv = 1.0 / cnt
            vx, vy = sxx - sx * (sx * inv), syy - sy * (sy * inv)
            val = (sxy - sx * (sy * inv)) / (np.sqrt(vx * vy) * rt)
            if shift:
                cx, cy = cx | (vx == 0), cy | (vy == 0)
            return np.where((cnt < 2) | cx | cy, np.nan, val)

    order = np.argsort(~M, axis=1, kind="stable")
    Mc = np.arange(T)[None, :] < n[:, None]
    cc, vc = np.take_along_axis(c, order, 1), np.take_along_axis(v, order, 1)
    P1 = Mc.copy()
    P1[:, 0] = False
    prev = lambda a: np.concatenate([a[:, :1], a[:, :-1]], axis=1)
    c0, v0 = cc[:, 0], vc[:, 0]
    put("corr_pv", pear(cc, vc, Mc, c0, v0), st_val)
    put("corr_pvd", pear(cc, prev(vc), P1, c0, v0), st_val)
    put("corr_pvl", pear(prev(cc), vc, P1, c0, v0), st_val)
    pc = np.where(P1, _quot(cc - prev(cc), prev(cc), P1, quot), 0.0)
    put("corr_prv", pear(pc, vc, P1, pc[:, 1], v0), st_val)
    Z = M & (v != 0)
    oz = np.argsort(~Z, axis=1, kind="stable")
    Zc = np.arange(T)[None, :] < Z.sum(axis=1)[:, None]
    cz, vz = np.take_along_axis(c, oz, 1), np.take_along_axis(v, oz, 1)
    PZ = Zc.copy()
    PZ[:, 0] = False
    pcz = np.where(PZ, _quot(cz - prev(cz), prev(cz), PZ, quot), 0.0)
    pvz = np.where(PZ, _quot(vz - prev(vz), np.where(PZ, prev(vz), 1.0), PZ, quot), 0.0)
    st_z = np.where(Z.any(axis=1), VALUE, ABSENT).astype(np.uint8)
    put("corr_prvr", pear(pcz, pvz, PZ, pcz[:, 1], pvz[:, 1]), st_z)
    put("corr_pvr", pear(cz, pvz, PZ, cz[:, 1], pvz[:, 1]), st_z)

    # OLS: 50 x the window (co)variances
    ok = sliding_window_view(M, 50, axis=1).all(axis=2)
    wx, wy = sliding_window_view(lo, 50, axis=1), sliding_window_view(h, 50, axis=1)
    cx = (wx == wx[:, :, :1]).all(axis=2)
    cy = (wy == wy[:, :, :1]).all(axis=2)
    x0, y0 = _first(lo, M), _first(h, M)
    if ols == "slide":
        dx, dy = np.where(M, lo - x0[:, None], 0.0), np.where(M, h - y0[:, None], 0.0)
        S = [np.zeros(N, acc) for _ in range(5)]
        keep = np.zeros((5, N, T - 49))
        for m in range(T):
            terms = (dx[:, m], dy[:, m], dx[:, m] * dx[:, m], dy[:, m] * dy[:, m], dx[:, m] * dy[:, m])
            S = [a + t.astype(acc) for a, t in zip(S, terms)]
            if m >= 50:
                k = m - 50
                terms = (dx[:, k], dy[:, k], dx[:, k] * dx[:, k], dy[:, k] * dy[:, k], dx[:, k] * dy[:, k])
                S = [a - t.astype(acc) for a, t in zip(S, terms)]
            if m >= 49:
                for i in range(5):
                    keep[i, :, m - 49] = S[i]
        Sx, Sy, Sxx, Syy, Sxy = keep
        mx, my = x0[:, None] + Sx * 0.02, y0[:, None] + Sy * 0.02
    else:  # differences of unshifted prefix sums
        pre = lambda a: np.concatenate([np.zeros((N, 1)), np.cumsum(np.where(M, a, 0.0), axis=1)], axis=1)
        win = lambda a: pre(a)[:, 50:] - pre(a)[:, :-50]
        Sx, Sy, Sxx, Syy, Sxy = win(lo), win(h), win(lo * lo), win(h * h), win(lo * h)
        mx, my = Sx * 0.02, Sy * 0.02
    with np.errstate(all="ignore"):
        Vx, Vy, Cv = (Sxx - Sx * 0.02 * Sx) / 50, (Syy - Sy * 0.02 * Sy) / 50, (Sxy - Sx * 0.02 * Sy) / 50
        vz = ~cx & (Vx != 0)
        prod = Vx * Vy
        qw = ok & ~cx & ~cy & (prod != 0)
        beta = np.where(vz, np.where(cy, 0.0, Cv) / Vx, my / mx)
        W, Wq = ok.sum(axis=1), qw.sum(axis=1)
        mean = lambda a, m_, k: np.where(m_, a, 0.0).sum(axis=1) / k
        csm = np.where((qw & np.isnan(np.sqrt(Cv))).any(axis=1), np.nan, mean(np.sqrt(Cv) / prod, qw, Wq))
        cs, cr = mean(Cv * Cv / prod, qw, Wq), mean(Cv / np.sqrt(prod), qw, Wq)
        j0 = ok.argmax(axis=1)
        b0 = beta[np.arange(N), j0]
        db = np.where(ok, beta - b0[:, None], 0.0)
        bd1, bd2 = db.sum(axis=1), (db * db).sum(axis=1)
        bmean = b0 + bd1 / W
        bstd = np.sqrt((bd2 - bd1 * bd1 / W) / (W - 1))
        bl = beta[np.arange(N), T - 50 - ok[:, ::-1].argmax(axis=1)]
        has = (W >= 2) & (bstd != 0)
        z = (bl - bmean) / bstd
    st = np.where(W > 0, VALUE, ABSENT).astype(np.uint8)
    put("mmt_ols_qrs", np.where(has & (Wq > 0), csm * z, 0.0), st)
    put("mmt_ols_corr_square_mean", np.where(Wq > 0, cs, 0.0), st)
    put("mmt_ols_corr_mean", np.where(Wq > 0, cr, 0.0), st)
    put("mmt_ols_beta_mean", bmean, st)
    put("mmt_ols_beta_zscore_last", np.where(has & (bstd > 0), z, bmean), st)
    shape = p["present"].shape[:-1]
    return {nm: (a.reshape(shape), s_.reshape(shape)) for nm, (a, s_) in out.items()}


def _inside(impl, ref, label):
    out, und = ref
    bad, worst = [], {}
    for nm in R.NAMES:
        b, worst[nm] = R.check(impl[nm][0], impl[nm][1], out[nm], f"{label}/{nm}", und[nm])
        bad += b
    return bad, worst


def test_bounds_admit_the_two_pass_oracle(ref, oracle):
    bad, worst = _inside(oracle, ref, "oracle")
    print("\nworst |oracle - ref| / bound:", {k: float(f"{v:.3g}") for k, v in worst.items()})
    assert not bad, "\n".join(bad)


def test_bounds_admit_the_documented_f64_algorithm(panel, ref):
    bad, worst = _inside(kernel_f64(panel), ref, "one-pass f64")
    print("\nworst |one-pass f64 - ref| / bound:", {k: float(f"{v:.3g}") for k, v in worst.items()})
    assert not bad, "\n".join(bad)


# (a factor common to every root cancels in the up / down ratios: M5 does not touch them)
_STD = ["vol_return1min", "vol_upVol", "vol_downVol", "vol_volume1min", "vol_range1min"]
# what each mutant touches.  M1: the sets with a level -- volumes, high / low (level 1), closes; the
# returns and pct_changes are centred near zero (level <= range), so summing them unshifted is not
# ill-conditioned and MOMR / corr_prvr are not M1's.
MUTANTS = {
    "M1 unshifted f64 sums": (dict(shift=False), R.MOMV + R.MOMH + ["corr_prv", "corr_pv", "corr_pvd", "corr_pvl",
                                                                   "corr_pvr"]),
    "M2 sums in f32": (dict(acc=np.float32), R.NAMES),
    "M3 quotients in f32": (dict(quot=np.float32), R.MOMR + R.MOMH + ["corr_prv", "corr_prvr", "corr_pvr"]),
    "M4 OLS unshifted prefix sums": (dict(ols="prefix"), R.OLS),
    "M5 roots off by 2^-24": (dict(root=2.0 ** -24), _STD + R.CORR),
}


def _plain_days():
    """[D][S]: the seeded control stock-days (plain prices, plain volumes), the inputs the suite had."""
    D, S = stage1_cases.D, stage1_cases.S
    return np.array([stage1_cases.spec(sd)[:2] == ("plain", "plain") for sd in range(D * S)]).reshape(D, S)


def _c5_misses(gv, gs, ov, os_, nm):
    """Entries that tests/parity.py's C5 rule rejects (bool array)."""
    from parity import ATOL, ATOL_DEFAULT, RTOL
    with np.errstate(invalid="ignore"):
        fin = np.isfinite(gv) & np.isfinite(ov)
        off = np.abs(gv - ov) > RTOL * np.maximum(np.abs(gv), np.abs(ov)) + ATOL.get(nm, ATOL_DEFAULT)
    return (gs != os_) | (np.isnan(gv) != np.isnan(ov)) | (fin & off)


@pytest.mark.parametrize("which", list(MUTANTS))
def test_bounds_have_teeth(panel, ref, oracle, which):
    """Each mutant leaves the bound on at least one entry of every factor it touches.  Printed:
    how many entries the bound and C5 (tests/parity.py) reject, over the panel and over its
    plain control days alone -- the measured size of the gap this module closes."""
    kw, touched = MUTANTS[which]
    out, und = ref
    mut = kernel_f64(panel, **kw)
    plain = _plain_days()
    missed, c5_blind, c5_blind_plain = [], [], []
    print(f"\n{which}: entries rejected   bound  C5 | on the plain days: bound  C5")
    for nm in touched:
        gv, gs = mut[nm]
        rv, rs, rb = out[nm]
        bad, ratio = R.check(gv, gs, out[nm], nm, und[nm])
        with np.errstate(invalid="ignore"):
            over = ~und[nm] & ((gs != rs) | (np.isnan(gv) != np.isnan(rv)) | (np.abs(gv - rv) > rb))
        c5 = _c5_misses(gv, gs, oracle[nm][0], oracle[nm][1], nm)
        assert bool(over.any()) == bool(bad) and bool(c5.any()) == bool(compare(gv, gs, *oracle[nm], nm))
        print(f"  {nm:26s} {int(over.sum()):5d} {int(c5.sum()):5d} | {int((over & plain).sum()):5d} "
              f"{int((c5 & plain).sum()):5d}")
        if not bad:
            missed.append(f"{nm} (worst ratio {ratio:.3g})")
        if not c5.any():
            c5_blind.append(nm)
        if not (c5 & plain).any():
            c5_blind_plain.append(nm)
    print(f"{which}: C5 passes {len(c5_blind)} of {len(touched)} factors on the panel: {c5_blind}")
    print(f"{which}: C5 passes {len(c5_blind_plain)} of {len(touched)} on the plain days: {c5_blind_plain}")
    assert not missed, f"{which} stays inside every bound of: {missed}"


def test_undecided_cap(ref):
    out, und = ref
    for nm in R.NAMES:
        k = int(und[nm].sum())
        if nm in R.OLS:
            assert k <= 0.01 * und[nm].size, (nm, k)
        else:
            assert k == 0, (nm, k)
