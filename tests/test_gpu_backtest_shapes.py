"""Back-test kernels (csrc/mff_ic.hip, csrc/mff_bt.hip, k_calendar) beyond one wavefront
per date and one workgroup per kernel: strided reductions, multi-block launches, the
global-memory sort of k_bt_qcut (M > SORT_CAP keys), its grid-stride loop over more than
2048 dates, group counts up to BT_MAXG, and every bin of every date of mff_bt_qcut
compared exactly with pandas qcut (oracle_qcut).

Finite exposures only: +-inf values make numpy's lerp produce NaN edges, which the
kernel does not restate (out of scope here)."""
import datetime as dt
import functools
import math
from fractions import Fraction

import numpy as np
import pandas as pd
import pytest

import mff_oracle as O
from parity import compare

torch = pytest.importorskip("torch")

@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def _t(a, dev):
    return torch.from_numpy(np.array(a, order="C")).to(dev)  # a copy: the shared inputs are read-only


def _ro(*arrays):
    """Shared references stay unchanged: hand them out read-only."""
    for a in arrays:
        a.setflags(write=False)
    return arrays


# --------------------------------------------------------------------------- qcut, direct
def _gpu_qcut(dev, x, st, G, shards=None):
    """mff_bt_qcut on [D][S] rows -> group [D][S] (numpy int64).  shards: None (R = 1) or
    a list of (s0, s1) stock blocks: the [R][D][S_all] planes are built by hand (short
    shards padded with ABSENT) and the kernel runs once per shard on its local rows."""
    from mff import _lib
    lib = _lib.load()
    D, S = x.shape
    shards = shards or [(0, S)]
    R = len(shards)
    S_all = max(s1 - s0 for s0, s1 in shards)
    xa = np.full((R, D, S_all), 123.0)  # a padded slot's value must not count
    sa = np.full((R, D, S_all), O.ABSENT, np.uint8)
    for r, (s0, s1) in enumerate(shards):
        xa[r, :, :s1 - s0] = x[:, s0:s1]
        sa[r, :, :s1 - s0] = st[:, s0:s1]
    xa_d, sa_d = _t(xa, dev), _t(sa, dev)
    out = np.empty((D, S), np.int64)
    for s0, s1 in shards:
        xl, sl = _t(x[:, s0:s1], dev), _t(st[:, s0:s1], dev)
        ws = torch.empty(lib.mff_bt_qcut_workspace_bytes(D, S_all, R), dtype=torch.uint8, device=dev)
        grp = torch.full((D, s1 - s0), -99, dtype=torch.int8, device=dev)  # -99: never written
        _lib.check(lib.mff_bt_qcut(_lib.ptr(xl), _lib.ptr(sl), D, s1 - s0, _lib.ptr(xa_d), _lib.ptr(sa_d),
                                   R, S_all, G, _lib.ptr(grp), _lib.ptr(ws),
                                   torch.cuda.current_stream(dev).cuda_stream), "mff_bt_qcut")
        torch.cuda.synchronize()
        out[:, s0:s1] = grp.cpu().numpy()
    return out


def _included(x, st):
    return (st == O.VALUE) & ~np.isnan(x)


def _oracle_bins(x, st, G):
    return np.stack([O.oracle_qcut(x[d], _included(x[d], st[d]), G) for d in range(x.shape[0])])


def _assert_bins(got, ref, G):
    assert got.shape == ref.shape
    bad = [d for d in range(ref.shape[0]) if not np.array_equal(got[d], ref[d])]
    detail = [(d, int((got[d] != ref[d]).sum())) for d in bad[:20]]
    assert not bad, f"G={G}: {len(bad)} dates differ from pandas qcut, (date, stocks): {detail}"


LADDER_S, LADDER_D = 130, 128
LADDER_G = [2, 3, 5, 6, 7, 10, 11, 13, 20, 63]


@functools.lru_cache(maxsize=None)
def _ladder(kind):
    """Date d holds n = d + 2 VALUE stocks scattered over the row (the rest ABSENT, with a
    value that would move every edge if it counted).  'step3': x = 1 + 3k, where the
    virtual index (n-1) q often rounds to an integer without being one, so an edge
    coincides with a data value; 'tenth': x = k / 10 rounded to one decimal
    (non-representable steps); 'ties': each tenth held by three stocks."""
    rng = np.random.default_rng(31)
    x = np.full((LADDER_D, LADDER_S), 1e9)
    st = np.full((LADDER_D, LADDER_S), O.ABSENT, np.uint8)
    for d in range(LADDER_D):
        n = d + 2
        k = rng.permutation(n).astype(np.float64)
        pos = rng.permutation(LADDER_S)[:n]
        x[d, pos] = {"step3": 1.0 + 3.0 * k, "tenth": np.round(k / 10.0, 1),
                     "ties": np.round((k // 3) / 10.0, 1)}[kind]
        st[d, pos] = O.VALUE
    return _ro(x, st)


@functools.lru_cache(maxsize=None)
def _ladder_ref(kind, G):
    return _ro(_oracle_bins(*_ladder(kind), G))[0]


def _fma(a, b, c):
    """round(a * b + c) with one rounding (a device v_fma_f64), by exact rationals."""
    r = Fraction(a) * Fraction(b) + Fraction(c)
    return float(r) if r else 0.0


def _kernel_bins(x, ok, G, contracted):
    """k_bt_qcut / np_quantile (csrc/mff_bt.hip) step for step.  contracted=False rounds
    every operation on its own (numpy's arithmetic); contracted=True fuses
    gamma = (n-1) q - floor and both lerps into FMAs, as a compiler that contracts
    floating-point expressions emits them."""
    v = np.sort(x[ok])
    n = v.size
    edges = []
    if n:
        step = 1.0 / G
        nm1 = float(n - 1)
        for i in range(G + 1):
            q = 1.0 if i == G else i * step
            q = (q * 100.0) / 100.0
            virt = nm1 * q
            prev = float(math.floor(virt))
            gam = _fma(nm1, q, -prev) if contracted else virt - prev
            lo = int(prev)
            hi = lo + 1
            if virt >= nm1:
                lo = hi = n - 1
            if virt < 0.0:
                lo = hi = 0
            a, b = float(v[lo]), float(v[hi])
            diff = b - a
            if gam >= 0.5:
                e = _fma(-diff, 1.0 - gam, b) if contracted else b - diff * (1.0 - gam)
            else:
                e = _fma(diff, gam, a) if contracted else a + diff * gam
            if not edges or e != edges[-1]:
                edges.append(e)
    out = np.full(x.size, -1, np.int64)
    k = len(edges)
    if k >= 2:
        e = np.asarray(edges)
        ids = np.searchsorted(e, x, side="left")  # #edges < x
        ids[x == e[0]] = 1
        hit = ok & (ids >= 1) & (ids <= k - 1)
        out[hit] = ids[hit] - 1
    return out


@pytest.mark.parametrize("kind", ["step3", "tenth", "ties"])
def test_qcut_ladder_formula_uncontracted_matches_pandas(kind):
    """The kernel's arithmetic with separately rounded operations gives pandas' bins on
    every date of the ladder for every group count of the GPU test."""
    x, st = _ladder(kind)
    for G in LADDER_G:
        ref = _ladder_ref(kind, G)
        got = np.stack([_kernel_bins(x[d], _included(x[d], st[d]), G, False) for d in range(LADDER_D)])
        _assert_bins(got, ref, G)


@pytest.mark.parametrize("G", [6, 10, 11, 13, 20])
def test_qcut_ladder_detects_contracted_edges(G):
    """The ladder has teeth: with gamma and the lerps fused into FMAs the same
    arithmetic puts at least one stock of the 'step3' ladder into another bin."""
    x, st = _ladder("step3")
    ref = _ladder_ref("step3", G)
    moved = sum(int((_kernel_bins(x[d], _included(x[d], st[d]), G, True) != ref[d]).sum())
                for d in range(LADDER_D))
    assert moved >= 1


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["step3", "tenth", "ties"])
@pytest.mark.parametrize("G", LADDER_G)
def test_qcut_ladder_bins_exact(dev, kind, G):
    """Every bin of every date, n = 2..129 included stocks per date."""
    x, st = _ladder(kind)
    _assert_bins(_gpu_qcut(dev, x, st, G), _ladder_ref(kind, G), G)


@functools.lru_cache(maxsize=None)
def _sort_rows(S, full):
    """Four dates over S stocks: 0 tie-heavy (one decimal), 1 distinct values with about
    10 % NULL / NaN / ABSENT interleaved, 2 all excluded, 3 all equal.  full=True: two
    dates on which every key is included (the included count equals M)."""
    rng = np.random.default_rng(S + int(full))
    if full:
        x = np.stack([np.round(rng.normal(size=S), 1), rng.permutation(S) * 0.37 - 11.0])
        return _ro(x, np.full((2, S), O.VALUE, np.uint8))
    x = np.empty((4, S))
    st = np.full((4, S), O.VALUE, np.uint8)
    x[0] = np.round(rng.normal(size=S), 1)
    st[0, rng.random(S) < 0.03] = O.NULLV
    x[1] = rng.permutation(S) * 0.37 - 11.0
    u = rng.random(S)
    st[1, u < 0.03] = O.NULLV
    st[1, (u >= 0.03) & (u < 0.06)] = O.ABSENT
    x[1, (u >= 0.06) & (u < 0.10)] = np.nan
    x[2] = rng.normal(size=S)
    st[2] = rng.choice(np.array([O.NULLV, O.ABSENT], np.uint8), S)
    x[2, ::3] = np.nan
    st[2, ::3] = O.VALUE  # VALUE but NaN: excluded too
    x[3] = 0.7
    return _ro(x, st)


@functools.lru_cache(maxsize=None)
def _sort_ref(S, full):
    return _ro(_oracle_bins(*_sort_rows(S, full), 10))[0]


@pytest.mark.gpu
@pytest.mark.parametrize("S,shards,full", [
    (8192, None, False),    # M = SORT_CAP (csrc/mff_sort.h): the last size sorted in LDS
    (8193, None, False),    # one chunk + one key, one merge pass
    (16385, None, False),   # three chunks, two merge passes, the last run one key
    (20000, None, False),
    (16385, None, True),    # every key included
    (8193, [(0, 4097), (4097, 8193)], False),      # R = 2, M = 2 * 4097 = 8194
    (20000, [(0, 9993), (9993, 20000)], False),    # R = 2, M = 2 * 10007, shard 0 padded
])
def test_qcut_sort_paths_bins_exact(dev, S, shards, full):
    """The LDS sort at its cap and the global-memory chunk + merge sort (workspace at
    blockIdx * 2 * M, the included count scanned over a global array), G = 10; with R = 2
    the key set is the two shards' planes, M = 2 * max shard width."""
    x, st = _sort_rows(S, full)
    ref = _sort_ref(S, full)
    assert full or ((ref[2] == -1).all() and (ref[3] == -1).all() and ref[1].max() == 9)
    _assert_bins(_gpu_qcut(dev, x, st, 10, shards), ref, 10)


@functools.lru_cache(maxsize=None)
def _stride_case():
    D, S = 2100, 70
    rng = np.random.default_rng(41)
    x = np.round(rng.normal(size=(D, S)), 1)
    st = np.full((D, S), O.VALUE, np.uint8)
    u = rng.random((D, S))
    st[u < 0.05] = O.NULLV
    st[(u >= 0.05) & (u < 0.12)] = O.ABSENT
    x[(u >= 0.12) & (u < 0.15)] = np.nan
    st[100] = O.ABSENT
    st[2077] = O.NULLV
    x[2090] = -3.5
    return _ro(x, st, _oracle_bins(x, st, 5))


@pytest.mark.gpu
def test_qcut_grid_stride_bins_exact(dev):
    """D = 2100 > 2048 workgroups: the dates >= 2048 are the second trip of the grid-stride
    loop.  All 2100 dates are compared with their own pandas cut."""
    x, st, ref = _stride_case()
    _assert_bins(_gpu_qcut(dev, x, st, 5), ref, 5)


# --------------------------------------------------------------------------- shared inputs
def _daily(rng, D, S, base=0):
    """test_gpu_ic._daily for any shape: suspension runs, nulls, a NaN pct, NaN / null
    exposures, with the edge stocks at indices base + 3, base + 4, base + 7."""
    pct = rng.normal(0, 0.02, (D, S))
    ps = np.full((D, S), O.VALUE, np.uint8)
    ps[5:9, base + 3] = O.ABSENT
    ps[10:30, base + 7] = O.ABSENT
    ps[rng.random((D, S)) < 0.01] = O.NULLV
    pct[min(12, D - 1), base + 4] = np.nan
    x = rng.normal(size=(D, S))
    xs = ps.copy()
    x[rng.random((D, S)) < 0.02] = np.nan
    xs[rng.random((D, S)) < 0.02] = O.NULLV
    return pct, ps, x, xs


# --------------------------------------------------------------------------- group returns
def _cell_bounds(x, xs, pct, ps, period_of, P, G, w, wst):
    """Per (period, group) cell of oracle_group_test: n = its row count and m = its mean
    absolute (weighted) return, sum |r| / n or sum |w r| / sum w over the rows whose
    weight counts -- the scale of the recursive-summation bound n 2^-52 m."""
    D, S = x.shape
    grp = _oracle_bins(x, xs, G)
    n = np.zeros((P, G))
    m = np.zeros((P, G))
    prev_g = np.full(S, -1, np.int64)
    prev_w = np.zeros(S)
    prev_wok = np.zeros(S, bool)
    for p in range(P):
        days = np.flatnonzero(period_of == p)
        row = xs[days] != O.ABSENT
        held = row.any(axis=0)
        fac = np.where(row & (ps[days] == O.VALUE), pct[days] + 1.0, 1.0)
        r = np.prod(fac, axis=0) - 1.0
        last = days[row.shape[0] - 1 - np.argmax(row[::-1], axis=0)]
        cols = np.arange(S)
        for g in range(G):
            sel = held & (prev_g == g)
            n[p, g] = sel.sum()
            if not sel.any():
                continue
            if w is None:
                m[p, g] = np.abs(r[sel]).sum() / sel.sum()
            else:
                k = sel & prev_wok
                sw = prev_w[k].sum()
                m[p, g] = np.abs(prev_w[k] * r[k]).sum() / sw if sw != 0 else 0.0
        prev_g = np.where(held, grp[last, cols], prev_g)
        if w is not None:
            prev_w = np.where(held, w[last, cols], prev_w)
            prev_wok = np.where(held, wst[last, cols] == O.VALUE, prev_wok)
    return n, m


@functools.lru_cache(maxsize=None)
def _bt_case(S, D, G, weighted, large=False):
    from mff.factor import rebalance_periods
    rng = np.random.default_rng(1000 + S)
    pct, ps, x, xs = _daily(rng, D, S)
    x = np.round(x, 2)  # ties inside the quantile cut
    x[2] = 1.25         # a date without a cut: fewer than two edges
    xs[3] = O.ABSENT
    xs[3, :1] = O.VALUE
    w = rng.uniform(1, 5, (D, S))
    wst = ps.copy()
    wst[(rng.random((D, S)) < 0.05) & (ps != O.ABSENT)] = O.NULLV
    if large:
        period_of = np.arange(D) // 5
        P = int(period_of[-1]) + 1
    else:
        dates = [dt.date(2024, 1, 1) + dt.timedelta(days=i) for i in range(D)]
        period_of, labels = rebalance_periods(dates, "weekly")
        P = len(labels)
    wa = (w, wst) if weighted else (None, None)
    oret, opres = O.oracle_group_test(x, xs, pct, ps, period_of, P, G, *wa)
    n, m = _cell_bounds(x, xs, pct, ps, period_of, P, G, *wa)
    assert np.array_equal(n > 0, opres == 1)  # the bound's cells are the oracle's cells
    return _ro(x, xs, pct, ps, w, wst, np.asarray(period_of, np.int32), oret, opres, n, m) + (P,)


def _check_group_returns(dev, case, G, weighted, R):
    from mff import dist, engine
    x, xs, pct, ps, w, wst, period_of, oret, opres, n, m, P = case
    S = x.shape[1]
    assert 2 * int(opres.sum()) >= P * G  # at least half of the cells hold stocks

    def rank_fn(comm):
        s0, s1 = dist.shard_bounds(S, R, comm.rank) if comm is not None else (0, S)
        sl = slice(s0, s1)
        args = [_t(a[:, sl], dev) for a in (x, xs, pct, ps)]
        wa = (_t(w[:, sl], dev), _t(wst[:, sl], dev)) if weighted else (None, None)
        ret, pres = engine.group_returns(*args, _t(period_of, dev), P, G, *wa, comm=comm)
        torch.cuda.synchronize()
        return ret.cpu().numpy(), pres.cpu().numpy()

    outs = [rank_fn(None)] if R == 1 else dist.run_threads(R, rank_fn)
    tol = 1e-9 * np.abs(oret) + n * 2.0 ** -52 * m
    k = (opres == 1) & ~np.isnan(oret)  # a NaN pct_change makes its cell's mean NaN
    for ret, pres in outs:
        assert np.array_equal(pres, opres)
        assert np.array_equal(np.isnan(ret), np.isnan(oret))
        err = np.abs(ret - oret)
        assert (err[k] <= tol[k]).all(), (float((err[k] - tol[k]).max()), np.argwhere(k & (err > tol))[:5])


@pytest.mark.gpu
@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("G", [1, 3, 10, 63])
@pytest.mark.parametrize("S", [64, 65, 200])
def test_group_returns_beyond_one_wave(dev, S, G, weighted):
    """k_bt_periods over more than one wave of stocks, k_bt_reduce's strided loop taking
    further trips, P * G no multiple of the four waves of a reduce block, group counts up
    to BT_MAXG (with 63 groups over 64 stocks many cells are empty)."""
    _check_group_returns(dev, _bt_case(S, 70, G, weighted), G, weighted, 1)


@pytest.mark.gpu
@pytest.mark.parametrize("R", [1, 2])
def test_group_returns_large(dev, R):
    """S = 8300 > SORT_CAP: the cut sorts in global memory inside engine.group_returns,
    as one rank and as two stock shards (M = 2 * 4150)."""
    _check_group_returns(dev, _bt_case(8300, 24, 10, True, True), 10, True, R)


@pytest.mark.gpu
def test_factor_group_test_deciles_end_to_end(dev):
    """group_num reaches the kernel: Factor.group_test(group_num=10) at S = 130."""
    from mff import frames
    from mff.factor import Factor, rebalance_periods
    rng = np.random.default_rng(51)
    D, S = 70, 130
    pct, ps, x, xs = _daily(rng, D, S)
    x = np.round(x, 1)
    w = rng.uniform(1, 5, (D, S))
    wst = ps.copy()
    wst[(rng.random((D, S)) < 0.05) & (ps != O.ABSENT)] = O.NULLV
    dates = [dt.date(2024, 1, 1) + dt.timedelta(days=i) for i in range(D)]
    codes = [f"{i:06d}.SZ" for i in range(S)]
    ex = frames.to_long(x, xs, codes, dates, "f")
    pv = frames.to_long(pct, ps, codes, dates, "pct_change")
    pv["tmc"] = frames.to_long(w, wst, codes, dates, "tmc")["tmc"]
    g = Factor("f", ex).group_test(frequency="weekly", weight_param="tmc", group_num=10, plot_out=False,
                                   return_df=True, pv_data=pv, device=dev)
    period_of, labels = rebalance_periods(dates, "weekly")
    oret, opres = O.oracle_group_test(x, xs, pct, ps, period_of, len(labels), 10, w, wst)
    p_idx, g_idx = np.nonzero(opres)
    assert set(g_idx) == set(range(10))
    exp = pd.DataFrame({"date": [labels[p] for p in p_idx], "group": [f"group_{k + 1}" for k in g_idx],
                        "pct_change": oret[p_idx, g_idx]}).sort_values(["date", "group"]).reset_index(drop=True)
    assert list(g["date"]) == list(exp["date"]) and list(g["group"]) == list(exp["group"])
    np.testing.assert_allclose(g["pct_change"].to_numpy(), exp["pct_change"].to_numpy(), rtol=1e-9)


# --------------------------------------------------------------------------- IC series
IC_D = 12
IC_FIRST70, IC_CONST, IC_ONE, IC_LAST_SHARD, IC_OFFSET = 1, 2, 3, 4, 5


def _pearson_longdouble(x, y):
    x, y = x.astype(np.longdouble), y.astype(np.longdouble)
    dx, dy = x - x.sum() / x.size, y - y.sum() / y.size
    return float((dx * dy).sum() / np.sqrt((dx * dx).sum() * (dy * dy).sum()))


@functools.lru_cache(maxsize=None)
def _ic_case(S):
    """12 dates of exposure x and future return y (oracle_future_return, N = 2, so the
    last two dates hold no pair), with the dates IC_*: the first 70 stocks excluded; a
    constant exposure; one pair; every pair in the last third of the stocks (the last of
    three shards); x = 1e6 + N(0, 1) against y = 1e3 + N(0, 0.02)."""
    from mff import dist
    rng = np.random.default_rng(2000 + S)
    pct, ps, x, xs = _daily(rng, IC_D, S)
    fv, fs = O.oracle_future_return(pct, ps, 2)
    xs[IC_FIRST70, :70] = O.NULLV
    x[IC_CONST] = 1.25
    xs[IC_ONE] = O.ABSENT
    xs[IC_ONE, S - 1] = O.VALUE
    fs[IC_ONE, S - 1] = O.VALUE
    fv[IC_ONE, S - 1] = 0.01
    xs[IC_LAST_SHARD, :dist.shard_bounds(S, 3, 2)[0]] = O.ABSENT
    x[IC_OFFSET] = 1e6 + rng.normal(size=S)
    fv[IC_OFFSET] = 1e3 + rng.normal(0, 0.02, S)
    fs[IC_OFFSET] = O.VALUE
    oic, oric = O.oracle_ic(x, xs, fv, fs)
    ok = (xs[IC_OFFSET] == O.VALUE) & ~np.isnan(x[IC_OFFSET])
    oic[IC_OFFSET] = _pearson_longdouble(x[IC_OFFSET, ok], fv[IC_OFFSET, ok])
    return _ro(x, xs, fv, fs, oic, oric)


@pytest.mark.gpu
@pytest.mark.parametrize("R", [1, 3])
@pytest.mark.parametrize("S", [64, 65, 129, 1000])
def test_ic_series_beyond_one_wave(dev, S, R):
    """k_ic_moments' strided loops and its first-pair search past the first 64 stocks,
    the Chan combine skipping ranks without pairs, the shifted two-pass at a large
    offset; the constant-exposure date is exactly NaN for every R."""
    from mff import dist, engine
    x, xs, fv, fs, oic, oric = _ic_case(S)
    assert np.isnan(oic[[IC_CONST, IC_ONE, IC_D - 2, IC_D - 1]]).all()
    assert np.isnan(oic[IC_FIRST70]) == (S <= 71) and not np.isnan(oic[[IC_LAST_SHARD, IC_OFFSET]]).any()

    def rank_fn(comm):
        s0, s1 = dist.shard_bounds(S, R, comm.rank) if comm is not None else (0, S)
        sl = slice(s0, s1)
        ic, ric = engine.ic_series(*[_t(a[:, sl], dev) for a in (x, xs, fv, fs)], comm=comm)
        torch.cuda.synchronize()
        return ic.cpu().numpy(), ric.cpu().numpy()

    outs = [rank_fn(None)] if R == 1 else dist.run_threads(R, rank_fn)
    k = ~np.isnan(oic)
    for ic, ric in outs:
        assert np.array_equal(np.isnan(ic), np.isnan(oic))
        np.testing.assert_allclose(ic[k], oic[k], rtol=1e-9, atol=1e-12)
        np.testing.assert_allclose(ric[k], oric[k], rtol=1e-9, atol=1e-12)


# --------------------------------------------------------------------------- future return
FR_D = 120


@functools.lru_cache(maxsize=None)
def _fr_case(S, N):
    """Daily rows with pattern stocks at the end of the first 256-thread block and at the
    start of the second and third (where S reaches them): exactly N present rows; all
    rows ABSENT; a null every N-th present row; a -100 % day and a +inf day; N + 1
    present rows."""
    rng = np.random.default_rng(3000 + S + N)
    pct, ps, _, _ = _daily(rng, FR_D, S)
    for b in (250, 256, 512):
        for j in range(5):
            s = b + j
            if s >= S:
                continue
            ps[:, s] = O.VALUE
            if j in (0, 4):
                keep = np.sort(rng.permutation(FR_D)[:min(FR_D, N + j // 4)])
                ps[:, s] = O.ABSENT
                ps[keep, s] = O.VALUE
            elif j == 1:
                ps[:, s] = O.ABSENT
            elif j == 2:
                ps[40:55, s] = O.ABSENT
                rows = np.flatnonzero(ps[:, s] != O.ABSENT)
                ps[rows[N - 1::N], s] = O.NULLV
            else:
                pct[30, s] = -1.0
                pct[77, s] = np.inf
    return _ro(pct, ps, *O.oracle_future_return(pct, ps, N))


@pytest.mark.gpu
@pytest.mark.parametrize("N", [1, 20, 119, 130])
@pytest.mark.parametrize("S", [256, 257, 600])
def test_future_return_beyond_one_block(dev, S, N):
    """k_future_return with a second and a third 256-thread block; N = 130 > D leaves
    every present stock-day NULL."""
    from mff import engine
    pct, ps, ov, os_ = _fr_case(S, N)
    assert (os_ == O.VALUE).any() == (N < FR_D)
    gv, gs = engine.future_return(_t(pct, dev), _t(ps, dev), N)
    assert not compare(gv.cpu().numpy(), gs.cpu().numpy(), ov, os_, "future_return", atol=1e-12)


# --------------------------------------------------------------------------- calendar
@functools.lru_cache(maxsize=None)
def _cal_case():
    from mff.factor import calendar_windows
    _, _, x, xs = _daily(np.random.default_rng(61), 75, 300, base=256)
    x[10:17, 261] = 2.5      # constant week (z -> NaN), in the second block
    xs[10:17, 261] = O.VALUE
    x[2, 256:] = 1.25
    xs[3, 257:] = O.ABSENT   # single-row windows around it (std null)
    dates = [dt.date(2024, 1, 1) + dt.timedelta(days=i) for i in range(75)]
    pstart, _ = calendar_windows(dates, "weekly")
    return _ro(x, xs, pstart)


@functools.lru_cache(maxsize=None)
def _cal_ref(method):
    x, xs, pstart = _cal_case()
    return _ro(*O.oracle_calendar(x, xs, pstart, method))


@pytest.mark.gpu
@pytest.mark.parametrize("method", ["o", "m", "z", "std"])
def test_calendar_beyond_one_block(dev, method):
    """k_calendar with a second 256-thread block holding the edge rows: suspensions,
    nulls, NaN, a constant window, a window whose last row is null."""
    from mff import engine
    x, xs, pstart = _cal_case()
    ov, os_ = _cal_ref(method)
    assert (os_[:, 256:] == O.NULLV).any() and (os_[:, 256:] == O.ABSENT).any()
    gv, gs = engine.calendar(_t(x, dev), _t(xs, dev), _t(pstart, dev), method)
    assert not compare(gv.cpu().numpy(), gs.cpu().numpy(), ov, os_, f"calendar-{method}", atol=1e-12)
