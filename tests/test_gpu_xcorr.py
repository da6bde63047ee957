"""mff_xs_corr_* on the GPU (per-day F x F pairwise-complete correlation, f64 MFMA) against
its numpy restatement tests/xs_corr_ref.py: n and the NaN pattern exact, finite values within
rtol = atol = 1e-9 (the tolerance of tests/test_gpu_neutralize.py: both sides are f64
computations of O(1) outputs).  Every comparison prints its worst error."""
import datetime as dt

import numpy as np
import pytest

import xs_corr_ref as ref
from xs_corr_ref import ABSENT, NULL, VALUE

torch = pytest.importorskip("torch")

TOL = dict(rtol=1e-9, atol=1e-9)


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def _t(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _panel(seed, rows, D, S, decimals=None):
    """t(3) exposures; every segment of S >= 16 stocks holds an ABSENT run, NULLs, NaN, +inf,
    -inf, -0.0 and +0.0.  Row 2 (when there) = 0.7 row 0 + 0.3 noise, row 3 = -row 1 (values
    only: each row keeps its own states)."""
    rng = np.random.default_rng(seed)
    x = rng.standard_t(3, (rows, D, S))
    if rows > 2:
        x[2] = 0.7 * x[0] + 0.3 * x[2]
    if rows > 3:
        x[3] = -x[1]
    if decimals is not None:
        x = np.round(x, decimals)
    st = np.full((rows, D, S), VALUE, np.uint8)
    st[rng.random((rows, D, S)) < 0.03] = NULL
    for r in range(rows if S >= 16 else 0):
        for d in range(D):
            a = int(rng.integers(0, S))
            st[r, d, a:a + max(1, S // 9)] = ABSENT
            p = rng.permutation(S)[:5]
            for q, v in zip(p, (np.nan, np.inf, -np.inf, -0.0, 0.0)):
                x[r, d, q] = v
                st[r, d, q] = VALUE
    return x, st


def _run(dev, x, st, **kw):
    from mff import engine
    c, n = engine.factor_corr(_t(x, dev), _t(st, dev), **kw)
    torch.cuda.synchronize()
    return c.cpu().numpy(), n.cpu().numpy()


def _check(got, want, name):
    gc, gn = got
    wc, wn = want
    assert gc.shape == wc.shape and gn.shape == wn.shape and gn.dtype == np.int32
    assert np.array_equal(gn, wn), f"{name}: n differs at {np.argwhere(gn != wn)[:5].tolist()}"
    m = np.isfinite(gc) & np.isfinite(wc)
    worst = float(np.abs(gc[m] - wc[m]).max()) if m.any() else 0.0
    print(f"{name}: {int(m.sum())} finite, {int(np.isnan(wc).sum())} NaN, worst abs err {worst:.3e}")
    bad = np.argwhere(np.isnan(gc) != np.isnan(wc))
    assert not len(bad), f"{name}: NaN pattern differs at {bad[:5].tolist()}"
    np.testing.assert_allclose(gc, wc, equal_nan=True, err_msg=name, **TOL)
    _properties(gc, name)


def _properties(c, name):
    assert np.array_equal(c.view(np.int64), np.swapaxes(c, 1, 2).view(np.int64)), f"{name}: not bitwise symmetric"
    dg = np.diagonal(c, axis1=1, axis2=2)
    assert ((dg == 1.0) | np.isnan(dg)).all(), f"{name}: diagonal"
    f = c[np.isfinite(c)]
    assert ((f >= -1.0) & (f <= 1.0)).all(), f"{name}: outside [-1, 1]"


@pytest.mark.gpu
@pytest.mark.parametrize("rows", [1, 2, 15, 16, 17, 58, 64, 65, 130])
def test_row_boundaries(dev, rows):
    """The 16-row MFMA padding and the 64-row block edge (65, 130: off-diagonal blocks)."""
    x, st = _panel(100 + rows, rows, 2, 257)
    _check(_run(dev, x, st), ref.corr(x, st), f"rows={rows}")


@pytest.mark.gpu
@pytest.mark.parametrize("S", [1, 2, 3, 4, 5, 63, 64, 65, 127, 128, 129, 255, 256, 257, 511, 512, 513, 1023, 1024,
                               1025, 5003])
def test_stock_boundaries(dev, S):
    """The MFMA k = 4 step and the stock tile (any tile width up to 1,024)."""
    x, st = _panel(200 + S, 17, 2, S)
    _check(_run(dev, x, st), ref.corr(x, st), f"S={S}")


@pytest.mark.gpu
def test_empty_day_and_stock_axes(dev):
    from mff import _lib, engine
    lib = _lib.load()
    c, n = engine.factor_corr(torch.zeros((3, 0, 5), dtype=torch.float64, device=dev),
                              torch.zeros((3, 0, 5), dtype=torch.uint8, device=dev))
    assert tuple(c.shape) == (0, 3, 3) and tuple(n.shape) == (0, 3, 3)
    m, days = engine.factor_corr_mean(c)
    torch.cuda.synchronize()
    assert bool(torch.isnan(m).all()) and bool((days == 0).all()) and tuple(m.shape) == (3, 3)
    c, n = engine.factor_corr(torch.zeros((3, 2, 0), dtype=torch.float64, device=dev),
                              torch.zeros((3, 2, 0), dtype=torch.uint8, device=dev))
    torch.cuda.synchronize()
    assert tuple(c.shape) == (2, 3, 3) and bool(torch.isnan(c).all()) and bool((n == 0).all())
    # the C entry points themselves: 0 for D == 0 and for S == 0
    buf = torch.full((64,), 7.0, dtype=torch.float64, device=dev)
    wsp = torch.zeros(64, dtype=torch.float64, device=dev)
    ib = torch.zeros(64, dtype=torch.int32, device=dev)
    p, w = buf.data_ptr(), wsp.data_ptr()
    assert lib.mff_xs_corr_moments(None, None, 2, 0, 5, p, None) == 0
    assert lib.mff_xs_corr_sums(None, None, 2, 0, 5, None, p, w, None) == 0
    assert lib.mff_xs_corr_finalize(p, 1, 2, 0, 2, p, ib.data_ptr(), None) == 0
    torch.cuda.synchronize()
    assert bool((buf == 7.0).all())
    assert lib.mff_xs_corr_moments(None, None, 2, 3, 0, w, None) == 0
    assert lib.mff_xs_corr_sums(None, None, 2, 3, 0, None, p, w, None) == 0   # sums [3][4][2][2]
    torch.cuda.synchronize()
    assert bool((buf[:48] == 0.0).all()) and bool((buf[48:] == 7.0).all()) and bool((wsp[:12] == 0.0).all())


@pytest.mark.gpu
def test_affine_invariance(dev):
    """Row a x + b for (a, b / sd) in {(1e-8, 0), (1e8, 0), (1, 1e6), (-3, -1e6)} gives the
    same matrix up to sign."""
    x, st = _panel(31, 6, 2, 1201)
    base = _run(dev, x, st)
    _check(base, ref.corr(x, st), "base")
    sign = np.ones(6)
    x2 = x.copy()
    for r, (a, b) in zip((0, 1, 4, 5), ((1e-8, 0.0), (1e8, 0.0), (1.0, 1e6), (-3.0, -1e6))):
        sd = np.std(x[r][ref.usable(x[r], st[r])])
        with np.errstate(invalid="ignore"):
            x2[r] = a * x[r] + b * sd
        sign[r] = np.sign(a)
    got = _run(dev, x2, st)
    want = base[0] * (sign[:, None] * sign[None, :])[None]
    m = np.isfinite(want)
    print(f"affine: worst abs err {np.abs(got[0][m] - want[m]).max():.3e}")
    assert np.array_equal(got[1], base[1]) and np.array_equal(np.isnan(got[0]), np.isnan(want))
    np.testing.assert_allclose(got[0], want, equal_nan=True, **TOL)
    _check(got, ref.corr(x2, st), "affine vs restatement")


@pytest.mark.gpu
def test_degenerate_pairs(dev):
    rng = np.random.default_rng(5)
    S = 300
    x = rng.standard_t(3, (11, 1, S))
    st = np.full((11, 1, S), ABSENT, np.uint8)
    st[0] = VALUE                               # the full row
    st[1, 0, :100] = VALUE                      # rows 1 / 2: disjoint coverage (n = 0)
    st[2, 0, 100:200] = VALUE
    st[3, 0, 250] = VALUE                       # n = 1 with row 0
    st[4, 0, [7, 260]] = VALUE                  # n = 2 with row 0: +-1
    st[5, 0, :29] = VALUE                       # 29 and 30 stocks (min_pairs = 30)
    st[6, 0, :30] = VALUE
    st[7] = VALUE                               # constant on rows 1's set, not as a row
    x[7, 0, :100] = 2.5
    st[8] = VALUE                               # an all-equal row
    x[8] = -0.3
    st[9] = VALUE                               # a row of only +-inf
    x[9] = np.where(rng.random((1, S)) < 0.5, np.inf, -np.inf)
    st[10, 0, ::2] = NULL                       # NULL / VALUE alternating
    st[10, 0, 1::2] = VALUE
    for mp in (2, 30):
        got = _run(dev, x, st, min_pairs=mp)
        want = ref.corr(x, st, min_pairs=mp)
        _check(got, want, f"degenerate min_pairs={mp}")
        c, n = got
        assert n[0, 1, 2] == 0 and np.isnan(c[0, 1, 2])
        assert n[0, 0, 3] == 1 and np.isnan(c[0, 0, 3]) and np.isnan(c[0, 3, 3])
        assert n[0, 0, 9] == 0 and np.isnan(c[0, 9]).all()
        assert np.isnan(c[0, 8]).all() and n[0, 8, 8] == S
        assert n[0, 1, 7] == 100 and np.isnan(c[0, 1, 7]) and np.isfinite(c[0, 0, 7]) and c[0, 7, 7] == 1.0
        if mp == 2:
            assert n[0, 0, 4] == 2 and abs(abs(c[0, 0, 4]) - 1.0) <= 1e-9
            assert np.isfinite(c[0, 0, 5]) and np.isfinite(c[0, 0, 6])
        else:
            assert np.isnan(c[0, 0, 4])
            assert n[0, 0, 5] == 29 and np.isnan(c[0, 0, 5]) and np.isnan(c[0, 5, 5])
            assert n[0, 0, 6] == 30 and np.isfinite(c[0, 0, 6]) and c[0, 6, 6] == 1.0


@pytest.mark.gpu
def test_output_properties(dev):
    from mff import engine
    x, st = _panel(77, 70, 3, 700)
    a = _t(x, dev), _t(st, dev)
    c1, n1 = engine.factor_corr(*a)
    c2, n2 = engine.factor_corr(*a)
    torch.cuda.synchronize()
    assert torch.equal(c1.view(torch.int64), c2.view(torch.int64)) and torch.equal(n1, n2)  # bit patterns
    c, n = c1.cpu().numpy(), n1.cpu().numpy()
    _properties(c, "properties")
    u = ref.usable(x, st).astype(np.int32)
    assert np.array_equal(n, np.einsum("ids,jds->dij", u, u))
    assert (np.diagonal(c, axis1=1, axis2=2) == 1.0).all()
    # the engineered rows: 0.7 row 0 + 0.3 noise, and -row 1 (but for the +-0.0 set into either row)
    assert c[0, 0, 2] > 0.5 and c[0, 1, 3] < -0.9
    _check((c, n), ref.corr(x, st), "properties vs restatement")


@pytest.mark.gpu
def test_spearman_with_ties(dev):
    x, st = _panel(41, 9, 2, 777, decimals=1)
    _check(_run(dev, x, st, method="spearman"), ref.corr(x, st, method="spearman"), "spearman")


@pytest.mark.gpu
def test_mean_over_days(dev):
    from mff import engine
    x, st = _panel(51, 5, 6, 90)
    st[1, 2] = ABSENT                           # row 1 has no stock on day 2
    st[4, :, 3:] = ABSENT                       # row 4 x row 3: never 2 common stocks
    st[3, :, :3] = NULL
    want_c, _ = ref.corr(x, st)
    c, _ = engine.factor_corr(_t(x, dev), _t(st, dev))
    m, days = engine.factor_corr_mean(c)
    m2, days2 = engine.factor_corr_mean(_t(want_c, dev))
    torch.cuda.synchronize()
    wm, wd = ref.corr_mean(want_c)
    assert wd[1, 1] == 5 and wd[3, 4] == 0 and np.isnan(wm[3, 4])
    for (gm, gd), name in (((m, days), "mean of the GPU matrix"), ((m2, days2), "mean of the restatement's")):
        gm, gd = gm.cpu().numpy(), gd.cpu().numpy()
        assert gd.dtype == np.int32 and np.array_equal(gd, wd) and np.array_equal(np.isnan(gm), np.isnan(wm))
        ok = ~np.isnan(wm)
        print(f"{name}: worst abs err {np.abs(gm[ok] - wm[ok]).max():.3e}")
        np.testing.assert_allclose(gm, wm, equal_nan=True, **TOL)


@pytest.mark.gpu
@pytest.mark.parametrize("S", [29, 257])
@pytest.mark.parametrize("R", [2, 3])
def test_stock_shards_match_one_rank(dev, R, S):
    from mff import dist
    x, st = _panel(400 + R + S, 7, 3, S)
    s0, s1 = dist.shard_bounds(S, R, 0)         # uneven shards: 15 + 14, 10 + 10 + 9, 129 + 128, 86 + 86 + 85
    assert len({b - a for a, b in (dist.shard_bounds(S, R, r) for r in range(R))}) == 2
    st[4, 1, s0:s1] = ABSENT                    # rank 0 holds no usable stock of row 4 on day 1
    one = {m: _run(dev, x, st, method=m) for m in ("pearson", "spearman")}
    _check(one["pearson"], ref.corr(x, st), "one rank")

    def rank_fn(comm):
        a, b = dist.shard_bounds(S, R, comm.rank)
        return {m: _run(dev, x[:, :, a:b], st[:, :, a:b], method=m, comm=comm, stocks_total=S)
                for m in ("pearson", "spearman")}

    for r, got in enumerate(dist.run_threads(R, rank_fn)):
        for m in ("pearson", "spearman"):
            _check(got[m], one[m], f"{m} rank {r} of {R}, S={S}")


@pytest.mark.gpu
def test_errors_write_nothing(dev):
    from mff import _lib, engine
    lib = _lib.load()
    big = lib.mff_xs_corr_max_rows() + 1
    assert big > 256
    buf = torch.full((4096,), 7.0, dtype=torch.float64, device=dev)
    ib = torch.full((4096,), 9, dtype=torch.int32, device=dev)
    xv = torch.zeros((2, 1, 8), dtype=torch.float64, device=dev)
    xs = torch.full((2, 1, 8), VALUE, dtype=torch.uint8, device=dev)
    p, q = buf.data_ptr(), ib.data_ptr()
    assert lib.mff_xs_corr_moments(xv.data_ptr(), xs.data_ptr(), big, 1, 8, p, None) < 0
    assert lib.mff_xs_corr_sums(xv.data_ptr(), xs.data_ptr(), big, 1, 8, None, p, p, None) < 0
    assert lib.mff_xs_corr_finalize(p, 1, big, 1, 2, p, q, None) < 0
    assert lib.mff_xs_corr_mean(p, big, 1, p, q, None) < 0
    assert lib.mff_xs_corr_finalize(p, 1, 2, 1, 1, p, q, None) < 0       # min_pairs = 1
    assert b"min_pairs" in lib.mff_last_error()
    assert lib.mff_xs_corr_sums(xv.data_ptr(), xs.data_ptr(), 0, 1, 8, None, p, p, None) < 0
    assert lib.mff_xs_corr_sums(xv.data_ptr(), xs.data_ptr(), 2, -1, 8, None, p, p, None) < 0
    torch.cuda.synchronize()
    assert bool((buf == 7.0).all()) and bool((ib == 9).all())
    with pytest.raises(ValueError):
        engine.factor_corr(xv, xs, min_pairs=1)
    with pytest.raises(ValueError):
        engine.factor_corr(xv, xs, method="kendall")
    with pytest.raises(_lib.MffError):
        engine.factor_corr(torch.zeros((big, 1, 1), dtype=torch.float64, device=dev),
                           torch.zeros((big, 1, 1), dtype=torch.uint8, device=dev))


@pytest.mark.gpu
def test_factor_correlation_surface(dev):
    import pandas as pd

    import mff
    from mff import frames
    from mff.factor import Factor, factor_correlation
    assert mff.factor_correlation is factor_correlation
    rng = np.random.default_rng(9)
    D, S = 6, 40
    codes = [f"{i:06d}.SZ" for i in range(S)]
    dates = [dt.date(2024, 3, 1) + dt.timedelta(days=i) for i in range(D)]
    base = rng.standard_t(3, (D, S))
    specs = {"alpha": (slice(0, D), slice(0, 32)), "beta": (slice(1, D), slice(6, S)), "gamma": (slice(0, D - 1), slice(0, S))}
    fs, wide = [], {}
    for k, (nm, (ds, ss)) in enumerate(specs.items()):
        x = 0.6 * base + 0.4 * rng.standard_t(3, (D, S))
        st = np.full((D, S), ABSENT, np.uint8)
        st[ds, ss] = VALUE
        st[2, 10 + k] = NULL
        x[3, 12 + k] = np.nan
        fs.append(Factor(nm, frames.to_long(x, st, codes, dates, nm)))
        wide[nm] = np.where((st == VALUE) & np.isfinite(x), x, np.nan)
    names = list(specs)
    means = {}
    for method in ("pearson", "spearman"):
        means[method] = mean, daily = factor_correlation(fs, method=method, min_pairs=5, return_daily=True, device=dev)
        assert list(mean.index) == names and list(mean.columns) == names
        assert list(daily.columns) == ["date", "factor_a", "factor_b", "corr", "n"]
        per_day = []
        for d in range(D):
            # (pandas re-ranks inside each pair set: compare Spearman on the ranks of each column instead)
            df = pd.DataFrame({nm: wide[nm][d] for nm in names})
            if method == "spearman":
                df = df.rank()
            per_day.append(df.corr(min_periods=5).to_numpy())
        per_day = np.array(per_day)
        with np.errstate(invalid="ignore"):
            want = np.nanmean(per_day, axis=0)
        print(f"surface {method}: worst abs err {np.nanmax(np.abs(mean.to_numpy() - want)):.3e}")
        np.testing.assert_allclose(mean.to_numpy(), want, equal_nan=True, **TOL)
        key = list(zip(daily["date"], daily["factor_a"], daily["factor_b"]))
        assert key == sorted(key) and len(set(key)) == len(key)
        order = {nm: i for i, nm in enumerate(names)}
        assert all(order[a] <= order[b] for a, b in zip(daily["factor_a"], daily["factor_b"]))
        cnt = sum(int((~np.isnan(wide[a][d]) & ~np.isnan(wide[b][d])).any())
                  for d in range(D) for i, a in enumerate(names) for b in names[i:])
        assert (daily["n"] >= 1).all() and len(daily) == cnt == 6 * D - 6  # beta misses day 0, gamma the last
        for dte, a, b, cv, nv in daily.itertuples(index=False):
            d = dates.index(dte)
            ok = ~np.isnan(wide[a][d]) & ~np.isnan(wide[b][d])
            assert nv == ok.sum()
            w = per_day[d][order[a], order[b]]
            assert (np.isnan(cv) and np.isnan(w)) or abs(cv - w) <= 2e-9
    only_mean = factor_correlation({"u": fs[0], "v": fs[1]}, device=dev)
    assert list(only_mean.index) == ["u", "v"]
    assert abs(only_mean.loc["u", "v"] - means["pearson"][0].loc["alpha", "beta"]) <= 1e-12
    row = fs[0].corr_with(fs[1:], device=dev)
    assert list(row.index) == ["beta", "gamma"]
    np.testing.assert_allclose(row.to_numpy(), factor_correlation(fs, device=dev).loc["alpha", ["beta", "gamma"]])
    with pytest.raises(ValueError, match="duplicate"):
        factor_correlation([fs[0], fs[0]], device=dev)
    with pytest.raises(ValueError, match="method"):
        factor_correlation(fs, method="kendall", device=dev)
    with pytest.raises(ValueError, match="min_pairs"):
        factor_correlation(fs, min_pairs=1, device=dev)
