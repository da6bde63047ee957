"""mff_xs_neutralize on the GPU (MAD winsorise, industry / size neutralise, standardise)
against its numpy restatement tests/xs_neutralize_ref.py: states exact, NaN / inf exact,
finite values within rtol = atol = 1e-9 (both sides are f64 computations of O(1) outputs;
they differ by summation order only).  Every comparison prints its worst error."""
import datetime as dt

import numpy as np
import pytest

import xs_neutralize_ref as ref
from parity import compare
from xs_neutralize_ref import ABSENT, NULL, VALUE

torch = pytest.importorskip("torch")

TOL = dict(rtol=1e-9, atol=1e-9)


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def _t(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _panel(seed, rows, D, S, G):
    """Heavy-tailed exposures where every segment holds an ABSENT run, NULLs, NaN, +inf,
    -inf, -0.0 and +0.0; industries with stocks that have none; sizes with NULL and
    non-finite entries."""
    rng = np.random.default_rng(seed)
    x = rng.standard_t(3, (rows, D, S))
    st = np.full((rows, D, S), VALUE, np.uint8)
    st[rng.random((rows, D, S)) < 0.03] = NULL
    for r in range(rows if S >= 16 else 0):  # (a tiny segment keeps its few stocks)
        for d in range(D):
            a = int(rng.integers(0, S))
            st[r, d, a:a + max(1, S // 9)] = ABSENT
            p = rng.permutation(S)[:5]
            for q, v in zip(p, (np.nan, np.inf, -np.inf, -0.0, 0.0)):
                x[r, d, q] = v
                st[r, d, q] = VALUE
    g = rng.integers(0, G, (D, S)).astype(np.int32)
    g[rng.random((D, S)) < 0.05] = -1
    z = rng.normal(23.0, 1.5, (D, S))
    zst = np.full((D, S), VALUE, np.uint8)
    zst[rng.random((D, S)) < 0.03] = NULL
    z[rng.random((D, S)) < 0.02] = np.nan
    z[rng.random((D, S)) < 0.01] = np.inf
    x += 0.3 * np.where(np.isfinite(z), z - 23.0, 0.0)[None] + 0.05 * g[None]
    return x, st, g, z, zst


def _run(dev, x, st, g=None, G=None, z=None, zst=None, winsor=3.0, standardize=True, **kw):
    from mff import engine
    ov, os_ = engine.neutralize(_t(x, dev), _t(st, dev), None if g is None else _t(g, dev),
                                None if z is None else _t(z, dev), None if z is None else _t(zst, dev),
                                G=G, winsor=winsor, standardize=standardize, **kw)
    torch.cuda.synchronize()
    return ov.cpu().numpy(), os_.cpu().numpy()


def _check(got, want, name):
    gv, gs = got
    wv, ws = want
    m = (gs == VALUE) & (ws == VALUE) & np.isfinite(gv) & np.isfinite(wv)
    worst = float(np.abs(gv[m] - wv[m]).max()) if m.any() else 0.0
    print(f"{name}: {int(m.sum())} values, {int((ws == NULL).sum())} nulls, worst abs err {worst:.3e}")
    bad = compare(gv, gs, wv, ws, name, **TOL)
    assert not bad, "\n".join(bad)


@pytest.mark.gpu
@pytest.mark.parametrize("S", [1, 2, 3, 63, 64, 65, 255, 256, 257, 1000, 8192])
def test_boundary_sizes(dev, S):
    """Lane, wave, workgroup and register-tile boundaries of the 256-thread kernel."""
    G = 7 if S >= 63 else 1  # (S <= 3: one industry, or nearly every stock would be alone in its own)
    x, st, g, z, zst = _panel(1000 + S, 3, 4, S, G)
    _check(_run(dev, x, st, g, G, z, zst), ref.neutralize(x, st, g, G, z, zst), f"S={S}")


@pytest.mark.gpu
def test_too_many_stocks_is_an_error_and_writes_nothing(dev):
    from mff import _lib, engine
    lib = _lib.load()
    S = lib.mff_xs_neutralize_max_stocks() + 1
    x = torch.zeros((1, 1, S), dtype=torch.float64, device=dev)
    st = torch.full((1, 1, S), VALUE, dtype=torch.uint8, device=dev)
    with pytest.raises(_lib.MffError, match=f"S={S}"):
        engine.neutralize(x, st)
    ov = torch.full_like(x, 7.0)
    os_ = torch.full_like(st, 9)
    rc = lib.mff_xs_neutralize(x.data_ptr(), st.data_ptr(), 1, 1, S, None, 0, None, None, 3.0, 1,
                               ov.data_ptr(), os_.data_ptr(), None, None)
    torch.cuda.synchronize()
    assert rc < 0
    assert bool((ov == 7.0).all()) and bool((os_ == 9).all())


def _embed(rng, cols, S):
    """Each column's values at random places of an S-stock segment, ABSENT elsewhere."""
    x = np.zeros((len(cols), 1, S))
    st = np.full((len(cols), 1, S), ABSENT, np.uint8)
    for r, c in enumerate(cols):
        p = rng.permutation(S)[:len(c)]
        x[r, 0, p] = c
        st[r, 0, p] = VALUE
    return x, st


@pytest.mark.gpu
@pytest.mark.parametrize("standardize", [False, True])
def test_median_and_mad_cases(dev, standardize):
    rng = np.random.default_rng(7)
    B = (3.0 * 1.4826) * 2.0
    tied = np.sort(rng.standard_t(3, 200))
    tied[95:105] = tied[99]                      # the two middle values equal (and their neighbours)
    cols = [
        rng.standard_t(3, 200),                  # even n
        rng.standard_t(3, 201),                  # odd n
        tied,
        np.r_[np.full(120, 1.25), rng.standard_t(3, 80) * 10],   # more than half tied: mad == 0, no clipping
        np.array([-50.0, -B, -2, -1, 0, 1, 2, B, 50.0]),          # med 0, mad 2: -B and B sit on the bounds
        np.array([1.0, 2.0, 3.0, 4.0, 5.0, 100.0]),               # even n by hand: med 3.5, mad 1.5
        np.r_[rng.standard_t(3, 150), -rng.standard_t(3, 151) * 1e-300, 1e300],  # tiny and huge magnitudes
        np.array([4.0, -9.0]),                   # n = 2
        np.array([4.0, -9.0, 1e6]),              # n = 3
    ]
    assert np.median(np.abs(cols[3] - np.median(cols[3]))) == 0
    x, st = _embed(rng, cols, 320)
    got = _run(dev, x, st, winsor=3.0, standardize=standardize)
    _check(got, ref.neutralize(x, st, winsor_k=3.0, standardize=standardize), f"median/mad std={standardize}")
    if not standardize:  # the hand-made columns, against the numbers worked out by hand
        v = np.sort(got[0][4, 0][st[4, 0] == VALUE])
        np.testing.assert_allclose(v, [-B, -B, -2, -1, 0, 1, 2, B, B], rtol=0, atol=1e-12)
        v = np.sort(got[0][5, 0][st[5, 0] == VALUE])
        w = np.array([1, 2, 3, 4, 5, 3.5 + 3 * 1.4826 * 1.5])
        np.testing.assert_allclose(v, w - w.mean(), rtol=0, atol=1e-12)


@pytest.mark.gpu
@pytest.mark.parametrize("with_size", [False, True])
@pytest.mark.parametrize("G", [1, 31, 256])
def test_industries(dev, G, with_size):
    """Empty and single-member industries (G = 256 over 1,000 stocks), a day on which every
    usable stock is alone in its industry (all NULL), days with n - k == 1."""
    rows, D, S = 3, 4, 1000
    x, st, g, z, zst = _panel(2000 + G, rows, D, S, G)
    m = min(G, 200)
    rng = np.random.default_rng(G)
    for d in range(3):  # day d: m stocks alone in their industries + d more in industry 0
        p = rng.permutation(S)[:m + d]
        st[:, d] = NULL
        st[:, d, ::7] = ABSENT
        st[:, d, p] = VALUE
        x[:, d, p] = rng.standard_t(3, (rows, m + d))
        g[d, p[:m]] = np.arange(m)
        g[d, p[m:]] = 0
        zst[d, p] = VALUE
        z[d, p] = rng.normal(23.0, 1.5, m + d)
    args = (g, G, z, zst) if with_size else (g, G)
    want = ref.neutralize(x, st, *args)
    # day 0: n - k <= 0; day 1: n - k = 1 without the covariate, 0 with it; day 2: 2 and 1
    assert not (want[1][:, 0] == VALUE).any()
    assert (want[1][:, 1] == VALUE).any() != with_size
    assert (want[1][:, 2] == VALUE).any()
    if G == 256:
        cnt = np.bincount(g[3][g[3] >= 0], minlength=G)
        assert (cnt == 0).any() and (cnt == 1).any()
    _check(_run(dev, x, st, *args), want, f"G={G} size={with_size}")


@pytest.mark.gpu
def test_option_grid(dev):
    from mff import engine
    G = 7
    x, st, g, z, zst = _panel(31, 3, 4, 257, G)
    for winsor in (0.0, 3.0):
        for standardize in (False, True):
            for gg in (None, g):
                for zz in (None, z):
                    got = _run(dev, x, st, gg, G if gg is not None else None, zz, zst, winsor, standardize)
                    want = ref.neutralize(x, st, gg, G, zz, zst if zz is not None else None, winsor, standardize)
                    _check(got, want, f"winsor={winsor} std={standardize} industry={gg is not None} "
                                      f"size={zz is not None}")
    # no industry, no size, no winsorisation, standardise == the stage-3 z-score
    xf = np.random.default_rng(5).standard_t(3, (3, 4, 257))
    sf = np.full(xf.shape, VALUE, np.uint8)
    zv, zs_ = engine.cross_section(_t(xf, dev), _t(sf, dev), "z")
    torch.cuda.synchronize()
    _check(_run(dev, xf, sf, winsor=0.0, standardize=True), (zv.cpu().numpy(), zs_.cpu().numpy()), "== xs z")


@pytest.mark.gpu
def test_deterministic_and_right_at_5000_stocks(dev):
    from mff import engine
    G = 31
    x, st, g, z, zst = _panel(77, 4, 3, 5000, G)
    a = [_t(v, dev) for v in (x, st, g, z, zst)]
    o1 = engine.neutralize(*a, G=G)
    o2 = engine.neutralize(*a, G=G)
    torch.cuda.synchronize()
    assert torch.equal(o1[0].view(torch.int64), o2[0].view(torch.int64))  # bit patterns: NaN == NaN
    assert torch.equal(o1[1], o2[1])
    _check((o1[0].cpu().numpy(), o1[1].cpu().numpy()), ref.neutralize(x, st, g, G, z, zst), "S=5000")


@pytest.mark.gpu
@pytest.mark.parametrize("R", [2, 3])
def test_stock_shards_match_one_rank(dev, R):
    from mff import dist
    G, S = 5, 61
    x, st, g, z, zst = _panel(400 + R, 3, 4, S, G)
    s0, s1 = dist.shard_bounds(S, R, 0)
    st[:, 1, s0:s1] = ABSENT  # rank 0 holds no usable stock on day 1
    one = _run(dev, x, st, g, G, z, zst)
    _check(one, ref.neutralize(x, st, g, G, z, zst), "one rank")

    def rank_fn(comm):
        a, b = dist.shard_bounds(S, R, comm.rank)
        return _run(dev, x[:, :, a:b], st[:, :, a:b], g[:, a:b], G, z[:, a:b], zst[:, a:b], comm=comm,
                    stocks_total=S)

    for r, got in enumerate(dist.run_threads(R, rank_fn)):
        a, b = dist.shard_bounds(S, R, r)
        _check(got, (one[0][:, :, a:b], one[1][:, :, a:b]), f"rank {r} of {R}")


@pytest.mark.gpu
def test_shards_wider_than_the_kernel_raise(dev):
    from mff import _lib, dist, engine

    def rank_fn(comm):
        x = torch.zeros((1, 1, 4100), dtype=torch.float64, device=dev)
        st = torch.full((1, 1, 4100), VALUE, dtype=torch.uint8, device=dev)
        with pytest.raises(_lib.MffError, match="8200"):
            engine.neutralize(x, st, comm=comm, stocks_total=8200)
        return True

    assert dist.run_threads(2, rank_fn) == [True, True]


@pytest.mark.gpu
def test_factor_neutralize_surface(dev):
    import pandas as pd

    from mff import frames
    from mff.factor import Factor
    rng = np.random.default_rng(9)
    D, S = 10, 24
    codes = [f"{i:06d}.SZ" for i in range(S)]
    dates = [dt.date(2024, 3, 1) + dt.timedelta(days=i) for i in range(D)]
    x = rng.standard_t(3, (D, S))
    xs = np.full((D, S), VALUE, np.uint8)
    xs[2:4, 5] = ABSENT
    xs[6, 7] = NULL
    x[4, 3] = np.nan
    pct = rng.normal(0, 0.02, (D, S))
    ps = np.full((D, S), VALUE, np.uint8)
    cap = np.exp(rng.normal(23.0, 1.5, (D, S)))
    cst = ps.copy()
    cst[1, 2] = NULL          # a null cap
    cap[3, 4] = 0.0           # a zero cap
    cap[5, 6] = -2.0e9        # a negative cap
    labels = np.array(["bank", "steel", "tech", "food"], dtype=object)
    gid = rng.integers(0, 4, (D, S))
    ind = pd.DataFrame({"code": np.tile(np.asarray(codes, dtype=object), D),
                        "date": np.repeat(np.asarray(dates, dtype=object), S),
                        "industry": labels[gid.reshape(-1)]})
    gid = gid.astype(np.int32)
    ind = ind.drop(index=[0 * S + 9]).reset_index(drop=True)   # code 9 has no industry on day 0
    gid[0, 9] = -1
    ind.loc[(ind["code"] == codes[11]) & (ind["date"] == dates[2]), "industry"] = None  # a null label
    gid[2, 11] = -1
    ex = frames.to_long(x, xs, codes, dates, "f")
    pv = frames.to_long(pct, ps, codes, dates, "pct_change")
    pv["cmc"] = frames.to_long(cap, cst, codes, dates, "cmc")["cmc"]
    before = ex.copy(deep=True)
    f = Factor("f", ex)
    out = f.neutralize(industry=ind, size="cmc", pv_data=pv, device=dev)
    assert type(out) is Factor and out.factor_name == "f_neu" and out is not f
    pd.testing.assert_frame_equal(f.factor_exposure, before)
    zok = (cst == VALUE) & np.isfinite(cap) & (cap > 0)
    z = np.where(zok, np.log(np.where(zok, cap, 1.0)), 0.0)
    zst = np.where(zok, VALUE, NULL).astype(np.uint8)
    wv, ws = ref.neutralize(x[None], xs[None], gid, 4, z, zst)
    want = frames.to_long(wv[0], ws[0], codes, dates, "f_neu")
    got = out.factor_exposure
    assert list(got.columns) == ["code", "date", "f_neu"]
    assert got["code"].tolist() == want["code"].tolist() and got["date"].tolist() == want["date"].tolist()
    gnull, wnull = got["f_neu"].isna().to_numpy(), want["f_neu"].isna().to_numpy()
    assert np.array_equal(gnull, wnull) and wnull.sum() >= 6
    a = got["f_neu"].to_numpy(dtype=np.float64, na_value=0.0)
    b = want["f_neu"].to_numpy(dtype=np.float64, na_value=0.0)
    print(f"surface: worst abs err {np.nanmax(np.abs(a - b)):.3e}")
    np.testing.assert_allclose(a, b, rtol=1e-9, atol=1e-9, equal_nan=True)
    ic = out.ic_test(future_days=2, plot_out=False, return_df=True, pv_data=pv, device=dev)
    assert len(ic) >= 2 and np.isfinite(out.IC) and np.isfinite(out.rank_IC)
    # a static [code, industry] frame, no covariate
    static = pd.DataFrame({"code": codes, "industry": [i % 3 for i in range(S)]})
    out2 = f.neutralize(industry=static, size=None, winsor=0, standardize=False, device=dev)
    g2 = np.tile((np.arange(S) % 3).astype(np.int32), (D, 1))
    wv, ws = ref.neutralize(x[None], xs[None], g2, 3, winsor_k=0.0, standardize=False)
    want2 = frames.to_long(wv[0], ws[0], codes, dates, "f_neu")
    np.testing.assert_allclose(out2.factor_exposure["f_neu"].to_numpy(dtype=np.float64, na_value=0.0),
                               want2["f_neu"].to_numpy(dtype=np.float64, na_value=0.0), rtol=1e-9, atol=1e-9,
                               equal_nan=True)
