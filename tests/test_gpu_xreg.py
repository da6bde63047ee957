"""mff_xs_reg_* on the GPU (per-day multi-factor cross-sectional regression, f64 MFMA Gram +
Cholesky) against its numpy restatement tests/xs_reg_ref.py: n, dof, status and the NaN
pattern exact, finite values within rtol = atol = 1e-9 (the tolerance of
tests/test_gpu_xcorr.py and tests/test_gpu_neutralize.py).  The panels are built with mutual
correlations <= 0.7, so the unit-diagonal Gram's condition number stays below 1e3 (asserted
from the restatement) and 1e-9 is seven decades above cond * 2^-53.  Every comparison prints
its worst error; the worst over all cases is quoted in DESIGN.md §11."""
import datetime as dt

import numpy as np
import pytest

import xs_reg_ref as ref
from xs_reg_ref import ABSENT, NULL, VALUE

torch = pytest.importorskip("torch")

TOL = dict(rtol=1e-9, atol=1e-9)
COND_MAX = 1e3


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def _t(a, dev):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _panel(seed, K, D, S, G=None, weights=True):
    """K exposure rows = 0.5 common + 0.87 own noise (pairwise correlation 0.25), y = a linear
    combination + industry effect + noise, weights = sqrt of a lognormal cap.  From 16 stocks
    on every day holds, spread over DIFFERENT rows (x rows, y, the weight): an ABSENT run,
    NULLs, NaN, +inf, -inf (each drops its stock from the listwise set only through that one
    row) and -0.0 / +0.0 values; a zero, a negative and a NaN weight; stocks without industry.
    With G >= 3: industry 1 is empty and industry 2 has a single member per day."""
    rng = np.random.default_rng(seed)
    common = rng.standard_normal((D, S))
    x = 0.5 * common[None] + np.sqrt(0.75) * rng.standard_normal((K, D, S))
    xs = np.full((K, D, S), VALUE, np.uint8)
    grp = None
    eff = 0.0
    if G is not None:
        grp = rng.integers(0, G, (D, S)).astype(np.int32)
        if G >= 3:
            grp[grp == 1] = 0
            grp[grp == 2] = G - 1 if G > 3 else 0
            for d in range(D):
                grp[d, int(rng.integers(0, S))] = 2
        eff = 0.3 * rng.standard_normal(G)[grp]
    coef = rng.standard_normal(K) / np.sqrt(K)
    y = np.tensordot(coef, x, axes=1) + eff + 0.5 * rng.standard_normal((D, S))
    ys = np.full((D, S), VALUE, np.uint8)
    w = ws = None
    if weights:
        w = np.sqrt(np.exp(rng.normal(3.0, 1.0, (D, S))))
        ws = np.full((D, S), VALUE, np.uint8)
    if S >= 16:
        for d in range(D):
            hit = rng.permutation(S)[:max(8, S // 10)]
            kinds = ("absent", "null", np.nan, np.inf, -np.inf, -0.0, 0.0)
            for i, s in enumerate(hit):
                r = int(rng.integers(0, K + 1 + (1 if weights else 0)))
                kind = kinds[i % len(kinds)]
                val_, st_ = (x[r], xs[r]) if r < K else ((y, ys) if r == K else (w, ws))
                if kind == "absent":
                    st_[d, s:s + max(1, S // (20 * (K + 1)))] = ABSENT
                elif kind == "null":
                    st_[d, s] = NULL
                else:
                    val_[d, s] = kind
            if weights:
                for s, v in zip(rng.permutation(S)[:3], (0.0, -1.5, np.nan)):
                    w[d, s] = v
            if grp is not None:
                grp[d, rng.permutation(S)[:2]] = (-1, G + 5)
    return dict(x=x, xs=xs, y=y, ys=ys, w=w, ws=ws, group=grp, G=G)


def _run(dev, p, min_obs=0, residual=True, **kw):
    from mff import engine
    r = engine.factor_regress(_t(p["x"], dev), _t(p["xs"], dev), _t(p["y"], dev), _t(p["ys"], dev), _t(p["w"], dev),
                              _t(p["ws"], dev), _t(p["group"], dev), G=p["G"], min_obs=min_obs, residual=residual,
                              **kw)
    torch.cuda.synchronize()
    out = dict(beta=r.beta.cpu().numpy(), t=r.tstat.cpu().numpy(), r2=r.r2.cpu().numpy(), n=r.n.cpu().numpy(),
               dof=r.dof.cpu().numpy(), status=r.status.cpu().numpy())
    if residual:
        out["resid_val"], out["resid_state"] = r.resid_val.cpu().numpy(), r.resid_state.cpu().numpy()
    return out


def _want(p, min_obs=0):
    return ref.regress(p["x"], p["xs"], p["y"], p["ys"], p["w"], p["ws"], p["group"], p["G"], min_obs=min_obs)


def _check(got, want, name, cond=True):
    for k in ("n", "dof", "status"):
        assert got[k].dtype == np.int32 and np.array_equal(got[k], want[k]), \
            f"{name}: {k} differs: {got[k].tolist()[:8]} vs {want[k].tolist()[:8]}"
    if cond and (want["status"] == 0).any():
        c = np.nanmax(want["cond"])
        assert c < COND_MAX, f"{name}: panel too ill-conditioned for the tolerance (cond {c:.3g})"
    worst = 0.0
    for k in ("beta", "t", "r2") + (("resid_val",) if "resid_val" in got else ()):
        g, w = got[k], want[k]
        assert g.shape == w.shape, f"{name}: {k} shape"
        bad = np.argwhere(np.isnan(g) != np.isnan(w))
        assert not len(bad), f"{name}: NaN pattern of {k} differs at {bad[:5].tolist()}"
        m = np.isfinite(w)
        if m.any():
            worst = max(worst, float((np.abs(g[m] - w[m]) / (1.0 + np.abs(w[m]))).max()))
    print(f"{name}: status {np.bincount(want['status'], minlength=3).tolist()}, worst err / (1 + |ref|) {worst:.3e}")
    for k in ("beta", "t", "r2") + (("resid_val",) if "resid_val" in got else ()):
        np.testing.assert_allclose(got[k], want[k], equal_nan=True, err_msg=f"{name}: {k}", **TOL)
    if "resid_state" in got:
        assert np.array_equal(got["resid_state"], want["resid_state"]), f"{name}: residual states"


@pytest.mark.gpu
@pytest.mark.parametrize("K", [1, 2, 15, 16, 17, 58, 63])
def test_factor_boundaries(dev, K):
    """The 16-row MFMA padding (C = K + 1 = 16, 17) and the full 64-row block (K = 63)."""
    p = _panel(100 + K, K, 2, 257, G=3)
    want = _want(p)
    assert (want["status"] == 0).all()
    _check(_run(dev, p), want, f"K={K}")


@pytest.mark.gpu
@pytest.mark.parametrize("S", [7, 63, 64, 65, 127, 128, 129, 257, 1023, 1025, 5003])
def test_stock_boundaries(dev, S):
    """K = 5: S = K + 2 (dof = 1), the MFMA k = 4 step, the 32-stock tile, and the sizes at
    which the two-day call splits the stocks into runs (S > 256)."""
    from mff import engine
    p = _panel(200 + S, 5, 2, S)
    want = _want(p)
    assert (want["status"] == 0).all()
    assert (engine.reg_splits(2, S) > 1) == (S > 256)
    _check(_run(dev, p), want, f"S={S}")


@pytest.mark.gpu
@pytest.mark.parametrize("G", [None, 1, 3, 31, 256])
def test_group_boundaries(dev, G):
    """No industries, one, a few (one empty, one with a single member), 31 and the 256 limit."""
    p = _panel(300 + (G or 0), 4, 2, 1201, G=G)
    want = _want(p)
    assert (want["status"] == 0).all()
    if G and G >= 3:
        u = ref.usable(p["x"], p["xs"], p["y"], p["ys"], p["w"], p["ws"], p["group"], G)
        cnt = np.bincount(p["group"][0][u[0]], minlength=G)
        assert cnt[1] == 0 and cnt[2] <= 1
    _check(_run(dev, p), want, f"G={G}")


def _degenerate_panel():
    K, D, S, G = 4, 10, 120, 3
    p = _panel(7, K, D, S, G=G)
    x, xs, y, ys, grp = p["x"], p["xs"], p["y"], p["ys"], p["group"]
    x[2, 1], xs[2, 1] = x[1, 1], xs[1, 1]                     # day 1: a duplicated column
    with np.errstate(invalid="ignore"):
        x[3, 2] = x[0, 2] + x[1, 2]                           # day 2: a sum of two others
    x[2, 3] = np.where(grp[3] >= 0, 1.5 * grp[3] + 0.25, 0.0)  # day 3: constant within industries
    u = ref.usable(x, xs, y, ys, p["w"], p["ws"], grp, G)
    for d, keep in ((4, K + 3), (5, K + 4)):                  # days 4 / 5: dof = 0 / 1 (3 industries)
        grp[d] = np.arange(S) % 3
        idx = np.nonzero(u[d] & (grp[d] >= 0))[0]
        ys[d] = ABSENT
        ys[d, idx[:keep]] = VALUE
    ys[6] = NULL                                              # day 6: an empty U
    y[7] = 0.5                                                # day 7: a constant y
    ys[8, 60:] = ABSENT                                       # day 8: about half the stocks (min_obs)
    return p


@pytest.mark.gpu
def test_degenerate_days(dev):
    """One degenerate day each; the other days of the same call are unaffected."""
    p = _degenerate_panel()
    want = _want(p)
    assert want["status"].tolist() == [0, 2, 2, 2, 1, 0, 1, 0, 0, 0]
    assert want["dof"][4] == 0 and want["dof"][5] == 1 and want["n"][6] == 0
    assert want["min_pivot"][1] < 1e-12 and want["min_pivot"][2] < 1e-12      # exactly dependent
    ok = [0, 5, 8, 9]
    assert (want["min_pivot"][ok] > 1e-3).all(), want["min_pivot"]             # nothing near the threshold
    got = _run(dev, p)
    _check(got, want, "degenerate", cond=False)
    assert (got["beta"][7] == 0.0).all() and np.isnan(got["t"][7]).all()
    clean = _panel(7, 4, 10, 120, G=3)
    base = _run(dev, clean)
    for d in (0, 9):                                          # untouched days: the same bits
        assert np.array_equal(got["beta"][d].view(np.int64), base["beta"][d].view(np.int64))
    n8 = int(want["n"][8])
    assert n8 < want["n"][[0, 9]].min()
    at, above = _run(dev, p, min_obs=n8), _run(dev, p, min_obs=n8 + 1)
    _check(at, _want(p, min_obs=n8), "min_obs at n", cond=False)
    _check(above, _want(p, min_obs=n8 + 1), "min_obs above n", cond=False)
    assert at["status"][8] == 0 and above["status"][8] == 1 and above["status"][0] == 0 and above["status"][5] == 1


@pytest.mark.gpu
def test_equivariance(dev):
    """Row j -> a x_j + b sd_j gives beta_j / a, t_j sign(a), the same r2 and other rows;
    y -> c y scales beta by c."""
    p = _panel(31, 6, 2, 1201, G=31)
    base = _run(dev, p)
    _check(base, _want(p), "base")
    q = dict(p, x=p["x"].copy())
    scale, sign = np.ones(6), np.ones(6)
    for r, (a, b) in zip((0, 1, 4, 5), ((1e-8, 0.0), (1e8, 0.0), (1.0, 1e6), (-3.0, -1e6))):
        sd = np.std(p["x"][r][np.isfinite(p["x"][r])])
        with np.errstate(invalid="ignore"):
            q["x"][r] = a * p["x"][r] + b * sd
        scale[r], sign[r] = a, np.sign(a)
    got = _run(dev, q)
    for k in ("n", "dof", "status"):
        assert np.array_equal(got[k], base[k])
    worst = max(np.abs(got["beta"] * scale - base["beta"]).max(), np.abs(got["t"] * sign - base["t"]).max(),
                np.abs(got["r2"] - base["r2"]).max())
    print(f"equivariance: worst abs err {worst:.3e}")
    np.testing.assert_allclose(got["beta"] * scale, base["beta"], **TOL)
    np.testing.assert_allclose(got["t"] * sign, base["t"], **TOL)
    np.testing.assert_allclose(got["r2"], base["r2"], **TOL)
    with np.errstate(invalid="ignore"):
        got = _run(dev, dict(p, y=-2.5 * p["y"]))
    np.testing.assert_allclose(got["beta"], -2.5 * base["beta"], **TOL)
    np.testing.assert_allclose(got["t"], -base["t"], **TOL)
    np.testing.assert_allclose(got["r2"], base["r2"], **TOL)


@pytest.mark.gpu
def test_residual_properties(dev):
    """On status-0 days sum_U w x~_j e and every per-industry sum w e are 0 within 1e-9 of
    sum w |x~_j| |e|; the states are as defined."""
    G = 5
    p = _panel(41, 7, 3, 900, G=G)
    p["ys"][2] = NULL                                          # a day without a result
    got = _run(dev, p)
    _check(got, _want(p), "residual")
    u = ref.usable(p["x"], p["xs"], p["y"], p["ys"], p["w"], p["ws"], p["group"], G)
    rv, rs = got["resid_val"], got["resid_state"]
    assert got["status"].tolist() == [0, 0, 1]
    assert (rs[2] == NULL).all() and np.array_equal(rs[:2] == VALUE, u[:2])
    keep = p["ys"][:2] != VALUE
    assert np.array_equal(rs[:2][keep], p["ys"][:2][keep]) and (rs[:2][~keep & ~u[:2]] == NULL).all()
    worst = 0.0
    for d in range(2):
        m = u[d]
        w, e, g = p["w"][d][m], rv[d][m], p["group"][d][m]
        for gi in np.unique(g):
            s = g == gi
            worst = max(worst, abs((w[s] * e[s]).sum()) / max((w[s] * np.abs(e[s])).sum(), 1e-300))
        for j in range(7):
            xt = ref._demean(p["x"][j, d][m], w, g)
            worst = max(worst, abs((w * xt * e).sum()) / (w * np.abs(xt) * np.abs(e)).sum())
    print(f"residual orthogonality: worst relative {worst:.3e}")
    assert worst <= 1e-9


@pytest.mark.gpu
def test_bit_identical_runs(dev):
    from mff import engine
    p = _panel(51, 58, 3, 5003, G=31)
    a = [_t(p[k], dev) for k in ("x", "xs", "y", "ys", "w", "ws", "group")]
    r1 = engine.factor_regress(*a, G=31, residual=True)
    r2 = engine.factor_regress(*a, G=31, residual=True)
    torch.cuda.synchronize()
    for u, v in zip(r1, r2):
        assert torch.equal(u.view(torch.int64) if u.dtype == torch.float64 else u,
                           v.view(torch.int64) if v.dtype == torch.float64 else v)
    assert bool((r1.status == 0).all())
    m1, o1 = engine.factor_regress_mean(r1)
    m2, o2 = engine.factor_regress_mean(r2)
    torch.cuda.synchronize()
    assert torch.equal(m1.view(torch.int64), m2.view(torch.int64)) and torch.equal(o1.view(torch.int64), o2.view(torch.int64))


@pytest.mark.gpu
def test_time_aggregate(dev):
    from mff import engine
    p = _degenerate_panel()
    want = _want(p)
    wa, wo = ref.aggregate(want)
    r = engine.factor_regress(*[_t(p[k], dev) for k in ("x", "xs", "y", "ys", "w", "ws", "group")], G=3)
    agg, overall = engine.factor_regress_mean(r)
    torch.cuda.synchronize()
    agg, overall = agg.cpu().numpy(), overall.cpu().numpy()
    assert tuple(engine.REG_AGG_COLUMNS) == tuple(ref.AGG_COLUMNS)
    assert np.array_equal(agg[:, 0], wa[:, 0]) and wa[0, 0] == 5
    print(f"aggregate: worst abs err {np.nanmax(np.abs(agg - wa)):.3e}, overall {np.abs(overall - wo).max():.3e}")
    assert np.array_equal(np.isnan(agg), np.isnan(wa))
    np.testing.assert_allclose(agg, wa, equal_nan=True, **TOL)
    np.testing.assert_allclose(overall, wo, equal_nan=True, **TOL)
    # no status-0 day at all, and a single one
    none = engine.factor_regress_mean(engine.RegressResult(r.beta[4:5], r.tstat[4:5], r.r2[4:5], r.n[4:5], r.dof[4:5],
                                                           r.status[4:5]))
    one = engine.factor_regress_mean(engine.RegressResult(r.beta[:1], r.tstat[:1], r.r2[:1], r.n[:1], r.dof[:1],
                                                          r.status[:1]))
    torch.cuda.synchronize()
    a0, a1 = none[0].cpu().numpy(), one[0].cpu().numpy()
    assert (a0[:, 0] == 0).all() and np.isnan(a0[:, 1:]).all() and np.isnan(none[1].cpu().numpy()).all()
    assert (a1[:, 0] == 1).all() and np.isnan(a1[:, 2:4]).all()
    np.testing.assert_allclose(a1[:, 1], want["beta"][0], **TOL)


@pytest.mark.gpu
@pytest.mark.parametrize("S", [29, 257])
@pytest.mark.parametrize("R", [2, 3])
def test_stock_shards_match_one_rank(dev, R, S):
    from mff import dist
    G = 3
    p = _panel(400 + R + S, 3, 3, S, G=G)
    bounds = [dist.shard_bounds(S, R, r) for r in range(R)]
    assert len({b - a for a, b in bounds}) == 2               # uneven shards
    s0, s1 = bounds[0]
    grp = p["group"]
    grp[grp == 2] = 0
    grp[:, s0:s0 + 6] = 2                                      # industry 2 wholly on rank 0
    one = _run(dev, p)
    _check(one, _want(p), "one rank", cond=False)
    assert (one["status"] == 0).all()

    def rank_fn(comm):
        a, b = bounds[comm.rank]
        q = {k: (v[..., a:b] if isinstance(v, np.ndarray) else v) for k, v in p.items()}
        return _run(dev, q, comm=comm, stocks_total=S)

    for r, got in enumerate(dist.run_threads(R, rank_fn)):
        a, b = bounds[r]
        want = dict(one, resid_val=one["resid_val"][:, a:b], resid_state=one["resid_state"][:, a:b])
        _check(got, want, f"rank {r} of {R}, S={S}", cond=False)


@pytest.mark.gpu
def test_split_matches_unsplit(dev):
    p = _panel(61, 9, 3, 1500, G=5)
    one = _run(dev, p, split=1)
    _check(one, _want(p), "unsplit")
    for ns in (2, 7, 47, 64):                                  # 47 = one tile per run, 64: empty runs too
        got = _run(dev, p, split=ns)
        _check(got, one, f"split={ns}", cond=False)
    p = _panel(62, 3, 2, 700, G=100)                           # above 64 industries: the wave-per-columns group pass
    one = _run(dev, p, split=1)
    _check(one, _want(p), "unsplit, G=100")
    _check(_run(dev, p, split=5), one, "split=5, G=100", cond=False)


def _sentinels(dev):
    buf = torch.full((8192,), 7.0, dtype=torch.float64, device=dev)
    ib = torch.full((4096,), 9, dtype=torch.int32, device=dev)
    return buf, ib


@pytest.mark.gpu
def test_errors_write_nothing(dev):
    from mff import _lib, engine
    lib = _lib.load()
    assert lib.mff_xs_reg_max_factors() == 63 and lib.mff_xs_reg_max_groups() == 256
    buf, ib = _sentinels(dev)
    K, D, S = 2, 1, 8
    xv = torch.zeros((K, D, S), dtype=torch.float64, device=dev)
    xs = torch.full((K, D, S), VALUE, dtype=torch.uint8, device=dev)
    yv = torch.zeros((D, S), dtype=torch.float64, device=dev)
    ys = torch.full((D, S), VALUE, dtype=torch.uint8, device=dev)
    gp = torch.zeros((D, S), dtype=torch.int32, device=dev)
    ws = torch.full((1 << 16,), 3, dtype=torch.uint8, device=dev)
    p, q, w = buf.data_ptr(), ib.data_ptr(), ws.data_ptr()
    X, XS, Y, YS, GP = xv.data_ptr(), xs.data_ptr(), yv.data_ptr(), ys.data_ptr(), gp.data_ptr()

    def groups(K=K, D=D, S=S, wv=None, wst=None, g=None, G=0, ns=1):
        return lib.mff_xs_reg_groups(X, XS, K, D, S, Y, YS, wv, wst, g, G, ns, p, w, None)

    for kw in (dict(K=0), dict(K=64), dict(D=-1), dict(S=-1), dict(g=GP, G=0), dict(g=GP, G=257), dict(ns=0),
               dict(wv=Y), dict(wst=YS)):
        assert groups(**kw) < 0, kw
        assert lib.mff_last_error()
    assert b"weight" in lib.mff_last_error()
    for K_, G_ in ((0, 0), (64, 0), (2, 257), (2, -1)):
        assert lib.mff_xs_reg_gram(X, K_, D, S, Y, None, G_, p, 1, 1, p, w, None) < 0
        assert lib.mff_xs_reg_residual(X, K_, D, S, Y, YS, G_, p, q, p, YS, w, None) < 0
    assert lib.mff_xs_reg_gram(X, K, D, S, Y, None, 0, p, 0, 1, p, w, None) < 0      # R = 0
    assert lib.mff_xs_reg_gram(X, K, D, S, Y, None, 0, p, 1, 0, p, w, None) < 0      # nsplit = 0
    assert lib.mff_xs_reg_gram(X, K, -1, S, Y, None, 0, p, 1, 1, p, w, None) < 0
    for K_, D_, mo in ((0, 1, 0), (64, 1, 0), (2, -1, 0), (2, 1, -1)):
        assert lib.mff_xs_reg_solve(p, 1, K_, D_, mo, p, p, p, q, q, q, w, None) < 0
    assert b"min_obs" in lib.mff_last_error()
    assert lib.mff_xs_reg_solve(p, 0, 2, 1, 0, p, p, p, q, q, q, w, None) < 0
    assert lib.mff_xs_reg_mean(p, p, p, q, q, 0, 1, p, p, None) < 0
    assert lib.mff_xs_reg_mean(p, p, p, q, q, 64, 1, p, p, None) < 0
    assert lib.mff_xs_reg_mean(p, p, p, q, q, 2, -1, p, p, None) < 0
    torch.cuda.synchronize()
    assert bool((buf == 7.0).all()) and bool((ib == 9).all()) and bool((ws == 3).all())
    assert bool((ys == VALUE).all())
    with pytest.raises(ValueError):
        engine.factor_regress(xv, xs, yv, ys, min_obs=-1)
    with pytest.raises(ValueError):
        engine.factor_regress(xv, xs, yv, ys, weight=yv)
    with pytest.raises(_lib.MffError):
        engine.factor_regress(xv, xs, yv, ys, group=gp, G=257)
    with pytest.raises(_lib.MffError):
        engine.factor_regress(torch.zeros((64, 1, 8), dtype=torch.float64, device=dev),
                              torch.zeros((64, 1, 8), dtype=torch.uint8, device=dev), yv, ys)


@pytest.mark.gpu
def test_empty_day_and_stock_axes(dev):
    from mff import _lib, engine
    lib = _lib.load()
    z = lambda shape, dtype: torch.zeros(shape, dtype=dtype, device=dev)
    r = engine.factor_regress(z((3, 0, 5), torch.float64), z((3, 0, 5), torch.uint8), z((0, 5), torch.float64),
                              z((0, 5), torch.uint8), residual=True)
    assert tuple(r.beta.shape) == (0, 3) and tuple(r.n.shape) == (0,) and tuple(r.resid_val.shape) == (0, 5)
    agg, overall = engine.factor_regress_mean(r)
    torch.cuda.synchronize()
    assert bool((agg[:, 0] == 0).all()) and bool(torch.isnan(agg[:, 1:]).all()) and bool(torch.isnan(overall).all())
    r = engine.factor_regress(z((3, 2, 0), torch.float64), z((3, 2, 0), torch.uint8), z((2, 0), torch.float64),
                              z((2, 0), torch.uint8), residual=True)
    torch.cuda.synchronize()
    assert bool(torch.isnan(r.beta).all()) and bool(torch.isnan(r.tstat).all()) and bool(torch.isnan(r.r2).all())
    assert r.n.tolist() == [0, 0] and r.status.tolist() == [1, 1] and r.dof.tolist() == [-4, -4]
    # the C entry points themselves: 0 for D == 0, nothing written
    buf, ib = _sentinels(dev)
    p, q = buf.data_ptr(), ib.data_ptr()
    assert lib.mff_xs_reg_groups(None, None, 2, 0, 5, None, None, None, None, None, 0, 1, p, p, None) == 0
    assert lib.mff_xs_reg_gram(None, 2, 0, 5, None, None, 0, p, 1, 1, p, p, None) == 0
    assert lib.mff_xs_reg_solve(p, 1, 2, 0, 0, p, p, p, q, q, q, p, None) == 0
    assert lib.mff_xs_reg_residual(None, 2, 0, 5, None, None, 0, p, q, p, p, p, None) == 0
    assert lib.mff_xs_reg_residual(None, 2, 3, 0, None, None, 0, p, q, p, p, p, None) == 0
    torch.cuda.synchronize()
    assert bool((buf == 7.0).all()) and bool((ib == 9).all())


@pytest.mark.gpu
def test_factor_returns_surface(dev):
    import pandas as pd

    import mff
    from mff import engine, frames
    from mff.factor import Factor, factor_returns
    assert mff.factor_returns is factor_returns
    rng = np.random.default_rng(9)
    D, S = 7, 60
    codes = [f"{i:06d}.SZ" for i in range(S)]
    dates = [dt.date(2024, 3, 1) + dt.timedelta(days=i) for i in range(D)]
    specs = {"alpha": (slice(0, D), slice(0, 52)), "beta": (slice(1, D), slice(6, S)), "gamma": (slice(0, D - 2), slice(0, S))}
    base = rng.standard_normal((D, S))
    K = len(specs)
    x, xs = np.zeros((K, D, S)), np.full((K, D, S), ABSENT, np.uint8)
    fs = []
    for k, (nm, (ds, ss)) in enumerate(specs.items()):
        x[k] = 0.5 * base + 0.8 * rng.standard_normal((D, S))
        xs[k][ds, ss] = VALUE
        xs[k, 2, 10 + k] = NULL
        x[k, 3, 12 + k] = np.nan
        fs.append(Factor(nm, frames.to_long(x[k], xs[k], codes, dates, nm)))
    pct = 0.02 * rng.standard_normal((D, S))
    cap = np.exp(rng.normal(8.0, 1.0, (D, S)))
    cap[1, 20], cap[1, 21] = -1.0, 0.0
    full = np.full((D, S), VALUE, np.uint8)
    pv = frames.to_long(pct, full, codes, dates, "pct_change").merge(frames.to_long(cap, full, codes, dates, "cmc"),
                                                                     on=["code", "date"])
    labels = np.array(["bank", "tech", "coal"], dtype=object)[np.arange(S) % 3]
    labels[5] = None
    industry = pd.DataFrame({"code": codes, "industry": labels})
    # the restatement on the same dense arrays: y = the next day's return
    y, ys = np.zeros((D, S)), np.full((D, S), NULL, np.uint8)
    y[:-1], ys[:-1] = np.exp(np.log1p(pct[1:])) - 1.0, VALUE
    grp = np.tile(np.where(labels == None, -1, np.arange(S) % 3).astype(np.int32), (D, 1))  # noqa: E711
    with np.errstate(invalid="ignore"):
        okw = np.isfinite(cap) & (cap > 0)
        w = np.where(okw, np.sqrt(np.where(okw, cap, 1.0)), 0.0)
    want = ref.regress(x, xs, y, ys, w, np.where(okw, VALUE, NULL).astype(np.uint8), grp, 3)
    wa, wo = ref.aggregate(want)
    names = list(specs)
    out, daily, per_date, spec = factor_returns(fs, industry=industry, weight="cmc", return_daily=True,
                                                return_residual=True, pv_data=pv, device=dev)
    assert list(out.index) == names
    assert list(out.columns) == list(engine.REG_AGG_COLUMNS) + ["mean_r2", "mean_n"]
    print(f"surface: worst abs err {np.nanmax(np.abs(out.to_numpy()[:, :6].astype(float) - wa)):.3e}")
    np.testing.assert_allclose(out.to_numpy()[:, :6].astype(float), wa, equal_nan=True, **TOL)
    np.testing.assert_allclose(out[["mean_r2", "mean_n"]].to_numpy()[0], wo, **TOL)
    assert want["status"].tolist() == [1, 0, 0, 0, 0, 1, 1]   # beta misses day 0, gamma days 5 and 6, no return after day 6
    assert list(daily.columns) == ["date", "factor", "ret", "t"] and len(daily) == 4 * K
    assert list(daily["date"]) == [d for d in dates[1:5] for _ in range(K)] and list(daily["factor"]) == names * 4
    np.testing.assert_allclose(daily["ret"].to_numpy().reshape(4, K), want["beta"][1:5], **TOL)
    np.testing.assert_allclose(daily["t"].to_numpy().reshape(4, K), want["t"][1:5], **TOL)
    assert list(per_date.columns) == ["date", "n", "dof", "r2", "status"] and list(per_date["date"]) == dates
    assert np.array_equal(per_date["n"], want["n"]) and np.array_equal(per_date["status"], want["status"])
    assert np.array_equal(per_date["dof"], want["dof"])
    np.testing.assert_allclose(per_date["r2"].to_numpy(), want["r2"], equal_nan=True, **TOL)
    assert isinstance(spec, Factor) and spec.factor_name == "specific_return"
    sv, ss_, _, _ = frames.from_long(spec.factor_exposure, "specific_return", codes=codes, dates=dates)
    assert np.array_equal(ss_, want["resid_state"])
    np.testing.assert_allclose(sv, want["resid_val"], **TOL)
    ic = spec.ic_test(future_days=1, plot_out=False, return_df=True, pv_data=pv, device=dev)
    assert list(ic.columns) == ["date", "IC", "rank_IC"] and len(ic) >= 1
    # the mapping form, the mean-only form, return_with, errors
    only = factor_returns({"u": fs[0], "v": fs[1], "w": fs[2]}, industry=industry, weight="cmc", pv_data=pv, device=dev)
    assert list(only.index) == ["u", "v", "w"] and np.array_equal(only.to_numpy(), out.to_numpy(), equal_nan=True)
    row = fs[0].return_with(fs[1:], industry=industry, weight="cmc", pv_data=pv, device=dev)
    assert row.name == "alpha" and np.array_equal(row.to_numpy(dtype=float), out.loc["alpha"].to_numpy(dtype=float),
                                                    equal_nan=True)
    row, dly, _ = fs[0].return_with(fs[1:], industry=industry, weight="cmc", pv_data=pv, device=dev, return_daily=True)
    assert set(dly["factor"]) == {"alpha"} and len(dly) == 4
    plain = factor_returns(fs, pv_data=pv, device=dev)         # no industries, no weights
    wp, _ = ref.aggregate(ref.regress(x, xs, y, ys))
    np.testing.assert_allclose(plain.to_numpy()[:, :6].astype(float), wp, equal_nan=True, **TOL)
    with pytest.raises(ValueError, match="duplicate"):
        factor_returns([fs[0], fs[0]], pv_data=pv, device=dev)
    with pytest.raises(ValueError, match="duplicate"):
        fs[0].return_with({"alpha": fs[1]}, pv_data=pv, device=dev)
    with pytest.raises(ValueError, match="weight"):
        factor_returns(fs, weight="mcap", pv_data=pv, device=dev)
    with pytest.raises(ValueError, match="min_obs"):
        factor_returns(fs, min_obs=-1, pv_data=pv, device=dev)
    # Factor.neutralize through the shared industry helper = a direct engine.neutralize call
    neu = fs[0].neutralize(industry=industry, size=None, pv_data=pv, device=dev)
    c0, d0 = frames.universe(fs[0].factor_exposure)
    v0, s0, _, _ = frames.from_long(fs[0].factor_exposure, "alpha", codes=c0, dates=d0)
    g0 = np.tile(np.where(labels[:52] == None, -1, np.arange(52) % 3).astype(np.int32), (len(d0), 1))  # noqa: E711
    ov, os_ = engine.neutralize(_t(v0[None], dev), _t(s0[None], dev), _t(g0, dev), G=3)
    torch.cuda.synchronize()
    nv, ns, _, _ = frames.from_long(neu.factor_exposure, "alpha_neu", codes=c0, dates=d0)
    assert np.array_equal(ns, os_[0].cpu().numpy())
    m = ns == VALUE
    assert np.array_equal(nv[m].view(np.int64), ov[0].cpu().numpy()[m].view(np.int64))
