"""mff_xs_orth_* on the GPU (per-day factor orthogonalisation: f64 MFMA Gram, Jacobi
eigensolver / Cholesky in LDS, f64 MFMA apply) against its numpy restatement
tests/xs_orth_ref.py: n, status, states and NaN patterns exact, finite values within rtol =
atol = 1e-9 (the tolerance of tests/test_gpu_xreg.py).  The panels are built as there (mutual
correlation 0.25), so the condition number of the day's correlation matrix stays below 1e3
(asserted from the restatement before any comparison) and 1e-9 is seven decades above
cond * 2^-53.  Every comparison prints its worst error; the worst over all cases is quoted in
DESIGN.md §12."""
import datetime as dt

import numpy as np
import pytest

import xs_orth_ref as ref
from xs_orth_ref import ABSENT, NULL, VALUE

torch = pytest.importorskip("torch")

TOL = dict(rtol=1e-9, atol=1e-9)
COND_MAX = 1e3
METHODS = ref.METHODS
VALUES = ("val", "T", "eig", "keep")


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def _t(a, dev):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _panel(seed, K, D, S):
    """K exposure rows = 0.5 common + sqrt(0.75) own noise (pairwise correlation 0.25).  From
    16 stocks on every day holds, spread over DIFFERENT rows: an ABSENT run, NULLs, NaN, +inf,
    -inf (each drops its stock from the listwise set through that one row) and -0.0 / +0.0."""
    rng = np.random.default_rng(seed)
    common = rng.standard_normal((D, S))
    x = 0.5 * common[None] + np.sqrt(0.75) * rng.standard_normal((K, D, S))
    xs = np.full((K, D, S), VALUE, np.uint8)
    if S >= 16:
        for d in range(D):
            hit = rng.permutation(S)[:max(8, S // 10)]
            kinds = ("absent", "null", np.nan, np.inf, -np.inf, -0.0, 0.0)
            for i, s in enumerate(hit):
                r = int(rng.integers(0, K))
                kind = kinds[i % len(kinds)]
                if kind == "absent":
                    xs[r, d, s:s + max(1, S // (20 * (K + 1)))] = ABSENT
                elif kind == "null":
                    xs[r, d, s] = NULL
                else:
                    x[r, d, s] = kind
    return x, xs


def _run(dev, x, xs, method="symmetric", min_obs=0, **kw):
    from mff import engine
    r = engine.factor_orthogonalize(_t(x, dev), _t(xs, dev), method=method, min_obs=min_obs, **kw)
    torch.cuda.synchronize()
    return dict(val=r.val.cpu().numpy(), state=r.state.cpu().numpy(), T=r.transform.cpu().numpy(),
                eig=r.eig.cpu().numpy(), keep=r.keep.cpu().numpy(), n=r.n.cpu().numpy(), status=r.status.cpu().numpy())


def _check(got, want, name, cond=True, tol=TOL):
    if cond and (want["status"] == 0).any():
        c = np.nanmax(want["cond"])
        assert c < COND_MAX, f"{name}: panel too ill-conditioned for the tolerance (cond {c:.3g})"
    for k in ("n", "status"):
        assert got[k].dtype == np.int32 and np.array_equal(got[k], want[k]), \
            f"{name}: {k} differs: {got[k].tolist()[:8]} vs {want[k].tolist()[:8]}"
    assert got["state"].dtype == np.uint8 and np.array_equal(got["state"], want["state"]), f"{name}: states"
    assert (got["val"][got["state"] != VALUE] == 0.0).all(), f"{name}: a non-VALUE entry is not 0.0"
    worst = 0.0
    for k in VALUES:
        g, w = got[k], want[k]
        assert g.shape == w.shape and g.dtype == np.float64, f"{name}: {k} shape"
        bad = np.argwhere(np.isnan(g) != np.isnan(w))
        assert not len(bad), f"{name}: NaN pattern of {k} differs at {bad[:5].tolist()}"
        m = np.isfinite(w)
        if m.any():
            worst = max(worst, float((np.abs(g[m] - w[m]) / (1.0 + np.abs(w[m]))).max()))
    print(f"{name}: status {np.bincount(want['status'], minlength=3).tolist()}, worst err / (1 + |ref|) {worst:.3e}")
    for k in VALUES:
        np.testing.assert_allclose(got[k], want[k], equal_nan=True, err_msg=f"{name}: {k}", **tol)
    return worst


@pytest.mark.gpu
@pytest.mark.parametrize("method", METHODS)
@pytest.mark.parametrize("K", [1, 2, 15, 16, 17, 58, 63, 64])
def test_factor_boundaries(dev, K, method):
    """The odd-K round-robin padding, the 16-row MFMA padding (15, 16, 17) and the full block."""
    x, xs = _panel(100 + K, K, 2, 257)
    want = ref.orthogonalize(x, xs, method)
    assert (want["status"] == 0).all()
    _check(_run(dev, x, xs, method), want, f"K={K} {method}")


@pytest.mark.gpu
@pytest.mark.parametrize("S", [5, 7, 63, 64, 65, 127, 128, 129, 257, 1023, 1025, 5003])
def test_stock_boundaries(dev, S):
    """K = 3: S = K + 2, the MFMA k = 4 step, the 32-stock tile, the 512-stock chunk of the
    apply pass and the sizes at which the two-day call splits the stocks into runs (S > 256)."""
    x, xs = _panel(200 + S, 3, 2, S)
    for method in METHODS:
        want = ref.orthogonalize(x, xs, method)
        assert (want["status"] == 0).all()
        _check(_run(dev, x, xs, method), want, f"S={S} {method}")


def _degenerate_panel():
    """Days: 0 normal, 1 an empty U, 2 n = K, 3 n = K + 1, 4 a constant column, 5 a duplicated
    column, 6 all ABSENT, 7 normal."""
    K, D, S = 3, 8, 120
    x, xs = _panel(7, K, D, S)
    xs[1, 1] = NULL
    u = ref.usable(x, xs)
    idx = np.nonzero(u[2])[0]
    xs[0, 2] = ABSENT
    xs[0, 2, idx[:K]] = VALUE
    idx = np.nonzero(u[3])[0]
    for start in range(len(idx) - K):                          # K + 1 stocks with a well-conditioned R
        pick = idx[start:start + K + 1]
        if ref.orth_day(x[:, 3][:, pick].T)["cond"] < 50.0:
            break
    xs[2, 3] = NULL
    xs[2, 3, pick] = VALUE
    x[1, 4] = 2.5
    x[2, 5], xs[2, 5] = x[0, 5], xs[0, 5]
    xs[:, 6] = ABSENT
    return x, xs


@pytest.mark.gpu
@pytest.mark.parametrize("method", METHODS)
def test_degenerate_days(dev, method):
    """One degenerate day each; the other days of the same call are unaffected."""
    x, xs = _degenerate_panel()
    want = ref.orthogonalize(x, xs, method)
    assert want["status"].tolist() == [0, 1, 1, 0, 2, 2, 1, 0]
    assert want["n"][[1, 2, 3, 6]].tolist() == [0, 3, 4, 0] and want["n"][4] > 50 and want["n"][5] > 50
    assert np.nanmax(want["cond"]) < COND_MAX
    got = _run(dev, x, xs, method)
    _check(got, want, f"degenerate {method}")
    assert (got["state"][:, 6] == ABSENT).all() and (got["state"][:, [1, 4, 5]] != VALUE).all()
    cx, cxs = _panel(7, 3, 8, 120)
    base = _run(dev, cx, cxs, method)
    for d in (0, 7):                                           # untouched days: the same bits
        for k in VALUES:
            a, b = (got[k][:, d], base[k][:, d]) if k == "val" else (got[k][d], base[k][d])
            assert np.array_equal(a.view(np.int64), b.view(np.int64)), (d, k)
    n0 = int(want["n"][0])
    at, above = _run(dev, x, xs, method, min_obs=n0), _run(dev, x, xs, method, min_obs=n0 + 1)
    _check(at, ref.orthogonalize(x, xs, method, min_obs=n0), "min_obs at n", cond=False)
    _check(above, ref.orthogonalize(x, xs, method, min_obs=n0 + 1), "min_obs above n", cond=False)
    assert at["status"][0] == 0 and above["status"][0] == 1 and at["status"][3] == 1


@pytest.mark.gpu
def test_output_properties(dev):
    """On U the outputs have mean 0 and the identity as sample covariance; the symmetric
    transform is bitwise symmetric and permutes with the rows; Gram-Schmidt is upper triangular,
    keeps the first row's z-score and ends in the regression residual of the last row."""
    from mff import engine
    K, D, S = 7, 3, 900
    x, xs = _panel(41, K, D, S)
    u = ref.usable(x, xs)
    res = {}
    for method in METHODS:
        want = ref.orthogonalize(x, xs, method)
        got = res[method] = _run(dev, x, xs, method)
        _check(got, want, f"properties {method}")
        assert (got["status"] == 0).all()
        wm = wc = 0.0
        for d in range(D):
            f = got["val"][:, d][:, u[d]]
            assert np.array_equal(got["state"][:, d] == VALUE, np.tile(u[d], (K, 1)))
            wm = max(wm, np.abs(f.mean(axis=1)).max())
            wc = max(wc, np.abs(np.cov(f, ddof=1) - np.eye(K)).max())
        print(f"properties {method}: worst |mean| {wm:.3e}, worst |cov - I| {wc:.3e}")
        assert wm <= 1e-12 and wc <= 1e-9
    sym, gs = res["symmetric"], res["schmidt"]
    assert np.array_equal(sym["T"].view(np.int64), sym["T"].transpose(0, 2, 1).view(np.int64))
    perm = np.array([3, 0, 6, 1, 5, 2, 4])
    pg = _run(dev, x[perm], xs[perm], "symmetric")
    worst = max(np.abs(pg["val"] - sym["val"][perm]).max(), np.abs(pg["keep"] - sym["keep"][:, perm]).max(),
                np.abs(pg["T"] - sym["T"][:, perm][:, :, perm]).max())
    print(f"row permutation: worst abs err {worst:.3e}")
    assert np.array_equal(pg["state"], sym["state"][perm])
    np.testing.assert_allclose(pg["val"], sym["val"][perm], **TOL)
    np.testing.assert_allclose(pg["keep"], sym["keep"][:, perm], **TOL)
    np.testing.assert_allclose(pg["eig"], sym["eig"], **TOL)
    np.testing.assert_allclose(pg["T"], sym["T"][:, perm][:, :, perm], **TOL)
    il = np.tril_indices(K, -1)
    assert (gs["T"][:, il[0], il[1]] == 0.0).all() and not np.signbit(gs["T"][:, il[0], il[1]]).any()
    reg = engine.factor_regress(_t(x[:K - 1], dev), _t(xs[:K - 1], dev), _t(x[K - 1], dev), _t(xs[K - 1], dev),
                                residual=True)
    torch.cuda.synchronize()
    assert bool((reg.status == 0).all())
    rv, rs = reg.resid_val.cpu().numpy(), reg.resid_state.cpu().numpy()
    w1 = wk = 0.0
    for d in range(D):
        m = u[d]
        assert np.array_equal(rs[d] == VALUE, m)
        z1 = (x[0, d][m] - x[0, d][m].mean()) / x[0, d][m].std(ddof=1)
        e = rv[d][m] / rv[d][m].std(ddof=1)
        w1 = max(w1, np.abs(gs["val"][0, d][m] - z1).max())
        wk = max(wk, np.abs(gs["val"][K - 1, d][m] - e).max())
    print(f"schmidt: first row vs z-score {w1:.3e}, last row vs factor_regress residual {wk:.3e}")
    assert w1 <= 1e-9 and wk <= 1e-9


@pytest.mark.gpu
@pytest.mark.parametrize("method", METHODS)
def test_equivariance(dev, method):
    """Scaling a row by 1e-8 / 1e8 changes nothing within 1e-9; shifting a row by 1e6 of its
    standard deviations stays within 1e-7 of the restatement on the unshifted panel (1e6 * 2^-53
    = 1.1e-10 sd of input rounding, times the condition bound 1e3)."""
    K = 6
    x, xs = _panel(31, K, 2, 1201)
    want = ref.orthogonalize(x, xs, method)
    base = _run(dev, x, xs, method)
    _check(base, want, f"base {method}")
    q = x.copy()
    for r, a in ((0, 1e-8), (1, 1e8), (4, -3.0)):
        q[r] = a * x[r]
    sign = np.ones(K)
    sign[4] = -1.0
    got = _run(dev, q, xs, method)
    assert np.array_equal(got["n"], base["n"]) and np.array_equal(got["status"], base["status"])
    assert np.array_equal(got["state"], base["state"])
    flipped = got["val"] * sign[:, None, None]                 # a negative scale flips that row's output only
    worst = max(np.abs(flipped - base["val"]).max(), np.abs(got["keep"] - base["keep"]).max(),
                np.abs(got["eig"] - base["eig"]).max())
    print(f"scaling {method}: worst abs err {worst:.3e}")
    np.testing.assert_allclose(flipped, base["val"], **TOL)
    np.testing.assert_allclose(got["keep"], base["keep"], **TOL)
    np.testing.assert_allclose(got["eig"], base["eig"], **TOL)
    q = x.copy()
    for r, b in ((2, 1e6), (5, -1e6)):
        sd = np.std(x[r][np.isfinite(x[r])])
        with np.errstate(invalid="ignore"):
            q[r] = x[r] + b * sd
    got = _run(dev, q, xs, method)
    worst = _check(got, want, f"shift by 1e6 sd {method}", tol=dict(rtol=1e-7, atol=1e-7))
    print(f"shift {method}: worst err / (1 + |ref|) {worst:.3e}")


@pytest.mark.gpu
@pytest.mark.parametrize("method", METHODS)
def test_bit_identical_runs(dev, method):
    from mff import engine
    x, xs = _panel(51, 58, 3, 1025)
    a, b = _t(x, dev), _t(xs, dev)
    r1 = engine.factor_orthogonalize(a, b, method=method)
    r2 = engine.factor_orthogonalize(a, b, method=method)
    torch.cuda.synchronize()
    for u, v in zip(r1, r2):
        assert torch.equal(u.view(torch.int64) if u.dtype == torch.float64 else u,
                           v.view(torch.int64) if v.dtype == torch.float64 else v)
    assert bool((r1.status == 0).all())


@pytest.mark.gpu
@pytest.mark.parametrize("S", [29, 257])
@pytest.mark.parametrize("R", [2, 3])
def test_stock_shards_match_one_rank(dev, R, S):
    from mff import dist
    x, xs = _panel(400 + R + S, 3, 3, S)
    bounds = [dist.shard_bounds(S, R, r) for r in range(R)]
    assert len({b - a for a, b in bounds}) == 2               # uneven shards
    for method in METHODS:
        one = _run(dev, x, xs, method)
        _check(one, ref.orthogonalize(x, xs, method), f"one rank {method}")
        assert (one["status"] == 0).all()

        def rank_fn(comm):
            a, b = bounds[comm.rank]
            return _run(dev, x[..., a:b], xs[..., a:b], method, comm=comm, stocks_total=S)

        for r, got in enumerate(dist.run_threads(R, rank_fn)):
            a, b = bounds[r]
            want = dict(one, val=one["val"][..., a:b], state=one["state"][..., a:b])
            _check(got, want, f"rank {r} of {R}, S={S} {method}", cond=False)


@pytest.mark.gpu
@pytest.mark.parametrize("method", METHODS)
def test_split_matches_unsplit(dev, method):
    x, xs = _panel(61, 9, 3, 1300)
    one = _run(dev, x, xs, method, split=1)
    _check(one, ref.orthogonalize(x, xs, method), f"unsplit {method}")
    for ns in (2, 5):
        _check(_run(dev, x, xs, method, split=ns), one, f"split={ns} {method}", cond=False)


def _run_c_abi(dev, x, xs, method, fill):
    """The four C calls on one workspace whose every f64 slot holds `fill` beforehand."""
    from mff import _lib
    lib = _lib.load()
    K, D, S = x.shape
    f64 = torch.float64
    xv, xst = _t(x, dev), _t(xs, dev)
    nbytes = lib.mff_xs_orth_workspace_bytes(K, D, S)
    assert nbytes % 8 == 0
    ws = torch.full((nbytes // 8,), fill, dtype=f64, device=dev)
    sums = torch.empty((1, D, 2 * K + 1), dtype=f64, device=dev)
    gram = torch.empty((1, D, K, K), dtype=f64, device=dev)
    tr = torch.empty((D, K, K), dtype=f64, device=dev)
    eig, keep = (torch.empty((D, K), dtype=f64, device=dev) for _ in range(2))
    n, status = (torch.empty(D, dtype=torch.int32, device=dev) for _ in range(2))
    ov, os_ = torch.empty_like(xv), torch.empty_like(xst)
    P = lambda t_: t_.data_ptr()
    _lib.check(lib.mff_xs_orth_sums(P(xv), P(xst), K, D, S, 1, P(sums), P(ws), None), "sums")
    _lib.check(lib.mff_xs_orth_gram(P(xv), K, D, S, P(sums), 1, 1, P(gram), P(ws), None), "gram")
    _lib.check(lib.mff_xs_orth_solve(P(gram), 1, K, D, METHODS.index(method), 0, P(tr), P(eig), P(keep), P(n),
                                     P(status), P(ws), None), "solve")
    _lib.check(lib.mff_xs_orth_apply(P(xv), P(xst), K, D, S, P(status), P(ov), P(os_), P(ws), None), "apply")
    torch.cuda.synchronize()
    return dict(val=ov.cpu().numpy(), state=os_.cpu().numpy(), T=tr.cpu().numpy(), eig=eig.cpu().numpy(),
                keep=keep.cpu().numpy(), n=n.cpu().numpy(), status=status.cpu().numpy())


@pytest.mark.gpu
@pytest.mark.parametrize("method", METHODS)
def test_full_block_constant_last_row_on_a_poisoned_workspace(dev, method):
    """K = 64 fills every one of the 2K + 1 = 129 per-day scalars, the last being the raw sum of
    squares behind the constant rule of row 63.  The workspace holds NaN, then -1e300, before
    the calls: nothing stale may reach the result -- the healthy days stay status 0 (a NaN
    there would turn them singular), the day whose last row is constant is status 2, and the
    two runs agree bit for bit."""
    x, xs = _panel(164, 64, 3, 257)
    x[63, 1] = 2.5
    want = ref.orthogonalize(x, xs, method)
    assert want["status"].tolist() == [0, 2, 0] and want["n"][1] > 65
    runs = [_run_c_abi(dev, x, xs, method, fill) for fill in (float("nan"), -1e300)]
    for got, name in zip(runs, ("NaN", "-1e300")):
        _check(got, want, f"K=64, constant row 63, workspace of {name}, {method}")
    for k in VALUES:
        assert np.array_equal(runs[0][k].view(np.int64), runs[1][k].view(np.int64)), k
    assert np.array_equal(runs[0]["state"], runs[1]["state"])
    _check(_run(dev, x, xs, method), want, f"K=64, constant row 63, engine, {method}")


def _sentinels(dev):
    buf = torch.full((8192,), 7.0, dtype=torch.float64, device=dev)
    ib = torch.full((4096,), 9, dtype=torch.int32, device=dev)
    return buf, ib


@pytest.mark.gpu
def test_errors_write_nothing(dev):
    from mff import _lib, engine
    lib = _lib.load()
    assert lib.mff_xs_orth_max_factors() == 64
    buf, ib = _sentinels(dev)
    K, D, S = 2, 1, 8
    xv = torch.zeros((K, D, S), dtype=torch.float64, device=dev)
    xs = torch.full((K, D, S), VALUE, dtype=torch.uint8, device=dev)
    os_ = torch.full((K, D, S), 5, dtype=torch.uint8, device=dev)
    ws = torch.full((1 << 16,), 3, dtype=torch.uint8, device=dev)
    p, q, w, X, XS, OS = buf.data_ptr(), ib.data_ptr(), ws.data_ptr(), xv.data_ptr(), xs.data_ptr(), os_.data_ptr()
    for K_, D_, S_, ns in ((0, D, S, 1), (65, D, S, 1), (K, -1, S, 1), (K, D, -1, 1), (K, D, S, 0)):
        assert lib.mff_xs_orth_sums(X, XS, K_, D_, S_, ns, p, w, None) < 0
        assert lib.mff_last_error()
    for K_, D_, S_, R_, ns in ((0, D, S, 1, 1), (65, D, S, 1, 1), (K, -1, S, 1, 1), (K, D, -1, 1, 1), (K, D, S, 0, 1),
                               (K, D, S, 1, 0)):
        assert lib.mff_xs_orth_gram(X, K_, D_, S_, p, R_, ns, p, w, None) < 0
    for P_, K_, D_, m_, mo in ((0, K, D, 0, 0), (1, 0, D, 0, 0), (1, 65, D, 0, 0), (1, K, -1, 0, 0), (1, K, D, 2, 0),
                               (1, K, D, -1, 0), (1, K, D, 0, -1)):
        assert lib.mff_xs_orth_solve(p, P_, K_, D_, m_, mo, p, p, p, q, q, w, None) < 0
    assert b"min_obs" in lib.mff_last_error()
    for K_, D_, S_ in ((0, D, S), (65, D, S), (K, -1, S), (K, D, -1)):
        assert lib.mff_xs_orth_apply(X, XS, K_, D_, S_, q, p, OS, w, None) < 0
    torch.cuda.synchronize()
    assert bool((buf == 7.0).all()) and bool((ib == 9).all()) and bool((ws == 3).all()) and bool((os_ == 5).all())
    with pytest.raises(ValueError, match="min_obs"):
        engine.factor_orthogonalize(xv, xs, min_obs=-1)
    with pytest.raises(ValueError, match="method must be one of"):
        engine.factor_orthogonalize(xv, xs, method="pca")
    with pytest.raises(ValueError, match="split"):
        engine.factor_orthogonalize(xv, xs, split=0)
    with pytest.raises(_lib.MffError):
        engine.factor_orthogonalize(torch.zeros((65, 1, 8), dtype=torch.float64, device=dev),
                                    torch.zeros((65, 1, 8), dtype=torch.uint8, device=dev))


@pytest.mark.gpu
def test_empty_day_and_stock_axes(dev):
    from mff import _lib, engine
    lib = _lib.load()
    z = lambda shape, dtype: torch.zeros(shape, dtype=dtype, device=dev)
    for method in METHODS:
        r = engine.factor_orthogonalize(z((3, 0, 5), torch.float64), z((3, 0, 5), torch.uint8), method=method)
        assert tuple(r.val.shape) == (3, 0, 5) and tuple(r.transform.shape) == (0, 3, 3) and tuple(r.n.shape) == (0,)
        r = engine.factor_orthogonalize(z((3, 2, 0), torch.float64), z((3, 2, 0), torch.uint8), method=method)
        torch.cuda.synchronize()
        assert tuple(r.val.shape) == (3, 2, 0) and tuple(r.state.shape) == (3, 2, 0)
        assert bool(torch.isnan(r.transform).all()) and bool(torch.isnan(r.eig).all()) and bool(torch.isnan(r.keep).all())
        assert r.n.tolist() == [0, 0] and r.status.tolist() == [1, 1]
    buf, ib = _sentinels(dev)
    p, q = buf.data_ptr(), ib.data_ptr()
    assert lib.mff_xs_orth_sums(None, None, 2, 0, 5, 1, p, p, None) == 0
    assert lib.mff_xs_orth_gram(None, 2, 0, 5, p, 1, 1, p, p, None) == 0
    assert lib.mff_xs_orth_solve(p, 1, 2, 0, 0, 0, p, p, p, q, q, p, None) == 0
    assert lib.mff_xs_orth_apply(None, None, 2, 0, 5, q, p, p, p, None) == 0
    assert lib.mff_xs_orth_apply(None, None, 2, 3, 0, q, p, p, p, None) == 0
    torch.cuda.synchronize()
    assert bool((buf == 7.0).all()) and bool((ib == 9).all())


def _same_frame(a, b, name, codes, dates):
    """Two long frames hold the same rows in the same order with the same bits (NaN included)."""
    from mff import frames
    if list(a.columns) != list(b.columns) or list(a["code"]) != list(b["code"]) or list(a["date"]) != list(b["date"]):
        return False
    (av, as_, _, _), (bv, bs, _, _) = (frames.from_long(f, name, codes=codes, dates=dates) for f in (a, b))
    return np.array_equal(as_, bs) and np.array_equal(av.view(np.int64), bv.view(np.int64))


@pytest.mark.gpu
def test_orthogonalize_surface(dev):
    import mff
    from mff import frames
    from mff.factor import Factor, MinFreqFactor, orthogonalize
    assert mff.orthogonalize is orthogonalize
    rng = np.random.default_rng(9)
    D, S = 6, 60
    codes = [f"{i:06d}.SZ" for i in range(S)]
    dates = [dt.date(2024, 3, 1) + dt.timedelta(days=i) for i in range(D)]
    specs = {"alpha": (slice(0, D), slice(0, 52)), "beta": (slice(1, D), slice(6, S)),
             "gamma": (slice(0, D - 1), slice(0, S)), "delta": (slice(0, D), slice(3, S))}
    base = rng.standard_normal((D, S))
    K = len(specs)
    x, xs = np.zeros((K, D, S)), np.full((K, D, S), ABSENT, np.uint8)
    fs = []
    for k, (nm, (ds, ss)) in enumerate(specs.items()):
        x[k] = 0.5 * base + 0.8 * rng.standard_normal((D, S))
        xs[k][ds, ss] = VALUE
        xs[k, 2, 10 + k] = NULL
        x[k, 3, 12 + k] = np.nan
        cls = MinFreqFactor if nm == "beta" else Factor
        fs.append(cls(nm, frames.to_long(x[k], xs[k], codes, dates, nm)))
    x = np.where(xs == VALUE, x, 0.0)
    names = list(specs)
    before = [(f.factor_exposure, f.factor_exposure.copy()) for f in fs]
    for method in METHODS:
        want = ref.orthogonalize(x, xs, method)
        assert want["status"].tolist() == [1, 0, 0, 0, 0, 1] and np.nanmax(want["cond"]) < COND_MAX
        out, per_date, per_factor = orthogonalize(fs, method=method, return_info=True, device=dev)
        assert list(out) == names
        worst = 0.0
        for k, nm in enumerate(names):
            f = out[nm]
            assert type(f) is type(fs[k]) and f.factor_name == f"{nm}_orth"
            assert list(f.factor_exposure.columns) == ["code", "date", f"{nm}_orth"]
            ref_frame = frames.to_long(want["val"][k], want["state"][k], codes, dates, f"{nm}_orth")
            assert list(f.factor_exposure["code"]) == list(ref_frame["code"])
            assert list(f.factor_exposure["date"]) == list(ref_frame["date"])
            v, s, _, _ = frames.from_long(f.factor_exposure, f"{nm}_orth", codes=codes, dates=dates)
            assert np.array_equal(s, want["state"][k])            # null / absent mapping
            worst = max(worst, np.abs(v - want["val"][k]).max())
            np.testing.assert_allclose(v, want["val"][k], **TOL)
        print(f"surface {method}: worst abs err {worst:.3e}")
        assert list(per_date.columns) == ["date", "n", "status", "eig_min", "eig_max", "cond"]
        assert list(per_date["date"]) == dates and np.array_equal(per_date["n"], want["n"])
        assert np.array_equal(per_date["status"], want["status"])
        np.testing.assert_allclose(per_date["eig_min"].to_numpy(), want["eig"][:, 0], equal_nan=True, **TOL)
        np.testing.assert_allclose(per_date["eig_max"].to_numpy(), want["eig"][:, -1], equal_nan=True, **TOL)
        np.testing.assert_allclose(per_date["cond"].to_numpy(), want["cond"], equal_nan=True, **TOL)
        assert list(per_factor.index) == names and list(per_factor.columns) == ["days", "mean_keep", "min_keep"]
        ok = want["keep"][want["status"] == 0]
        assert (per_factor["days"] == 4).all()
        np.testing.assert_allclose(per_factor["mean_keep"].to_numpy(), ok.mean(axis=0), **TOL)
        np.testing.assert_allclose(per_factor["min_keep"].to_numpy(), ok.min(axis=0), **TOL)
    for f, (obj, copy) in zip(fs, before):                        # the inputs are untouched
        assert f.factor_exposure is obj and _same_frame(obj, copy, f.factor_name, codes, dates)
    # the mapping form, the plain form, orthogonal_to, errors
    gs = orthogonalize(fs, method="schmidt", device=dev)
    assert isinstance(gs, dict) and list(gs) == names
    mp = orthogonalize({"u": fs[0], "v": fs[1]}, device=dev)
    assert list(mp) == ["u", "v"] and mp["u"].factor_name == "u_orth" and type(mp["v"]) is MinFreqFactor
    last = fs[3].orthogonal_to(fs[:3], device=dev)
    assert type(last) is Factor and last.factor_name == "delta_orth"
    assert _same_frame(last.factor_exposure, gs["delta"].factor_exposure, "delta_orth", codes, dates)
    one = fs[3].orthogonal_to({"a": fs[0], "b": fs[1], "c": fs[2]}, device=dev)
    assert _same_frame(one.factor_exposure, gs["delta"].factor_exposure, "delta_orth", codes, dates)
    with pytest.raises(ValueError, match="duplicate"):
        orthogonalize([fs[0], fs[0]], device=dev)
    with pytest.raises(ValueError, match="duplicate"):
        fs[0].orthogonal_to({"alpha": fs[1]}, device=dev)
    with pytest.raises(ValueError, match="method must be one of"):
        orthogonalize(fs, method="pca", device=dev)
    with pytest.raises(ValueError, match="min_obs must be an integer >= 0"):
        orthogonalize(fs, min_obs=-1, device=dev)
