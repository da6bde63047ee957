"""mff_xs_comb_* on the GPU (composite factor: one-pass batched moments and ICs, trailing-window
equal / ic / icir / max_icir weights, renormalised weighted z-score sum) against its numpy
restatement tests/xs_combine_ref.py: states, status, count, n_pairs and NaN patterns exact,
finite values within rtol = atol = 1e-9 (the tolerance of tests/test_gpu_xreg.py and
test_gpu_xorth.py).  The panels are built with mutual factor correlation 0.25 and a planted IC,
and the condition number of the scaled, shrunk IC covariance stays below 1e3 (asserted from the
restatement before any comparison).

No parity panel may pass on empty output: before comparing, the restatement alone must show
status 0 on every date d >= h + m - 1 and a VALUE on at least 90 % of the stock-days that hold
any factor.  The share is taken over the dates d >= h + m - 1: at D = 40, h = 2, m = 4 the five
dates before them cannot have weights, which alone is 12.5 % of the panel ('equal' has weights
on every date and is held to 90 % of the whole panel).  Every comparison prints its worst
err / (1 + |ref|); the worst over all cases is quoted in DESIGN.md §13."""
import datetime as dt

import numpy as np
import pytest

import xs_combine_ref as ref
from xs_combine_ref import ABSENT, NULL, VALUE

torch = pytest.importorskip("torch")

TOL = dict(rtol=1e-9, atol=1e-9)
COND_MAX = 1e3
METHODS = ref.METHODS
VALUES = ("val", "weights", "ic")
INTS = ("n_pairs", "count", "status")
D, H, W, M = 40, 2, 8, 4
KW = dict(future_days=H, window=W, min_periods=M)


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def _t(a, dev):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _run(dev, x, xs, y, ys, method, **kw):
    from mff import engine
    r = engine.factor_combine(_t(x, dev), _t(xs, dev), _t(y, dev), _t(ys, dev), method=method, **kw)
    torch.cuda.synchronize()
    return {k: getattr(r, k).cpu().numpy() for k in r._fields}


def _precheck(want, xs, method, name, first=None, h=H, m=M):
    """The restatement alone: weights from date `first` on, a composite on >= 90 % of the
    stock-days that hold a factor, a well-conditioned covariance."""
    first = (0 if method == "equal" else h + m - 1) if first is None else first
    assert (want["status"][first:] == 0).all(), f"{name}: restatement status {want['status'].tolist()}"
    held = (xs != ABSENT).any(axis=0)[first:]
    share = (want["state"][first:] == VALUE).sum() / max(int(held.sum()), 1)
    assert share >= 0.9, f"{name}: only {share:.3f} of the stock-days with a factor get a composite"
    if method == "max_icir":
        c = np.nanmax(want["cond"])
        assert c < COND_MAX, f"{name}: panel too ill-conditioned for the tolerance (cond {c:.3g})"


def _check(got, want, name, tol=TOL):
    for k in INTS:
        assert got[k].dtype == np.int32 and np.array_equal(got[k], want[k]), \
            f"{name}: {k} differs: {got[k].ravel().tolist()[:12]} vs {want[k].ravel().tolist()[:12]}"
    assert got["state"].dtype == np.uint8 and np.array_equal(got["state"], want["state"]), f"{name}: states"
    assert (got["val"][got["state"] != VALUE] == 0.0).all(), f"{name}: a non-VALUE entry is not 0.0"
    worst = 0.0
    for k in VALUES:
        g, w = got[k], want[k]
        assert g.shape == w.shape and g.dtype == np.float64, f"{name}: {k} shape"
        bad = np.argwhere(np.isnan(g) != np.isnan(w))
        assert not len(bad), f"{name}: NaN pattern of {k} differs at {bad[:5].tolist()}"
        fin = np.isfinite(w)
        if fin.any():
            worst = max(worst, float((np.abs(g[fin] - w[fin]) / (1.0 + np.abs(w[fin]))).max()))
    print(f"{name}: status {np.bincount(want['status'], minlength=3).tolist()}, worst err / (1 + |ref|) {worst:.3e}")
    for k in VALUES:
        np.testing.assert_allclose(got[k], want[k], equal_nan=True, err_msg=f"{name}: {k}", **tol)
    return worst


def _parity(dev, panel, name, methods=METHODS, ics=ref.IC_KINDS, strict=True, first=None, **kw):
    x, xs, y, ys = panel
    args = dict(KW, **kw)
    for ic in ics:
        for method in methods:
            want = ref.combine(x, xs, y, ys, method, ic=ic, **args)
            if strict:
                _precheck(want, xs, method, f"{name} {method} {ic}", first, args["future_days"], args["min_periods"])
            _check(_run(dev, x, xs, y, ys, method, ic=ic, **args), want, f"{name} {method} {ic}")


@pytest.mark.gpu
@pytest.mark.parametrize("ic", ref.IC_KINDS)
@pytest.mark.parametrize("K", [1, 2, 15, 16, 17, 58, 64])
def test_factor_boundaries(dev, K, ic):
    """The four waves' factor striding (K = 1, 2), the 16-factor edge and the full 64 lanes."""
    _parity(dev, ref.make_panel(100 + K, K, D, 257, h=H), f"K={K}", ics=(ic,))


@pytest.mark.gpu
@pytest.mark.parametrize("S", [1, 2, 63, 64, 65, 257, 511, 512, 513, 1023, 1024, 1025, 5003])
def test_stock_boundaries(dev, S):
    """K = 3: the wave, the 512-stock chunk of the moments pass and the 1024-stock chunk of the
    apply pass, each minus one, exact and plus one; ten chunks.  One and two stocks have no
    z-score / a +-1 IC: exact agreement only, no share of VALUEs is asked of them."""
    _parity(dev, ref.make_panel(200 + S, 3, D, S, h=H), f"S={S}", strict=S >= 63,
            ics=ref.IC_KINDS if S in (65, 513, 1025) else ("pearson",))


@pytest.mark.gpu
def test_window_edges(dev):
    panel = ref.make_panel(31, 3, D, 257, h=H)
    _parity(dev, panel, "W=1", methods=("equal", "ic"), window=1, min_periods=1)
    x, xs, y, ys = panel
    for method in ("icir", "max_icir"):                        # one date has no std
        want = ref.combine(x, xs, y, ys, method, future_days=H, window=1, min_periods=1)
        assert (want["status"] == 1).all()
        _check(_run(dev, x, xs, y, ys, method, future_days=H, window=1, min_periods=1), want, f"W=1 {method}")
    _parity(dev, panel, "W>D", window=5 * D)
    for method in METHODS[1:]:
        for name, kw in (("h>=D", dict(future_days=D, window=W, min_periods=M)),
                         ("h>D", dict(future_days=D + 7, window=W, min_periods=M)),
                         ("m>W", dict(future_days=H, window=W, min_periods=W + 1))):
            want = ref.combine(x, xs, y, ys, method, **kw)
            assert (want["status"] == 1).all() and (want["state"] != VALUE).all()
            _check(_run(dev, x, xs, y, ys, method, **kw), want, f"{name} {method}")
    _parity(dev, panel, "h=1 m=1", future_days=1, window=3, min_periods=1, methods=("ic",))
    _parity(dev, panel, "m=W", window=6, min_periods=6)


@pytest.mark.gpu
def test_coverage_starting_on_date_10(dev):
    """Factor 2 starts on date 10: its own count lags the others' (ic / icir give it weight 0
    until it has m ICs), while the listwise window of max_icir holds no date before 10."""
    x, xs, y, ys = ref.make_panel(41, 4, D, 257, h=H)
    xs[2, :10] = ABSENT
    for method in METHODS:
        want = ref.combine(x, xs, y, ys, method, **KW)
        if method in ("ic", "icir"):
            assert (want["weights"][H + M - 1:10 + H + M - 1, 2] == 0.0).all()
            assert (want["weights"][10 + H + M - 1:, 2] != 0.0).all()
            assert want["count"][14].tolist() == [W, W, 3, W]
        if method == "max_icir":
            assert (want["status"][:10 + H + M - 1] == 1).all() and want["count"][14].tolist() == [3] * 4
    _parity(dev, (x, xs, y, ys), "late factor", methods=("equal", "ic", "icir"))
    _parity(dev, (x, xs, y, ys), "late factor", methods=("max_icir",), first=10 + H + M - 1)


def _degenerate_panel():
    """Days: 3 an inf inside factor 1's pair set (its Pearson IC is NaN), 6 all ABSENT, 8 factor 0
    constant, 12 y all NULL, 20 one stock only."""
    x, xs, y, ys = ref.make_panel(7, 3, D, 120, h=H)
    s = np.nonzero((xs[1, 3] == VALUE) & (ys[3] == VALUE) & np.isfinite(x[1, 3]))[0][0]
    x[1, 3, s] = -np.inf
    xs[:, 6] = ABSENT
    x[0, 8] = 2.5
    ys[12] = NULL
    xs[:, 20, 1:] = ABSENT
    xs[:, 20, 0] = VALUE
    x[:, 20, 0] = 1.0
    return x, xs, y, ys


@pytest.mark.gpu
@pytest.mark.parametrize("ic", ref.IC_KINDS)
def test_degenerate_days(dev, ic):
    x, xs, y, ys = _degenerate_panel()
    for method in METHODS:
        want = ref.combine(x, xs, y, ys, method, ic=ic, **KW)
        assert np.isnan(want["ic"][1, 3]) == (ic == "pearson") and np.isnan(want["ic"][:, [6, 8, 12, 20]][0]).all()
        assert (want["state"][6] == ABSENT).all() and (want["zmom"][0, 8, 2] == 0.0)
        assert (want["state"][20] != VALUE).all() and want["state"][20, 0] == NULL
        if method != "max_icir":
            assert (want["status"][H + M - 1:] == 0).all() and (want["state"][8] == VALUE).sum() > 100
        else:
            assert set(want["status"].tolist()) == {0, 1} and np.nanmax(want["cond"]) < COND_MAX
        _check(_run(dev, x, xs, y, ys, method, ic=ic, **KW), want, f"degenerate {method} {ic}")
    # a duplicated factor: singular without shrinkage (status 2), fine with it; a constant IC series
    x, xs, y, ys = ref.make_panel(8, 4, D, 120, h=H, holes=False)
    x[3] = x[0]
    kw = dict(future_days=H, window=12, min_periods=5, ic=ic)
    w0 = ref.combine(x, xs, y, ys, "max_icir", shrink=0.0, **kw)
    w5 = ref.combine(x, xs, y, ys, "max_icir", shrink=0.5, **kw)
    assert (w0["status"][H + 4:] == 2).all() and (w5["status"][H + 4:] == 0).all() and np.nanmax(w5["cond"]) < COND_MAX
    _check(_run(dev, x, xs, y, ys, "max_icir", shrink=0.0, **kw), w0, f"duplicate, shrink 0 {ic}")
    _check(_run(dev, x, xs, y, ys, "max_icir", shrink=0.5, **kw), w5, f"duplicate, shrink 0.5 {ic}")
    _check(_run(dev, x, xs, y, ys, "max_icir", shrink=1.0, **kw),
           ref.combine(x, xs, y, ys, "max_icir", shrink=1.0, **kw), f"duplicate, shrink 1 {ic}")


@pytest.mark.gpu
def test_min_obs_and_min_factors(dev):
    x, xs, y, ys = ref.make_panel(51, 5, D, 257, h=H)
    xs[1:, :, 40:60] = NULL                                    # twenty stocks hold one factor only
    n = ref.combine(x, xs, y, ys, "icir", **KW)["n_pairs"]
    cut = int(np.median(n[:, :D - H]))
    for kw in (dict(min_obs=cut), dict(min_factors=2), dict(min_factors=5)):
        want = ref.combine(x, xs, y, ys, "icir", **KW, **kw)
        _check(_run(dev, x, xs, y, ys, "icir", **KW, **kw), want, f"icir {kw}")
        if "min_obs" in kw:
            assert np.isnan(want["ic"][:, :D - H]).any() and np.isfinite(want["ic"]).any()
        else:
            assert (want["state"][H + M - 1:, 40:60] == NULL).all() and (want["state"] == VALUE).any()


@pytest.mark.gpu
@pytest.mark.parametrize("method", METHODS[1:])
def test_no_look_ahead(dev, method):
    """Everything after date d0 - h perturbed: the weights up to d0 keep their bits."""
    x, xs, y, ys = ref.make_panel(61, 6, D, 257, h=H)
    d0 = 21
    base = _run(dev, x, xs, y, ys, method, **KW)
    rng = np.random.default_rng(5)
    q, r = x.copy(), y.copy()
    q[:, d0 - H + 1:] += rng.standard_normal(q[:, d0 - H + 1:].shape)
    r[d0 - H + 1:] = rng.standard_normal(r[d0 - H + 1:].shape)
    got = _run(dev, q, xs, r, ys, method, **KW)
    assert (base["status"][H + M - 1:] == 0).all()
    assert np.array_equal(got["weights"][:d0 + 1].view(np.int64), base["weights"][:d0 + 1].view(np.int64))
    assert np.array_equal(got["count"][:d0 + 1], base["count"][:d0 + 1])
    assert np.array_equal(got["status"][:d0 + 1], base["status"][:d0 + 1])
    assert np.array_equal(got["ic"][:, :d0 - H + 1].view(np.int64), base["ic"][:, :d0 - H + 1].view(np.int64))
    assert np.array_equal(got["val"][:d0 - H + 1].view(np.int64), base["val"][:d0 - H + 1].view(np.int64))
    assert not np.array_equal(got["weights"][d0 + 1:], base["weights"][d0 + 1:])


@pytest.mark.gpu
@pytest.mark.parametrize("method", METHODS)
def test_scale_invariance(dev, method):
    """A factor times 1e8 changes nothing within tolerance; times -3 flips that factor's weight
    (and IC) and leaves the composite alone -- for the IC-driven methods: equal weights do not
    know a factor's sign, so 'equal' gets the 1e8 only."""
    K = 6
    x, xs, y, ys = ref.make_panel(71, K, D, 257, h=H)
    want = ref.combine(x, xs, y, ys, method, **KW)
    _precheck(want, xs, method, f"scale {method}")
    base = _run(dev, x, xs, y, ys, method, **KW)
    _check(base, want, f"scale base {method}")
    q = x.copy()
    q[1] = 1e8 * x[1]
    sign = np.ones(K)
    if method != "equal":                                      # (equal weights do not know a factor's sign)
        q[4] = -3.0 * x[4]
        sign[4] = -1.0
    got = _run(dev, q, xs, y, ys, method, **KW)
    for k in INTS + ("state",):
        assert np.array_equal(got[k], base[k]), k
    worst = max(np.nanmax(np.abs(got["weights"] * sign - base["weights"])), np.abs(got["val"] - base["val"]).max())
    print(f"scaling {method}: worst abs err {worst:.3e}")
    np.testing.assert_allclose(got["weights"] * sign, base["weights"], equal_nan=True, **TOL)
    np.testing.assert_allclose(got["ic"] * sign[:, None], base["ic"], equal_nan=True, **TOL)
    np.testing.assert_allclose(got["val"], base["val"], **TOL)


@pytest.mark.gpu
def test_rank_ic_sees_the_order_only(dev):
    """exp of a factor: the rank IC keeps its bits (so do the weights), in one batch and in
    day batches of the ranked planes."""
    from mff import engine
    x, xs, y, ys = ref.make_panel(81, 4, D, 257, h=H)
    base = _run(dev, x, xs, y, ys, "icir", ic="rank", **KW)
    q = x.copy()
    with np.errstate(over="ignore"):
        q[2] = np.exp(x[2])
    got = _run(dev, q, xs, y, ys, "icir", ic="rank", **KW)
    assert np.isfinite(base["ic"][:, :D - H]).all()
    for k in ("ic", "weights"):
        assert np.array_equal(got[k].view(np.int64), base[k].view(np.int64)), k
    keep = engine.COMBINE_RANK_BYTES
    try:
        engine.COMBINE_RANK_BYTES = 7 * 2 * 4 * 257 * 9          # seven days a batch
        batched = _run(dev, x, xs, y, ys, "icir", ic="rank", **KW)
    finally:
        engine.COMBINE_RANK_BYTES = keep
    for k in base:
        assert np.array_equal(batched[k].view(np.uint8), base[k].view(np.uint8)), k


@pytest.mark.gpu
@pytest.mark.parametrize("method", METHODS)
def test_bit_identical_runs(dev, method):
    x, xs, y, ys = ref.make_panel(91, 58, D, 1025, h=H)
    for ic in ref.IC_KINDS if method == "icir" else ("pearson",):
        a, b = (_run(dev, x, xs, y, ys, method, ic=ic, **KW) for _ in range(2))
        for k in a:
            assert np.array_equal(a[k].view(np.uint8), b[k].view(np.uint8)), k
        assert (a["status"][H + M - 1:] == 0).all() and (a["state"] == VALUE).mean() > 0.8


@pytest.mark.gpu
@pytest.mark.parametrize("S", [29, 257, 1301])
@pytest.mark.parametrize("R", [2, 3])
def test_stock_shards_match_one_rank(dev, R, S):
    from mff import dist
    x, xs, y, ys = ref.make_panel(400 + R + S, 3, D, S, h=H)
    bounds = [dist.shard_bounds(S, R, r) for r in range(R)]
    assert len({b - a for a, b in bounds}) == 2               # uneven shards
    for method, ic in (("equal", "pearson"), ("ic", "pearson"), ("icir", "rank"), ("max_icir", "pearson")):
        want = ref.combine(x, xs, y, ys, method, ic=ic, **KW)
        _precheck(want, xs, method, f"shards {method}")
        one = _run(dev, x, xs, y, ys, method, ic=ic, **KW)
        _check(one, want, f"one rank S={S} {method} {ic}")

        def rank_fn(comm):
            a, b = bounds[comm.rank]
            return _run(dev, x[..., a:b], xs[..., a:b], y[..., a:b], ys[..., a:b], method, ic=ic, comm=comm,
                        stocks_total=S, **KW)

        for r, got in enumerate(dist.run_threads(R, rank_fn)):
            a, b = bounds[r]
            _check(got, dict(one, val=one["val"][..., a:b], state=one["state"][..., a:b]),
                   f"rank {r} of {R}, S={S} {method} {ic}")


def _run_c_abi(dev, x, xs, y, ys, method, fill, shrink=0.5):
    """The four C calls with every output and intermediate buffer holding `fill` beforehand."""
    from mff import _lib
    lib = _lib.load()
    K, D_, S = x.shape
    f64, i32 = torch.float64, torch.int32
    xv, xst, yv, yst = _t(x, dev), _t(xs, dev), _t(y, dev), _t(ys, dev)
    full = lambda shape: torch.full(shape, fill, dtype=f64, device=dev)
    ifull = lambda shape: torch.full(shape, -77, dtype=i32, device=dev)
    part, zmom, ic, w, ov = full((K, D_, 9)), full((K, D_, 3)), full((K, D_)), full((D_, K)), full((D_, S))
    npairs, count, status = ifull((K, D_)), ifull((D_, K)), ifull((D_,))
    os_ = torch.full((D_, S), 9, dtype=torch.uint8, device=dev)
    P = lambda t_: t_.data_ptr()
    _lib.check(lib.mff_xs_comb_moments(P(xv), P(xst), K, D_, S, P(yv), P(yst), 1, P(part), None), "moments")
    _lib.check(lib.mff_xs_comb_finalize(P(part), 1, K, D_, 0, P(zmom), P(ic), P(npairs), None), "finalize")
    _lib.check(lib.mff_xs_comb_weights(P(ic), K, D_, METHODS.index(method), H, W, M, shrink, P(w), P(count), P(status),
                                       None), "weights")
    _lib.check(lib.mff_xs_comb_apply(P(xv), P(xst), K, D_, S, P(zmom), P(w), P(status), 1, P(ov), P(os_), None), "apply")
    torch.cuda.synchronize()
    return dict(val=ov.cpu().numpy(), state=os_.cpu().numpy(), weights=w.cpu().numpy(), ic=ic.cpu().numpy(),
                n_pairs=npairs.cpu().numpy(), count=count.cpu().numpy(), status=status.cpu().numpy())


@pytest.mark.gpu
@pytest.mark.parametrize("method", METHODS)
def test_c_abi_on_poisoned_buffers(dev, method):
    """K = 64 fills every lane of the weights kernel; nothing stale may reach the result."""
    x, xs, y, ys = ref.make_panel(164, 64, D, 257, h=H)
    want = ref.combine(x, xs, y, ys, method, **KW)
    _precheck(want, xs, method, f"poisoned {method}")
    runs = [_run_c_abi(dev, x, xs, y, ys, method, fill) for fill in (float("nan"), -1e300)]
    for got, name in zip(runs, ("NaN", "-1e300")):
        _check(got, want, f"K=64, buffers of {name}, {method}")
    for k in runs[0]:
        assert np.array_equal(runs[0][k].view(np.uint8), runs[1][k].view(np.uint8)), k
    eng = _run(dev, x, xs, y, ys, method, **KW)
    for k in eng:
        assert np.array_equal(eng[k].view(np.uint8), runs[0][k].view(np.uint8)), k


@pytest.mark.gpu
def test_errors_write_nothing(dev):
    from mff import _lib, engine
    lib = _lib.load()
    buf = torch.full((8192,), 7.0, dtype=torch.float64, device=dev)
    ib = torch.full((4096,), 9, dtype=torch.int32, device=dev)
    K, D_, S = 2, 1, 8
    xv = torch.zeros((K, D_, S), dtype=torch.float64, device=dev)
    xs = torch.full((K, D_, S), VALUE, dtype=torch.uint8, device=dev)
    os_ = torch.full((D_, S), 5, dtype=torch.uint8, device=dev)
    p, q, X, XS, OS = buf.data_ptr(), ib.data_ptr(), xv.data_ptr(), xs.data_ptr(), os_.data_ptr()
    for K_, D2, S_, Ky, Y in ((0, D_, S, 1, X), (65, D_, S, 1, X), (K, -1, S, 1, X), (K, D_, -1, 1, X), (K, D_, S, 3, X),
                              (K, D_, S, 0, X), (K, D_, S, 1, None), (K, D_, S, 2, None)):
        assert lib.mff_xs_comb_moments(X, XS, K_, D2, S_, Y, None if Y is None else XS, Ky, p, None) < 0
        assert lib.mff_last_error()
    for R_, K_, D2, mo in ((0, K, D_, 0), (1, 0, D_, 0), (1, 65, D_, 0), (1, K, -1, 0), (1, K, D_, -1)):
        assert lib.mff_xs_comb_finalize(p, R_, K_, D2, mo, p, p, q, None) < 0
    for K_, D2, me, h, w, m, sh in ((0, D_, 1, 1, 5, 2, 0.5), (65, D_, 1, 1, 5, 2, 0.5), (K, -1, 1, 1, 5, 2, 0.5),
                                    (K, D_, 4, 1, 5, 2, 0.5), (K, D_, -1, 1, 5, 2, 0.5), (K, D_, 1, 0, 5, 2, 0.5),
                                    (K, D_, 1, 1, 0, 2, 0.5), (K, D_, 1, 1, 5, 0, 0.5), (K, D_, 3, 1, 5, 2, 1.5),
                                    (K, D_, 3, 1, 5, 2, -0.1), (K, D_, 3, 1, 5, 2, float("nan"))):
        assert lib.mff_xs_comb_weights(p, K_, D2, me, h, w, m, sh, p, q, q, None) < 0
    assert b"shrink" in lib.mff_last_error()
    for K_, D2, S_, mf in ((0, D_, S, 1), (65, D_, S, 1), (K, -1, S, 1), (K, D_, -1, 1), (K, D_, S, 0), (K, D_, S, 3)):
        assert lib.mff_xs_comb_apply(X, XS, K_, D2, S_, p, p, q, mf, p, OS, None) < 0
    assert b"min_factors=3" in lib.mff_last_error()
    torch.cuda.synchronize()
    assert bool((buf == 7.0).all()) and bool((ib == 9).all()) and bool((os_ == 5).all())
    yv, ys = torch.zeros((D_, S), dtype=torch.float64, device=dev), torch.full((D_, S), VALUE, dtype=torch.uint8, device=dev)
    for kw, word in ((dict(method="pca"), "method must be one of"), (dict(ic="kendall"), "ic must be one of"),
                     (dict(future_days=0), "future_days"), (dict(window=0), "window"), (dict(min_periods=0), "min_periods"),
                     (dict(shrink=1.5), "shrink"), (dict(min_obs=-1), "min_obs"), (dict(min_factors=0), "min_factors"),
                     (dict(min_factors=3), "min_factors"), (dict(window=2.5), "window")):
        with pytest.raises(ValueError, match=word):
            engine.factor_combine(xv, xs, yv, ys, **kw)
    with pytest.raises(ValueError, match="needs the forward return"):
        engine.factor_combine(xv, xs, method="icir")
    with pytest.raises(_lib.MffError):
        engine.factor_combine(torch.zeros((65, 1, 8), dtype=torch.float64, device=dev),
                              torch.zeros((65, 1, 8), dtype=torch.uint8, device=dev), method="equal")


@pytest.mark.gpu
def test_empty_day_and_stock_axes(dev):
    from mff import _lib, engine
    lib = _lib.load()
    z = lambda shape, dtype: torch.zeros(shape, dtype=dtype, device=dev)
    for method in METHODS:
        for ic in ref.IC_KINDS:
            r = engine.factor_combine(z((3, 0, 5), torch.float64), z((3, 0, 5), torch.uint8), z((0, 5), torch.float64),
                                      z((0, 5), torch.uint8), method=method, ic=ic)
            assert tuple(r.val.shape) == (0, 5) and tuple(r.weights.shape) == (0, 3) and tuple(r.ic.shape) == (3, 0)
            r = engine.factor_combine(z((3, 4, 0), torch.float64), z((3, 4, 0), torch.uint8), z((4, 0), torch.float64),
                                      z((4, 0), torch.uint8), method=method, ic=ic, **KW)
            torch.cuda.synchronize()
            assert tuple(r.val.shape) == (4, 0) and tuple(r.state.shape) == (4, 0)
            assert bool(torch.isnan(r.ic).all()) and r.n_pairs.tolist() == [[0] * 4] * 3
            if method == "equal":
                assert r.status.tolist() == [0] * 4 and bool((r.weights == 1.0 / 3).all())
            else:
                assert r.status.tolist() == [1] * 4 and bool(torch.isnan(r.weights).all())
    buf = torch.full((8192,), 7.0, dtype=torch.float64, device=dev)
    ib = torch.full((4096,), 9, dtype=torch.int32, device=dev)
    p, q = buf.data_ptr(), ib.data_ptr()
    assert lib.mff_xs_comb_moments(None, None, 2, 0, 5, None, None, 0, p, None) == 0
    assert lib.mff_xs_comb_finalize(p, 1, 2, 0, 0, p, p, q, None) == 0
    assert lib.mff_xs_comb_weights(None, 2, 0, 0, 1, 5, 2, 0.5, p, q, q, None) == 0
    assert lib.mff_xs_comb_apply(None, None, 2, 0, 5, p, p, q, 1, p, p, None) == 0
    assert lib.mff_xs_comb_apply(None, None, 2, 3, 0, p, p, q, 1, p, p, None) == 0
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
def test_combine_surface(dev):
    import mff
    import pandas as pd
    from mff import engine, frames
    from mff.factor import Factor, MinFreqFactor, combine
    assert mff.combine is combine
    rng = np.random.default_rng(9)
    D_, S = 30, 60
    codes = [f"{i:06d}.SZ" for i in range(S)]
    dates = [dt.date(2024, 3, 1) + dt.timedelta(days=i) for i in range(D_)]
    specs = {"alpha": (slice(0, D_), slice(0, 52)), "beta": (slice(1, D_), slice(6, S)),
             "gamma": (slice(0, D_ - 1), slice(0, S)), "delta": (slice(0, D_), slice(3, S))}
    K = len(specs)
    own = rng.standard_normal((K, D_, S))
    x = 0.5 * rng.standard_normal((D_, S))[None] + np.sqrt(0.75) * own
    pct = 0.01 * (0.3 * own.sum(axis=0) + rng.standard_normal((D_, S)))
    pct = np.roll(pct, 1, axis=0)                              # tomorrow's return follows today's exposure
    xs = np.full((K, D_, S), ABSENT, np.uint8)
    fs = []
    for k, (nm, (ds, ss)) in enumerate(specs.items()):
        xs[k][ds, ss] = VALUE
        xs[k, 2, 10 + k] = NULL
        x[k, 3, 12 + k] = np.nan
        cls = MinFreqFactor if nm == "beta" else Factor
        fs.append(cls(nm, frames.to_long(x[k], xs[k], codes, dates, nm)))
    x = np.where(xs == VALUE, x, 0.0)
    names = list(specs)
    ps = np.full((D_, S), VALUE, np.uint8)
    ps[5, 7] = NULL
    pv = frames.to_long(pct, ps, codes, dates, "pct_change")
    before = [(f.factor_exposure, f.factor_exposure.copy()) for f in fs]
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    fv, fst = engine.future_return(t(np.where(ps == VALUE, pct, 0.0)), t(ps), 1)
    y, ys = fv.cpu().numpy(), fst.cpu().numpy()
    kw = dict(future_days=1, window=6, min_periods=3)
    for method in METHODS:
        for ic in ref.IC_KINDS:
            eq = method == "equal"                                # reads no pv_data: every IC is NaN
            want = ref.combine(x, xs, None if eq else y, None if eq else ys, method, ic=ic, **kw)
            first = 4 if method == "max_icir" else 3              # (beta starts a date late: the listwise window)
            assert (want["status"][first:] == 0).all() and (want["state"] == VALUE).mean() > 0.8
            out, wf, icf = combine(fs, method=method, ic=ic, return_info=True, pv_data=pv, device=dev, name="combo", **kw)
            assert type(out) is Factor and out.factor_name == "combo"
            assert list(out.factor_exposure.columns) == ["code", "date", "combo"]
            ref_frame = frames.to_long(want["val"], want["state"], codes, dates, "combo")
            assert list(out.factor_exposure["code"]) == list(ref_frame["code"])
            assert list(out.factor_exposure["date"]) == list(ref_frame["date"])
            v, s, _, _ = frames.from_long(out.factor_exposure, "combo", codes=codes, dates=dates)
            assert np.array_equal(s, want["state"])
            print(f"surface {method} {ic}: worst abs err {np.abs(v - want['val']).max():.3e}")
            np.testing.assert_allclose(v, want["val"], **TOL)
            assert list(wf.columns) == ["date", "status"] + names and list(wf["date"]) == dates
            assert np.array_equal(wf["status"], want["status"])
            np.testing.assert_allclose(wf[names].to_numpy(), want["weights"], equal_nan=True, **TOL)
            assert list(icf.columns) == ["date"] + names and list(icf["date"]) == dates
            np.testing.assert_allclose(icf[names].to_numpy(), want["ic"].T, equal_nan=True, **TOL)
    for f, (obj, copy) in zip(fs, before):                        # the inputs are untouched
        assert f.factor_exposure is obj and _same_frame(obj, copy, f.factor_name, codes, dates)
    # the plain form, the mapping form, combine_with, 'equal' without pv_data, errors
    plain = combine(fs, pv_data=pv, device=dev, **kw)
    assert isinstance(plain, Factor) and plain.factor_name == "composite"
    mp = combine({"u": fs[0], "v": fs[1]}, pv_data=pv, device=dev, return_info=True, **kw)
    assert list(mp[1].columns) == ["date", "status", "u", "v"] and list(mp[2].columns) == ["date", "u", "v"]
    cw = fs[0].combine_with(fs[1:], pv_data=pv, device=dev, **kw)
    assert _same_frame(cw.factor_exposure, plain.factor_exposure, "composite", codes, dates)
    cm = fs[0].combine_with({"beta": fs[1], "gamma": fs[2], "delta": fs[3]}, pv_data=pv, device=dev, **kw)
    assert _same_frame(cm.factor_exposure, plain.factor_exposure, "composite", codes, dates)
    eq = combine(fs, method="equal", device=dev)                  # reads no pv_data
    v, s, _, _ = frames.from_long(eq.factor_exposure, "composite", codes=codes, dates=dates)
    we = ref.combine(x, xs, None, None, "equal")
    assert np.array_equal(s, we["state"])
    np.testing.assert_allclose(v, we["val"], **TOL)
    # the composite goes through ic_test
    df = plain.ic_test(future_days=1, plot_out=False, return_df=True, pv_data=pv, device=dev)
    assert isinstance(df, pd.DataFrame) and len(df) > 15 and np.isfinite(plain.IC) and plain.IC > 0.05
    with pytest.raises(ValueError, match="duplicate"):
        combine([fs[0], fs[0]], pv_data=pv, device=dev)
    with pytest.raises(ValueError, match="duplicate"):
        fs[0].combine_with({"alpha": fs[1]}, pv_data=pv, device=dev)
    for bad, word in ((dict(method="pca"), "method must be one of"), (dict(ic="kendall"), "ic must be one of"),
                      (dict(window=0), "window must be an integer >= 1"), (dict(shrink=2), "shrink must be a number in"),
                      (dict(min_factors=5), "min_factors"), (dict(future_days=0), "future_days"), (dict(name=""), "name")):
        with pytest.raises(ValueError, match=word):
            combine(fs, pv_data=pv, device=dev, **bad)
    with pytest.raises(ValueError, match="pv_data has no column"):
        combine(fs, pv_data=pv.rename(columns={"pct_change": "ret"}), device=dev)
