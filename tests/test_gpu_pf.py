"""Daily group portfolios on the GPU (csrc/mff_pf.hip, engine.group_portfolios,
mff.portfolio_tests) against tests/pf_ref.py.

Bounds.  Every summed term is positive (pct > -1, weights in [1, 5]), so a sum of n terms has a
relative error of at most (n - 1) 2^-53 in ANY order: the kernels' order (the stocks j, j + J, ...
of a tile per bin, tiles in order, the J bins in order, ranks in order) and the reference's
(numpy's pairwise sums) each stay inside it.  The growth c(d) and the term u c(d) are the same
IEEE operations in the same order on both sides: bit-identical.  With
beta = (n + L + 4) 2^-52 (n members, L dates of the period):
  V = A / U: two sums and a division on each side                    -> |V - ref| <= beta V
  ret = V(d) / V(d-) - 1: two such V, a division, a subtraction      -> <= 2 beta (1 + |ref|)
  traded = sum |t - b|: sum t <= 1 with U inside beta(p), sum b <= 1 with A_end inside
  beta(p - 1), and a sum of at most m terms that total at most 2     -> <= 2 beta + (m + 1) 2^-52,
  beta the larger of the two periods', m the stocks in either membership.
  compounded over a period, prod (1 + ret) - 1 adds at most three roundings per date (the
  division, the -1, the +1 of the product), 1.5 L 2^-52, to the sums' n 2^-52 and to
  engine.group_returns' own n 2^-52: inside 2 beta (1 + |ref|) as well.
The group plane of both sides is mff_bt_qcut's (unchanged here, pinned bin for bin against pandas
in test_gpu_backtest_shapes.py)."""
import datetime as dt
import functools

import numpy as np
import pytest

import pf_ref as ref
from pf_ref import ABSENT, NULLV, VALUE

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -52
LENS = [1, 3, 70, 2, 5]     # a one-date period; one longer than any 64-date tile
D81 = sum(LENS)
PERIOD81 = np.repeat(np.arange(len(LENS)), LENS).astype(np.int32)


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def _t(a, dev):
    return torch.from_numpy(np.array(a, order="C")).to(dev)


def _ro(*arrays):
    for a in arrays:
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return arrays


def _st(dev):
    return torch.cuda.current_stream(dev).cuda_stream


# --------------------------------------------------------------------------- inputs
@functools.lru_cache(maxsize=None)
def _panel(S, D, K, seed=0):
    """Suspension runs, about 1 % null pct, NaN / null exposures, rows that differ between the
    factors; pct > -1 and weights in [1, 5].  With S >= 8: stock 7 is absent on dates 1..3 (the
    whole of period 1 of LENS), stock 5 on dates 74..75 (the whole of period 3), stock 3 on 5..8."""
    rng = np.random.default_rng(7000 + 31 * S + D + seed)
    pct = np.clip(rng.normal(0, 0.02, (D, S)), -0.9, None)
    ps = np.full((D, S), VALUE, np.uint8)
    if S >= 8 and D >= 76:
        ps[1:4, 7] = ABSENT
        ps[74:76, 5] = ABSENT
        ps[5:9, 3] = ABSENT
    ps[(rng.random((D, S)) < 0.01) & (ps != ABSENT)] = NULLV
    x = np.round(rng.normal(size=(K, D, S)), 2)
    xs = np.repeat(ps[None], K, axis=0)
    x[rng.random((K, D, S)) < 0.02] = np.nan
    xs[(rng.random((K, D, S)) < 0.02) & (xs != ABSENT)] = NULLV
    xs[(rng.random((K, D, S)) < 0.01)] = ABSENT     # the factors' rows differ
    w = rng.uniform(1, 5, (D, S))
    wst = ps.copy()
    wst[(rng.random((D, S)) < 0.05) & (ps != ABSENT)] = NULLV
    return _ro(x, xs, pct, ps, w, wst)


_DEV = {}


def _bins(x, xs, G):
    """mff_bt_qcut per factor on [K][D][S] -> int8 [K][D][S] (numpy)."""
    from mff import _lib
    lib = _lib.load()
    dev = _DEV["dev"]
    K, D, S = x.shape
    out = np.empty((K, D, S), np.int8)
    ws = torch.empty(lib.mff_bt_qcut_workspace_bytes(D, S, 1), dtype=torch.uint8, device=dev)
    for k in range(K):
        xv, xst = _t(x[k], dev), _t(xs[k], dev)
        grp = torch.empty((D, S), dtype=torch.int8, device=dev)
        _lib.check(lib.mff_bt_qcut(_lib.ptr(xv), _lib.ptr(xst), D, S, _lib.ptr(xv), _lib.ptr(xst), 1, S, G,
                                   _lib.ptr(grp), _lib.ptr(ws), _st(dev)), "mff_bt_qcut")
        torch.cuda.synchronize()
        out[k] = grp.cpu().numpy()
    return out


@functools.lru_cache(maxsize=None)
def _case(S, G, weighted, D=D81, K=3, weekly=False):
    """(inputs, the group planes, the reference per factor), computed once."""
    x, xs, pct, ps, w, wst = _panel(S, D, K)
    period_of = (np.arange(D) // 5).astype(np.int32) if weekly else PERIOD81[:D]
    P = int(period_of[-1]) + 1
    group = _bins(x, xs, G)
    wa = (w, wst) if weighted else (None, None)
    refs = tuple(ref.portfolios(group[k].astype(np.int64), xs[k], pct, ps, period_of, P, G, *wa) for k in range(K))
    return _ro(x, xs, pct, ps, w, wst, period_of, group) + (P, refs)


def _beta(r, period_of):
    """beta [P][G] of a reference result."""
    L = np.bincount(period_of, minlength=r.count.shape[0])
    return (r.count + L[:, None] + 4) * EPS


# --------------------------------------------------------------------------- the kernels, direct
def _poison(shape, dtype, dev, byte=0xFF):
    n = int(np.prod(shape)) * torch.empty((), dtype=dtype).element_size()
    return torch.full((max(n, 1),), byte, dtype=torch.uint8, device=dev)[:n].view(dtype).reshape(shape)


def _raw(dev, group, xs, pct, ps, period_of, P, G, w=None, wst=None):
    """The five entry points on one rank over poisoned outputs (0xFF bytes: a NaN, or -1; the
    int8 membership plane, where -1 is a value, gets 0x55) -> numpy dict."""
    from mff import _lib
    lib = _lib.load()
    K, D, S = xs.shape
    st = _st(dev)
    f64 = torch.float64
    g_d, xs_d, pct_d, ps_d, per_d = (_t(a, dev) for a in (group, xs, pct, ps, period_of))
    w_d = wst_d = None
    if w is not None:
        w_d, wst_d = _t(w, dev), _t(wst, dev)
    m = _poison((K, P, S), torch.int8, dev, 0x55)
    u, cend = _poison((K, P, S), f64, dev), _poison((K, P, S), f64, dev)
    a, nu = _poison((K, D, G), f64, dev), _poison((K, P, G, 2), f64, dev)
    ret, count = _poison((K, D, G), f64, dev), _poison((K, P, G), torch.int32, dev)
    tot, part, traded = _poison((K, P, G, 2), f64, dev), _poison((K, P, G), f64, dev), _poison((K, P, G), f64, dev)
    p = _lib.ptr
    _lib.check(lib.mff_pf_signal(p(xs_d), p(g_d), p(pct_d), p(ps_d), p(w_d), p(wst_d), p(per_d), K, D, S, P,
                                 p(m), p(u), p(cend), st), "mff_pf_signal")
    _lib.check(lib.mff_pf_sums(p(xs_d), p(pct_d), p(ps_d), p(per_d), p(m), p(u), K, D, S, P, G, p(a), p(nu), st),
               "mff_pf_sums")
    _lib.check(lib.mff_pf_finalize(p(a), p(nu), p(per_d), 1, K, D, P, G, p(ret), p(count), p(tot), st),
               "mff_pf_finalize")
    _lib.check(lib.mff_pf_traded(p(m), p(u), p(cend), p(tot), K, P, S, G, p(part), st), "mff_pf_traded")
    _lib.check(lib.mff_pf_traded_finalize(p(part), 1, K, P, G, p(traded), st), "mff_pf_traded_finalize")
    torch.cuda.synchronize()
    out = dict(m=m, u=u, cend=cend, a=a, nu=nu, ret=ret, count=count, tot=tot, part=part, traded=traded)
    return {k: v.cpu().numpy() for k, v in out.items()}


def _assert_written(o):
    """No output element keeps its poison."""
    assert (o["m"] != 0x55).all()
    assert (o["count"] != -1).all()
    for k in ("u", "cend", "a", "nu", "ret", "tot", "part", "traded"):
        assert (o[k].view(np.int64) != -1).all(), k


def _bt_periods(dev, group, xs, pct, ps, period_of, P, w=None, wst=None):
    """mff_bt_periods of one factor -> (p_ret, p_group)."""
    from mff import _lib
    lib = _lib.load()
    D, S = xs.shape
    g_d, xs_d, pct_d, ps_d, per_d = (_t(a, dev) for a in (group, xs, pct, ps, period_of))
    w_d, wst_d = (None, None) if w is None else (_t(w, dev), _t(wst, dev))
    pr = torch.empty((P, S), dtype=torch.float64, device=dev)
    pg = torch.empty((P, S), dtype=torch.int8, device=dev)
    pw = torch.empty((P, S), dtype=torch.float64, device=dev)
    pws = torch.empty((P, S), dtype=torch.uint8, device=dev)
    _lib.check(lib.mff_bt_periods(_lib.ptr(xs_d), _lib.ptr(g_d), _lib.ptr(pct_d), _lib.ptr(ps_d), _lib.ptr(w_d),
                                  _lib.ptr(wst_d), _lib.ptr(per_d), D, S, P, _lib.ptr(pr), _lib.ptr(pg),
                                  _lib.ptr(pw), _lib.ptr(pws), _st(dev)), "mff_bt_periods")
    torch.cuda.synchronize()
    return pr.cpu().numpy(), pg.cpu().numpy()


def _compare(ret, count, traded, r, period_of, what=""):
    """ret [D][G], count, traded [P][G] of one factor against the reference r, inside the bounds
    of the module docstring; NaN exactly where the reference has NaN."""
    beta = _beta(r, period_of)
    assert np.array_equal(count, r.count), what
    assert np.array_equal(np.isnan(ret), np.isnan(r.ret)), what
    ok = ~np.isnan(r.ret)
    err = np.abs(ret - r.ret)
    tol = 2.0 * beta[period_of] * (1.0 + np.abs(r.ret))
    assert (err[ok] <= tol[ok]).all(), (what, float((err[ok] / tol[ok]).max()))
    assert np.array_equal(np.isnan(traded), np.isnan(r.traded)), what
    bt = beta.copy()
    bt[1:] = np.maximum(beta[1:], beta[:-1])
    tol = 2.0 * bt + (r.union + 1) * EPS
    ok = ~np.isnan(r.traded)
    err = np.abs(traded - r.traded)
    assert (err[ok] <= tol[ok]).all(), (what, float((err[ok] / tol[ok]).max()))
    assert (traded[0] == 0).all()


@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("K", [1, 3])
@pytest.mark.parametrize("G", [1, 5, 63])
@pytest.mark.parametrize("S", [1, 63, 64, 65, 257])
def test_kernels_against_the_reference(dev, S, G, K, weighted):
    """Stock tiles of one thread, one short of a wave, a wave, one more, two tiles of 256 with a
    remainder of one; the 70-date period takes several 16-date tiles and, with G = 63, several
    chunks of the LDS bins (the re-walk of the earlier dates); J = 16 bins per group (G = 1, 5)
    and J = 2 (G = 63)."""
    _DEV["dev"] = dev
    x, xs, pct, ps, w, wst, period_of, group, P, refs = _case(S, G, weighted)
    wa = (w, wst) if weighted else (None, None)
    if G == 5 and S >= 63:   # at least half of the (period >= 1, group) cells hold stocks
        for r in refs[:K]:
            assert 2 * int((r.count[1:] > 0).sum()) >= (P - 1) * G
    o = _raw(dev, group[:K], xs[:K], pct, ps, period_of, P, G, *wa)
    _assert_written(o)
    for k in range(K):
        r = refs[k]
        assert np.array_equal(o["m"][k], r.sig.m) and np.array_equal(o["u"][k], r.sig.u)
        assert np.array_equal(o["cend"][k], r.sig.cend)
        # the merged path's numbers, bit for bit
        p_ret, p_group = _bt_periods(dev, group[k], xs[k], pct, ps, period_of, P, *wa)
        assert np.array_equal(o["m"][k], p_group) and np.array_equal(o["cend"][k] - 1.0, p_ret)
        U = o["tot"][k, :, :, 0]
        assert np.array_equal(o["nu"][k, :, :, 0], r.count) and np.array_equal(U > 0, r.U > 0)
        V = np.where(U[period_of] > 0, o["a"][k] / np.where(U > 0, U, 1.0)[period_of], 1.0)
        beta = _beta(r, period_of)[period_of]
        assert (np.abs(V - r.V) <= beta * r.V).all(), float((np.abs(V - r.V) / (beta * r.V)).max())
        _compare(o["ret"][k], o["count"][k], o["traded"][k], r, period_of, (S, G, K, weighted, k))


@pytest.mark.parametrize("D,P", [(10, 1), (1, 1)])
def test_one_period_holds_nothing(dev, D, P):
    """P = 1: no stock has an earlier signal, so nothing is ever held; D = 1."""
    _DEV["dev"] = dev
    x, xs, pct, ps, w, wst = _panel(65, D, 2, seed=1)
    period_of = np.zeros(D, np.int32)
    group = _bins(x, xs, 5)
    o = _raw(dev, group, xs, pct, ps, period_of, P, 5, w, wst)
    _assert_written(o)
    assert (o["m"] == -1).all() and (o["u"] == 0).all()
    assert (o["ret"] == 0).all() and (o["count"] == 0).all() and (o["traded"] == 0).all() and (o["a"] == 0).all()
    for k in range(2):
        r = ref.portfolios(group[k].astype(np.int64), xs[k], pct, ps, period_of, P, 5, w, wst)
        assert np.array_equal(o["cend"][k], r.sig.cend) and np.array_equal(o["ret"][k], r.ret)


def test_two_runs_are_bit_identical(dev):
    """Two runs over poisoned outputs: the same bits in every output, every element written."""
    _DEV["dev"] = dev
    x, xs, pct, ps, w, wst, period_of, group, P, refs = _case(257, 5, True)
    a = _raw(dev, group, xs, pct, ps, period_of, P, 5, w, wst)
    b = _raw(dev, group, xs, pct, ps, period_of, P, 5, w, wst)
    _assert_written(a)
    for k in a:
        assert a[k].tobytes() == b[k].tobytes(), k


# --------------------------------------------------------------------------- edge semantics
def test_hand_case_is_exact(dev):
    """The dyadic case of test_pf.py (a stock absent for a whole period, a null pct on a row, a
    null-group signal): every sum is exact in any order, so the kernels give the written numbers."""
    from test_pf import _hand
    group, xs, pct, ps, period_of = _hand()
    o = _raw(dev, group[None].astype(np.int8), xs[None], pct, ps, period_of.astype(np.int32), 3, 2)
    _assert_written(o)
    assert o["m"][0].tolist() == [[-1, -1, -1, -1], [0, 1, -1, -1], [1, 1, 0, 0]]
    assert o["ret"][0].tolist() == [[0, 0], [0, 0], [0.5, 0.0], [0.25, 0.25], [0.0, 0.5]]
    assert o["count"][0].tolist() == [[0, 0], [1, 1], [2, 2]]
    assert o["traded"][0].tolist() == [[0, 0], [1, 1], [2, 1]]
    assert o["tot"][0].tolist() == [[[0, 0], [0, 0]], [[1, 1.5], [1, 1.0]], [[2, 2.5], [2, 3.75]]]


def _edge():
    """70 stocks, 9 dates in three periods, G = 2, the group plane written by hand: stocks
    0..34 in group 0, 35..69 in group 1, every stock present."""
    S, D = 70, 9
    rng = np.random.default_rng(77)
    period_of = np.repeat(np.arange(3), 3).astype(np.int32)
    group = np.tile((np.arange(S) >= 35).astype(np.int8), (1, D, 1))
    xs = np.full((1, D, S), VALUE, np.uint8)
    pct = rng.normal(0, 0.02, (D, S))
    ps = np.full((D, S), VALUE, np.uint8)
    w = rng.uniform(1, 5, (D, S))
    wst = np.full((D, S), VALUE, np.uint8)
    return group, xs, pct, ps, period_of, w, wst


def test_group_without_weight_sits_in_cash(dev):
    """Every member of group 1 carries a zero, negative, infinite, NaN or null weight on the
    signal row of period 0: period 1 has 35 members, V = 1, ret = 0, t = 0 -- nothing is bought,
    and nothing of it is sold into period 2."""
    group, xs, pct, ps, period_of, w, wst = _edge()
    w[2, 35:] = np.resize([0.0, -1.0, np.inf, np.nan, 3.0], 35)
    wst[2, 35:] = np.resize([VALUE, VALUE, VALUE, VALUE, NULLV], 35)
    o = _raw(dev, group, xs, pct, ps, period_of, 3, 2, w, wst)
    r = ref.portfolios(group[0].astype(np.int64), xs[0], pct, ps, period_of, 3, 2, w, wst)
    assert o["count"][0].tolist() == [[0, 0], [35, 35], [35, 35]]
    assert (o["u"][0][1, 35:] == 0).all() and o["tot"][0][1, 1].tolist() == [0.0, 0.0]
    assert (o["ret"][0][3:6, 1] == 0).all() and o["traded"][0][1, 1] == 0
    assert (o["ret"][0][3:6, 0] != 0).all() and (o["ret"][0][6:, 1] != 0).all()
    assert abs(o["traded"][0][2, 1] - 1.0) <= 40 * EPS   # built from cash in period 2
    _compare(o["ret"][0], o["count"][0], o["traded"][0], r, period_of)


def test_nan_pct_poisons_its_cell_until_the_period_ends(dev):
    """A NaN pct of a member of group 0 on the second date of period 1: NaN on that date and the
    next, clean again in period 2, whose traded (it divides by A_end of period 1) is NaN; group
    1 never sees it.  The NaN positions are the reference's."""
    group, xs, pct, ps, period_of, w, wst = _edge()
    pct[4, 3] = np.nan
    for wa in ((None, None), (w, wst)):
        o = _raw(dev, group, xs, pct, ps, period_of, 3, 2, *wa)
        r = ref.portfolios(group[0].astype(np.int64), xs[0], pct, ps, period_of, 3, 2, *wa)
        assert np.isnan(o["ret"][0]).tolist() == [[False, False]] * 4 + [[True, False]] * 2 + [[False, False]] * 3
        assert np.isnan(o["traded"][0]).tolist() == [[False, False], [False, False], [True, False]]
        _compare(o["ret"][0], o["count"][0], o["traded"][0], r, period_of)


# --------------------------------------------------------------------------- engine
def _engine(dev, case, K, G, weighted, R=1, sl=None):
    from mff import dist, engine
    x, xs, pct, ps, w, wst, period_of, group, P, refs = case
    S = x.shape[2]

    def rank_fn(comm):
        s0, s1 = dist.shard_bounds(S, R, comm.rank) if comm is not None else (0, S)
        c = slice(s0, s1)
        wa = (_t(w[:, c], dev), _t(wst[:, c], dev)) if weighted else (None, None)
        ks = sl if sl is not None else slice(0, K)
        res = engine.group_portfolios(_t(x[ks, :, c], dev), _t(xs[ks, :, c], dev), _t(pct[:, c], dev),
                                      _t(ps[:, c], dev), _t(period_of, dev), P, G, *wa, comm=comm)
        torch.cuda.synchronize()
        return tuple(t.cpu().numpy() for t in res)

    return [rank_fn(None)] if R == 1 else dist.run_threads(R, rank_fn)


@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("S,G", [(65, 5), (257, 5), (257, 63), (64, 1)])
def test_engine_compounds_to_group_returns(dev, S, G, weighted):
    """engine.group_portfolios (its own cut) against the reference, and its daily return
    compounded over each period against engine.group_returns on the same inputs, inside the
    same bound; the present cells are equal."""
    from mff import engine
    _DEV["dev"] = dev
    case = _case(S, G, weighted)
    x, xs, pct, ps, w, wst, period_of, group, P, refs = case
    (ret, count, traded), = _engine(dev, case, 3, G, weighted)
    assert ret.shape == (3, D81, G) and count.shape == traded.shape == (3, P, G) and count.dtype == np.int32
    for k in range(3):
        _compare(ret[k], count[k], traded[k], refs[k], period_of, (S, G, weighted, k))
        wa = (_t(w, dev), _t(wst, dev)) if weighted else (None, None)
        gr, pres = engine.group_returns(_t(x[k], dev), _t(xs[k], dev), _t(pct, dev), _t(ps, dev),
                                        _t(period_of, dev), P, G, *wa)
        gr, pres = gr.cpu().numpy(), pres.cpu().numpy()
        assert np.array_equal(pres == 1, count[k] > 0)
        comp = np.stack([np.prod(1.0 + ret[k][period_of == p], axis=0) - 1.0 for p in range(P)])
        tol = 2.0 * _beta(refs[k], period_of) * (1.0 + np.abs(gr))
        assert (np.abs(comp - gr) <= tol).all(), float((np.abs(comp - gr) / tol).max())


def test_batch_is_bit_identical_to_single_calls(dev):
    _DEV["dev"] = dev
    case = _case(257, 5, True)
    (batch,) = _engine(dev, case, 3, 5, True)
    for k in range(3):
        (one,) = _engine(dev, case, 1, 5, True, sl=slice(k, k + 1))
        for a, b in zip(batch, one):
            assert a[k].tobytes() == b[0].tobytes()


@pytest.mark.parametrize("S", [65, 257])
def test_two_stock_shards(dev, S):
    """R = 2 on one device (33 + 32 and 129 + 128 stocks): the partials all-gathered and merged
    in rank order; both ranks hold the same result, inside the bounds of the reference."""
    _DEV["dev"] = dev
    case = _case(S, 5, True)
    period_of, refs = case[6], case[9]
    outs = _engine(dev, case, 3, 5, True, R=2)
    for ret, count, traded in outs:
        for k in range(3):
            _compare(ret[k], count[k], traded[k], refs[k], period_of, (S, k))
    for a, b in zip(*outs):
        assert a.tobytes() == b.tobytes()


def test_one_larger_run(dev):
    """S = 5000 (20 stock tiles), D = 250 in 50 five-date periods, K = 4, G = 10, weighted."""
    _DEV["dev"] = dev
    case = _case(5000, 10, True, D=250, K=4, weekly=True)
    period_of, P, refs = case[6], case[8], case[9]
    assert all(2 * int((r.count[1:] > 0).sum()) >= (P - 1) * 10 and r.count.max() > 256 for r in refs)
    (ret, count, traded), = _engine(dev, case, 4, 10, True)
    for k in range(4):
        _compare(ret[k], count[k], traded[k], refs[k], period_of, k)


# --------------------------------------------------------------------------- end to end
@functools.lru_cache(maxsize=None)
def _frames():
    from mff import frames
    D, S, K = 70, 40, 2
    x, xs, pct, ps, w, wst = _panel(S, D, K, seed=2)
    dates = [dt.date(2024, 1, 1) + dt.timedelta(days=i) for i in range(D)]
    codes = [f"{i:06d}.SZ" for i in range(S)]
    # every (code, date) keeps a row in some factor's frame and in pv: the universe is the full grid
    xs = xs.copy()
    xs[0][xs[0] == ABSENT] = NULLV
    exs = [frames.to_long(x[k], xs[k], codes, dates, f"f{k}") for k in range(K)]
    ps = np.where(ps == ABSENT, NULLV, ps).astype(np.uint8)
    wst = np.where(wst == ABSENT, NULLV, wst).astype(np.uint8)
    pv = frames.to_long(pct, ps, codes, dates, "pct_change")
    pv["cmc"] = frames.to_long(w, wst, codes, dates, "cmc")["cmc"]
    return x, xs, pct, ps, w, wst, dates, codes, exs, pv


def test_portfolio_tests_end_to_end(dev):
    """Factor.portfolio_test and mff.portfolio_tests on long frames, weekly, cmc-weighted, G = 5:
    the daily frame against the reference's ret and the host formulas (net return, nav), the
    period frame against its count and traded, the summary against pf_ref.summary.  A cost of
    0.001 leaves ret, count and turnover as they are and moves ret_net, nav, the period cost and
    the summary columns that are read from the net series."""
    import mff
    from mff.factor import Factor, rebalance_periods
    _DEV["dev"] = dev
    x, xs, pct, ps, w, wst, dates, codes, exs, pv = _frames()
    fs = [Factor(f"f{k}", exs[k]) for k in range(2)]
    period_of, labels = rebalance_periods(dates, "weekly")
    P, G = len(labels), 5
    group = _bins(x, xs, G)
    out = {}
    for cost in (0.0, 0.001):
        out[cost] = mff.portfolio_tests(fs, frequency="weekly", weight_param="cmc", group_num=G, cost=cost,
                                        return_daily=True, pv_data=pv, device=dev)
    for cost, (summ, daily, per) in out.items():
        assert list(summ.columns) == ["factor", "portfolio", "days", "total_return", "annual_return", "annual_vol",
                                      "sharpe", "max_drawdown", "mean_turnover", "total_cost"]
        assert list(daily.columns) == ["date", "factor", "portfolio", "ret", "ret_net", "nav"]
        assert list(per.columns) == ["date", "factor", "group", "count", "turnover", "cost"]
        for k in range(2):
            r = ref.portfolios(group[k].astype(np.int64), xs[k], pct, ps, period_of, P, G, w, wst)
            p0 = int(np.flatnonzero((r.count > 0).any(axis=1))[0])
            d0 = int(np.searchsorted(period_of, p0))
            tol = 2.0 * _beta(r, period_of)[period_of]
            for g in range(G):
                dg = daily[(daily["factor"] == f"f{k}") & (daily["portfolio"] == f"group_{g + 1}")]
                assert list(dg["date"]) == dates[d0:]
                got = dg["ret"].to_numpy()
                assert (np.abs(got - r.ret[d0:, g]) <= (tol[:, g] * (1 + np.abs(r.ret[:, g])))[d0:]).all()
                pg = per[(per["factor"] == f"f{k}") & (per["group"] == f"group_{g + 1}")]
                assert list(pg["date"]) == labels[p0:] and np.array_equal(pg["count"].to_numpy(), r.count[p0:, g])
                np.testing.assert_allclose(pg["turnover"].to_numpy(), r.traded[p0:, g] / 2, rtol=0, atol=1e-12)
                np.testing.assert_allclose(pg["cost"].to_numpy(), cost * r.traded[p0:, g], rtol=0, atol=1e-14)
                net = ref.net_series(r.ret[:, g], r.traded[:, g], period_of, cost)[d0:]
                np.testing.assert_allclose(dg["ret_net"].to_numpy(), net, rtol=0, atol=1e-12)
                np.testing.assert_allclose(dg["nav"].to_numpy(), np.cumprod(1 + net), rtol=1e-11)
                row = summ[(summ["factor"] == f"f{k}") & (summ["portfolio"] == f"group_{g + 1}")].iloc[0]
                for col, v in ref.summary(net, 252).items():
                    np.testing.assert_allclose(row[col], v, rtol=1e-9, atol=1e-12, err_msg=col)
                pres = r.count[p0:, g] > 0
                np.testing.assert_allclose(row["mean_turnover"], (r.traded[p0:, g][pres] / 2).mean(), rtol=1e-9)
                np.testing.assert_allclose(row["total_cost"], cost * r.traded[p0:, g].sum(), rtol=1e-9, atol=1e-15)
            ls = daily[(daily["factor"] == f"f{k}") & (daily["portfolio"] == "long_short")]
            np.testing.assert_allclose(ls["ret"].to_numpy(), (r.ret[:, G - 1] - r.ret[:, 0])[d0:], rtol=0, atol=1e-12)
            first = np.r_[True, period_of[1:] != period_of[:-1]]
            net = (r.ret[:, G - 1] - r.ret[:, 0]
                   - np.where(first, cost * (r.traded[:, G - 1] + r.traded[:, 0])[period_of], 0.0))[d0:]
            np.testing.assert_allclose(ls["ret_net"].to_numpy(), net, rtol=0, atol=1e-12)
            np.testing.assert_allclose(ls["nav"].to_numpy(), np.cumprod(1 + net), rtol=1e-11)
    (s0, d0_, p0_), (s1, d1_, p1_) = out[0.0], out[0.001]
    assert np.array_equal(d0_["ret"].to_numpy(), d0_["ret_net"].to_numpy())          # cost = 0
    assert d0_["ret"].equals(d1_["ret"]) and p0_["count"].equals(p1_["count"])
    assert p0_["turnover"].equals(p1_["turnover"])
    assert s0["days"].equals(s1["days"]) and s0["mean_turnover"].equals(s1["mean_turnover"])
    assert (s0["total_cost"] == 0).all() and (s1["total_cost"] > 0).all() and (p0_["cost"] == 0).all()
    assert (d1_["nav"].to_numpy()[-1] < d0_["nav"].to_numpy()[-1]) and not d1_["ret_net"].equals(d0_["ret_net"])
    # the method: the same numbers without the factor column
    one = fs[1].portfolio_test(frequency="weekly", weight_param="cmc", group_num=G, cost=0.001, return_daily=True,
                               pv_data=pv, device=dev, plot_out=False, return_df=True)
    for got, full in zip(one, out[0.001]):
        exp = full[full["factor"] == "f1"].drop(columns="factor").reset_index(drop=True)
        assert "factor" not in got.columns and got.reset_index(drop=True).equals(exp)
    assert fs[1].portfolio_test(pv_data=pv, device=dev, plot_out=False, frequency="weekly") is None
