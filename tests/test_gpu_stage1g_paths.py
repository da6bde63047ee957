"""GPU: the two forms of the sorted-family group kernel k_stage1g.

A wave whose four stock-days hold all 240 bars outside the row set runs the body's
all-present (FULL) form: constant presence masks, n = 240, the result stores without the
row-set test.  MFF_STAGE1G_FULL=0 keeps every wave on the general form: both must give
the same bits, and the cells another kernel owns (exact list, row set) must come out as
before.  S = 37 (tiles of 16 / 16 / 5 stocks: the last block holds one wholly full wave, one
wave with a single active group, which must take the general form, and two inactive
waves), D = 3.

What these tests cannot tell: the two forms give the same bits by construction, so they
pass whichever form a wave took (and whether a listed stock-day went through the exact
list or not is visible only in its values).  That the FULL form runs on dense waves, and
what it saves, is in the counters and the census (648.5 -> 598.7 VALU
per stock-day on the dense panel).
"""
import copy

import numpy as np
import pytest

from parity import compare

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

S, D = 37, 3
LVL_ROWS = (39, 40, 41)
PDF_ROWS = (42, 43, 44, 45, 46)
ORDV_ROWS = (47, 48, 49)


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def _run(panel, dev, names=None):
    from mff import engine
    dp = engine.DevicePanel.from_host(panel, dev)
    val, state, _ = engine.compute_factors(dp, names)
    torch.cuda.synchronize()
    return val.cpu().numpy(), state.cpu().numpy()


def _oracle_bad(panel, *outs):
    """Mismatches of each (val, state) of `outs` against the oracle on `panel` (run once)."""
    import mff_oracle as O
    from mff import catalog
    ov, os_ = O.oracle_stage1(panel)
    bad = []
    for val, state in outs:
        for i, nm in enumerate(catalog.NAMES):
            bad += compare(val[i], state[i], ov[i], os_[i], nm)
    return bad


def _same_bits(a, b, what, rows=None, cells=None):
    """State bytes and value bits (the NaN pattern included) equal."""
    (av, as_), (bv, bs) = a, b
    rows = range(av.shape[0]) if rows is None else rows
    for r in rows:
        x, y, p, q = av[r], bv[r], as_[r], bs[r]
        if cells is not None:
            x, y, p, q = x[cells], y[cells], p[cells], q[cells]
        assert np.array_equal(p, q), f"{what}: row {r} states differ"
        assert np.array_equal(x.view(np.uint64), y.view(np.uint64)), f"{what}: row {r} value bits differ"


def _drop(panel, d, s, bars):
    panel["present"][d, s, bars] = False
    for k in ("open", "high", "low", "close", "volume"):
        panel[k][d, s, bars] = np.nan


@pytest.fixture(scope="module")
def dense(dev):
    """The dense panel (every stock-day 240 bars) and its default pass of all 58 factors;
    shared, never modified (the tests work on copies)."""
    from mff import synth
    panel = synth.make_panel(S, D, config=61)
    assert panel["present"].all()
    out = _run(panel, dev)
    return panel, out


def test_full_and_general_forms_same_bits(dev, dense, monkeypatch):
    panel, full = dense
    monkeypatch.setenv("MFF_STAGE1G_FULL", "0")
    general = _run(panel, dev)
    monkeypatch.delenv("MFF_STAGE1G_FULL")
    _same_bits(full, general, "full vs general")
    bad = _oracle_bad(panel, full, general)
    assert not bad, "\n".join(bad)


def test_mixed_waves(dev, dense, monkeypatch):
    """Holes, each in a wave whose other three stock-days are full (the wave takes the
    general form); the other waves stay wholly full."""
    panel = copy.deepcopy(dense[0])
    _drop(panel, 0, 1, [0])                                  # first bar
    _drop(panel, 0, 6, [239])                                # last bar
    _drop(panel, 0, 9, [15, 16])                             # a lane boundary
    _drop(panel, 1, 2, np.arange(240))                       # suspended
    _drop(panel, 1, 18, np.delete(np.arange(240), 100))      # a single present bar
    pres = panel["present"]
    # every hole's wave (4 consecutive stocks of a 16-stock tile) has three full stock-days,
    # and wholly full waves remain on each day
    fullsd = pres.all(axis=2)
    for d, s in ((0, 1), (0, 6), (0, 9), (1, 2), (1, 18)):
        w = fullsd[d, s - s % 4: s - s % 4 + 4]
        assert not fullsd[d, s] and w.sum() == 3
    assert fullsd[0, 12:16].all() and fullsd[1, 4:8].all() and fullsd[2, 32:36].all()
    out = _run(panel, dev)
    monkeypatch.setenv("MFF_STAGE1G_FULL", "0")
    general = _run(panel, dev)
    monkeypatch.delenv("MFF_STAGE1G_FULL")
    _same_bits(out, general, "mixed: full vs general")
    bad = _oracle_bad(panel, out)
    assert not bad, "\n".join(bad)


def test_exact_list_cells_on_full_path(dev, dense, monkeypatch):
    """A doc_pdf tie and a wide day inside wholly full waves: the FULL form lists them for
    the exact kernel and stores their ABSENT / NULL placeholders, the exact kernel's
    values stay."""
    import mff_oracle as O
    from mff import catalog
    base, base_out = dense
    panel = copy.deepcopy(base)
    tie, wide = (1, 5), (1, 22)
    # 240 distinct closes, every volume 100: 20 * cum == 12 * sum(v) exactly at level 144
    c0 = float(panel["close"][tie][0])
    panel["close"][tie] = (np.round(c0 * 100) + np.arange(240)).astype(np.float64).astype(np.float32) * np.float32(0.01)
    assert np.unique(panel["close"][tie]).size == 240
    panel["volume"][tie] = 100.0
    for k in ("open", "high", "low"):
        panel[k][tie] = panel["close"][tie]
    # a close at least twice another
    panel["close"][wide] = (panel["close"][wide] * np.linspace(0.6, 2.4, 240, dtype=np.float32)).astype(np.float32)
    assert panel["close"][wide].max() >= 2 * panel["close"][wide].min()
    for k in ("high", "low", "open"):
        panel[k][wide] = panel["close"][wide]
    # the tie on the CPU: the level sums are integers, level l (descending close) ends at
    # cumulative volume 100 (l + 1); the oracle's query for 0.6 sits at that level or the
    # next, whichever its float order decides
    v = panel["volume"][tie].astype(np.int64)
    cum = np.cumsum(v[np.argsort(-panel["close"][tie])])
    assert (20 * cum == 12 * v.sum()).sum() == 1 and 20 * cum[143] == 12 * v.sum()
    # the oracle's own cumulative shares (polars cum_sum) reach 0.6 at that level up to
    # rounding only, so its `> 0.6` there is decided by the float order: the case the
    # kernel leaves to the exact list
    cs = O.pl_cum_sum((v / v.sum()).tolist())
    assert abs(cs[143] - 0.6) < 1e-14 and cs[142] < 0.6 - 1e-3 and cs[144] > 0.6 + 1e-3
    ov, os_ = O.oracle_stage1(panel)
    out = _run(panel, dev)
    monkeypatch.setenv("MFF_STAGE1_IMPL", "w64")
    w64 = _run(panel, dev)
    monkeypatch.delenv("MFF_STAGE1_IMPL")
    rows = LVL_ROWS + PDF_ROWS
    for cell in (tie, wide):
        _same_bits(out, w64, f"cell {cell} vs w64", rows=rows, cells=cell)
    bad = []
    for i in rows + ORDV_ROWS:
        bad += compare(out[0][i], out[1][i], ov[i], os_[i], catalog.NAMES[i])
    assert not bad, "\n".join(bad)
    # the neighbours in the two waves keep the full path's values: the rows of one
    # stock-day alone (LVL, ORDV) are those of the panel without the special days
    for d, s in (tie, wide):
        for n in range(s - s % 4, s - s % 4 + 4):
            if n != s:
                _same_bits(out, base_out, f"neighbour {(d, n)}", rows=LVL_ROWS + ORDV_ROWS, cells=(d, n))


@pytest.mark.parametrize("names", [["doc_vol10_ratio"], ["doc_kurt"], ["doc_pdf60"], ["doc_vol5_ratio", "doc_skew"]])
def test_factor_subsets(dev, dense, names):
    """The ORD-only, LVL-only and combined launches with row = -1 for the rest."""
    from mff import catalog
    panel, allf = dense
    val, state = _run(panel, dev, names)
    assert val.shape[0] == len(names)
    for r, nm in enumerate(names):
        i = catalog.ID[nm]
        assert np.array_equal(state[r], allf[1][i]), nm
        assert np.array_equal(val[r].view(np.uint64), allf[0][i].view(np.uint64)), nm


def test_row_set_on_dense_panel(dev, dense):
    """Nulls on a dense panel (synth.add_nulls: a null volume, a null close, ... on kept
    stock-days): the families the row set owns come from mff_stage1_rows (oracle parity);
    a stock-day without a null keeps the bits of the pass without nulls on every row that
    depends on the stock-day alone (the doc_pdf rows rank across the day's stocks)."""
    from mff import engine, synth
    base, base_out = dense
    panel = synth.add_nulls(copy.deepcopy(base), seed=7, rate=0.0005)
    dp = engine.DevicePanel.from_host(panel, dev)
    assert dp.rows is not None and dp.rows.K >= 10
    w = dp.mask.view(-1, 8)[dp.rows.sd.long()].cpu().numpy().view(np.uint32)
    assert ((w[:, 7] & 0x40000000) != 0).sum() >= 5  # kept stock-days
    nb = panel["null"]
    assert ((nb & 16) != 0).any() and ((nb & 8) != 0).any()
    val, state, _ = engine.compute_factors(dp)
    torch.cuda.synchronize()
    out = val.cpu().numpy(), state.cpu().numpy()
    bad = _oracle_bad(panel, out)
    assert not bad, "\n".join(bad)
    untouched = ~(nb != 0).any(axis=2)
    assert untouched.sum() >= 20
    _same_bits(out, base_out, "untouched stock-days", rows=[r for r in range(58) if r not in PDF_ROWS],
               cells=untouched)
