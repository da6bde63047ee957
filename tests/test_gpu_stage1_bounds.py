"""The serial stage-1 kernels (k_stage1s_pair, k_stage1s<A|B|H>, the wave64 kernel) against
tests/stage1_ref.py on the panel of tests/stage1_cases.py: states, NaN pattern and infinities
exact, finite values inside the reference's derived f64 bound -- the 23 factors of the
cancelling families (MOMR, MOMV, MOMH, CORR, OLS), which tests/parity.py's 1e-6 admits a
lost shift, an f32 sum or an f32 quotient on (tests/test_stage1_ref.py measures that).  Every
other factor of a pass still goes through parity.compare against the oracle.  Run with -s for
the worst |gpu - ref| / bound per factor (DESIGN.md §4 quotes them)."""
import numpy as np
import pytest

import stage1_cases
import stage1_ref as R
from parity import compare

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

FIELDS = ("open", "high", "low", "close", "volume")
VALUE = 2


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def panel():
    return stage1_cases.panel()


@pytest.fixture(scope="module")
def ref(panel):
    return R.reference(*(panel[k] for k in FIELDS), panel["present"])


@pytest.fixture(scope="module")
def oracle(panel):
    """The factors outside the 23 (and the 23 too), from the oracle: {name: (val, state)}."""
    import mff_oracle as O
    ov, os_ = O.oracle_stage1(panel)
    return {nm: (ov[i], os_[i]) for i, nm in enumerate(O.ORACLE_NAMES)}


def _run(panel, dev, names=None):
    from mff import catalog, engine
    dp = engine.DevicePanel.from_host(panel, dev)
    val, state, ids = engine.compute_factors(dp, names)
    torch.cuda.synchronize()
    val, state = val.cpu().numpy(), state.cpu().numpy()
    return {catalog.NAMES[i]: (val[r], state[r]) for r, i in enumerate(ids)}


@pytest.fixture(scope="module")
def full(panel, dev):
    return _run(panel, dev)


def _check(got, ref, oracle, label):
    """The 23 by the bound, every other factor by C5; returns the worst ratios."""
    out, und = ref
    bad, worst = [], {}
    for nm, (gv, gs) in got.items():
        if nm in out:
            b, worst[nm] = R.check(gv, gs, out[nm], f"{label}/{nm}", und[nm])
            bad += b
        else:
            bad += compare(gv, gs, oracle[nm][0], oracle[nm][1], f"{label}/{nm}")
    print(f"\n{label}: worst |gpu - ref| / bound")
    for nm in R.NAMES:
        if nm in worst:
            print(f"  {nm:26s} {worst[nm]:.3g}")
    assert not bad, "\n".join(bad)
    return worst


def _same_bits(a, b):
    return (np.array_equal(a[1], b[1]) and np.array_equal(np.isnan(a[0]), np.isnan(b[0]))
            and np.array_equal(np.nan_to_num(a[0], nan=0.0).view(np.int64), np.nan_to_num(b[0], nan=0.0).view(np.int64)))


def test_all_58_pair_kernel_and_set_h(full, ref, oracle):
    """The default pass: k_stage1s_pair and k_stage1s<kSerH, true>."""
    assert len(full) == 58
    _check(full, ref, oracle, "default")


def test_equal_level_volumes_give_nan_level_moments(panel, full, oracle):
    """C7 on the group kernel's level path: price levels of equal integral volume have
    identical shares, so doc_kurt / doc_skew / doc_std are NaN -- also with 120 levels (a
    ramp day of 1,000,000-share bars with every other bar missing), where a shift taken after
    the scaling by 1 / sum(v) once left a rounding residual per level and a doc_kurt of -5e17."""
    c, v, m = (panel[k].reshape(-1, 240) for k in ("close", "volume", "present"))
    many = []
    for sd in range(c.shape[0]):
        lv = {}
        for a, b in zip(c[sd][m[sd]], v[sd][m[sd]]):
            lv[a] = lv.get(a, 0.0) + b
        if len(lv) >= 100 and len(set(lv.values())) == 1:
            many.append(sd)
    assert many
    for nm in ("doc_kurt", "doc_skew", "doc_std"):
        gv, gs = (a.reshape(-1) for a in full[nm])
        assert (gs[many] == VALUE).all() and np.isnan(gv[many]).all(), (nm, gv[many])
        assert np.isnan(oracle[nm][0].reshape(-1)[many]).all()


def test_w64_kernel(panel, dev, ref, oracle, monkeypatch):
    """MFF_STAGE1_IMPL=w64: the wave-per-stock-day kernel computes the same 23 factors."""
    monkeypatch.setenv("MFF_STAGE1_IMPL", "w64")
    _check(_run(panel, dev), ref, oracle, "w64")


def _family_names(fams):
    from mff import catalog
    return [n for n in catalog.NAMES if catalog.FAMILY[n] in fams]


SUBSETS = {
    "set A, FULL": lambda: _family_names(("SEG", "MOMR", "TRD", "ORD")),         # k_stage1s<kSerA, true>
    "set B, FULL": lambda: _family_names(("MOMV", "SUMV", "SUMC", "CORR")),       # k_stage1s<kSerB, true>
    "set A, one family": lambda: ["shape_skew"],                                  # <kSerA, false>
    "set B, two families": lambda: ["corr_pvl", "shape_kurtVol"],                 # <kSerB, false>
    "set H, one family": lambda: ["mmt_ols_qrs"],                                 # <kSerH, false>
}


@pytest.mark.parametrize("which", list(SUBSETS))
def test_subsets_reach_the_non_pair_kernels(panel, dev, full, ref, oracle, which):
    """A request without one of the sets A / B leaves the wave pair for k_stage1s<SET, FULL>.
    DESIGN.md §3 promises no bit equality between those forms and the pair (other chunking,
    other register budget), so every row must meet the bound on its own; whether the bits do
    agree with the 58-factor pass is printed."""
    names = SUBSETS[which]()
    got = _run(panel, dev, names)
    assert list(got) == names
    _check(got, ref, oracle, which)
    differ = [nm for nm in names if not _same_bits(got[nm], full[nm])]
    print(f"{which}: rows whose bits differ from the 58-factor pass: {differ or 'none'}")


def test_serial_schedule_same_bits(panel, dev, full, monkeypatch):
    """MFF_STAGE1_SERIAL=1 (engine.SERIAL, read once at import) only moves the launches onto
    one stream: bit-identical on this panel."""
    from mff import engine
    monkeypatch.setattr(engine, "SERIAL", True)
    got = _run(panel, dev)
    differ = [nm for nm in full if not _same_bits(got[nm], full[nm])]
    assert not differ, differ


def test_equal_close_and_open_is_a_zero_return(panel, full):
    """mff_fmath.h: a / b is exactly 1 for a == b, so a bar with close == open is neither an
    up nor a down member.  The member counts are no outputs; what they imply is: with fewer
    than two bars of close > open (close < open), exact comparisons of the fp32 planes,
    vol_upVol (vol_downVol) is exactly 0 -- one flat bar counted as a member would make the
    subset non-constant and the value positive -- and a stock-day of flat bars only has
    vol_return1min exactly 0 and NaN skew / kurtosis (C3)."""
    n, nu, nd, nflat = R.counts(panel["open"], panel["close"], panel["present"])
    assert (nu + nd + nflat == n).all()
    assert ((nflat > 100) & (nu == 1)).any() and ((nflat > 100) & (nu == 0) & (nd > 0)).any()
    assert ((nflat > 100) & (nd == 2)).any() and ((nflat > 100) & (nu == 2)).any()
    for nm, k in (("vol_upVol", nu), ("vol_downVol", nd)):
        v, s = full[nm]
        few = (n > 0) & (k < 2)
        assert few.sum() > 10
        assert (s[few] == VALUE).all() and (v[few] == 0.0).all(), nm
    flat = (n >= 2) & (nflat == n)
    assert flat.sum() >= 4
    assert (full["vol_return1min"][0][flat] == 0.0).all()
    assert np.isnan(full["shape_skew"][0][flat]).all() and np.isnan(full["shape_kurt"][0][flat]).all()
    assert np.isnan(full["vol_upRatio"][0][flat]).all()
