"""Stage 2 (mff_stage2: k_stage2_reg<N>, k_stage2_slide, k_stage2_ring) at the shapes where
the block decode, the day segments, the chunk fast path and the partial last block can go
wrong: several rows x several stock blocks x several segments at once, every row seeded
differently.  Each result is compared with tests/stage2_ref.py (long-double two-pass) inside
its per-entry f64 error bound; constant and non-finite windows must match exactly.  Every
test prints the worst |error| / bound per method."""
import numpy as np
import pytest

import stage2_cases
import stage2_ref

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

ROLL = ("m", "z", "std")
_REFS = {}


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


@pytest.fixture(autouse=True)
def _no_stage2_env(monkeypatch):
    monkeypatch.delenv("MFF_S2_SEG_DAYS", raising=False)
    monkeypatch.delenv("MFF_STAGE2_IMPL", raising=False)


def _ref(key, val, state, N):
    """The reference of one (panel, N), computed once and shared (never modified)."""
    k = (key, N)
    if k not in _REFS:
        _REFS[k] = stage2_ref.rolling_all(val, state, N)
    return _REFS[k]


def _gpu(dev, val, state, N, methods=stage2_ref.METHODS):
    from mff import engine
    v, s = torch.from_numpy(val).to(dev), torch.from_numpy(state).to(dev)
    out = {}
    for meth in methods:
        rv, rs = engine.rolling(v, s, N, meth)
        torch.cuda.synchronize()
        out[meth] = (rv.cpu().numpy(), rs.cpu().numpy())
    return out


def _judge(out, ref, tag, worst):
    bad = []
    for meth, (gv, gs) in out.items():
        b, ratio = stage2_ref.check(gv, gs, ref[meth], f"{tag}/{meth}")
        bad += b
        worst[meth] = max(worst.get(meth, 0.0), ratio)
    return bad


def _report(name, worst):
    print(f"{name}: worst |gpu - ref| / bound " + ", ".join(f"{m} {worst[m]:.3f}" for m in ROLL if m in worst))


def _some_values(ref, methods=ROLL):
    """The case really has finite non-constant windows and exact (bound 0) ones."""
    return all((ref[m][2] > 0).any() for m in methods)


@pytest.mark.parametrize("N", [3, 20])
@pytest.mark.parametrize("S,D", [(1, 100), (63, 100), (64, 100), (65, 100), (255, 100), (256, 100), (257, 100),
                                  (513, 100), (257, 102), (513, 99)])
def test_reg_decode_grid(dev, S, D, N, monkeypatch):
    """k_stage2_reg's blockIdx.x -> (segment, row, stock block): 3 rows x 1..3 stock blocks
    x 13 / 3 segments (MFF_S2_SEG_DAYS = 8 / 40, the last one shorter), S around the wave
    and the block size, D = 102 / 99 ending a segmented run in tail days; 5 % ABSENT and, in
    the last stock block of the last row, a suspension, a late listing and a sparse stock."""
    val, state = stage2_cases.panel(3, D, S, 1000 + S)
    stage2_cases.ragged_tail(state)
    ref = _ref(("grid", S, D), val, state, N)
    assert S < 3 or _some_values(ref)
    bad, worst = [], {}
    for seg in (8, 40):
        monkeypatch.setenv("MFF_S2_SEG_DAYS", str(seg))
        bad += _judge(_gpu(dev, val, state, N), ref, f"S{S}/D{D}/N{N}/seg{seg}", worst)
    _report(f"reg grid S={S} D={D} N={N}", worst)
    assert not bad, "\n".join(bad[:20])


@pytest.mark.parametrize("N,D", [(20, 1000), (1, 150), (2, 150), (3, 150)])
def test_reg_default_segments(dev, N, D):
    """The segmentation mff_stage2 chooses itself, as the benchmark runs it: D = 1000 at
    N = 20 is four segments of 320, 320, 320 and 40 days; D = 150 at N <= 3 is four segments
    of 40 / 48 days, the last shorter; 2 rows x 2 stock blocks."""
    val, state = stage2_cases.panel(2, D, 257, 2000 + D + N)
    stage2_cases.ragged_tail(state)
    ref = _ref(("default", D, N), val, state, N)
    assert _some_values(ref, ROLL if N > 1 else ())
    worst = {}
    bad = _judge(_gpu(dev, val, state, N), ref, f"default/D{D}/N{N}", worst)
    _report(f"reg default segments D={D} N={N}", worst)
    assert not bad, "\n".join(bad[:20])


def _fast_path_panel(S, N):
    """No ABSENT entries but one stock's run across a boundary.  NULLs on the last 1 .. N
    days before a segment boundary and on the 3 days after it, a different offset per stock:
    row 0 around day 120 (a boundary at 12- and at 40-day segments), row 1 around day 80
    (40-day) for even stocks and day 84 (12-day) for odd ones."""
    D = 160
    val, state = stage2_cases.panel(2, D, S, 3000 + 10 * S + N, absent=0.0, null=0.3 / N, nan=0.15 / N)
    for s in range(S):
        for r, b, k in ((0, 120, s % (N + 3)), (1, 80 + 4 * (s % 2), (s // 2) % (N + 3))):
            d = b - 1 - k if k < N else b + (k - N)
            if d >= 0:
                state[r, d, s] = 1
    state[0, 116:124, 9 % S] = 0  # wave 0 leaves the fast path across the boundary; the others stay
    state[1, 78:87, 9 % S] = 0
    return val, state


@pytest.mark.parametrize("N", [4, 20, 59, 60, 61, 64])
@pytest.mark.parametrize("S", [65, 257])
def test_reg_fast_path_with_replay(dev, S, N, monkeypatch):
    """The chunk fast path fed by a replayed window: after a segment boundary the extended
    null mask nm >> (u + 1) and the count min(cnt + u + 1, N) come from the replay.  NULLs at
    every distance 1 .. N before a boundary (the NULL leaves the window exactly at / after
    the boundary) and just after it.  N = 61, 64 take the per-day path only."""
    val, state = _fast_path_panel(S, N)
    ref = _ref(("fast", S), val, state, N)
    assert _some_values(ref)
    bad, worst = [], {}
    for seg in (12, 40):
        monkeypatch.setenv("MFF_S2_SEG_DAYS", str(seg))
        bad += _judge(_gpu(dev, val, state, N, ROLL), ref, f"fast/S{S}/N{N}/seg{seg}", worst)
    _report(f"reg fast path + replay S={S} N={N}", worst)
    assert not bad, "\n".join(bad[:20])


@pytest.mark.parametrize("N", [3, 20])
@pytest.mark.parametrize("ragged", [True, False])
def test_reg_segment_invariance(dev, ragged, N, monkeypatch):
    """Segments are multiples of 4 days from day 0, so the chunk alignment and the fast /
    per-day choice do not depend on the segment length, and a rebuilt window holds the same
    values as a carried one: the outputs at 4-, 8-, 40-day segments and at one segment are
    bit-identical, values (NaN payloads included) and states."""
    D, S = 150, 257
    val, state = stage2_cases.panel(2, D, S, 4000 + N, absent=0.05 if ragged else 0.0)
    if ragged:
        stage2_cases.ragged_tail(state)
    ref = _ref(("inv", ragged), val, state, N)
    monkeypatch.setenv("MFF_S2_SEG_DAYS", "4096")
    one = _gpu(dev, val, state, N)
    worst = {}
    bad = _judge(one, ref, f"inv/ragged{ragged}/N{N}", worst)
    for seg in (4, 8, 40):
        monkeypatch.setenv("MFF_S2_SEG_DAYS", str(seg))
        got = _gpu(dev, val, state, N)
        for meth in stage2_ref.METHODS:
            dv = got[meth][0].view(np.uint64) != one[meth][0].view(np.uint64)
            ds = got[meth][1] != one[meth][1]
            if dv.any() or ds.any():
                i = tuple(np.argwhere(dv | ds)[0])
                bad.append(f"seg {seg} / {meth}: {int((dv | ds).sum())} entries differ from one segment, first at "
                           f"{i}: {got[meth][0][i]!r}/{got[meth][1][i]} vs {one[meth][0][i]!r}/{one[meth][1][i]}")
    _report(f"reg segment invariance ragged={ragged} N={N}", worst)
    assert not bad, "\n".join(bad[:20])


def _slide_panel(S, N, D):
    return stage2_cases.panel(3, D, S, 5000 + S + N + D, null=min(0.02, 0.3 / N), nan=min(0.01, 0.15 / N))


@pytest.mark.parametrize("impl,N,D", [(None, 65, 300), (None, 120, 300), ("slide", 1, 150), ("slide", 7, 150),
                                      ("slide", 64, 150)])
@pytest.mark.parametrize("S", [1, 255, 256, 257, 513])
def test_slide_shapes(dev, S, impl, N, D, monkeypatch):
    """k_stage2_slide (256 threads, one lane per stock): 3 rows x 1..3 stock blocks with a
    partial last block, as the path of N > 64 and forced for N <= 64; the 1e15 outlier leaves
    the window (rebuild of the sums) and the trend column drifts away from the shift."""
    if impl:
        monkeypatch.setenv("MFF_STAGE2_IMPL", impl)
    val, state = _slide_panel(S, N, D)
    stage2_cases.ragged_tail(state)
    ref = _ref(("slide", S, D), val, state, N)
    assert S < 7 or N == 1 or _some_values(ref)
    worst = {}
    bad = _judge(_gpu(dev, val, state, N), ref, f"slide/S{S}/N{N}/D{D}", worst)
    _report(f"slide S={S} N={N} D={D}", worst)
    assert not bad, "\n".join(bad[:20])


@pytest.mark.parametrize("N,D", [(65, 64), (65, 65), (120, 119), (120, 120), (65, 1)])
def test_slide_window_not_shorter_than_panel(dev, N, D):
    """D < N: every present entry NULL; D = N: only the last day of a stock without ABSENT,
    NULL or a gap can hold a value."""
    val, state = stage2_cases.panel(3, D, 257, 5500 + N + D, absent=0.01, null=0.002, nan=0.002)
    ref = _ref(("slide-short", D), val, state, N)
    if D == N:
        assert (ref["m"][1][:, D - 1] == 2).any() and not (ref["m"][1][:, : D - 1] == 2).any()
    else:
        assert not (ref["m"][1] == 2).any()
    worst = {}
    bad = _judge(_gpu(dev, val, state, N), ref, f"slide/N{N}/D{D}", worst)
    _report(f"slide N={N} D={D}", worst)
    assert not bad, "\n".join(bad[:20])


@pytest.mark.parametrize("N", [1, 7, 32, 33])
@pytest.mark.parametrize("S", [1, 63, 64, 65, 129])
def test_ring_shapes(dev, S, N, monkeypatch):
    """k_stage2_ring (64 threads, LDS ring [N][64]): 3 rows x 1..3 stock blocks, D = 1, 3, 4, 5
    (the 4-day prefetch clamped at D - 1) and 150; N = 33 is past the ring's limit and falls
    through to k_stage2_slide."""
    monkeypatch.setenv("MFF_STAGE2_IMPL", "ring")
    bad, worst = [], {}
    for D in (1, 3, 4, 5, 150):
        val, state = stage2_cases.panel(3, D, S, 6000 + S + D)
        stage2_cases.ragged_tail(state)
        ref = _ref(("ring", S, D), val, state, N)
        bad += _judge(_gpu(dev, val, state, N), ref, f"ring/S{S}/N{N}/D{D}", worst)
    assert S < 7 or N == 1 or _some_values(ref)
    _report(f"ring S={S} N={N}", worst)
    assert not bad, "\n".join(bad[:20])


def test_kernels_agree(dev, monkeypatch):
    """The three kernels on one ragged panel, N = 20: bit-identical states, every value
    inside the bound, and on constant windows exactly 0 std, exactly the value as the mean
    and NaN z -- including a constant window that begins right after a NaN and one right
    after a NULL."""
    N, D, S = 20, 150, 257
    val, state = stage2_cases.panel(2, D, S, 7000)
    stage2_cases.ragged_tail(state)
    for s, after in ((10, "nan"), (140, "null")):
        state[0, 30:70, s] = 2
        val[0, 30, s] = np.nan
        if after == "null":
            state[0, 30, s] = 1
        val[0, 31:70, s] = 4.5 + s
    ref = _ref("agree", val, state, N)
    for s in (10, 140):  # the case is there: the first constant window ends on day 50
        assert (ref["std"][1][0, 50:70, s] == 2).all() and (ref["std"][0][0, 50:70, s] == 0.0).all()
        assert (ref["m"][0][0, 50:70, s] == 4.5 + s).all() and np.isnan(ref["z"][0][0, 50:70, s]).all()
        assert (ref["std"][2][0, 50:70, s] == 0.0).all()
    assert ref["std"][1][0, 49, 140] == 1 and np.isnan(ref["m"][0][0, 49, 10])
    const = (ref["std"][1] == 2) & (ref["std"][0] == 0.0)
    assert const[:, :, 3].sum() > 50 and const[0, 50:70, 10].all()
    outs, bad = {}, []
    for impl in ("reg", "ring", "slide"):
        if impl == "reg":
            monkeypatch.delenv("MFF_STAGE2_IMPL", raising=False)
        else:
            monkeypatch.setenv("MFF_STAGE2_IMPL", impl)
        outs[impl] = _gpu(dev, val, state, N)
        worst = {}
        bad += _judge(outs[impl], ref, impl, worst)
        _report(f"kernels agree {impl}", worst)
        gm, gz, gsd = (outs[impl][m][0] for m in ROLL)
        if not ((gsd[const] == 0.0).all() and (gm[const] == ref["m"][0][const]).all() and np.isnan(gz[const]).all()):
            bad.append(f"{impl}: constant windows not exact")
    for impl in ("ring", "slide"):
        for meth in stage2_ref.METHODS:
            if not np.array_equal(outs[impl][meth][1], outs["reg"][meth][1]):
                bad.append(f"{impl}/{meth}: states differ from the register kernel's")
    assert not bad, "\n".join(bad[:20])
