"""GPU: stage 3 (csrc/mff_stage3.hip) at the shapes the rest of the suite never runs.

A1  the segment loops of the rank kernels: more (row, day) segments than workgroups, so every
    workgroup ranks a second segment on the LDS counters its first one left behind, several
    workgroups append to the hand-over list and the sorting kernel strides over more listed
    segments than it has workgroups.  Days are tiled from a few patterns whose ranks the CPU
    oracle computes once; the comparison runs on the device and is bit-exact.
A2  mff_xs_rank with R > 1 (the public multi-rank form: k_xs_rank_bucket<.., LOCAL=false> and
    k_xs_rank through XsLoader), called directly per shard, exact against the oracle.
A3  the z-score: every k_xs_zscore_local<PER> form on both sides of each edge, more segments
    than one launch slice of mff_xs_zscore, and R = 2, 3, 5 moments combined, against a
    two-pass mean / ddof-1 standard deviation in np.longdouble at rtol = atol = 1e-9.
    Inputs keep |mean| <= 1e3 sd per day: the kernels shift by the first included value and
    centre by the mean before squaring, so their error is a few ulp of |x - mean| / sd plus
    |mean| / sd ulps (about 1e-12 here), far inside the tolerance.
"""
import numpy as np
import pytest

from parity import compare
from stage3_cases import ABSENT, NULLV, VALUE, pattern_days

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

SORT_CAP = 8192        # values one LDS bitonic sort holds (csrc/mff_sort.h)
XS_RANK_GRID = 2048    # workgroups of k_xs_rank; the bucketed kernels launch up to 4x as many
Z_TOL = 1e-9
WORST_Z = {"err": 0.0}  # worst |z - reference| seen by this module (printed by every z test)


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def _lib():
    from mff import _lib as L
    return L, L.load()


def _xs_rank(val, state, val_all, state_all, R, S_all):
    """mff_xs_rank called directly; returns (out_val, out_state, hand-over list count).  The
    count is the first u32 of the list, which mff.h places 256 bytes into the workspace when
    R * S_all <= 8192 and behind the g * 2 * M * 8 bytes of sort buffers otherwise."""
    L, lib = _lib()
    rows, D, S_loc = val.shape
    dev = val.device
    nseg = rows * D
    M = R * S_all
    nbytes = lib.mff_xs_rank_workspace_bytes(rows, D, S_all, R)
    off = 256 if M <= SORT_CAP else min(nseg, XS_RANK_GRID) * 2 * M * 8
    assert nbytes >= off + 4 * (nseg + 1)
    ws = torch.zeros(nbytes, dtype=torch.uint8, device=dev)
    ov = torch.full_like(val, -7.0)
    os_ = torch.full_like(state, 9)
    st = torch.cuda.current_stream(dev).cuda_stream
    L.check(lib.mff_xs_rank(L.ptr(val), L.ptr(state), rows, D, S_loc, L.ptr(val_all), L.ptr(state_all), R, S_all,
                            L.ptr(ov), L.ptr(os_), L.ptr(ws), st), "mff_xs_rank")
    torch.cuda.synchronize()
    count = int(ws[off:off + 4].view(torch.int32)[0].item())
    return ov, os_, count


# ---------------------------------------------------------------------------------------
# A1: segment loops by tiling
# ---------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def rank_patterns():
    """S, handover -> (val [P][S], state, names, hand-over index, oracle ranks [P][S], oracle
    states): every pattern day ranked once on the CPU."""
    import mff_oracle as O
    cache = {}

    def get(S, handover=True):
        key = (S, handover)
        if key not in cache:
            v, s, names, hand = pattern_days(S, 1000 + S, handover)
            rv, rs = O.oracle_stage3(v, s, "rank")
            cache[key] = (v, s, names, hand, rv, rs)
        return cache[key]

    return get


def _tile_ids(P, hand, nseg, seed):
    """A seeded random sequence of pattern ids, 27 % of them the hand-over day (if any)."""
    rng = np.random.default_rng(seed)
    if hand is None:
        return rng.integers(0, P, nseg)
    others = np.array([p for p in range(P) if p != hand])
    ids = others[rng.integers(0, others.size, nseg)]
    ids[rng.choice(nseg, (27 * nseg + 99) // 100, replace=False)] = hand
    return ids


def _first_bad_segment(ov, os_, ref_v, ref_s, ids, S):
    """Device comparison of tiled outputs [nseg][S] with the tiled reference: states equal,
    NaN exactly where the reference is NaN, every other value bit-equal.  Returns None or the
    first bad segment."""
    rv = ref_v.index_select(0, ids)
    rs = ref_s.index_select(0, ids)
    ov, os_ = ov.view(-1, S), os_.view(-1, S)
    rnan = torch.isnan(rv)
    good = (os_ == rs) & (torch.isnan(ov) == rnan) & (rnan | (ov.view(torch.int64) == rv.view(torch.int64)))
    bad = (~good).any(dim=1)
    if not bool(bad.any().item()):
        return None
    return int(torch.nonzero(bad)[0].item())


# (kernel form, S, MFF_XS_RANK_IMPL, segments, hand-over day tiled in, workgroups of the form)
TILE_CASES = [
    ("day<512,2>", 1000, "", 8400, True, 4 * XS_RANK_GRID),
    ("day<512,4>", 1500, "", 8400, True, 4 * XS_RANK_GRID),
    ("day<1024,3>", 2500, "", 8400, True, 4 * XS_RANK_GRID),
    ("day<1024,4>", 3500, "", 8400, True, 4 * XS_RANK_GRID),
    ("day<1024,5>", 5000, "", 8400, True, 4 * XS_RANK_GRID),
    ("bucket<5,true>", 1100, "bucket", 8400, True, 4 * XS_RANK_GRID),
    ("bucket<8,true>", 5200, "", 8400, True, 4 * XS_RANK_GRID),
    ("sort-merge", 8200, "", 2100, False, XS_RANK_GRID),
    ("sort-lds", 1000, "sort", 2100, True, XS_RANK_GRID),
]


@pytest.mark.parametrize("form,S,impl,nseg,handover,grid", TILE_CASES, ids=[c[0] for c in TILE_CASES])
def test_rank_segment_loops(dev, rank_patterns, monkeypatch, form, S, impl, nseg, handover, grid):
    """Every rank kernel form with more segments than workgroups (a second trip of the
    `seg += gridDim.x` loop on every workgroup) and, for the bucketed forms, more than 2,048
    handed-over segments (k_xs_rank strides over the list)."""
    if impl:
        monkeypatch.setenv("MFF_XS_RANK_IMPL", impl)
    else:
        monkeypatch.delenv("MFF_XS_RANK_IMPL", raising=False)
    listed = bool(handover) and impl != "sort"
    assert nseg > grid, "every workgroup must take a second segment"
    pv, ps, names, hand, rv, rs = rank_patterns(S, handover)
    rows, D = 2, nseg // 2
    ids_h = _tile_ids(len(names), hand, nseg, 7 * S + nseg)
    ids = torch.from_numpy(ids_h).to(dev)
    val = torch.from_numpy(pv).to(dev).index_select(0, ids).view(rows, D, S)
    state = torch.from_numpy(ps).to(dev).index_select(0, ids).view(rows, D, S)
    ov, os_, count = _xs_rank(val, state, val, state, 1, S)
    if listed:
        n_hand = int((ids_h == hand).sum())
        assert n_hand > XS_RANK_GRID, "inputs: the list must exceed the sorting kernel's grid"
        assert count >= n_hand and count >= 2049, f"{form}: {count} listed segments, {n_hand} hand-over days"
        assert count <= nseg
    seg = _first_bad_segment(ov, os_, torch.from_numpy(rv).to(dev), torch.from_numpy(rs).to(dev), ids, S)
    if seg is not None:
        prev = seg - grid
        g = ov.view(-1, S)[seg].cpu().numpy()
        gs = os_.view(-1, S)[seg].cpu().numpy()
        p = int(ids_h[seg])
        detail = compare(g, gs, rv[p], rs[p], names[p], rtol=0.0, atol=0.0)
        raise AssertionError(
            f"{form} S={S}: first bad segment {seg} (pattern {names[p]}); previous tenant of its workgroup: "
            + (f"segment {prev} (pattern {names[int(ids_h[prev])]})" if prev >= 0 else "none")
            + "\n" + "\n".join(detail))


# ---------------------------------------------------------------------------------------
# A2: mff_xs_rank with R > 1
# ---------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def sharded_rank_days():
    """S_total -> (val [2][P][S_total], state, hand-over index, oracle ranks, oracle states)."""
    import mff_oracle as O
    cache = {}

    def get(S_total):
        if S_total not in cache:
            parts = [pattern_days(S_total, 50 + 3 * S_total + r) for r in range(2)]
            hand = parts[0][3]
            v = np.stack([p[0] for p in parts])
            s = np.stack([p[1] for p in parts])
            ref = [O.oracle_stage3(v[r], s[r], "rank") for r in range(2)]
            cache[S_total] = (v, s, hand, np.stack([x[0] for x in ref]), np.stack([x[1] for x in ref]))
        return cache[S_total]

    return get


R_CASES = [(3, 300, ""), (2, 1500, ""), (4, 1280, ""), (2, 2561, ""), (2, 4096, ""), (2, 4097, ""), (3, 3000, ""),
           (3, 300, "sort"), (2, 2561, "sort")]


@pytest.mark.parametrize("R,S_all,impl", R_CASES)
def test_rank_sharded_direct(dev, sharded_rank_days, monkeypatch, R, S_all, impl):
    """mff_xs_rank as a multi-rank caller uses it: every rank passes its own columns
    [rows][D][S_loc] and all ranks' columns [R][rows][D][S_all] (ABSENT-padded); the
    concatenated ranks equal the oracle's ranks of the unsharded days."""
    from mff import dist
    if impl:
        monkeypatch.setenv("MFF_XS_RANK_IMPL", impl)
    else:
        monkeypatch.delenv("MFF_XS_RANK_IMPL", raising=False)
    S_total = R * S_all - 1  # the last shard one stock short of S_all
    bounds = [dist.shard_bounds(S_total, R, r) for r in range(R)]
    assert bounds[0][1] - bounds[0][0] == S_all and bounds[-1][1] - bounds[-1][0] < S_all
    v, s, hand, rv, rs = sharded_rank_days(S_total)
    rows, D = v.shape[:2]
    va = np.zeros((R, rows, D, S_all))
    sa = np.full((R, rows, D, S_all), ABSENT, np.uint8)
    for r, (a, b) in enumerate(bounds):
        va[r, :, :, :b - a] = v[:, :, a:b]
        sa[r, :, :, :b - a] = s[:, :, a:b]
    va_d, sa_d = torch.from_numpy(va).to(dev), torch.from_numpy(sa).to(dev)
    gv, gs = [], []
    for r, (a, b) in enumerate(bounds):
        own_v = torch.from_numpy(np.ascontiguousarray(v[:, :, a:b])).to(dev)
        own_s = torch.from_numpy(np.ascontiguousarray(s[:, :, a:b])).to(dev)
        ov, os_, count = _xs_rank(own_v, own_s, va_d, sa_d, R, S_all)
        if R * S_all <= SORT_CAP and not impl:
            assert count >= rows, f"rank {r}: the hand-over day was not handed over (list count {count})"
            assert count <= rows * D
        gv.append(ov.cpu().numpy())
        gs.append(os_.cpu().numpy())
    gv, gs = np.concatenate(gv, axis=2), np.concatenate(gs, axis=2)
    bad = []
    for row in range(rows):
        bad += compare(gv[row], gs[row], rv[row], rs[row], f"R{R}/S_all{S_all}/row{row}", rtol=0.0, atol=0.0)
    assert not bad, "\n".join(bad[:20])


# ---------------------------------------------------------------------------------------
# A3: z-score
# ---------------------------------------------------------------------------------------

def z_reference(val, state):
    """Two-pass mean and ddof-1 standard deviation in np.longdouble over the included set
    (state VALUE and not NaN) of each day [..., S]; the state rules of k_xs_zscore: excluded
    rows keep their state (VALUE-NaN stays NaN, others 0.0), n < 2 -> NULL.  Returns (val,
    state, exact [...]): `exact` is False for days holding an infinity or one constant value,
    which are NaN throughout and compared by NaN pattern and state only."""
    val, state = np.asarray(val), np.asarray(state)
    S = val.shape[-1]
    v2, s2 = val.reshape(-1, S), state.reshape(-1, S)
    ov = np.zeros_like(v2)
    os_ = s2.copy()
    exact = np.ones(v2.shape[0], bool)
    for d in range(v2.shape[0]):
        inc = (s2[d] == VALUE) & ~np.isnan(v2[d])
        ov[d, (s2[d] == VALUE) & np.isnan(v2[d])] = np.nan
        x = v2[d, inc].astype(np.longdouble)
        if x.size < 2:
            os_[d, inc] = NULLV
            continue
        if np.isinf(x).any() or x.min() == x.max():
            ov[d, inc] = np.nan
            exact[d] = False
            continue
        mean = x.sum() / x.size
        dl = x - mean
        sd = np.sqrt((dl * dl).sum() / (x.size - 1))
        ov[d, inc] = (dl / sd).astype(np.float64)
    return ov.reshape(val.shape), os_.reshape(state.shape), exact.reshape(val.shape[:-1])


def _z_check(gv, gs, rv, rs, exact, name):
    """compare() at the z tolerance; days that are not `exact` by NaN pattern and state."""
    bad = []
    S = rv.shape[-1]
    gv, gs, rv, rs = (np.asarray(a).reshape(-1, S) for a in (gv, gs, rv, rs))
    ex = np.asarray(exact).reshape(-1)
    bad += compare(gv[ex], gs[ex], rv[ex], rs[ex], name, rtol=Z_TOL, atol=Z_TOL)
    if (~ex).any():
        if not np.array_equal(gs[~ex], rs[~ex]):
            bad.append(f"{name}: state mismatch on an inf / constant day")
        if not np.array_equal(np.isnan(gv[~ex]), np.isnan(rv[~ex])):
            bad.append(f"{name}: NaN pattern mismatch on an inf / constant day")
    m = (rs[ex] == VALUE) & (gs[ex] == VALUE) & np.isfinite(rv[ex]) & np.isfinite(gv[ex])
    if m.any():
        WORST_Z["err"] = max(WORST_Z["err"], float(np.abs(gv[ex][m] - rv[ex][m]).max()))
    print(f"{name}: worst |z - longdouble reference| so far {WORST_Z['err']:.3e}")
    return bad


def _z_local(val, state, dev):
    L, lib = _lib()
    rows, D, S = val.shape
    v, s = torch.from_numpy(val).to(dev), torch.from_numpy(state).to(dev)
    ov, os_ = torch.full_like(v, -7.0), torch.full_like(s, 9)
    st = torch.cuda.current_stream(dev).cuda_stream
    rc = lib.mff_xs_zscore_local(L.ptr(v), L.ptr(s), rows, D, S, L.ptr(ov), L.ptr(os_), st)
    torch.cuda.synchronize()
    return rc, ov.cpu().numpy(), os_.cpu().numpy()


def _moments(v, s):
    L, lib = _lib()
    rows, D, S = v.shape
    mom = torch.full((rows, D, 3), -7.0, dtype=torch.float64, device=v.device)
    st = torch.cuda.current_stream(v.device).cuda_stream
    L.check(lib.mff_xs_moments(L.ptr(v), L.ptr(s), rows, D, S, L.ptr(mom), st), "mff_xs_moments")
    return mom


def _zscore(v, s, mom_all, R):
    L, lib = _lib()
    rows, D, S = v.shape
    ov, os_ = torch.full_like(v, -7.0), torch.full_like(s, 9)
    st = torch.cuda.current_stream(v.device).cuda_stream
    L.check(lib.mff_xs_zscore(L.ptr(v), L.ptr(s), rows, D, S, L.ptr(mom_all), R, L.ptr(ov), L.ptr(os_), st),
            "mff_xs_zscore")
    torch.cuda.synchronize()
    return ov, os_


def _offset_normal(rng, n, ratio):
    """n normal values of a random scale with mean = ratio * sd (|ratio| <= 1e3)."""
    sd = 10.0 ** rng.uniform(-3, 5)
    return sd * (ratio + rng.normal(size=n))


def _z_local_days(S, seed):
    """[2][6][S]: where the first included value sits (stock 0, the last column, beyond the
    first 256 stocks: another register index of k_xs_zscore_local), a first included +inf,
    n = 0 / 1 / 2, a constant day, an interior -inf, and mixed states."""
    rng = np.random.default_rng(seed)
    val = np.empty((2, 6, S))
    state = np.full((2, 6, S), VALUE, np.uint8)

    def scatter_excluded(v, s, upto):
        k = rng.integers(0, 3, upto)
        s[:upto] = np.where(k == 0, ABSENT, np.where(k == 1, NULLV, VALUE))
        v[:upto] = np.where(k == 2, np.nan, v[:upto])

    # row 0
    val[0, 0] = _offset_normal(rng, S, 1e3)           # first included at stock 0, mean = 1e3 sd
    val[0, 1] = _offset_normal(rng, S, -50.0)         # only the last column included: n = 1
    scatter_excluded(val[0, 1], state[0, 1], S - 1)
    val[0, 2] = _offset_normal(rng, S, -1e3)          # first included beyond the first 256 stocks
    scatter_excluded(val[0, 2], state[0, 2], min(300, max(S - 2, 0)))
    val[0, 3] = _offset_normal(rng, S, 3.0)           # first included value +inf: x0 = 0
    val[0, 3, 0] = np.inf
    val[0, 4] = rng.normal(size=S)                    # n = 0
    scatter_excluded(val[0, 4], state[0, 4], S)
    val[0, 5] = _offset_normal(rng, S, 700.0)         # n = 2 (or S if smaller), far apart columns
    scatter_excluded(val[0, 5], state[0, 5], S)
    for c in {0, S - 1}:
        state[0, 5, c] = VALUE
        val[0, 5, c] = 5.0 + c
    # row 1
    val[1, 0] = 0.1                                   # constant
    val[1, 1] = _offset_normal(rng, S, 0.0)
    val[1, 2] = _offset_normal(rng, S, 10.0)          # -inf in the middle
    val[1, 2, S // 2] = -np.inf
    val[1, 3] = _offset_normal(rng, S, 1e3)           # 10 % each NaN / NULL / ABSENT
    val[1, 3, rng.random(S) < 0.1] = np.nan
    state[1, 3, rng.random(S) < 0.1] = NULLV
    state[1, 3, rng.random(S) < 0.1] = ABSENT
    val[1, 4] = _offset_normal(rng, S, -400.0)        # only the last two columns: n = 2
    scatter_excluded(val[1, 4], state[1, 4], max(S - 2, 0))
    val[1, 5] = _offset_normal(rng, S, 1.0)
    return val, state


Z_LOCAL_S = [1, 2, 255, 256, 257, 1024, 1025, 2048, 2049, 3072, 3073, 4096, 4097, 5120, 5121, 6144, 6145, 8191, 8192]


def _per_form(S):
    per = (S + 255) // 256
    return next(p for p in (4, 8, 12, 16, 20, 24, 32) if per <= p)


def test_zscore_local_sizes_cover_every_form():
    """Z_LOCAL_S launches each k_xs_zscore_local<PER> at its largest S and the next form at
    that S + 1."""
    assert {_per_form(S) for S in Z_LOCAL_S} == {4, 8, 12, 16, 20, 24, 32}
    for edge, (lo, hi) in zip((1024, 2048, 3072, 4096, 5120, 6144), zip((4, 8, 12, 16, 20, 24), (8, 12, 16, 20, 24, 32))):
        assert edge in Z_LOCAL_S and edge + 1 in Z_LOCAL_S
        assert _per_form(edge) == lo and _per_form(edge + 1) == hi


@pytest.mark.parametrize("S", Z_LOCAL_S)
def test_zscore_local_forms(dev, S):
    val, state = _z_local_days(S, 31 * S + 5)
    rv, rs, exact = z_reference(val, state)
    if S >= 302:  # the crafted day whose first included value lies beyond the first 256 stocks
        inc = (state[0, 2] == VALUE) & ~np.isnan(val[0, 2])
        assert int(np.argmax(inc)) >= 256
    rc, gv, gs = _z_local(val, state, dev)
    assert rc == 0
    bad = _z_check(gv, gs, rv, rs, exact, f"z-local/S{S}")
    assert not bad, "\n".join(bad[:20])


def test_zscore_local_rejects_more_than_max_stocks(dev):
    L, lib = _lib()
    assert lib.mff_xs_zscore_local_max_stocks() == 8192
    val, state = np.zeros((1, 1, 8193)), np.full((1, 1, 8193), VALUE, np.uint8)
    rc, _, _ = _z_local(val, state, dev)
    assert rc != 0
    assert b"mff_xs_zscore_local" in lib.mff_last_error()


def _z_pattern_days(S, seed):
    """A handful of z days [P][S] for tiling."""
    rng = np.random.default_rng(seed)
    days = []

    def add(v, s=None):
        days.append((np.asarray(v, np.float64), np.full(S, VALUE, np.uint8) if s is None else s))

    add(_offset_normal(rng, S, 1e3))
    v = _offset_normal(rng, S, -20.0)
    s = np.full(S, VALUE, np.uint8)
    v[rng.random(S) < 0.15] = np.nan
    s[rng.random(S) < 0.15] = NULLV
    s[rng.random(S) < 0.15] = ABSENT
    add(v, s)
    add(np.full(S, 2.5))                                   # constant
    add(rng.normal(size=S), np.full(S, ABSENT, np.uint8))  # n = 0
    s = np.full(S, NULLV, np.uint8)                        # n = 1
    s[S - 1] = VALUE
    add(rng.normal(size=S), s)
    s = np.full(S, ABSENT, np.uint8)                       # n = 2
    s[[3, S - 2]] = VALUE
    add(_offset_normal(rng, S, 500.0), s)
    v = rng.normal(size=S)                                 # an infinity
    v[S // 3] = np.inf
    add(v)
    return np.stack([d[0] for d in days]), np.stack([d[1] for d in days])


def test_zscore_launch_slices(dev):
    """mff_xs_moments + mff_xs_zscore, R = 1, nseg = 65,703: two launch slices of the
    z-score's grid.y (65,535) and a last moments workgroup with one of its four waves idle
    (D = 21,901: 3 x 21,900 segments would fill the last workgroup)."""
    rows, D, S = 3, 21901, 40
    nseg = rows * D
    assert nseg > 65535 and nseg % 4 != 0
    pv, ps = _z_pattern_days(S, 77)
    rv, rs, exact = z_reference(pv, ps)
    ids_h = np.random.default_rng(78).integers(0, pv.shape[0], nseg)
    ids_h[[0, 65534, 65535, 65536, nseg - 1]] = [0, 1, 0, 1, 0]  # offset-mean days around the slice edge
    ids = torch.from_numpy(ids_h).to(dev)
    val = torch.from_numpy(pv).to(dev).index_select(0, ids).view(rows, D, S)
    state = torch.from_numpy(ps).to(dev).index_select(0, ids).view(rows, D, S)
    ov, os_ = _zscore(val, state, _moments(val, state), 1)
    ref_v = torch.from_numpy(rv).to(dev).index_select(0, ids)
    ref_s = torch.from_numpy(rs).to(dev).index_select(0, ids)
    ex = torch.from_numpy(exact).to(dev).index_select(0, ids).unsqueeze(1)
    ov, os_ = ov.view(-1, S), os_.view(-1, S)
    rnan = torch.isnan(ref_v)
    err = torch.where(rnan | torch.isnan(ov), torch.zeros_like(ov), (ov - ref_v).abs())
    lim = Z_TOL * torch.maximum(ov.abs(), ref_v.abs()).nan_to_num(0.0) + Z_TOL
    good = (os_ == ref_s) & (torch.isnan(ov) == rnan) & (~ex | (err <= lim))
    WORST_Z["err"] = max(WORST_Z["err"], float(torch.where(ex.expand_as(err), err, torch.zeros_like(err)).max().item()))
    print(f"z-slices: worst |z - longdouble reference| so far {WORST_Z['err']:.3e}")
    bad = (~good).any(dim=1)
    if bool(bad.any().item()):
        seg = int(torch.nonzero(bad)[0].item())
        p = int(ids_h[seg])
        detail = _z_check(ov[seg].cpu().numpy(), os_[seg].cpu().numpy(), rv[p], rs[p], exact[p], f"pattern {p}")
        raise AssertionError(f"{int(bad.sum().item())} bad segments, first {seg} (pattern {p})\n" + "\n".join(detail))


def _z_sharded_days(S_total, bounds, seed):
    """[2][8][S_total] for R shards at `bounds`: a middle shard (the first one at R = 2) without
    any included value, only the last shard with some, total n = 1 and n = 2, a constant
    day, n = 0, mixed states; row 1 repeats the kinds with other draws and an infinity."""
    rng = np.random.default_rng(seed)
    R = len(bounds)
    mid = bounds[R // 2] if R > 2 else bounds[0]
    last = bounds[-1]
    val = np.empty((2, 8, S_total))
    state = np.full((2, 8, S_total), VALUE, np.uint8)
    for row in range(2):
        v, s = val[row], state[row]
        v[0] = _offset_normal(rng, S_total, 1e3 if row == 0 else -1e3)
        v[1] = _offset_normal(rng, S_total, 30.0)           # a middle shard with nothing included
        k = rng.integers(0, 3, mid[1] - mid[0])
        s[1, mid[0]:mid[1]] = np.where(k == 0, ABSENT, np.where(k == 1, NULLV, VALUE))
        v[1, mid[0]:mid[1]][k == 2] = np.nan
        v[2] = _offset_normal(rng, S_total, -200.0)         # only the last shard has any
        s[2, :last[0]] = rng.choice(np.array([ABSENT, NULLV], np.uint8), last[0])
        v[3] = rng.normal(size=S_total)                     # total n = 1
        s[3] = ABSENT
        s[3, bounds[R // 2][0] + 1] = VALUE
        v[4] = _offset_normal(rng, S_total, 900.0)          # total n = 2, in the first and last shard
        s[4] = NULLV
        s[4, [1, S_total - 1]] = VALUE
        v[5] = 1e-3 * (7 + row)                             # constant
        v[6] = rng.normal(size=S_total)                     # n = 0
        s[6] = rng.choice(np.array([ABSENT, NULLV], np.uint8), S_total)
        v[7] = _offset_normal(rng, S_total, 5.0)
        v[7, rng.random(S_total) < 0.1] = np.nan
        s[7, rng.random(S_total) < 0.1] = NULLV
        s[7, rng.random(S_total) < 0.1] = ABSENT
        if row == 1:
            v[7, S_total // 2] = -np.inf
    return val, state


@pytest.mark.parametrize("S_total", [130, 3000, 9000])
@pytest.mark.parametrize("R", [2, 3, 5])
def test_zscore_sharded_direct(dev, R, S_total):
    """Per-shard mff_xs_moments stacked into [R][rows][D][3] and mff_xs_zscore per shard
    (uneven shards) meet the reference; so do the R = 1 route and, for S_total <= 8192, the
    one-pass local kernel on the same days."""
    from mff import dist
    # dist.shard_bounds with the first boundary moved up by 3: uneven whatever S_total % R is
    bounds = [dist.shard_bounds(S_total, R, r) for r in range(R)]
    bounds[0] = (0, bounds[0][1] + 3)
    bounds[1] = (bounds[1][0] + 3, bounds[1][1])
    assert len({b - a for a, b in bounds}) > 1 and bounds[-1][1] == S_total, "uneven shards"
    assert all(bounds[r][1] == bounds[r + 1][0] for r in range(R - 1))
    val, state = _z_sharded_days(S_total, bounds, 13 * S_total + R)
    rv, rs, exact = z_reference(val, state)
    shards = [(torch.from_numpy(np.ascontiguousarray(val[:, :, a:b])).to(dev),
               torch.from_numpy(np.ascontiguousarray(state[:, :, a:b])).to(dev)) for a, b in bounds]
    mom_all = torch.stack([_moments(v, s) for v, s in shards]).contiguous()
    mh = mom_all.cpu().numpy()
    mid = R // 2 if R > 2 else 0
    assert (mh[mid, :, 1, 0] == 0).all() and (mh[:-1, :, 2, 0] == 0).all() and (mh[-1, :, 2, 0] > 0).all()
    assert (mh[:, :, 3, 0].sum(0) == 1).all() and (mh[:, :, 4, 0].sum(0) == 2).all()
    outs = [_zscore(v, s, mom_all, R) for v, s in shards]
    gv = np.concatenate([o[0].cpu().numpy() for o in outs], axis=2)
    gs = np.concatenate([o[1].cpu().numpy() for o in outs], axis=2)
    bad = _z_check(gv, gs, rv, rs, exact, f"z/R{R}/S{S_total}")
    fv, fs = torch.from_numpy(val).to(dev), torch.from_numpy(state).to(dev)
    ov, os_ = _zscore(fv, fs, _moments(fv, fs), 1)
    bad += _z_check(ov.cpu().numpy(), os_.cpu().numpy(), rv, rs, exact, f"z/R1/S{S_total}")
    if S_total <= 8192:
        rc, lv, ls = _z_local(val, state, dev)
        assert rc == 0
        bad += _z_check(lv, ls, rv, rs, exact, f"z/local/S{S_total}")
    assert not bad, "\n".join(bad[:20])
