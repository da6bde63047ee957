"""GPU: the stock-sharded half of doc_pdf (csrc/mff_pdf.hip: mff_pdf_sort with R > 1, the
non-fused mff_pdf_count on deduplicated lists, mff_pdf_origin_counts, mff_pdf_finalize_own)
and the frame path past one slice per kernel, at day offsets d0 > 0, exact against the CPU
oracle.

B1  the sharded exchange with more than 12,900 distinct queries per day: several count
    slices around the split key and two origin slices (packed u32 and u64 counters).
B2  d0 > 0: single-rank day batches and sharded windows.
B3  mff_pdf_sort with R > 1 called directly on crafted query sets, a window of days.
B4  the sharded exchange fed by the global-merge sort (M > 32,768 queries per day).
B5  the frame path (mff_pdf_count_frame + mff_pdf_finalize) with two slices each.
Every oracle result is computed once per module."""
import numpy as np
import pytest

from parity import compare
from test_gpu_pdf_sort import _cases, _ord64

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

PDF_NAMES = ["doc_pdf60", "doc_pdf70", "doc_pdf80", "doc_pdf90", "doc_pdf95"]
PDF_KCAP = 12900    # sorted queries per slice of the day-aligned count (csrc/mff_pdf.hip)
PDF_ZQ32 = 12500    # ... of the origin lookup and the frame count (packed counters)
PDF_ZQ = 9160       # ... of mff_pdf_finalize (u64 words)
SORT_BINNED_MAX = 32768  # queries per day the binned sort holds; above: chunk sort + global merge


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def _panel_and_oracle(*args, **kw):
    import mff_oracle as O
    from mff import synth
    panel = synth.make_panel(*args, **kw)
    return panel, O.oracle_stage1(panel, PDF_NAMES)


@pytest.fixture(scope="module")
def wide_two_days():
    """3,400 stocks x 2 days: 14,168 and 13,958 distinct doc_pdf queries per day."""
    return _panel_and_oracle(3400, 2, config=71, ragged=True)


@pytest.fixture(scope="module")
def widest_one_day():
    """6,600 stocks x 1 day: 33,000 queries."""
    return _panel_and_oracle(6600, 1, config=72)


@pytest.fixture(scope="module")
def five_days():
    return _panel_and_oracle(300, 5, ragged=True)


@pytest.fixture(scope="module")
def frame_four_days():
    import mff_oracle as O
    from mff import synth
    panel = synth.make_panel(800, 4, config=12, ragged=True)
    return panel, O.oracle_frame_doc_pdf(panel)


def _run(panel, dev, R, names=PDF_NAMES, **kw):
    """compute_factors of `names` on one rank or on R stock shards (threads sharing the
    device); returns the gathered (val, state) [5][D][S]."""
    from mff import dist, engine, synth
    S = len(panel["codes"])

    def rank_fn(comm):
        sub = panel
        if comm is not None:
            s0, s1 = dist.shard_bounds(S, comm.world_size, comm.rank)
            sub = synth.subpanel(panel, stocks=slice(s0, s1))
        dp = engine.DevicePanel.from_host(sub, dev)
        val, state, _ = engine.compute_factors(dp, names, comm=comm, **kw)
        torch.cuda.synchronize()
        return val.cpu().numpy(), state.cpu().numpy()

    outs = [rank_fn(None)] if R == 1 else dist.run_threads(R, rank_fn)
    return np.concatenate([o[0] for o in outs], axis=2), np.concatenate([o[1] for o in outs], axis=2)


def _exact(gv, gs, ov, os_, tag):
    bad = []
    for i, nm in enumerate(PDF_NAMES):
        bad += compare(gv[i], gs[i], ov[i], os_[i], f"{nm}/{tag}", rtol=0.0, atol=0.0)
    assert not bad, "\n".join(bad[:20])


def _record_phases(monkeypatch):
    """Wrap the device phases of the sharded exchange, calling through; returns the list the
    wrappers append (phase, list width, d0) to."""
    from mff import engine
    seen = []
    sort, count, origin = engine.PdfKernels.sort, engine.PdfKernels.count, engine.PdfKernels.origin

    def sort_w(self, q_all, R, S_all, nd):
        seen.append(("sort", R * 5 * S_all, 0))
        return sort(self, q_all, R, S_all, nd)

    def count_w(self, q_sorted, d0=0):
        seen.append(("count", int(q_sorted.shape[1]), d0))
        return count(self, q_sorted, d0)

    def origin_w(self, q_all, R, S_all, q_sorted, counts):
        seen.append(("origin", int(q_sorted.shape[1]), int(q_sorted.shape[0])))
        return origin(self, q_all, R, S_all, q_sorted, counts)

    monkeypatch.setattr(engine.PdfKernels, "sort", sort_w)
    monkeypatch.setattr(engine.PdfKernels, "count", count_w)
    monkeypatch.setattr(engine.PdfKernels, "origin", origin_w)
    return seen


# B1 --------------------------------------------------------------------------------------

@pytest.mark.parametrize("R,u64", [(2, False), (3, False), (2, True)])
def test_sharded_exchange_past_one_slice(dev, wide_two_days, monkeypatch, R, u64):
    """R = 3: rank 2 owns no day (nd_max = 1).  u64: MFF_PDF_U64=1, the u64 counters of the
    non-fused count (the path of shards wider than 8,738 stocks)."""
    panel, (ov, os_) = wide_two_days
    if u64:
        monkeypatch.setenv("MFF_PDF_U64", "1")
    else:
        monkeypatch.delenv("MFF_PDF_U64", raising=False)
    seen = _record_phases(monkeypatch)
    gv, gs = _run(panel, dev, R)
    widths = [w for ph, w, _ in seen if ph in ("count", "origin")]
    assert len(widths) == 2 * R
    # inputs: more than one full count slice besides the split, at least two origin slices
    assert min(widths) > PDF_KCAP > PDF_ZQ32, widths
    _exact(gv, gs, ov, os_, f"R{R}" + ("/u64" if u64 else ""))


# B2 --------------------------------------------------------------------------------------

def test_single_rank_day_batch_of_one_three_slices(dev, wide_two_days):
    """pdf_day_batch = 1: mff_pdf_sort / mff_pdf_rank_local at d0 = 1, 17,000 queries a day
    (two count slices and the split's)."""
    panel, (ov, os_) = wide_two_days
    assert 5 * len(panel["codes"]) > PDF_KCAP
    gv, gs = _run(panel, dev, 1, pdf_day_batch=1)
    _exact(gv, gs, ov, os_, "batch1")


@pytest.mark.parametrize("R,batch", [(1, 2), (2, 1)])
def test_day_windows(dev, five_days, monkeypatch, R, batch):
    """Five days in windows of 2, 2 and 1: single rank d0 = 0, 2, 4; two ranks count at
    d0 = 0, 2, 4 and the last window's second owner holds only padding."""
    panel, (ov, os_) = five_days
    seen = _record_phases(monkeypatch)
    gv, gs = _run(panel, dev, R, pdf_day_batch=batch)
    if R > 1:
        assert sorted({d0 for ph, _, d0 in seen if ph == "count"}) == [0, 2, 4]
        assert sum(ph == "sort" for ph, _, _ in seen) == 5  # rank 1 owns no day of the last window
    _exact(gv, gs, ov, os_, f"R{R}/batch{batch}")


# B3 --------------------------------------------------------------------------------------

def _sharded_queries(R, S_all, seed):
    """[R][5][7][S_all] crafted queries (the days of test_gpu_pdf_sort._cases over all R * 5 *
    S_all keys), rank r's trailing r + 1 columns NaN (rank 0 full): uneven shards."""
    q = _cases(R * S_all, seed)                       # [5][7][R * S_all]: day d holds 5 R S_all keys
    D = q.shape[1]
    q = q.transpose(1, 0, 2).reshape(D, R, 5, S_all)  # each day's keys as [R][5][S_all]
    q = np.ascontiguousarray(q.transpose(1, 2, 0, 3))
    for r in range(1, R):
        q[r, :, :, S_all - (r + 1):] = np.nan
    return q


@pytest.mark.parametrize("R,S_all", [(2, 700), (3, 1700), (2, 3277), (3, 2185)])
def test_pdf_sort_sharded_direct(dev, R, S_all):
    """(2, 3277): M = 32,770, one past the binned sort; (3, 2185): M = 32,775.  A second call
    sorts days 2 .. 4 of 7 only and leaves the rows behind them untouched."""
    from mff import _lib
    lib = _lib.load()
    q = _sharded_queries(R, S_all, 11 * S_all + R)
    D, M = q.shape[2], R * 5 * S_all
    if S_all in (3277, 2185):
        assert M > SORT_BINNED_MAX
    want = np.stack([np.sort(_ord64(q[:, :, d, :].reshape(-1))) for d in range(D)])
    qd = torch.from_numpy(q).to(dev)
    st = torch.cuda.current_stream(dev).cuda_stream
    fill = 0x5A5A5A5A5A5A5A5A
    for d0, nd in ((0, D), (2, 3)):
        out = torch.full((D, M), fill, dtype=torch.int64, device=dev)
        ws = torch.empty(lib.mff_pdf_workspace_bytes(S_all, R, nd), dtype=torch.uint8, device=dev)
        _lib.check(lib.mff_pdf_sort(_lib.ptr(qd), R, S_all, D, d0, nd, _lib.ptr(out), _lib.ptr(ws), st),
                   "mff_pdf_sort")
        torch.cuda.synchronize()
        got = out.cpu().numpy().view(np.uint64)
        for k in range(nd):
            assert np.array_equal(got[k], want[d0 + k]), \
                f"R={R} S_all={S_all} d0={d0} day {d0 + k}: {int((got[k] != want[d0 + k]).sum())} keys differ"
        assert (got[nd:] == np.uint64(fill)).all(), f"d0={d0}: rows past the {nd} sorted days were written"


# B4 --------------------------------------------------------------------------------------

def test_sharded_exchange_merge_sort(dev, widest_one_day, monkeypatch):
    """R = 2, one day of 33,000 queries: the chunk sort + global merge feeds the dedup, the
    non-fused count and the origin lookup; rank 1 owns no day."""
    panel, (ov, os_) = widest_one_day
    seen = _record_phases(monkeypatch)
    gv, gs = _run(panel, dev, 2)
    sorts = [w for ph, w, _ in seen if ph == "sort"]
    assert sorts == [2 * 5 * 3300] and sorts[0] > SORT_BINNED_MAX
    _exact(gv, gs, ov, os_, "R2/merge")


# B5 --------------------------------------------------------------------------------------

@pytest.mark.parametrize("R", [1, 2])
def test_frame_path_past_one_slice(dev, frame_four_days, R):
    """One frame of 4 days x 800 stocks: M = 16,000 queries in one list, two slices in
    mff_pdf_count_frame and two in mff_pdf_finalize."""
    import mff_oracle as O
    panel, fx = frame_four_days
    M = 5 * 4 * len(panel["codes"])
    assert PDF_ZQ32 < M <= 2 * PDF_ZQ
    gv, gs = _run(panel, dev, R, names=O.FRAME_RANK_NAMES, frame=True)
    bad = []
    for t, nm in enumerate(O.FRAME_RANK_NAMES):
        bad += compare(gv[t], gs[t], *fx[nm], f"{nm}/frame/R{R}", rtol=0.0, atol=0.0)
    assert not bad, "\n".join(bad[:20])
