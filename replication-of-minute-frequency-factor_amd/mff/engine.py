"""Device engine: dense panels in HBM -> libmff.so kernels.

Everything here works on torch tensors that already live on one GPU (torch is only the
buffer / stream carrier); each function issues asynchronous libmff calls on the
current torch stream.  Multi-GPU collectives (doc_pdf frame-wide rank, stage-3
cross-sections) are delegated to a ``comm`` object (:mod:`mff.dist`), so the same code
runs single-GPU (``comm=None``) and stock-sharded.

Stage map:
  :func:`compute_factors`  stage 1, the 58 cal_* of MinuteFrequentFactorCalculateMethodsCICC.py
  :func:`rolling`          stage 2, MinFreqFactor.cal_final_exposure(mode='days') (MF:187-240)
  :func:`cross_section`    stage 3, per-day z-score / average rank
  :func:`neutralize`       per-day MAD winsorise, industry / size neutralise, standardise
"""
from __future__ import annotations

import os
import threading
from dataclasses import dataclass, field
from typing import List, NamedTuple, Optional, Sequence

import numpy as np
import torch

from . import _lib, catalog
from .synth import ROW_DTYPE, ROWS_KEEP, ROWS_NULL_SHIFT, ols_unsorted_cells, pack_mask, row_set, stack_fields

ABSENT, NULL, VALUE = 0, 1, 2
VOLUME_MAX = 2 ** 32 - 2  # MFF_VOLUME_MAX: u32 shares per bar (all-ones = absent sort key)
ROLL_METHODS = {"o": 0, "m": 1, "z": 2, "std": 3}


def _stream(device) -> int:
    return torch.cuda.current_stream(device).cuda_stream


ROWS_MAX = 255  # MFF_ROWS_MAX
ROWS_LISTED = -2 ** 31  # MFF_ROWS_LISTED: mask word 7 of a listed stock-day (int32 view)


def first_row_flags(off: np.ndarray, rows: np.ndarray) -> np.ndarray:
    """uint32 [K]: the row-set flags of each listed stock-day (its first row's `reserved`,
    include/mff.h MFF_ROWS_KEEP; 0 for a stock-day without rows)."""
    off = np.asarray(off, dtype=np.int64)
    fl = np.zeros(len(off) - 1, np.uint32)
    has = off[1:] > off[:-1]
    if has.any():
        fl[has] = rows["reserved"][off[:-1][has]]
    return fl


def _i32(x: torch.Tensor) -> torch.Tensor:
    """u32 values held in int64 -> their int32 bit pattern."""
    return torch.where(x >= 2 ** 31, x - 2 ** 32, x).to(torch.int32)


def mark_listed(mask: torch.Tensor, sd, flags=None) -> None:
    """Clear the mask words of the stock-days ``sd`` (d*S + s) and set their row-set flag
    (include/mff.h MFF_ROWS_LISTED): the grid kernels see them ABSENT and store nothing.
    ``flags`` (optional, [K]): a stock-day whose flags hold MFF_ROWS_KEEP keeps its
    presence bits and gets LISTED | its flags in word 7 -- the grid kernels then store the
    families that read none of its null fields (the same flags must be in its first row's
    ``reserved``: mff_stage1_rows computes the others)."""
    flat = mask.view(-1, 8)
    idx = torch.as_tensor(sd, device=mask.device).long()
    if flags is None:
        flat[idx] = 0
        flat[idx, 7] = ROWS_LISTED
        return
    fl = torch.as_tensor(flags, device=mask.device).to(torch.int64) & 0xFFFFFFFF
    keep = (fl & ROWS_KEEP) != 0
    w = flat[idx].clone()
    w[~keep] = 0
    w7 = w[:, 7].to(torch.int64) & 0xFFFF  # bars 224..239
    w[:, 7] = _i32(torch.where(keep, w7 | (fl & 0x7FFF0000), torch.zeros_like(w7)) | 0x80000000)
    flat[idx] = w


@dataclass
class RowSet:
    """The stock-days of a panel computed from their own rows (include/mff.h, row set):
    those holding a polars null (a row that exists with a null field) and those with a row
    off the 240-bar grid or at a duplicate time.  ``sd`` int32 [K] (d*S + s, ascending),
    ``off`` int32 [K+1], ``rows`` the MffRow records (32 B each, a uint8 tensor [R*32]) in
    (time, frame) order per stock-day.  The panel's own mask holds zeros there.  All on the
    panel's device."""

    sd: torch.Tensor
    off: torch.Tensor
    rows: torch.Tensor

    @property
    def K(self) -> int:
        return int(self.sd.numel())

    @classmethod
    def from_host(cls, sd, off, rows, device) -> Optional["RowSet"]:
        """sd int [K], off int [K+1], rows ROW_DTYPE [R] numpy -> device (None when K = 0)."""
        if len(sd) == 0:
            return None
        rows = np.ascontiguousarray(rows, dtype=ROW_DTYPE)
        t = lambda a_: torch.from_numpy(np.ascontiguousarray(a_, dtype=np.int32)).to(device)
        return cls(t(sd), t(off), torch.from_numpy(rows.view(np.uint8).reshape(-1).copy()).to(device))

    def host(self):
        """(sd int64 [K], off int64 [K+1], rows ROW_DTYPE [R]) numpy copies."""
        return (self.sd.cpu().numpy().astype(np.int64), self.off.cpu().numpy().astype(np.int64),
                self.rows.cpu().numpy().view(ROW_DTYPE).copy())

    def shard(self, S: int, s0: int, s1: int, device=None) -> Optional["RowSet"]:
        """The listed stock-days of stocks [s0, s1) re-indexed to a shard of s1 - s0 stocks."""
        sd, off, rows = self.host()
        d, s = sd // S, sd % S
        keep = np.flatnonzero((s >= s0) & (s < s1))
        nsd = d[keep] * (s1 - s0) + (s[keep] - s0)
        parts = [rows[off[i]:off[i + 1]] for i in keep]
        n = np.array([len(x) for x in parts], dtype=np.int64)
        noff = np.concatenate([[0], np.cumsum(n)])
        nrows = np.concatenate(parts) if parts else np.zeros(0, ROW_DTYPE)
        return RowSet.from_host(nsd, noff, nrows, device or self.sd.device)

    @classmethod
    def from_panel(cls, bars: torch.Tensor, mask: torch.Tensor, sd: torch.Tensor,
                   null_bits: Optional[torch.Tensor] = None, clear: bool = True,
                   keep: bool = True) -> "RowSet":
        """List the grid stock-days ``sd`` (int32 device tensor, ascending) of a device panel
        as rows (mff_rows_from_panel), with optional null bits int32 [K][5][8]; ``clear``:
        mark them in the mask (mark_listed): ``keep`` -- a stock-day with a null on a present
        bar keeps its grid bars and only the families reading a null field come from its
        rows (MFF_ROWS_KEEP in word 7 and its first row); every other one is zeroed (the
        grid kernels see it ABSENT)."""
        lib = _lib.load()
        D, S = int(bars.shape[1]), int(bars.shape[2])
        K = int(sd.numel())
        dev = bars.device
        st = _stream(dev)
        counts = torch.empty(K, dtype=torch.int32, device=dev)
        b = bars
        _lib.check(lib.mff_rows_from_panel(None, None, None, None, None, _lib.ptr(mask), S, D, _lib.ptr(sd),
                                           None, K, None, _lib.ptr(counts), None, st), "mff_rows_from_panel(count)")
        off = torch.zeros(K + 1, dtype=torch.int32, device=dev)
        off[1:] = torch.cumsum(counts, 0)
        R = int(off[-1].item())
        rows = torch.empty(max(R, 1) * ROW_DTYPE.itemsize, dtype=torch.uint8, device=dev)
        _lib.check(lib.mff_rows_from_panel(_lib.ptr(b[0]), _lib.ptr(b[1]), _lib.ptr(b[2]), _lib.ptr(b[3]),
                                           _lib.ptr(b[4]), _lib.ptr(mask), S, D, _lib.ptr(sd), _lib.ptr(null_bits),
                                           K, _lib.ptr(off), None, _lib.ptr(rows), st), "mff_rows_from_panel")
        flags = None
        if keep and null_bits is not None and K > 0:
            pres = mask.view(-1, 8)[sd.long()].to(torch.int64) & 0xFFFFFFFF  # before marking
            nb = (null_bits.view(K, 5, 8).to(torch.int64) & 0xFFFFFFFF) & pres[:, None, :]
            fields = ((nb != 0).any(dim=2).to(torch.int64) << torch.arange(5, device=dev)).sum(dim=1)
            has = (fields != 0) & (off[1:] > off[:-1])
            flags = torch.where(has, ROWS_KEEP | (fields << ROWS_NULL_SHIFT), torch.zeros_like(fields))
            if bool(has.any()):
                first = off[:-1].long()[has]
                rows.view(torch.int32).view(-1, 8)[first, 7] = _i32(flags[has])
        if clear:
            mark_listed(mask, sd, flags)
        return cls(sd, off, rows)


@dataclass
class DevicePanel:
    """One device's dense panel.

    bars: [5][D][S][240] 4-byte words: open, high, low, close (float32) and the volume
          plane's u32 shares (include/mff.h); a float32 tensor, plane 4 viewed as ints
    mask: int32 [D][S][8] presence bits (bit m%32 of word m//32); zero for the stock-days
          listed in ``rows``
    rows: the row set -- the stock-days computed from their own rows (nulls, rows off the
          grid or at a duplicate time; mff_stage1_rows), or None
    """

    bars: torch.Tensor
    mask: torch.Tensor
    codes: List[str] = field(default_factory=list)
    dates: List = field(default_factory=list)
    # ingest with skip_bad: {input table index: reason} of the tables dropped (the
    # stock-day cells a dropped table wrote hold no bars; other tables' cells of the same
    # dates keep theirs)
    dropped: dict = field(default_factory=dict)
    rows: Optional[RowSet] = None
    # stock-sharded panels: the number of stocks over all ranks (shards by
    # dist.shard_bounds), so the exchange's padded shard width is known without a
    # collective; None = agree on it with one all-reduce
    stocks_total: Optional[int] = None
    # T2 (oracle/mff_oracle.py): the cells (int64 d*S + s, on the device) of every frame
    # whose minute_in_trade decreases inside a stock-day -- the reference's five
    # cal_mmt_ols_* calls raise on such a frame (rolling(), CM:114-118), so their rows of
    # the whole frame come out ABSENT; the other 53 factors are computed as usual
    ols_drop: Optional[torch.Tensor] = None
    # {input table index: (factor names, reason)} of those frames (ingest)
    partial: dict = field(default_factory=dict)

    @property
    def D(self) -> int:
        return int(self.bars.shape[1])

    @property
    def S(self) -> int:
        return int(self.bars.shape[2])

    @property
    def device(self):
        return self.bars.device

    def plane(self, k: int) -> torch.Tensor:
        return self.bars[k]

    @classmethod
    def from_host(cls, panel, device="cuda") -> "DevicePanel":
        """Host dict (see :mod:`mff.synth`) -> device tensors.  Validates the input
        contract the kernels rely on (include/mff.h)."""
        validate_host_panel(panel)
        bars = torch.from_numpy(np.ascontiguousarray(stack_fields(panel))).to(device)
        words = pack_mask(panel["present"])
        sd, off, rows = row_set(panel)
        if sd.size:  # the listed stock-days go to mff_stage1_rows (MFF_ROWS_LISTED / KEEP)
            w = words.reshape(-1, 8)
            fl = first_row_flags(off, rows)
            keep = (fl & ROWS_KEEP) != 0
            w[sd[~keep]] = 0
            w[sd[keep], 7] = (w[sd[keep], 7] & np.uint32(0xFFFF)) | (fl[keep] & np.uint32(0x7FFF0000))
            w[sd, 7] |= np.uint32(0x80000000)
        mask = torch.from_numpy(words.view(np.int32)).to(device)
        dp = cls(bars, mask, list(panel["codes"]), list(panel["dates"]),
                 rows=RowSet.from_host(sd, off, rows, device))
        bad = ols_unsorted_cells(panel)
        if bad.size:  # T2, one reference frame per day: every cell of those days
            D, S = panel["present"].shape[:2]
            days = np.unique(bad // S)
            cells = (days[:, None] * S + np.arange(S)[None, :]).reshape(-1)
            dp.ols_drop = torch.from_numpy(cells.astype(np.int64)).to(device)
        return dp


def validate_host_panel(panel) -> None:
    pres = panel["present"]
    nb = panel.get("null")
    ok = lambda i: pres if nb is None else pres & ((nb >> i) & 1 == 0)  # non-null present bars
    v = np.asarray(panel["volume"][ok(4)], dtype=np.float64)
    if v.size and (not np.all(np.isfinite(v)) or np.any(v < 0) or np.any(v > VOLUME_MAX)
                   or np.any(v != np.rint(v))):
        raise ValueError(f"volume must be integral and within [0, {VOLUME_MAX}] shares")
    for i, k in enumerate(("open", "high", "low", "close")):
        x = panel[k][ok(i)]
        if x.size and (not np.all(np.isfinite(x)) or np.any(x <= 0)):
            raise ValueError(f"{k} must be finite and > 0 on present bars")


def compute_factors(panel: DevicePanel, names: Optional[Sequence[str]] = None, comm=None,
                    pdf_day_batch: Optional[int] = None, events=None, frame: bool = False):
    """Stage 1 for the requested factors (default: all 58, reference order).

    ``frame``: the panel's D days are ONE reference frame (a cal_* handed a multi-date
    frame): doc_pdf60..95 rank over every row of every date (CM:1015-1017, `.rank()`
    outside `.over`) instead of per day (:func:`pdf_ranks_frame`).  Default: per day, the
    driver's one-call-per-day-file semantics (MF:22).

    ``events``: optional (start, end) torch.cuda.Event pair recorded on the launch stream
    around the whole stage-1 pass: every stage-1 launch and the doc_pdf rank phases
    (the end event follows the side stream's doc_pdf tail; bench.py's roofline timing).
    Returns (val float64 [nf][D][S], state uint8 [nf][D][S], ids)."""
    lib = _lib.load()
    ids = catalog.resolve(names)
    nf, D, S = len(ids), panel.D, panel.S
    dev = panel.device
    val = torch.empty((nf, D, S), dtype=torch.float64, device=dev)
    state = torch.empty((nf, D, S), dtype=torch.uint8, device=dev)
    need_pdf = any(i in catalog.PDF_IDS for i in ids)
    pdfq = torch.empty((5, D, S), dtype=torch.float64, device=dev) if need_pdf else None
    levels = (torch.empty(lib.mff_pdf_levels_bytes(S, D), dtype=torch.uint8, device=dev)
              if need_pdf else None)
    b = panel.bars
    ws = torch.empty(lib.mff_stage1_workspace_bytes(S, D), dtype=torch.uint8, device=dev)
    main = torch.cuda.current_stream(dev)
    args = [_lib.ptr(b[0]), _lib.ptr(b[1]), _lib.ptr(b[2]), _lib.ptr(b[3]), _lib.ptr(b[4]),
            _lib.ptr(panel.mask), S, D, _lib.int_array(ids), nf, _lib.ptr(val), _lib.ptr(state),
            _lib.ptr(pdfq), _lib.ptr(levels), _lib.ptr(ws), main.cuda_stream]
    rows = [ids.index(i) if i in ids else -1 for i in catalog.PDF_IDS]
    frame_pdf = frame and need_pdf and D > 1
    rs = panel.rows

    def rows_phase(phase: int, stream) -> None:
        """mff_stage1_rows for the row set's stock-days (ABSENT to every other launch):
        phase 1 = doc_pdf queries + levels (before the doc_pdf sort), 2 = the other rows
        (after every launch that writes them)."""
        if rs is None or (phase == 1 and not need_pdf):
            return
        _lib.check(lib.mff_stage1_rows(S, D, _lib.ptr(rs.sd), _lib.ptr(rs.off), _lib.ptr(rs.rows), rs.K,
                                       _lib.int_array(ids), nf, _lib.ptr(val), _lib.ptr(state),
                                       _lib.ptr(pdfq), _lib.ptr(levels), phase, stream.cuda_stream),
                   f"mff_stage1_rows({phase})")

    if events is not None:
        events[0].record(main)
    if need_pdf and not frame_pdf and not SERIAL:
        # Three streams.  Set H (OLS, MOMH: high / low only, its own rows only) from the
        # start on a high-priority stream: its blocks fill the registers the other
        # launches leave.  The sorted-group kernel (ORD thresholds, doc_pdf queries and
        # level lists) on the launch stream; then, on the doc_pdf side stream, the exact
        # list (LVL / PDF of the listed stock-days) and the doc_pdf sort, after which the
        # wave pair (which reads the ORD thresholds) starts on the launch stream while the
        # doc_pdf count runs beside it.  The row set's kernels (ABSENT to every grid
        # launch: MFF_ROWS_LISTED) run on their own stream from the level-list prologue on;
        # the sort waits for their queries and levels.  (Launch orders, priorities and
        # stream splits measured equal or slower are in DESIGN.md §5.)
        hl = _side_stream(dev, 1)
        hl.wait_stream(main)
        _lib.check(lib.mff_stage1_part(*(args[:-1] + [hl.cuda_stream]), 4), "mff_stage1_part(4)")
        part1 = 17
        rows_st = None
        if rs is not None:
            _lib.check(lib.mff_stage1_part(*args, 64), "mff_stage1_part(64)")
            rows_st = _side_stream(dev, 2)
            rows_st.wait_stream(main)
            rows_phase(3, rows_st)
            part1 |= 128
        _lib.check(lib.mff_stage1_part(*args, part1), "mff_stage1_part(1)")
        side = _side_stream(dev)
        side.wait_stream(main)
        _lib.check(lib.mff_stage1_part(*(args[:-1] + [side.cuda_stream]), 32), "mff_stage1_part(32)")
        if rows_st is not None:
            side.wait_stream(rows_st)  # the row set's queries and levels before the sort
        sorted_ev = torch.cuda.Event()
        with torch.cuda.stream(side):
            pdf_ranks(panel, pdfq, levels, rows, val, state, comm=comm, day_batch=pdf_day_batch,
                      after_sort=lambda: sorted_ev.record(side))
        main.wait_event(sorted_ev)  # the pair after the doc_pdf sort
        _lib.check(lib.mff_stage1_part(*args, 10), "mff_stage1_part(2)")
        main.wait_stream(side)
        main.wait_stream(hl)
        if rows_st is not None:
            main.wait_stream(rows_st)
    else:
        _lib.check(lib.mff_stage1(*args), "mff_stage1")
        rows_phase(1, main)
        if frame_pdf:
            pdf_ranks_frame(panel, pdfq, levels, rows, val, state, comm=comm)
        elif need_pdf:
            pdf_ranks(panel, pdfq, levels, rows, val, state, comm=comm, day_batch=pdf_day_batch)
        rows_phase(2, main)
    drop_ols(panel, ids, val, state, comm)
    if events is not None:  # after the doc_pdf tail on the side stream
        events[1].record(main)
    return val, state, ids


def drop_ols(panel: DevicePanel, ids: Sequence[int], val, state, comm=None) -> None:
    """T2: the five OLS rows of every frame whose minute_in_trade decreases inside a
    stock-day come out ABSENT for the whole frame (``panel.ols_drop``): the reference's
    cal_mmt_ols_* call raises on that frame and the driver drops it (MF:18-25, 95).  Stock
    shards (``comm``): a day frame spans every shard, so the days holding such a
    stock-day on any rank are agreed by one all-reduce (max) of a [D] flag vector."""
    rows = [r for r, i in enumerate(ids) if i in catalog.OLS_IDS]
    if not rows:
        return
    cells = panel.ols_drop
    if comm is not None:
        bad = torch.zeros(panel.D, dtype=torch.int32, device=panel.device)
        if cells is not None and cells.numel():
            bad[cells // panel.S] = 1
        comm.all_reduce_max(bad)
        for r in rows:
            state[r].masked_fill_(bad[:, None] != 0, ABSENT)
            val[r].masked_fill_(bad[:, None] != 0, 0.0)
        return
    if cells is None or cells.numel() == 0:
        return
    for r in rows:
        state[r].view(-1)[cells] = ABSENT
        val[r].view(-1)[cells] = 0.0


# MFF_STAGE1_SERIAL=1: every stage-1 launch on the launch stream, one after another (the
# standalone per-kernel durations of profiles/gpu_r3_prof.sh; results are identical,
# tests/test_gpu_schedules.py)
SERIAL = os.environ.get("MFF_STAGE1_SERIAL", "0") != "0"
# the high / low stream runs at high priority: its blocks are dispatched ahead of the pair's
# and the doc_pdf count's, so its long walk does not end last (+1.8 % pass, round 3)
HL_PRIO = -1

_SIDE = {}


def _side_stream(dev, which: int = 0) -> torch.cuda.Stream:
    key = (dev.index, threading.get_ident(), which)
    if key not in _SIDE:
        _SIDE[key] = torch.cuda.Stream(dev, priority=HL_PRIO if which == 1 else 0)
    return _SIDE[key]


def stage1_frame(panel: DevicePanel, ids: Sequence[int], val, state) -> None:
    """Overwrite the rows of the four factors whose windows run over('code') only
    (liq_amihud_1min, corr_prvr, trade_bottom20/50retRatio) with the semantics of ONE
    reference call on the panel's multi-date frame (mff_stage1_frame, csrc/mff_frame.hip),
    row-set stock-days included."""
    lib = _lib.load()
    b, rs = panel.bars, panel.rows
    _lib.check(lib.mff_stage1_frame(_lib.ptr(b[0]), _lib.ptr(b[3]), _lib.ptr(b[4]), _lib.ptr(panel.mask),
                                    panel.S, panel.D, _lib.ptr(rs.sd) if rs else None,
                                    _lib.ptr(rs.off) if rs else None, _lib.ptr(rs.rows) if rs else None,
                                    rs.K if rs else 0, _lib.int_array(list(ids)), len(ids), _lib.ptr(val),
                                    _lib.ptr(state), _stream(panel.device)), "mff_stage1_frame")


def pdf_ranks(panel: DevicePanel, pdfq: torch.Tensor, levels: torch.Tensor, rows: List[int], val, state,
              comm=None,
              day_batch: Optional[int] = None, workspace_budget: int = 2 << 30, after_sort=None):
    """doc_pdf frame-wide ranks (CM:1015-1017) for all days, in day batches.  ``after_sort``:
    optional callable, invoked once the first day batch's sort is enqueued (sharded: the
    first window's sort of this rank's days)."""
    lib = _lib.load()
    D, S = panel.D, panel.S
    dev = panel.device
    R = 1 if comm is None else comm.world_size
    S_all = S if comm is None else shard_width(comm, S, panel.stocks_total, dev)
    M = R * 5 * S_all
    st = _stream(dev)
    if comm is not None:
        if day_batch is None:
            # per day of a window: gathered + sorted lists (i64), counts + their copy by
            # owner (i32), the sort's ping-pong buffer
            per_day = 2 * M * 8 + 2 * M * 4 + lib.mff_pdf_workspace_bytes(S_all, R, 1)
            day_batch = max(1, workspace_budget // max(per_day, 1))
        _pdf_ranks_sharded(comm, pdfq, S_all, PdfKernels(lib, levels, S, D, rows, val, state, st),
                           day_batch=day_batch, after_sort=after_sort)
        return
    if day_batch is None:
        per_day = lib.mff_pdf_workspace_bytes(S, R, 1) + M * 8 + M * 8
        day_batch = max(1, min(D, workspace_budget // max(per_day, 1)))
    for d0 in range(0, D, day_batch):
        nd = min(day_batch, D - d0)
        ws = torch.empty(lib.mff_pdf_workspace_bytes(S, R, nd), dtype=torch.uint8, device=dev)
        q_sorted = torch.empty((nd, M), dtype=torch.int64, device=dev)
        _lib.check(lib.mff_pdf_sort(_lib.ptr(pdfq), R, S_all, D, d0, nd, _lib.ptr(q_sorted),
                                    _lib.ptr(ws), st), "mff_pdf_sort")
        if after_sort is not None and d0 == 0:
            after_sort()
        # single rank: count + finalize fused, no exchange
        _lib.check(lib.mff_pdf_rank_local(_lib.ptr(levels), _lib.ptr(pdfq), S, D, d0, nd,
                                          _lib.ptr(q_sorted), M,
                                          _lib.int_array(rows), _lib.ptr(val), _lib.ptr(state), st),
                   "mff_pdf_rank_local")


NBAR = 240
PDF_MAX_QUERIES = 1 << 24  # mff_pdf_count_frame: queries of one sorted list (PDF_MAXM)


def _pdf_ranks_frame_chunked(lib, panel, pdfq, levels, rows, val, state, chunk_days: int) -> None:
    """pdf_ranks_frame for a frame whose 5*S*D queries exceed one sorted list: the rank of
    a query is n_less + (n_eq + 1) / 2 over ALL keys of the frame, whatever list it sits
    in, so the queries go in day chunks -- each chunk's queries sorted as one list and
    counted against the level keys of every day of the frame -- and each chunk's ranks are
    written row by row (its [5][Dc][S] queries copied to one contiguous list)."""
    D, S = panel.D, panel.S
    dev = panel.device
    st = _stream(dev)
    plane = D * S
    for d0 in range(0, D, chunk_days):
        d1 = min(D, d0 + chunk_days)
        DS = (d1 - d0) * S
        M = 5 * DS
        qc = pdfq[:, d0:d1].contiguous()  # [5][Dc][S] = the one-day view [5][1][Dc*S]
        ws = torch.empty(lib.mff_pdf_workspace_bytes(DS, 1, 1), dtype=torch.uint8, device=dev)
        q_sorted = torch.empty((1, M), dtype=torch.int64, device=dev)
        _lib.check(lib.mff_pdf_sort(_lib.ptr(qc), 1, DS, 1, 0, 1, _lib.ptr(q_sorted), _lib.ptr(ws), st),
                   "mff_pdf_sort(frame chunk)")
        counts = torch.zeros((1, M), dtype=torch.int32, device=dev)
        _lib.check(lib.mff_pdf_count_frame(_lib.ptr(levels), S, D, _lib.ptr(q_sorted), M, _lib.ptr(counts), st),
                   "mff_pdf_count_frame(chunk)")
        for t, r in enumerate(rows):  # one output row at a time: its chunk is contiguous
            if r < 0:
                continue
            one = [-1] * 5
            one[t] = 0
            off = r * plane + d0 * S
            _lib.check(lib.mff_pdf_finalize(_lib.ptr(qc), _lib.ptr(q_sorted), _lib.ptr(counts), DS, 1, 0, 1, M,
                                            _lib.int_array(one), val.data_ptr() + 8 * off,
                                            state.data_ptr() + off, st), "mff_pdf_finalize(frame chunk)")


def _pdf_ranks_frame_sharded(lib, comm, panel, pdfq, levels, rows, val, state,
                             chunk_days: Optional[int] = None) -> None:
    """pdf_ranks_frame over stock shards (CM:1015-1017: `.rank()` spans every row of every
    date and every code): per chunk of days, every rank's queries are all-gathered and
    sorted as ONE list (on every rank: this is the drop-in surface's multi-date frame, not
    the batched driver), each rank adds its own level keys of EVERY day of the frame to the
    words 2 n_less + n_eq at the list's positions (mff_pdf_count_frame), the words are
    summed over ranks (all-reduce) and each rank writes its own stock-days' ranks."""
    D, S = panel.D, panel.S
    dev = panel.device
    st = _stream(dev)
    R = comm.world_size
    S_all = shard_width(comm, S, panel.stocks_total, dev)
    if NBAR * S_all * R * D >= 2 ** 31:
        raise ValueError(f"a frame of {D} dates x {S_all * R} codes is too large for one frame-wide doc_pdf rank")
    if chunk_days is None:
        chunk_days = max(1, PDF_MAX_QUERIES // (5 * S_all * R))
    plane = D * S
    for d0 in range(0, D, chunk_days):
        d1 = min(D, d0 + chunk_days)
        Dc = d1 - d0
        q_own = pdfq[:, d0:d1].contiguous()  # [5][Dc][S]: one day of Dc * S stocks
        q_all = comm.all_gather(_pad_last(q_own, S_all, float("nan")))  # [R][5][Dc][S_all]
        M = R * 5 * Dc * S_all
        ws = torch.empty(lib.mff_pdf_workspace_bytes(Dc * S_all, R, 1), dtype=torch.uint8, device=dev)
        q_sorted = torch.empty((1, M), dtype=torch.int64, device=dev)
        _lib.check(lib.mff_pdf_sort(_lib.ptr(q_all), R, Dc * S_all, 1, 0, 1, _lib.ptr(q_sorted), _lib.ptr(ws), st),
                   "mff_pdf_sort(frame, sharded)")
        del q_all
        counts = torch.zeros((1, M), dtype=torch.int32, device=dev)
        _lib.check(lib.mff_pdf_count_frame(_lib.ptr(levels), S, D, _lib.ptr(q_sorted), M, _lib.ptr(counts), st),
                   "mff_pdf_count_frame(sharded)")
        comm.all_reduce_sum(counts)
        for t, r in enumerate(rows):  # one output row at a time: its chunk is contiguous
            if r < 0:
                continue
            one = [-1] * 5
            one[t] = 0
            off = r * plane + d0 * S
            _lib.check(lib.mff_pdf_finalize(_lib.ptr(q_own), _lib.ptr(q_sorted), _lib.ptr(counts), Dc * S, 1, 0, 1,
                                            M, _lib.int_array(one), val.data_ptr() + 8 * off,
                                            state.data_ptr() + off, st), "mff_pdf_finalize(frame, sharded)")


def pdf_ranks_frame(panel: DevicePanel, pdfq: torch.Tensor, levels: torch.Tensor, rows: List[int], val,
                    state, chunk_days: Optional[int] = None, comm=None):
    """doc_pdf ranks of a multi-date frame taken as ONE reference frame: `.rank()`
    (CM:1015-1017) is outside any `.over`, so a frame holding D dates ranks every row of
    every date.  The D days' 5*S queries are sorted as one list ([5][D][S] viewed as one
    day of D*S stocks), every day's level keys are counted against it (the words
    2 n_less + n_eq add up over days, mff_pdf_count_frame) and the ranks are written
    through the same one-day view of the output rows.  Beyond PDF_MAX_QUERIES queries
    (about 670 dates of 5,000 codes) the queries go in day chunks of ``chunk_days``
    (:func:`_pdf_ranks_frame_chunked`)."""
    lib = _lib.load()
    if comm is not None:
        _pdf_ranks_frame_sharded(lib, comm, panel, pdfq, levels, rows, val, state, chunk_days)
        return
    D, S = panel.D, panel.S
    dev = panel.device
    st = _stream(dev)
    if NBAR * S * D >= 2 ** 31:  # mff_pdf_count_frame: the words 2 n_less + n_eq stay in u32
        raise ValueError(f"a frame of {D} dates x {S} codes is too large for one frame-wide doc_pdf "
                         f"rank (240 * codes * dates must stay below 2^31); pass the day files as a "
                         f"list (per-day semantics) or split the frame by date")
    if chunk_days is None:
        chunk_days = max(1, PDF_MAX_QUERIES // (5 * S))
    if D > chunk_days:
        _pdf_ranks_frame_chunked(lib, panel, pdfq, levels, rows, val, state, chunk_days)
        return
    DS = D * S
    M = 5 * DS
    ws = torch.empty(lib.mff_pdf_workspace_bytes(DS, 1, 1), dtype=torch.uint8, device=dev)
    q_sorted = torch.empty((1, M), dtype=torch.int64, device=dev)
    _lib.check(lib.mff_pdf_sort(_lib.ptr(pdfq), 1, DS, 1, 0, 1, _lib.ptr(q_sorted), _lib.ptr(ws), st),
               "mff_pdf_sort(frame)")
    counts = torch.zeros((1, M), dtype=torch.int32, device=dev)
    _lib.check(lib.mff_pdf_count_frame(_lib.ptr(levels), S, D, _lib.ptr(q_sorted), M, _lib.ptr(counts), st),
               "mff_pdf_count_frame")
    _lib.check(lib.mff_pdf_finalize(_lib.ptr(pdfq), _lib.ptr(q_sorted), _lib.ptr(counts), DS, 1, 0, 1, M,
                                    _lib.int_array(rows), _lib.ptr(val), _lib.ptr(state), st),
               "mff_pdf_finalize(frame)")


def stage1_launch_times(panel: DevicePanel):
    """The stage-1 launches of all 58 factors one after another on the current stream
    (no overlap), each bracketed by HIP events: the per-kernel standalone durations and
    algorithmic bytes bench.py reports beside the pass (the pass itself overlaps them on
    three streams).  Returns {kernel: {"ms", "bytes"}}; bytes per stock-day are
    SURVEY §8(d)'s: the mask (32 B) + 960 B per plane a kernel reads + 9 B per output row,
    plus the doc_pdf side channel each doc_pdf launch reads or writes (queries 8 B x 5,
    the level list 9 B per level, counted from the launch's own output)."""
    lib = _lib.load()
    ids = catalog.resolve(None)
    nf, D, S = len(ids), panel.D, panel.S
    dev = panel.device
    st = torch.cuda.current_stream(dev)
    val = torch.empty((nf, D, S), dtype=torch.float64, device=dev)
    state = torch.empty((nf, D, S), dtype=torch.uint8, device=dev)
    pdfq = torch.empty((5, D, S), dtype=torch.float64, device=dev)
    levels = torch.empty(lib.mff_pdf_levels_bytes(S, D), dtype=torch.uint8, device=dev)
    ws = torch.empty(lib.mff_stage1_workspace_bytes(S, D), dtype=torch.uint8, device=dev)
    b = panel.bars
    args = [_lib.ptr(b[0]), _lib.ptr(b[1]), _lib.ptr(b[2]), _lib.ptr(b[3]), _lib.ptr(b[4]),
            _lib.ptr(panel.mask), S, D, _lib.int_array(ids), nf, _lib.ptr(val), _lib.ptr(state),
            _lib.ptr(pdfq), _lib.ptr(levels), _lib.ptr(ws), st.cuda_stream]
    rows = [ids.index(i) for i in catalog.PDF_IDS]
    M = 5 * S
    q_sorted = torch.empty((D, M), dtype=torch.int64, device=dev)
    sws = torch.empty(lib.mff_pdf_workspace_bytes(S, 1, D), dtype=torch.uint8, device=dev)
    steps = [
        ("k_stage1g<ORD|ORDV|LVL|PDF>", lambda: _lib.check(lib.mff_stage1_part(*args, 17), "part 17")),
        ("k_stage1 (exact list)", lambda: _lib.check(lib.mff_stage1_part(*args, 32), "part 32")),
        ("k_pdf_sort", lambda: _lib.check(lib.mff_pdf_sort(_lib.ptr(pdfq), 1, S, D, 0, D, _lib.ptr(q_sorted),
                                                            _lib.ptr(sws), st.cuda_stream), "sort")),
        ("k_pdf_count<fused>", lambda: _lib.check(lib.mff_pdf_rank_local(
            _lib.ptr(levels), _lib.ptr(pdfq), S, D, 0, D, _lib.ptr(q_sorted), M, _lib.int_array(rows),
            _lib.ptr(val), _lib.ptr(state), st.cuda_stream), "rank_local")),
        ("k_stage1s<OLS|MOMH>", lambda: _lib.check(lib.mff_stage1_part(*(args[:-1] + [st.cuda_stream]), 4),
                                                   "part 4")),
        ("k_stage1s_pair", lambda: _lib.check(lib.mff_stage1_part(*args, 10), "part 10")),
    ]
    evs = [torch.cuda.Event(enable_timing=True) for _ in range(len(steps) + 1)]
    evs[0].record(st)
    for i, (_, fn) in enumerate(steps):
        fn()
        evs[i + 1].record(st)
    torch.cuda.synchronize(dev)
    nlev = int(levels[:8 * D].view(torch.int32).to(torch.int64).sum().item())  # lists A + B per day
    sd = S * D
    fam_rows = {}
    for i in ids:
        fam_rows[catalog.FAMILY[catalog.NAMES[i]]] = fam_rows.get(catalog.FAMILY[catalog.NAMES[i]], 0) + 1
    nrows = lambda fams: sum(fam_rows.get(f, 0) for f in fams)
    plane = 960
    bytes_ = {
        # c, v planes + mask; ORD / ORDV / LVL rows and the five doc_pdf rows (NULL, filled
        # later); the queries; the level list (key 8 B + bars 1 B)
        "k_stage1g<ORD|ORDV|LVL|PDF>": sd * (32 + 2 * plane + 9 * (nrows(("ORDV", "LVL")) + 5) + 40) + 9 * nlev,
        "k_stage1 (exact list)": 0,
        "k_pdf_sort": sd * (40 + 40),
        "k_pdf_count<fused>": 9 * nlev + sd * (40 + 40 + 9 * 5),
        "k_stage1s<OLS|MOMH>": sd * (32 + 2 * plane + 9 * nrows(("OLS", "MOMH"))),
        "k_stage1s_pair": sd * (32 + 3 * plane + 9 * (nf - nrows(("ORDV", "LVL", "PDF", "OLS", "MOMH"))) + 12),
    }
    return {name: {"ms": evs[i].elapsed_time(evs[i + 1]), "bytes": bytes_[name]}
            for i, (name, _) in enumerate(steps)}


class PdfKernels:
    """The device phases of the stock-sharded doc_pdf rank (libmff, this rank's stream).
    `_pdf_ranks_sharded` only moves tensors between these phases and the collectives, so
    tests drive the same exchange with CPU stand-ins for the phases (gloo, world 2)."""

    def __init__(self, lib, levels, S_loc: int, D: int, rows, val, state, st):
        self.lib, self.levels, self.S, self.D = lib, levels, S_loc, D
        self.rows, self.val, self.state, self.st = rows, val, state, st

    def sort(self, q_all, R: int, S_all: int, nd: int):
        """q_all [R][5][nd_max][S_all] -> total-order keys of days 0..nd sorted, int64 [nd][M]."""
        lib, dev = self.lib, q_all.device
        M = R * 5 * S_all
        out = torch.empty((nd, M), dtype=torch.int64, device=dev)
        ws = torch.empty(lib.mff_pdf_workspace_bytes(S_all, R, nd), dtype=torch.uint8, device=dev)
        _lib.check(lib.mff_pdf_sort(_lib.ptr(q_all), R, S_all, int(q_all.shape[2]), 0, nd, _lib.ptr(out),
                                    _lib.ptr(ws), self.st), "mff_pdf_sort")
        return out

    def count(self, q_sorted, d0: int = 0):
        """This rank's level keys of days d0 .. d0 + nd against each of those days' full
        sorted list (q_sorted [nd][M]): int32 [nd][M] = 2 n_less + n_eq at each value's
        first sorted position."""
        nd, M = q_sorted.shape
        counts = torch.empty((nd, M), dtype=torch.int32, device=q_sorted.device)
        ws = torch.empty(256, dtype=torch.uint8, device=q_sorted.device)
        _lib.check(self.lib.mff_pdf_count(_lib.ptr(self.levels), self.S, self.D, d0, nd, _lib.ptr(q_sorted), M,
                                          _lib.ptr(counts), _lib.ptr(ws), self.st), "mff_pdf_count")
        return counts

    def origin(self, q_all, R: int, S_all: int, q_sorted, counts):
        """Counts of the owned days' lists at every query's position, in the queries'
        origin layout int32 [R][5][nd_max][S_all]."""
        nd_max, M = q_sorted.shape
        out = torch.empty((R, 5, nd_max, S_all), dtype=torch.int32, device=q_all.device)
        _lib.check(self.lib.mff_pdf_origin_counts(_lib.ptr(q_all), R, S_all, nd_max, 0, nd_max,
                                                  _lib.ptr(q_sorted), _lib.ptr(counts), M, _lib.ptr(out),
                                                  self.st), "mff_pdf_origin_counts")
        return out

    def finalize(self, q_local, own_counts):
        """own_counts int32 [5][D][S_loc] -> the doc_pdf rows of val / state."""
        _lib.check(self.lib.mff_pdf_finalize_own(_lib.ptr(q_local), _lib.ptr(own_counts), self.S, self.D,
                                                 _lib.int_array(self.rows), _lib.ptr(self.val),
                                                 _lib.ptr(self.state), self.st), "mff_pdf_finalize_own")


def _pdf_ranks_sharded(comm, pdfq, S_all: int, kern, day_batch: Optional[int] = None, after_sort=None):
    """doc_pdf across stock shards.  The days go in windows of at most
    ``day_batch`` x R days (the exchange buffers below are O(window x M) per rank; None:
    one window); inside a window, day d is owned by the rank whose contiguous day block
    holds it:
      1. all_to_all: every rank's queries of the owner's days -> the owner, which sorts
         them (the sort is not replicated: 1/R of the days per rank);
      2. all_gather of the sorted day lists, deduplicated [W][Mu];
      3. every rank counts its own level keys against each day's full list -> [W][M]
         (one word per sorted query, 2 n_less + n_eq: linear in the average rank);
      4. reduce_scatter (sum) of the counts by day block: each owner gets its days' totals;
      5. the owner looks every query of its days up (origin layout) and one all_to_all
         returns each rank the counts of its own queries.
    Each rank then finalizes its stock-days (rank = (c + 1) / 2) once for all windows.
    Only step 2 moves O(W x M) bytes per rank; step 4 replaces a ring all-reduce of the
    whole [W][M] (2x the bytes per rank on a link-bound ring).  pdfq: [5][D][S_loc]."""
    from .dist import shard_bounds

    D = int(pdfq.shape[1])
    S_loc = int(pdfq.shape[2])
    dev = pdfq.device
    R, rank = comm.world_size, comm.rank
    M = R * 5 * S_all
    W = D if day_batch is None else max(1, min(D, int(day_batch) * R))
    q_pad = _pad_last(pdfq, S_all, float("nan"))  # [5][D][S_all]
    own = torch.zeros((5, D, S_loc), dtype=torch.int32, device=dev)
    for w0 in range(0, D, W):  # every rank walks the same windows (same D, same W)
        w1 = min(D, w0 + W)
        blocks = [tuple(w0 + x for x in shard_bounds(w1 - w0, R, r)) for r in range(R)]
        nd_max = max(1, max(b1 - b0 for b0, b1 in blocks))
        send = torch.full((R, 5, nd_max, S_all), float("nan"), dtype=torch.float64, device=dev)
        for r, (b0, b1) in enumerate(blocks):
            send[r, :, :b1 - b0] = q_pad[:, b0:b1]
        recv = comm.all_to_all(send)  # [R][5][nd_max][S_all]: every rank's queries of my days
        del send
        b0, b1 = blocks[rank]
        nd = b1 - b0
        mine = torch.full((nd_max, M), -1, dtype=torch.int64, device=dev)  # -1 = NaN key (~0)
        if nd > 0:
            mine[:nd] = kern.sort(recv, R, S_all, nd)
        if after_sort is not None and w0 == 0:
            after_sort()
        # the distinct values of each sorted day list only (a day's queries hold long
        # exact ties: ~20 K distinct of 25 K at c4): the lists, the counts and their
        # reduce-scatter shrink with them; the counts of a value sit at its first position
        mine, Mu = _dedup_sorted(comm, mine)
        gathered = comm.all_gather(mine)  # [R][nd_max][Mu]
        q_sorted = torch.cat([gathered[r, :e - s] for r, (s, e) in enumerate(blocks)])  # [W][Mu]
        del gathered
        counts = kern.count(q_sorted, w0)  # [W][Mu], this rank's keys
        del q_sorted
        cs = torch.zeros((R, nd_max, Mu), dtype=torch.int32, device=dev)
        for r, (s, e) in enumerate(blocks):
            cs[r, :e - s] = counts[s - w0:e - w0]
        del counts
        my_counts = comm.reduce_scatter_sum(cs)  # [nd_max][M], summed over ranks
        del cs
        origin = kern.origin(recv, R, S_all, mine, my_counts)  # [R][5][nd_max][S_all]
        back = comm.all_to_all(origin)  # slice r: my queries' counts on rank r's days
        del origin, recv, mine, my_counts
        for r, (s, e) in enumerate(blocks):
            own[:, s:e] = back[r, :, :e - s, :S_loc]
        del back
    kern.finalize(pdfq, own)


def _dedup_sorted(comm, lists: torch.Tensor):
    """Rows of ascending int64 keys (u64 total-order images, -1 = the NaN key ~0) -> the
    distinct values of each row, left-aligned and padded with -1, at the width of the
    largest row over all ranks (one all-reduce of a scalar).  Returns (dedup, width)."""
    nd, M = lists.shape
    keep = torch.ones_like(lists, dtype=torch.bool)
    keep[:, 1:] = lists[:, 1:] != lists[:, :-1]
    width = _agreed_max(comm, int(keep.sum(1).max().item()) if nd else 1, lists.device)
    out = torch.full((nd, width), -1, dtype=lists.dtype, device=lists.device)
    pos = keep.to(torch.int64).cumsum(1) - 1
    rr = torch.arange(nd, device=lists.device).unsqueeze(1).expand(nd, M)
    out[rr[keep], pos[keep]] = lists[keep]
    return out, width


def shard_width(comm, S_loc: int, stocks_total: Optional[int], dev) -> int:
    """The padded stock width of the exchanges: the largest shard of dist.shard_bounds
    (rank 0's), from the global stock count when the caller knows it -- no collective,
    no host sync -- else agreed with one all-reduce."""
    if stocks_total is not None:
        from .dist import shard_bounds
        s0, s1 = shard_bounds(int(stocks_total), comm.world_size, 0)
        if S_loc > s1 - s0:
            raise ValueError(f"shard of {S_loc} stocks exceeds the widest shard of {stocks_total} "
                             f"over {comm.world_size} ranks")
        return s1 - s0
    return _agreed_max(comm, S_loc, dev)


def _agreed_max(comm, n: int, dev) -> int:
    t = torch.tensor([n], dtype=torch.int64, device=dev)
    comm.all_reduce_max(t)
    return int(t.item())


def _pad_last(t: torch.Tensor, n: int, fill) -> torch.Tensor:
    """Pad the last (stock) axis to n with `fill` (uneven shards before an all-gather)."""
    if t.shape[-1] == n:
        return t
    out = torch.full(tuple(t.shape[:-1]) + (n,), fill, dtype=t.dtype, device=t.device)
    out[..., : t.shape[-1]] = t
    return out


def rolling(val: torch.Tensor, state: torch.Tensor, N: int, method: str):
    """Stage 2 on [rows][D][S] (MF:187-240): returns (out_val, out_state)."""
    lib = _lib.load()
    if method not in ROLL_METHODS:
        raise ValueError("Unknown method")
    if not isinstance(N, int):
        raise ValueError(f"Unsupported frequency for days: {N}")
    rows, D, S = val.shape
    ov = torch.empty_like(val)
    os_ = torch.empty_like(state)
    _lib.check(lib.mff_stage2(_lib.ptr(val), _lib.ptr(state), rows, D, S, N, ROLL_METHODS[method],
                              _lib.ptr(ov), _lib.ptr(os_), _stream(val.device)), "mff_stage2")
    return ov, os_


def cross_section(val: torch.Tensor, state: torch.Tensor, kind: str, comm=None,
                  stocks_total: Optional[int] = None):
    """Stage 3 on [rows][D][S_loc]: per-day z-score ('z') or average rank ('rank').
    ``stocks_total``: the stocks over all ranks (sharded), or None (agreed by all-reduce)."""
    lib = _lib.load()
    rows, D, S = val.shape
    dev = val.device
    st = _stream(dev)
    ov = torch.empty_like(val)
    os_ = torch.empty_like(state)
    R = 1 if comm is None else comm.world_size
    if kind == "z" and comm is None and S <= lib.mff_xs_zscore_local_max_stocks():
        _lib.check(lib.mff_xs_zscore_local(_lib.ptr(val), _lib.ptr(state), rows, D, S, _lib.ptr(ov),
                                           _lib.ptr(os_), st), "mff_xs_zscore_local")
    elif kind == "z":
        mom = torch.empty((rows, D, 3), dtype=torch.float64, device=dev)
        _lib.check(lib.mff_xs_moments(_lib.ptr(val), _lib.ptr(state), rows, D, S, _lib.ptr(mom), st),
                   "mff_xs_moments")
        mom_all = mom if comm is None else comm.all_gather(mom)
        _lib.check(lib.mff_xs_zscore(_lib.ptr(val), _lib.ptr(state), rows, D, S, _lib.ptr(mom_all), R,
                                     _lib.ptr(ov), _lib.ptr(os_), st), "mff_xs_zscore")
    elif kind == "rank" and comm is None:
        _xs_rank_local(lib, val, state, ov, os_, st)
    elif kind == "rank":
        S_all = shard_width(comm, S, stocks_total, dev)
        ov, os_ = xs_rank_sharded(comm, val, state, S_all,
                                  lambda v, s_, o, os2: _xs_rank_local(lib, v, s_, o, os2, _stream(dev)))
    else:
        raise ValueError(kind)
    return ov, os_


def _xs_rank_local(lib, val, state, ov, os_, st) -> None:
    """mff_xs_rank on whole days held by one rank (R = 1: the one-rank kernels,
    k_xs_rank_day for S <= 5,120)."""
    rows, D, S = val.shape
    ws = torch.empty(lib.mff_xs_rank_workspace_bytes(rows, D, S, 1), dtype=torch.uint8, device=val.device)
    _lib.check(lib.mff_xs_rank(_lib.ptr(val), _lib.ptr(state), rows, D, S, _lib.ptr(val), _lib.ptr(state), 1,
                               S, _lib.ptr(ov), _lib.ptr(os_), _lib.ptr(ws), st), "mff_xs_rank")


def xs_rank_sharded(comm, val: torch.Tensor, state: torch.Tensor, S_all: int, rank_days):
    """Stage-3 rank of stock-sharded rows [rows][D][S_loc] by day owners (verdict r4 #5):
      1. all_to_all: each rank sends the owner of every day block its columns of those days
         ([R][rows][nd_max][S_all], shards padded to S_all with ABSENT);
      2. the owner ranks its days whole ([rows][nd][R * S_all], ``rank_days(v, s, out_v,
         out_s)``: the one-rank kernels -- k_xs_rank_day while R * S_all <= 5,120);
      3. all_to_all back: every rank receives its own columns' ranks of every day block.
    Each rank moves 2 x rows x D x S_loc x 9 B (values + states, there and back) instead of
    receiving (R - 1) x rows x D x S_all x 9 B, and ranks 1 / R of the days instead of all
    of them.  Returns (out_val, out_state) [rows][D][S_loc]."""
    from .dist import shard_bounds

    rows, D, S_loc = val.shape
    R, me = comm.world_size, comm.rank
    dev = val.device
    blocks = [shard_bounds(D, R, r) for r in range(R)]
    nd_max = max(1, max(b - a for a, b in blocks))
    sv = torch.zeros((R, rows, nd_max, S_all), dtype=val.dtype, device=dev)
    ss = torch.full((R, rows, nd_max, S_all), ABSENT, dtype=state.dtype, device=dev)
    for q, (a, b) in enumerate(blocks):
        sv[q, :, :b - a, :S_loc] = val[:, a:b]
        ss[q, :, :b - a, :S_loc] = state[:, a:b]
    rv, rs = comm.all_to_all(sv), comm.all_to_all(ss)  # slice q: rank q's columns of my days
    del sv, ss
    a, b = blocks[me]
    nd = b - a
    # my days whole: columns of rank 0, then rank 1, ... (each padded to S_all)
    fv = rv.permute(1, 2, 0, 3).reshape(rows, nd_max, R * S_all)[:, :nd].contiguous()
    fs = rs.permute(1, 2, 0, 3).reshape(rows, nd_max, R * S_all)[:, :nd].contiguous()
    del rv, rs
    back_v = torch.zeros((rows, nd_max, R * S_all), dtype=val.dtype, device=dev)
    back_s = torch.full((rows, nd_max, R * S_all), ABSENT, dtype=state.dtype, device=dev)
    if nd > 0:
        ov_ = torch.empty_like(fv)
        os_ = torch.empty_like(fs)
        rank_days(fv, fs, ov_, os_)
        back_v[:, :nd] = ov_
        back_s[:, :nd] = os_
    del fv, fs
    # slice q of the send = rank q's columns of my days
    tv = back_v.reshape(rows, nd_max, R, S_all).permute(2, 0, 1, 3).contiguous()
    ts = back_s.reshape(rows, nd_max, R, S_all).permute(2, 0, 1, 3).contiguous()
    gv, gs = comm.all_to_all(tv), comm.all_to_all(ts)  # slice q: my columns of q's days
    out_v = torch.empty_like(val)
    out_s = torch.empty_like(state)
    for q, (a, b) in enumerate(blocks):
        out_v[:, a:b] = gv[q, :, :b - a, :S_loc]
        out_s[:, a:b] = gs[q, :, :b - a, :S_loc]
    return out_v, out_s


NEUTRALIZE_MAX_GROUPS = 256  # mff_xs_neutralize_max_groups()


def _neutralize_local(lib, val, state, group, G, size_val, size_state, winsor, standardize):
    """mff_xs_neutralize on whole days held by one rank."""
    rows, D, S = val.shape
    dev = val.device
    ov = torch.empty_like(val)
    os_ = torch.empty_like(state)
    ws = None
    if group is not None:
        ws = torch.empty(max(lib.mff_xs_neutralize_workspace_bytes(D, S), 1), dtype=torch.uint8, device=dev)
    _lib.check(lib.mff_xs_neutralize(_lib.ptr(val), _lib.ptr(state), rows, D, S, _lib.ptr(group), int(G or 0),
                                     _lib.ptr(size_val), _lib.ptr(size_state), float(winsor), int(bool(standardize)),
                                     _lib.ptr(ov), _lib.ptr(os_), _lib.ptr(ws), _stream(dev)), "mff_xs_neutralize")
    return ov, os_


def neutralize(val: torch.Tensor, state: torch.Tensor, group: Optional[torch.Tensor] = None,
               size_val: Optional[torch.Tensor] = None, size_state: Optional[torch.Tensor] = None, *,
               G: Optional[int] = None, winsor: float = 3.0, standardize: bool = True, comm=None,
               stocks_total: Optional[int] = None):
    """Per-day MAD winsorisation, industry / size neutralisation and standardisation of
    exposure rows [rows][D][S_loc] (mff_xs_neutralize; the definition is on its declaration
    in include/mff.h).  ``group``: int32 [D][S_loc] industry ids in [0, G), -1 = none (None:
    no industries); ``G``: the number of industries (None: the largest id + 1, agreed over
    the ranks); ``size_val`` / ``size_state``: the size covariate [D][S_loc] (None: no
    covariate); ``winsor`` <= 0 turns the clipping off.

    Stock-sharded (``comm``): medians need whole days, so the columns travel to day owners
    through :func:`xs_rank_sharded`'s exchange with the side inputs as two extra rows (the
    size with its state; the industry id as an exactly representable float64, ABSENT where
    there is none), and each owner runs the one-rank kernel on its days.
    Returns (out_val, out_state) [rows][D][S_loc]."""
    lib = _lib.load()
    if val.dim() != 3 or state.shape != val.shape:
        raise ValueError("val and state must be [rows][D][S]")
    rows, D, S = val.shape
    dev = val.device
    if (size_val is None) != (size_state is None):
        raise ValueError("size_val and size_state go together")
    for name, t in (("group", group), ("size_val", size_val), ("size_state", size_state)):
        if t is not None and tuple(t.shape) != (D, S):
            raise ValueError(f"{name} must be [D][S] = [{D}][{S}], got {tuple(t.shape)}")
    val, state = val.contiguous(), state.contiguous()
    if group is not None:
        group = group.to(torch.int32).contiguous()
        if G is None:
            G = int(group.max().item()) + 1 if group.numel() else 1
            if comm is not None:
                G = _agreed_max(comm, G, dev)
            G = max(G, 1)
        if G > lib.mff_xs_neutralize_max_groups():
            raise _lib.MffError(f"neutralize: {G} industries above the kernel's "
                                f"{lib.mff_xs_neutralize_max_groups()}")
    if size_val is not None:
        size_val = size_val.to(torch.float64).contiguous()
        size_state = size_state.to(torch.uint8).contiguous()
    if comm is None:
        return _neutralize_local(lib, val, state, group, G, size_val, size_state, winsor, standardize)
    R = comm.world_size
    S_all = shard_width(comm, S, stocks_total, dev)
    if R * S_all > lib.mff_xs_neutralize_max_stocks():
        raise _lib.MffError(f"neutralize: {R} shards of up to {S_all} stocks make days of {R * S_all} columns, "
                            f"above the kernel's {lib.mff_xs_neutralize_max_stocks()}")
    extra_v, extra_s = [], []
    if size_val is not None:
        extra_v.append(size_val)
        extra_s.append(size_state)
    if group is not None:
        has = group >= 0
        extra_v.append(torch.where(has, group.to(torch.float64), torch.zeros((), dtype=torch.float64, device=dev)))
        extra_s.append(torch.where(has, VALUE, ABSENT).to(torch.uint8))
    ne = len(extra_v)
    xv = torch.cat([val] + [e[None] for e in extra_v]) if ne else val
    xs_ = torch.cat([state] + [e[None] for e in extra_s]) if ne else state

    def owner_days(v, s_, o, os2):
        """v, s_: [rows + ne][nd][R * S_all], the owner's days whole."""
        k = rows
        zv = zs = gd = None
        if size_val is not None:
            zv, zs = v[k].contiguous(), s_[k].contiguous()
            k += 1
        if group is not None:
            gd = torch.where(s_[k] == VALUE, v[k].to(torch.int32),
                             torch.full((), -1, dtype=torch.int32, device=dev)).contiguous()
        rv, rs = _neutralize_local(lib, v[:rows].contiguous(), s_[:rows].contiguous(), gd, G, zv, zs, winsor,
                                   standardize)
        o.zero_()
        os2.fill_(ABSENT)
        o[:rows] = rv
        os2[:rows] = rs

    ov, os_ = xs_rank_sharded(comm, xv, xs_, S_all, owner_days)
    return ov[:rows].contiguous(), os_[:rows].contiguous()


CORR_METHODS = ("pearson", "spearman")
CORR_GATHER_BYTES = 256 << 20  # cap of the gathered sum planes of one day batch (sharded)
CORR_PLANE_BYTES = 4 << 30     # cap of the sum planes of one day batch (single rank)


def _int_arg(name: str, v, lo: int) -> int:
    if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or v < lo:
        raise ValueError(f"{name} must be an integer >= {lo}, got {v!r}")
    return int(v)


def _factor_rows(val: torch.Tensor, state: torch.Tensor, fn: str, kmax: int, names: str = "x_val and x_state",
                 k: str = "K"):
    """The [K][D][S] check of the factor_* entry points -> (val float64, state uint8), contiguous."""
    if val.dim() != 3 or state.shape != val.shape:
        raise ValueError(f"{names} must be [{k}][D][S]")
    if val.shape[0] < 1 or val.shape[0] > kmax:
        raise _lib.MffError(f"{fn}: {k}={val.shape[0]} outside [1, {kmax}]")
    return val.to(torch.float64).contiguous(), state.to(torch.uint8).contiguous()


def _nsplit(split: Optional[int], D: int, S: int, comm) -> int:
    """Stock runs per day: ``split``, or :func:`reg_splits` (sharded: 1)."""
    nsplit = int(split) if split is not None else (reg_splits(D, S) if comm is None else 1)
    if nsplit < 1:
        raise ValueError(f"split must be >= 1, got {split!r}")
    return nsplit


def _day_batches(D: int, day_bytes: int, R: int, sharded: bool):
    """Day batches (d0, nd, whole) whose planes of ``day_bytes`` per day stay below
    CORR_PLANE_BYTES, or below CORR_GATHER_BYTES once the R shards' planes are gathered."""
    nd_max = max(1, (CORR_GATHER_BYTES // R if sharded else CORR_PLANE_BYTES) // day_bytes)
    for d0 in range(0, D, nd_max):
        nd = min(nd_max, D - d0)
        yield d0, nd, nd == D


def _days(t: Optional[torch.Tensor], d0: int, nd: int, whole: bool, dim: int = 0):
    """Days [d0, d0 + nd) along ``dim`` of t, contiguous; t itself for None or the whole batch."""
    return t if (t is None or whole) else t.narrow(dim, d0, nd).contiguous()


def factor_corr(val: torch.Tensor, state: torch.Tensor, method: str = "pearson", min_pairs: int = 2,
                comm=None, stocks_total: Optional[int] = None):
    """Per-day pairwise correlation of the exposure rows [F][D][S_loc] (mff_xs_corr_*; the
    definition is on the declarations in include/mff.h): pairwise-complete Pearson over the
    stocks where both rows hold a finite VALUE, NaN below ``min_pairs`` common stocks or when
    a side is constant on them.

    ``method='spearman'``: every row is first replaced, per day, by its average ranks over
    its OWN usable set (``cross_section(kind='rank')`` after non-finite values are masked to
    NULL), then the Pearson definition is applied to the ranks.  The ranks are NOT recomputed
    inside each pair set: this equals ``pandas.DataFrame.corr(method='spearman')`` when the
    rows share their coverage, and is the usual choice for factor panels.

    Stock-sharded (``comm``): the local (n, sum) of every row and day are all-gathered and
    combined into one common centre, the local sum planes are all-gathered in day batches
    (at most 256 MiB gathered at a time) and added in rank order; every rank returns the full
    result.  Returns (corr float64 [D][F][F], n int32 [D][F][F])."""
    lib = _lib.load()
    if method not in CORR_METHODS:
        raise ValueError(f"method must be one of {CORR_METHODS}, got {method!r}")
    min_pairs = _int_arg("min_pairs", min_pairs, 2)
    val, state = _factor_rows(val, state, "factor_corr", lib.mff_xs_corr_max_rows(), "val and state", "rows")
    rows, D, S = val.shape
    dev = val.device
    st = _stream(dev)
    if method == "spearman":
        masked = torch.where((state == VALUE) & ~torch.isfinite(val), torch.full_like(state, NULL), state)
        val, state = cross_section(val, masked, "rank", comm=comm, stocks_total=stocks_total)
    corr = torch.empty((D, rows, rows), dtype=torch.float64, device=dev)
    n = torch.empty((D, rows, rows), dtype=torch.int32, device=dev)
    if D == 0:
        return corr, n
    R = 1 if comm is None else comm.world_size
    center = None
    if comm is not None:
        mom = torch.empty((rows, D, 2), dtype=torch.float64, device=dev)
        _lib.check(lib.mff_xs_corr_moments(_lib.ptr(val), _lib.ptr(state), rows, D, S, _lib.ptr(mom), st),
                   "mff_xs_corr_moments")
        parts = comm.all_gather(mom)
        tot = parts[0]  # [rows][D][2], the ranks added in rank order: the same bits on every rank
        for r in range(1, R):
            tot = tot + parts[r]
        center = torch.where(tot[..., 0] > 0, tot[..., 1] / tot[..., 0].clamp(min=1.0),
                             torch.zeros((), dtype=torch.float64, device=dev)).contiguous()
    ws = torch.empty(max(lib.mff_xs_corr_workspace_bytes(rows, D, S), 8), dtype=torch.uint8, device=dev)
    for d0, nd, whole in _day_batches(D, 4 * rows * rows * 8, R, comm is not None):
        v, s_, c = _days(val, d0, nd, whole, 1), _days(state, d0, nd, whole, 1), _days(center, d0, nd, whole, 1)
        sums = torch.empty((nd, 4, rows, rows), dtype=torch.float64, device=dev)
        _lib.check(lib.mff_xs_corr_sums(_lib.ptr(v), _lib.ptr(s_), rows, nd, S, _lib.ptr(c), _lib.ptr(sums),
                                        _lib.ptr(ws), st), "mff_xs_corr_sums")
        sums_all = sums if comm is None else comm.all_gather(sums).contiguous()
        _lib.check(lib.mff_xs_corr_finalize(_lib.ptr(sums_all), R, rows, nd, min_pairs, _lib.ptr(corr[d0:]),
                                            _lib.ptr(n[d0:]), st), "mff_xs_corr_finalize")
    return corr, n


def factor_corr_mean(corr: torch.Tensor):
    """Time aggregate of :func:`factor_corr`'s corr [D][F][F]: per pair the mean over the
    days where it is not NaN (summed in day order; NaN when there is none) and that count.
    Returns (mean float64 [F][F], days int32 [F][F])."""
    lib = _lib.load()
    if corr.dim() != 3 or corr.shape[1] != corr.shape[2]:
        raise ValueError("corr must be [D][F][F]")
    D, rows, _ = corr.shape
    corr = corr.to(torch.float64).contiguous()
    dev = corr.device
    mean = torch.empty((rows, rows), dtype=torch.float64, device=dev)
    days = torch.empty((rows, rows), dtype=torch.int32, device=dev)
    _lib.check(lib.mff_xs_corr_mean(_lib.ptr(corr), rows, D, _lib.ptr(mean), _lib.ptr(days), _stream(dev)),
               "mff_xs_corr_mean")
    return mean, days


REG_SPLIT_DAYS = 256   # below one day per CU (256 on MI355X) the stocks of a day are split
REG_SPLIT_STOCKS = 256  # ... into runs of at least 8 tiles of 32 stocks
REG_AGG_COLUMNS = ("days", "mean", "std", "t_fm", "mean_abs_t", "share_abs_t_gt_2")


class RegressResult(NamedTuple):
    """factor_regress: per-day device tensors (resid_* None unless asked for)."""
    beta: torch.Tensor     # float64 [D][K]
    tstat: torch.Tensor    # float64 [D][K]
    r2: torch.Tensor       # float64 [D]
    n: torch.Tensor        # int32 [D]
    dof: torch.Tensor      # int32 [D]
    status: torch.Tensor   # int32 [D]: 0 ok, 1 too few observations, 2 singular
    resid_val: Optional[torch.Tensor] = None    # float64 [D][S_loc]
    resid_state: Optional[torch.Tensor] = None  # uint8 [D][S_loc]


def reg_splits(D: int, S: int) -> int:
    """Stock runs per day of the group and Gram passes: 1 from REG_SPLIT_DAYS days on (every CU has a
    day of its own), below that enough runs for about two workgroups per CU, none shorter
    than REG_SPLIT_STOCKS stocks."""
    if D >= REG_SPLIT_DAYS or D < 1:
        return 1
    return max(1, min(-(-S // REG_SPLIT_STOCKS), -(-2 * REG_SPLIT_DAYS // D)))


def factor_regress(x_val: torch.Tensor, x_state: torch.Tensor, y_val: torch.Tensor, y_state: torch.Tensor,
                   weight: Optional[torch.Tensor] = None, weight_state: Optional[torch.Tensor] = None,
                   group: Optional[torch.Tensor] = None, G: Optional[int] = None, min_obs: int = 0,
                   residual: bool = False, comm=None, stocks_total: Optional[int] = None,
                   split: Optional[int] = None) -> RegressResult:
    """Per-day weighted least squares of y [D][S_loc] on industry dummies and the K exposure
    rows x [K][D][S_loc] (mff_xs_reg_*; the definition is on the declarations in
    include/mff.h): coefficients, t-statistics, R^2, n, dof and status per day, and with
    ``residual=True`` the residual of the local stocks.

    ``weight`` / ``weight_state``: the WLS weight itself (None: 1); ``group``: int32 industry
    ids in [0, G), anything else = none (None: a plain intercept); ``G``: the number of
    industries (None: the largest id + 1, agreed over the ranks); ``min_obs``: fewer usable
    stocks give status 1.  ``split``: stock runs per day of the group and Gram passes
    (None: :func:`reg_splits`; sharded: 1); the runs are added like shards, in run order.

    Stock-sharded (``comm``): the local group sums are all-gathered and added in rank order
    into one common means table (a shard may hold no member of an industry), the local Gram
    planes are all-gathered in day batches (at most 256 MiB gathered at a time) and added in
    rank order; the residual is local; every rank returns the full per-day result."""
    lib = _lib.load()
    x_val, x_state = _factor_rows(x_val, x_state, "factor_regress", lib.mff_xs_reg_max_factors())
    K, D, S = x_val.shape
    min_obs = _int_arg("min_obs", min_obs, 0)
    if (weight is None) != (weight_state is None):
        raise ValueError("weight and weight_state go together")
    for name, t in (("y_val", y_val), ("y_state", y_state), ("weight", weight), ("weight_state", weight_state),
                    ("group", group)):
        if t is not None and tuple(t.shape) != (D, S):
            raise ValueError(f"{name} must be [D][S] = [{D}][{S}], got {tuple(t.shape)}")
    dev = x_val.device
    st = _stream(dev)
    f64, u8 = torch.float64, torch.uint8
    y_val, y_state = y_val.to(f64).contiguous(), y_state.to(u8).contiguous()
    if weight is not None:
        weight, weight_state = weight.to(f64).contiguous(), weight_state.to(u8).contiguous()
    Gk = 0
    if group is not None:
        group = group.to(torch.int32).contiguous()
        if G is None:
            G = int(group.max().item()) + 1 if group.numel() else 1
            if comm is not None:
                G = _agreed_max(comm, G, dev)
            G = max(G, 1)
        if G < 1 or G > lib.mff_xs_reg_max_groups():
            raise _lib.MffError(f"factor_regress: {G} industries outside [1, {lib.mff_xs_reg_max_groups()}]")
        Gk = int(G)
    Ge = max(Gk, 1)
    R = 1 if comm is None else comm.world_size
    beta = torch.empty((D, K), dtype=f64, device=dev)
    tstat = torch.empty((D, K), dtype=f64, device=dev)
    r2 = torch.empty(D, dtype=f64, device=dev)
    n = torch.empty(D, dtype=torch.int32, device=dev)
    dof = torch.empty(D, dtype=torch.int32, device=dev)
    status = torch.empty(D, dtype=torch.int32, device=dev)
    rv = torch.empty((D, S), dtype=f64, device=dev) if residual else None
    rs = torch.empty((D, S), dtype=u8, device=dev) if residual else None
    C = K + 1
    nsplit = _nsplit(split, D, S, comm)
    for d0, nd, whole in _day_batches(D, nsplit * C * C * 8, R, comm is not None):
        xv, xs = _days(x_val, d0, nd, whole, 1), _days(x_state, d0, nd, whole, 1)
        yv, ys, wv, ws_, gp = (_days(t_, d0, nd, whole) for t_ in (y_val, y_state, weight, weight_state, group))
        ws = torch.empty(max(lib.mff_xs_reg_workspace_bytes(K, nd, S, Gk), 8), dtype=u8, device=dev)
        gsums = torch.empty((nsplit, nd, Ge + 1, K + 3), dtype=f64, device=dev)
        _lib.check(lib.mff_xs_reg_groups(_lib.ptr(xv), _lib.ptr(xs), K, nd, S, _lib.ptr(yv), _lib.ptr(ys),
                                         _lib.ptr(wv), _lib.ptr(ws_), _lib.ptr(gp), Gk, nsplit, _lib.ptr(gsums),
                                         _lib.ptr(ws), st), "mff_xs_reg_groups")
        gs_all = gsums if comm is None else comm.all_gather(gsums).contiguous()
        gram = torch.empty((nsplit, nd, C, C), dtype=f64, device=dev)
        _lib.check(lib.mff_xs_reg_gram(_lib.ptr(xv), K, nd, S, _lib.ptr(yv), _lib.ptr(wv), Gk, _lib.ptr(gs_all),
                                       R * nsplit, nsplit, _lib.ptr(gram), _lib.ptr(ws), st), "mff_xs_reg_gram")
        gram_all = gram if comm is None else comm.all_gather(gram).contiguous()
        _lib.check(lib.mff_xs_reg_solve(_lib.ptr(gram_all), R * nsplit, K, nd, min_obs, _lib.ptr(beta[d0:]),
                                        _lib.ptr(tstat[d0:]), _lib.ptr(r2[d0:]), _lib.ptr(n[d0:]),
                                        _lib.ptr(dof[d0:]), _lib.ptr(status[d0:]), _lib.ptr(ws), st),
                   "mff_xs_reg_solve")
        if residual:
            _lib.check(lib.mff_xs_reg_residual(_lib.ptr(xv), K, nd, S, _lib.ptr(yv), _lib.ptr(ys), Gk,
                                               _lib.ptr(beta[d0:]), _lib.ptr(status[d0:]), _lib.ptr(rv[d0:]),
                                               _lib.ptr(rs[d0:]), _lib.ptr(ws), st), "mff_xs_reg_residual")
    return RegressResult(beta, tstat, r2, n, dof, status, rv, rs)


def factor_regress_mean(res: RegressResult):
    """Time aggregate (Fama-MacBeth) of :func:`factor_regress` over the status-0 days, in day
    order.  Returns (agg float64 [K][6] with the columns REG_AGG_COLUMNS, overall float64 [2]
    = (mean r2, mean n))."""
    lib = _lib.load()
    D, K = res.beta.shape
    dev = res.beta.device
    agg = torch.empty((K, len(REG_AGG_COLUMNS)), dtype=torch.float64, device=dev)
    overall = torch.empty(2, dtype=torch.float64, device=dev)
    _lib.check(lib.mff_xs_reg_mean(_lib.ptr(res.beta), _lib.ptr(res.tstat), _lib.ptr(res.r2), _lib.ptr(res.n),
                                   _lib.ptr(res.status), K, D, _lib.ptr(agg), _lib.ptr(overall), _stream(dev)),
               "mff_xs_reg_mean")
    return agg, overall


ORTH_METHODS = ("symmetric", "schmidt")


class OrthResult(NamedTuple):
    """factor_orthogonalize: the orthogonalised rows and the per-day diagnostics (device tensors)."""
    val: torch.Tensor        # float64 [K][D][S_loc]
    state: torch.Tensor      # uint8 [K][D][S_loc]
    transform: torch.Tensor  # float64 [D][K][K]: f_j = sum_k z_k T[k][j]
    eig: torch.Tensor        # float64 [D][K]: eigenvalues of the day's correlation matrix, ascending
    keep: torch.Tensor       # float64 [D][K]: corr_U(f_j, x_j)
    n: torch.Tensor          # int32 [D]
    status: torch.Tensor     # int32 [D]: 0 ok, 1 too few observations, 2 singular


def factor_orthogonalize(x_val: torch.Tensor, x_state: torch.Tensor, method: str = "symmetric", min_obs: int = 0,
                         comm=None, stocks_total: Optional[int] = None, split: Optional[int] = None) -> OrthResult:
    """Per-day orthogonalisation of the K exposure rows x [K][D][S_loc] (mff_xs_orth_*; the
    definition is on the declarations in include/mff.h): over the stocks where all K rows hold
    a finite value the rows are standardised and mapped to K uncorrelated unit-variance rows,
    ``method`` 'symmetric' (Loewdin: the closest orthonormal set, no row preferred) or
    'schmidt' (Gram-Schmidt in row order: row j with the rows before it taken out).

    ``min_obs``: fewer usable stocks (or fewer than K + 1) give status 1.  ``split``: stock
    runs per day of the sums and Gram passes (None: :func:`reg_splits`; sharded: 1); the runs
    are added like shards, in run order.

    Stock-sharded (``comm``): the local sums and the local Gram planes are all-gathered (the
    planes in day batches of at most 256 MiB gathered at a time) and added in rank order; the
    apply pass is local; every rank returns the full per-day diagnostics.  ``stocks_total`` is
    accepted for the call shape of :func:`factor_regress` and ignored: nothing here depends on
    the width of the other shards."""
    lib = _lib.load()
    x_val, x_state = _factor_rows(x_val, x_state, "factor_orthogonalize", lib.mff_xs_orth_max_factors())
    K, D, S = x_val.shape
    if method not in ORTH_METHODS:
        raise ValueError(f"method must be one of {ORTH_METHODS}, got {method!r}")
    min_obs = _int_arg("min_obs", min_obs, 0)
    dev = x_val.device
    st = _stream(dev)
    f64, u8 = torch.float64, torch.uint8
    R = 1 if comm is None else comm.world_size
    ov = torch.empty((K, D, S), dtype=f64, device=dev)
    os_ = torch.empty((K, D, S), dtype=u8, device=dev)
    tr = torch.empty((D, K, K), dtype=f64, device=dev)
    eig = torch.empty((D, K), dtype=f64, device=dev)
    keep = torch.empty((D, K), dtype=f64, device=dev)
    n = torch.empty(D, dtype=torch.int32, device=dev)
    status = torch.empty(D, dtype=torch.int32, device=dev)
    nsplit = _nsplit(split, D, S, comm)
    m = ORTH_METHODS.index(method)
    for d0, nd, whole in _day_batches(D, nsplit * K * K * 8, R, comm is not None):
        xv, xs = _days(x_val, d0, nd, whole, 1), _days(x_state, d0, nd, whole, 1)
        bv = ov if whole else torch.empty((K, nd, S), dtype=f64, device=dev)
        bs = os_ if whole else torch.empty((K, nd, S), dtype=u8, device=dev)
        ws = torch.empty(max(lib.mff_xs_orth_workspace_bytes(K, nd, S), 8), dtype=u8, device=dev)
        sums = torch.empty((nsplit, nd, 2 * K + 1), dtype=f64, device=dev)
        _lib.check(lib.mff_xs_orth_sums(_lib.ptr(xv), _lib.ptr(xs), K, nd, S, nsplit, _lib.ptr(sums), _lib.ptr(ws), st),
                   "mff_xs_orth_sums")
        sums_all = sums if comm is None else comm.all_gather(sums).contiguous()
        gram = torch.empty((nsplit, nd, K, K), dtype=f64, device=dev)
        _lib.check(lib.mff_xs_orth_gram(_lib.ptr(xv), K, nd, S, _lib.ptr(sums_all), R * nsplit, nsplit,
                                        _lib.ptr(gram), _lib.ptr(ws), st), "mff_xs_orth_gram")
        gram_all = gram if comm is None else comm.all_gather(gram).contiguous()
        _lib.check(lib.mff_xs_orth_solve(_lib.ptr(gram_all), R * nsplit, K, nd, m, min_obs, _lib.ptr(tr[d0:]),
                                         _lib.ptr(eig[d0:]), _lib.ptr(keep[d0:]), _lib.ptr(n[d0:]),
                                         _lib.ptr(status[d0:]), _lib.ptr(ws), st), "mff_xs_orth_solve")
        _lib.check(lib.mff_xs_orth_apply(_lib.ptr(xv), _lib.ptr(xs), K, nd, S, _lib.ptr(status[d0:]), _lib.ptr(bv),
                                         _lib.ptr(bs), _lib.ptr(ws), st), "mff_xs_orth_apply")
        if not whole:
            ov[:, d0:d0 + nd], os_[:, d0:d0 + nd] = bv, bs
    return OrthResult(ov, os_, tr, eig, keep, n, status)


COMBINE_METHODS = ("equal", "ic", "icir", "max_icir")
COMBINE_IC = ("pearson", "rank")
COMBINE_MAX_FACTORS = 64  # K of mff_xs_comb_*
COMBINE_RANK_BYTES = CORR_PLANE_BYTES  # cap of the ranked (x, y) planes of one day batch (ic='rank')


class CombineResult(NamedTuple):
    """factor_combine: the composite and what it was built from (device tensors)."""
    val: torch.Tensor      # float64 [D][S_loc]
    state: torch.Tensor    # uint8 [D][S_loc]
    weights: torch.Tensor  # float64 [D][K]: sum_k |w| = 1; NaN on a date with status != 0
    ic: torch.Tensor       # float64 [K][D]: per-date IC (Pearson or rank) of every factor
    n_pairs: torch.Tensor  # int32 [K][D]
    count: torch.Tensor    # int32 [D][K]: usable window dates behind each weight
    status: torch.Tensor   # int32 [D]: 0 ok, 1 too little history, 2 singular or degenerate


def _comb_moments(lib, xv, xs, yv, ys, Ky, min_obs, comm, st):
    """mff_xs_comb_moments + the shards' partials gathered + mff_xs_comb_finalize ->
    (zmom [K][D][3], ic [K][D], n_pairs [K][D])."""
    K, D, S = xv.shape
    dev = xv.device
    R = 1 if comm is None else comm.world_size
    part = torch.empty((K, D, 9), dtype=torch.float64, device=dev)
    _lib.check(lib.mff_xs_comb_moments(_lib.ptr(xv), _lib.ptr(xs), K, D, S, _lib.ptr(yv), _lib.ptr(ys), Ky,
                                       _lib.ptr(part), st), "mff_xs_comb_moments")
    part_all = part if comm is None else comm.all_gather(part).contiguous()
    zmom = torch.empty((K, D, 3), dtype=torch.float64, device=dev)
    ic = torch.empty((K, D), dtype=torch.float64, device=dev)
    npairs = torch.empty((K, D), dtype=torch.int32, device=dev)
    _lib.check(lib.mff_xs_comb_finalize(_lib.ptr(part_all), R, K, D, min_obs, _lib.ptr(zmom), _lib.ptr(ic),
                                        _lib.ptr(npairs), st), "mff_xs_comb_finalize")
    return zmom, ic, npairs


def factor_combine(x_val: torch.Tensor, x_state: torch.Tensor, y_val: Optional[torch.Tensor] = None,
                   y_state: Optional[torch.Tensor] = None, method: str = "icir", future_days: int = 5,
                   window: int = 60, min_periods: int = 20, ic: str = "pearson", shrink: float = 0.5,
                   min_obs: int = 0, min_factors: int = 1, comm=None,
                   stocks_total: Optional[int] = None) -> CombineResult:
    """One composite [D][S_loc] from the K exposure rows x [K][D][S_loc] (mff_xs_comb_*; the
    definition is on the declarations in include/mff.h): per date every factor's z-score,
    weighted by ``method`` -- 'equal', or from the factor's ICs against the forward return y
    [D][S_loc] over the trailing ``window`` dates whose ``future_days`` horizon has closed:
    'ic' (mean IC), 'icir' (mean / std), 'max_icir' (Sigma_s^-1 mu with the off-diagonal of the
    IC covariance shrunk by ``shrink``) -- and renormalised per stock over the factors it has
    (at least ``min_factors`` of them, else null).

    ``ic``: 'pearson', or 'rank' (per factor mff_ic_pairs then the stage-3 rank of the pair
    set, in day batches of at most COMBINE_RANK_BYTES of ranked planes).  ``min_periods``: the
    finite ICs a window needs; ``min_obs``: the pairs a date's IC needs (at least 2).  y may be
    None for 'equal' (every IC is then NaN).

    Stock-sharded (``comm``): the moment partials are all-gathered and merged in rank order,
    the weights are computed on every rank, the apply pass is local."""
    lib = _lib.load()
    x_val, x_state = _factor_rows(x_val, x_state, "factor_combine", COMBINE_MAX_FACTORS)
    K, D, S = x_val.shape
    if method not in COMBINE_METHODS:
        raise ValueError(f"method must be one of {COMBINE_METHODS}, got {method!r}")
    if ic not in COMBINE_IC:
        raise ValueError(f"ic must be one of {COMBINE_IC}, got {ic!r}")
    future_days = _int_arg("future_days", future_days, 1)
    window = _int_arg("window", window, 1)
    min_periods = _int_arg("min_periods", min_periods, 1)
    min_obs = _int_arg("min_obs", min_obs, 0)
    min_factors = _int_arg("min_factors", min_factors, 1)
    if min_factors > K:
        raise ValueError(f"min_factors must be at most the number of factors {K}, got {min_factors!r}")
    if isinstance(shrink, bool) or not isinstance(shrink, (int, float, np.integer, np.floating)) \
            or not 0.0 <= float(shrink) <= 1.0:
        raise ValueError(f"shrink must be a number in [0, 1], got {shrink!r}")
    if (y_val is None) != (y_state is None):
        raise ValueError("y_val and y_state go together")
    if y_val is None and method != "equal":
        raise ValueError(f"method {method!r} needs the forward return y")
    if y_val is not None and (tuple(y_val.shape) != (D, S) or y_state.shape != y_val.shape):
        raise ValueError("y_val and y_state must be [D][S]")
    dev = x_val.device
    st = _stream(dev)
    f64, u8 = torch.float64, torch.uint8
    if y_val is not None:
        y_val, y_state = y_val.to(f64).contiguous(), y_state.to(u8).contiguous()
    zmom, ics, npairs = _comb_moments(lib, x_val, x_state, y_val, y_state, 0 if y_val is None else 1, min_obs,
                                      comm, st)
    if ic == "rank" and y_val is not None and D > 0 and S > 0:
        S_w = S if comm is None else shard_width(comm, S, stocks_total, dev)  # the same batches on every rank
        nd_max = max(1, COMBINE_RANK_BYTES // (2 * K * S_w * 9))
        for d0 in range(0, D, nd_max):
            nd = min(nd_max, D - d0)
            rv = torch.empty((2, K, nd, S), dtype=f64, device=dev)
            rs = torch.empty((2, K, nd, S), dtype=u8, device=dev)
            pv = torch.empty((2, nd, S), dtype=f64, device=dev)
            ps = torch.empty((2, nd, S), dtype=u8, device=dev)
            yv, ys = y_val[d0:d0 + nd], y_state[d0:d0 + nd]
            for k in range(K):
                xv, xs = x_val[k, d0:d0 + nd], x_state[k, d0:d0 + nd]
                _lib.check(lib.mff_ic_pairs(_lib.ptr(xv), _lib.ptr(xs), _lib.ptr(yv), _lib.ptr(ys), nd, S,
                                            _lib.ptr(pv), _lib.ptr(ps), st), "mff_ic_pairs")
                kv, ks = cross_section(pv, ps, "rank", comm=comm, stocks_total=stocks_total)
                rv[:, k], rs[:, k] = kv, ks
            _, ic_b, _ = _comb_moments(lib, rv[0], rs[0], rv[1], rs[1], K, min_obs, comm, st)
            ics[:, d0:d0 + nd] = ic_b
    weights = torch.empty((D, K), dtype=f64, device=dev)
    count = torch.empty((D, K), dtype=torch.int32, device=dev)
    status = torch.empty(D, dtype=torch.int32, device=dev)
    _lib.check(lib.mff_xs_comb_weights(_lib.ptr(ics), K, D, COMBINE_METHODS.index(method), future_days, window,
                                       min_periods, float(shrink), _lib.ptr(weights), _lib.ptr(count),
                                       _lib.ptr(status), st), "mff_xs_comb_weights")
    ov = torch.empty((D, S), dtype=f64, device=dev)
    os_ = torch.empty((D, S), dtype=u8, device=dev)
    _lib.check(lib.mff_xs_comb_apply(_lib.ptr(x_val), _lib.ptr(x_state), K, D, S, _lib.ptr(zmom), _lib.ptr(weights),
                                     _lib.ptr(status), min_factors, _lib.ptr(ov), _lib.ptr(os_), st),
               "mff_xs_comb_apply")
    return CombineResult(ov, os_, weights, ics, npairs, count, status)


def future_return(pct_val: torch.Tensor, pct_state: torch.Tensor, N: int):
    """Factor.py:142-162 on dense [D][S] daily pct_change rows: compounded return of the
    next N present days per stock (mff_future_return).  Returns (val, state) [D][S]."""
    lib = _lib.load()
    D, S = pct_val.shape
    ov = torch.empty_like(pct_val)
    os_ = torch.empty_like(pct_state)
    _lib.check(lib.mff_future_return(_lib.ptr(pct_val), _lib.ptr(pct_state), D, S, N, _lib.ptr(ov),
                                     _lib.ptr(os_), _stream(pct_val.device)), "mff_future_return")
    return ov, os_


def ic_series(x_val: torch.Tensor, x_state: torch.Tensor, y_val: torch.Tensor,
              y_state: torch.Tensor, comm=None):
    """Factor.py:163-186: per-date Pearson IC and Spearman rank IC of exposure x [D][S_loc]
    against future return y [D][S_loc] over the stocks of all ranks.  Returns (ic, rank_ic)
    float64 [D] on the device; NaN = the reference drops that date."""
    lib = _lib.load()
    D, S = x_val.shape
    dev = x_val.device
    st = _stream(dev)
    R = 1 if comm is None else comm.world_size
    pv = torch.empty((2, D, S), dtype=torch.float64, device=dev)
    ps = torch.empty((2, D, S), dtype=torch.uint8, device=dev)
    _lib.check(lib.mff_ic_pairs(_lib.ptr(x_val), _lib.ptr(x_state), _lib.ptr(y_val), _lib.ptr(y_state),
                                D, S, _lib.ptr(pv), _lib.ptr(ps), st), "mff_ic_pairs")
    rv, rs = cross_section(pv, ps, "rank", comm=comm)
    out = []
    for v, s in ((pv, ps), (rv, rs)):
        part = torch.empty((D, 6), dtype=torch.float64, device=dev)
        _lib.check(lib.mff_ic_moments(_lib.ptr(v), _lib.ptr(s), D, S, _lib.ptr(part), st),
                   "mff_ic_moments")
        part_all = part if comm is None else comm.all_gather(part)
        ic = torch.empty(D, dtype=torch.float64, device=dev)
        _lib.check(lib.mff_ic_finalize(_lib.ptr(part_all), R, D, _lib.ptr(ic), st), "mff_ic_finalize")
        out.append(ic)
    return out[0], out[1]


def group_returns(x_val: torch.Tensor, x_state: torch.Tensor, pct_val: torch.Tensor,
                  pct_state: torch.Tensor, period_of: torch.Tensor, P: int, group_num: int = 5,
                  w_val: Optional[torch.Tensor] = None, w_state: Optional[torch.Tensor] = None,
                  comm=None, stocks_total: Optional[int] = None):
    """Factor.py:231-350 on dense [D][S_loc] rows: per-date quantile groups of the
    exposure (mff_bt_qcut), per-period compounding with the previous period's group and
    weight (mff_bt_periods), per (period, group) mean / weighted mean over all ranks
    (mff_bt_reduce + all-gather + mff_bt_finalize).  period_of: int32 [D] on the device.
    Returns (ret float64 [P][G], present uint8 [P][G])."""
    lib = _lib.load()
    D, S = x_val.shape
    dev = x_val.device
    st = _stream(dev)
    R = 1 if comm is None else comm.world_size
    G = int(group_num)
    S_all = S if comm is None else shard_width(comm, S, stocks_total, dev)
    v_all = x_val if comm is None else comm.all_gather(_pad_last(x_val, S_all, 0.0))
    s_all = x_state if comm is None else comm.all_gather(_pad_last(x_state, S_all, ABSENT))
    ws = torch.empty(lib.mff_bt_qcut_workspace_bytes(D, S_all, R), dtype=torch.uint8, device=dev)
    group = torch.empty((D, S), dtype=torch.int8, device=dev)
    _lib.check(lib.mff_bt_qcut(_lib.ptr(x_val), _lib.ptr(x_state), D, S, _lib.ptr(v_all), _lib.ptr(s_all),
                               R, S_all, G, _lib.ptr(group), _lib.ptr(ws), st), "mff_bt_qcut")
    p_ret = torch.empty((P, S), dtype=torch.float64, device=dev)
    p_group = torch.empty((P, S), dtype=torch.int8, device=dev)
    p_w = torch.empty((P, S), dtype=torch.float64, device=dev)
    p_ws = torch.empty((P, S), dtype=torch.uint8, device=dev)
    _lib.check(lib.mff_bt_periods(_lib.ptr(x_state), _lib.ptr(group), _lib.ptr(pct_val), _lib.ptr(pct_state),
                                  _lib.ptr(w_val), _lib.ptr(w_state), _lib.ptr(period_of), D, S, P,
                                  _lib.ptr(p_ret), _lib.ptr(p_group), _lib.ptr(p_w), _lib.ptr(p_ws), st),
               "mff_bt_periods")
    part = torch.empty((P, G, 4), dtype=torch.float64, device=dev)
    _lib.check(lib.mff_bt_reduce(_lib.ptr(p_ret), _lib.ptr(p_group), _lib.ptr(p_w), _lib.ptr(p_ws), P, S, G,
                                 _lib.ptr(part), st), "mff_bt_reduce")
    part_all = part if comm is None else comm.all_gather(part)
    ret = torch.empty((P, G), dtype=torch.float64, device=dev)
    present = torch.empty((P, G), dtype=torch.uint8, device=dev)
    _lib.check(lib.mff_bt_finalize(_lib.ptr(part_all), R, P, G, int(w_val is not None), _lib.ptr(ret),
                                   _lib.ptr(present), st), "mff_bt_finalize")
    return ret, present


PORTFOLIO_MAX_GROUPS = 63  # G of mff_bt_qcut / mff_pf_*
PORTFOLIO_BYTES = CORR_PLANE_BYTES  # cap of the exposure / group / signal planes of one factor chunk


class PortfolioResult(NamedTuple):
    """group_portfolios: the daily group portfolios of K factors (device tensors)."""
    ret: torch.Tensor     # float64 [K][D][G]: daily return of each group's drifting-weight portfolio
    count: torch.Tensor   # int32 [K][P][G]: members over all ranks; the cell is present when > 0
    traded: torch.Tensor  # float64 [K][P][G]: two-sided turnover of the rebalance into period p


def group_portfolios(x_val: torch.Tensor, x_state: torch.Tensor, pct_val: torch.Tensor,
                     pct_state: torch.Tensor, period_of: torch.Tensor, P: int, group_num: int = 5,
                     w_val: Optional[torch.Tensor] = None, w_state: Optional[torch.Tensor] = None,
                     comm=None, stocks_total: Optional[int] = None) -> PortfolioResult:
    """Daily simulation of the G quantile portfolios of the K exposure rows x [K][D][S_loc]
    (mff_pf_*; the definition is on the declarations in include/mff.h): per factor the cut of
    group_returns (mff_bt_qcut, unchanged), membership / weight / growth per stock and period
    (mff_pf_signal), the daily value sums (mff_pf_sums), and the turnover of every rebalance
    (mff_pf_traded).  pct and the optional weight are [D][S_loc], shared by the factors;
    period_of: int32 [D] on the device.  Compounded over a period, ``ret`` is group_returns'
    number for that period.

    Stock-sharded (``comm``): the partial sums are all-gathered and merged in rank order."""
    lib = _lib.load()
    if x_val.dim() != 3 or x_state.shape != x_val.shape:
        raise ValueError("x_val and x_state must be [K][D][S]")
    K, D, S = x_val.shape
    if K < 1:
        raise ValueError("group_portfolios needs at least one factor")
    G = _int_arg("group_num", group_num, 1)
    if G > PORTFOLIO_MAX_GROUPS:
        raise ValueError(f"group_num must be at most {PORTFOLIO_MAX_GROUPS}, got {group_num!r}")
    P = _int_arg("P", P, 0)
    if tuple(pct_val.shape) != (D, S) or pct_state.shape != pct_val.shape:
        raise ValueError("pct_val and pct_state must be [D][S]")
    if (w_val is None) != (w_state is None):
        raise ValueError("w_val and w_state go together")
    if w_val is not None and (tuple(w_val.shape) != (D, S) or w_state.shape != w_val.shape):
        raise ValueError("w_val and w_state must be [D][S]")
    if int(period_of.numel()) != D:
        raise ValueError("period_of must hold one period per date")
    dev = x_val.device
    st = _stream(dev)
    f64, u8, i8 = torch.float64, torch.uint8, torch.int8
    R = 1 if comm is None else comm.world_size
    x_val, x_state = x_val.to(f64).contiguous(), x_state.to(u8).contiguous()
    pct_val, pct_state = pct_val.to(f64).contiguous(), pct_state.to(u8).contiguous()
    period_of = period_of.to(torch.int32).contiguous()
    if w_val is not None:
        w_val, w_state = w_val.to(f64).contiguous(), w_state.to(u8).contiguous()
    ret = torch.zeros((K, D, G), dtype=f64, device=dev)
    count = torch.zeros((K, P, G), dtype=torch.int32, device=dev)
    traded = torch.zeros((K, P, G), dtype=f64, device=dev)
    if D == 0:
        return PortfolioResult(ret, count, traded)
    group = torch.full((K, D, S), -1, dtype=i8, device=dev)
    if S > 0:
        S_all = S if comm is None else shard_width(comm, S, stocks_total, dev)
        ws = torch.empty(lib.mff_bt_qcut_workspace_bytes(D, S_all, R), dtype=u8, device=dev)
        for k in range(K):
            v_all = x_val[k] if comm is None else comm.all_gather(_pad_last(x_val[k], S_all, 0.0))
            s_all = x_state[k] if comm is None else comm.all_gather(_pad_last(x_state[k], S_all, ABSENT))
            _lib.check(lib.mff_bt_qcut(_lib.ptr(x_val[k]), _lib.ptr(x_state[k]), D, S, _lib.ptr(v_all),
                                       _lib.ptr(s_all), R, S_all, G, _lib.ptr(group[k]), _lib.ptr(ws), st),
                       "mff_bt_qcut")
    m = torch.empty((K, P, S), dtype=i8, device=dev)
    u = torch.empty((K, P, S), dtype=f64, device=dev)
    cend = torch.empty((K, P, S), dtype=f64, device=dev)
    _lib.check(lib.mff_pf_signal(_lib.ptr(x_state), _lib.ptr(group), _lib.ptr(pct_val), _lib.ptr(pct_state),
                                 _lib.ptr(w_val), _lib.ptr(w_state), _lib.ptr(period_of), K, D, S, P,
                                 _lib.ptr(m), _lib.ptr(u), _lib.ptr(cend), st), "mff_pf_signal")
    del group
    alloc = torch.zeros if S == 0 else torch.empty  # a shard without stocks: nothing is launched
    a_part = alloc((K, D, G), dtype=f64, device=dev)
    nu_part = alloc((K, P, G, 2), dtype=f64, device=dev)
    _lib.check(lib.mff_pf_sums(_lib.ptr(x_state), _lib.ptr(pct_val), _lib.ptr(pct_state), _lib.ptr(period_of),
                               _lib.ptr(m), _lib.ptr(u), K, D, S, P, G, _lib.ptr(a_part), _lib.ptr(nu_part), st),
               "mff_pf_sums")
    a_all = a_part if comm is None else comm.all_gather(a_part).contiguous()
    nu_all = nu_part if comm is None else comm.all_gather(nu_part).contiguous()
    tot = torch.empty((K, P, G, 2), dtype=f64, device=dev)
    _lib.check(lib.mff_pf_finalize(_lib.ptr(a_all), _lib.ptr(nu_all), _lib.ptr(period_of), R, K, D, P, G,
                                   _lib.ptr(ret), _lib.ptr(count), _lib.ptr(tot), st), "mff_pf_finalize")
    t_part = alloc((K, P, G), dtype=f64, device=dev)
    _lib.check(lib.mff_pf_traded(_lib.ptr(m), _lib.ptr(u), _lib.ptr(cend), _lib.ptr(tot), K, P, S, G,
                                 _lib.ptr(t_part), st), "mff_pf_traded")
    t_all = t_part if comm is None else comm.all_gather(t_part).contiguous()
    _lib.check(lib.mff_pf_traded_finalize(_lib.ptr(t_all), R, K, P, G, _lib.ptr(traded), st),
               "mff_pf_traded_finalize")
    return PortfolioResult(ret, count, traded)


def calendar(val: torch.Tensor, state: torch.Tensor, period_start: torch.Tensor, method: str):
    """MinFreqFactor.cal_final_exposure(mode='calendar') (MF:130-186, the build's definition):
    dense [D][S] -> [P][S] per calendar window (period_start int32 [P+1] on the device)."""
    lib = _lib.load()
    D, S = val.shape
    P = int(period_start.numel()) - 1
    ov = torch.empty((P, S), dtype=torch.float64, device=val.device)
    os_ = torch.empty((P, S), dtype=torch.uint8, device=val.device)
    _lib.check(lib.mff_calendar(_lib.ptr(val), _lib.ptr(state), _lib.ptr(period_start), D, S, P,
                                ROLL_METHODS[method], _lib.ptr(ov), _lib.ptr(os_), _stream(val.device)),
               "mff_calendar")
    return ov, os_
