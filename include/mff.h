/*
 * mff.h — C ABI of libmff.so, the MI355X (gfx950) minute-factor engine.
 *
 * The reference (C-X-Lu/Replication-of-Minute-Frequency-Factor) has no FFI: its
 * operator API is a Python callable, `calculate_method(df) -> df`, handed to
 * `MinFreqFactor.cal_exposure_by_min_data` (MinuteFrequentFactorCICC.py:50-55) and
 * invoked per day file at MinuteFrequentFactorCICC.py:22.  Each entry point below
 * replaces one piece of that path; the reference interface it replaces is cited on
 * every declaration.  INTEGRATION.md shows the ctypes binding a maintainer adds.
 *
 * Conventions
 *  - All pointers are DEVICE pointers owned by the caller (the library never
 *    allocates or frees caller memory).  Host pointers are marked `host`.
 *  - `stream` is a hipStream_t passed as void* (NULL = default stream).  Every call
 *    is asynchronous on that stream; none synchronises, allocates, or copies, so a
 *    caller may capture them into a hipGraph.
 *  - Return 0 on success, negative on error; mff_last_error() gives a thread-local
 *    message.  No C++ exception crosses this ABI.
 *  - Panel layout: field planes open/high/low/close float32 and volume uint32 (shares),
 *    each [D][S][240] (day, stock, minute 0..239 = 09:30..11:29, 13:00..14:59); presence
 *    mask uint32 [D][S][8], bit (m % 32) of word (m / 32) set when bar m exists.
 *    Prices finite > 0; volume 0 <= v <= MFF_VOLUME_MAX (the all-ones word is the sorts'
 *    absent-bar key).  Values of absent bars are don't-care.
 *  - Output layout: val float64 [rows][D][S], state uint8 [rows][D][S] with
 *    0 = ABSENT (the reference emits no row), 1 = NULL (polars null),
 *    2 = VALUE (may be NaN / +-inf).
 */
#ifndef MFF_H
#define MFF_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MFF_NUM_FACTORS 58
#define MFF_STATE_ABSENT 0
#define MFF_STATE_NULL 1
#define MFF_STATE_VALUE 2

/* stage 2 methods, MinuteFrequentFactorCICC.py:190-238 */
#define MFF_ROLL_O 0   /* identity            MF:190-198 */
#define MFF_ROLL_M 1   /* rolling_mean        MF:199-209 */
#define MFF_ROLL_Z 2   /* (x-mean)/std(ddof0) MF:210-227 */
#define MFF_ROLL_STD 3 /* rolling_std(ddof0)  MF:228-238 */

/* stage 3 kinds */
#define MFF_XS_Z 0
#define MFF_XS_RANK 1

int mff_version(void);
const char* mff_last_error(void);
int mff_num_factors(void);
/* name of factor `id` (reference column name, e.g. "mmt_pm"); NULL if out of range */
const char* mff_factor_name(int id);

/* mff_ingest_rows volume column types */
#define MFF_VOLUME_F64 0
#define MFF_VOLUME_I64 1
#define MFF_VOLUME_F32 2
#define MFF_VOLUME_I32 3

/* mff_ingest_rows counters (uint32 errors[5]) */
#define MFF_INGEST_ERR_INDEX 0  /* stock / day index outside [0,S) x [0,D): row skipped */
#define MFF_INGEST_ERR_TIME 1   /* time off the 240-bar grid: row skipped (not an error: the
                                   caller lists the stock-day in the row set) */
#define MFF_INGEST_ERR_DUP 2    /* (stock, day, minute) already present (the same) */
#define MFF_INGEST_ERR_PRICE 3  /* open/high/low/close not finite > 0 */
#define MFF_INGEST_ERR_VOLUME 4 /* volume not integral in [0, MFF_VOLUME_MAX] */
#define MFF_VOLUME_MAX 4294967294u /* 2^32 - 2 shares per bar */

/*
 * Ingest: long day-frame rows -> dense panel.
 * Replaces: the per-file `pl.read_parquet` hand-off (MinuteFrequentFactorCICC.py:22)
 * and the time -> minute map minute_in_trade (CM:98-106).  Row i: stock[i] / day[i]
 * (dense indices into the caller's sorted code / date universes, int32), time[i]
 * (HHMMSSmmm, int64), the four prices (float64) and volume (volume_kind).  Writes the
 * four fp32 price planes and the u32 volume plane of `bars` [5][D][S][240] (4 B per bar
 * each; the caller views the volume plane as uint32) at (day, stock, minute), ORs the presence
 * bit into `valid` [D][S][8]; `valid` and `errors` (uint32[5], MFF_INGEST_ERR_*) must be
 * zeroed by the caller before the first call into a panel, so a panel may be filled by
 * several calls (day-file batches).  Contract violations are counted, never trapped;
 * the caller reads `errors` and rejects the panel if any is non-zero.
 */
int mff_ingest_rows(const int32_t* stock, const int32_t* day, const int64_t* time,
                    const double* open, const double* high, const double* low,
                    const double* close, const void* volume, int volume_kind, int64_t nrows,
                    int S, int D, float* bars, uint32_t* valid, uint32_t* errors, void* stream);

/*
 * Stage 1: the per-(stock, day) factor kernels.
 * Replaces: every `cal_<name>(df)` of MinuteFrequentFactorCalculateMethodsCICC.py
 * (CM:12-1406) applied per day file by `_process_single_file`
 * (MinuteFrequentFactorCICC.py:17-25), for D days x S stocks at once.
 * factor_ids (host, nf entries): catalogue ids in output-row order.
 * pdf_query: float64 [5][D][S] workspace, required when any doc_pdf* id is requested
 * (the doc_pdf values are then produced by mff_pdf_* below), else may be NULL.
 * pdf_levels: mff_pdf_levels_bytes(S, D) bytes, required with doc_pdf (else NULL): per
 * day, every stock-day's price levels as (key c_last/c_level, total-order u64; bars at
 * the level, u8) that mff_pdf_count / mff_pdf_rank_local bin against the sorted queries
 * (filled and counted by the call itself), in two lists split at a key the library sets
 * per call (the mean median doc_pdf query of earlier calls on the device; 1.0 before
 * any: any key gives the same ranks): the keys below it from the front of the day's
 * S*256 slots (at most 255 levels per stock-day: MFF_ROWS_MAX), the others from the back, with the per-day counts (u32 pairs A, B = one
 * u64 counter per day) and the split key u64 in front.
 * workspace: mff_stage1_workspace_bytes(S, D) bytes of device scratch (the list of
 * stock-days the exact general path finishes; zeroed by the call itself).
 * Environment MFF_STAGE1_IMPL=w64 selects the wave-per-stock-day kernel for everything;
 * MFF_STAGE1G_FULL=0 keeps the group kernel on its general (per-bar presence mask) form
 * for waves whose stock-days hold every bar (a test hook: the results are the same bits).
 */
size_t mff_stage1_workspace_bytes(int S, int D);
/* mff_stage1 in two calls with the same arguments: part 1 = the LVL/PDF group (
 * doc_pdf levels and queries, exact list), part 2 = ORD + the serial families.  Once part 1 is
 * done the mff_pdf_* phases may run on another stream, concurrently with part 2.
 * part 3 = mff_stage1.  part 4 = the high / low serial families (OLS, MOMH) alone, which
 * depend on no other launch (any stream, any time); part 10 / 11 = part 2 / 3 without them.
 * part 17 = part 1 without the exact list kernel, part 32 = that kernel alone (after part
 * 17, before the mff_pdf_* phases and before the LVL/PDF rows are read; part 2 need not
 * wait for it).  part 64 = part 1's prologue alone (zeroes the doc_pdf level-list counts,
 * sets the split key, zeroes the exact-list count: mff_stage1_rows phase 1 may start after
 * it), part 129 / 145 = part 1 / 17 without that prologue. */
int mff_stage1_part(const float* open, const float* high, const float* low,
                    const float* close, const uint32_t* volume, const uint32_t* valid,
                    int S, int D, const int32_t* factor_ids /* host */, int nf,
                    double* val, uint8_t* state, double* pdf_query, void* pdf_levels,
                    void* workspace, void* stream, int part);
size_t mff_pdf_levels_bytes(int S, int D);
int mff_stage1(const float* open, const float* high, const float* low,
               const float* close, const uint32_t* volume, const uint32_t* valid,
               int S, int D, const int32_t* factor_ids /* host */, int nf,
               double* val, uint8_t* state, double* pdf_query, void* pdf_levels,
               void* workspace, void* stream);

/*
 * Row set: the stock-days computed from their own rows instead of the 240-bar grid.
 * A stock-day is listed when a row of it holds a polars null (open / high / low / close /
 * volume) or sits off the grid (a time that is not a 09:30-11:29 / 13:00-14:59 minute:
 * a 09:25 or 15:00 bar, end-labelled bars, seconds) or shares its time with another row.
 * The panel's `valid` mask holds zeros for a listed stock-day except bit 31 of word 7
 * (MFF_ROWS_LISTED: bars end at 239), so the grid kernels see it ABSENT and store nothing
 * for it -- mff_stage1_rows writes all its rows and may run on another stream at the same
 * time.  A stock-day listed only for nulls on grid bars (its rows are its present bars)
 * may instead keep its presence bits in `valid` and carry MFF_ROWS_KEEP plus the null
 * fields (bit MFF_ROWS_NULL_SHIFT + i: field i = open, high, low, close, volume holds a
 * null on some bar) in word 7 AND in the `reserved` word of its first row: then a family
 * that reads none of those fields comes from the grid kernels (its values do not depend
 * on the null fields) and mff_stage1_rows computes only the families that read one.
 * The row set carries every one of its rows:
 *   rs_sd int32 [K]     d*S + s, ascending
 *   rs_off int32 [K+1]  rows of stock-day i: rs_rows[rs_off[i] .. rs_off[i+1]), at most
 *                       MFF_ROWS_MAX, in (time, frame) order (rows at one time
 *                       keep their frame order), minute_in_trade (CM:98-106) non-decreasing
 *   rs_rows MffRow [rs_off[K]]  time HHMMSSmmm in [0, 240000000), prices fp32, volume u32
 *                       shares, nulls = bit i set when field i (open, high, low, close,
 *                       volume) is null (its value is then don't-care), reserved = 0 except
 *                       on a kept stock-day's first row (MFF_ROWS_KEEP | null fields, as in
 *                       its `valid` word 7)
 */
#define MFF_ROWS_MAX 255
#define MFF_ROWS_LISTED 0x80000000u /* valid[d][s][7] of a listed stock-day */
#define MFF_ROWS_KEEP 0x40000000u   /* grid bars kept; only the families reading a null field listed */
#define MFF_ROWS_NULL_SHIFT 24      /* bits 24..28: the fields holding a null (with MFF_ROWS_KEEP) */
typedef struct MffRow {
  int32_t time;
  float open, high, low, close;
  uint32_t volume;
  uint32_t nulls;
  uint32_t reserved;
} MffRow; /* 32 B */

/*
 * Stage 1 of the row set.  Replaces the same `cal_*` calls (CM:12-1406) on those rows:
 * polars' null rules (only cal_liq_amihud_1min fills a null volume with 0, CM:743-744;
 * first()/last() return the null, CM:799, 829; sums / moments skip it; pl.corr drops the
 * pair, CM:841-931; pct_change forward-fills, CM:745, 861-866; top_k prefers non-null
 * values, CM:393-471; rank() leaves a null key unranked, CM:1016 -- the rules N1-N11 / C8
 * of oracle/mff_oracle.py), the time filters on each row's own time (CM:18-84, 770-815,
 * 1212-1387) and the 50-minute OLS windows over minute_in_trade (CM:98-129).
 * phase 1: doc_pdf queries + the stock-days' price levels appended to pdf_levels (call
 *          after mff_stage1_part 1 / 17 and before mff_pdf_sort);
 * phase 2: every other requested row (call after the stage-1 calls that write those rows);
 * phase 3: both (e.g. after mff_stage1 when no doc_pdf row is requested).
 */
int mff_stage1_rows(int S, int D, const int32_t* rs_sd, const int32_t* rs_off, const MffRow* rs_rows, int K,
                    const int32_t* factor_ids /* host */, int nf, double* val, uint8_t* state,
                    double* pdf_query, void* pdf_levels, int phase, void* stream);
/*
 * Grid stock-days -> rows (e.g. to list stock-days of a device-built panel): for each of
 * the K stock-days sd[K], its present bars in minute order, time = the bar's start label,
 * null bits from null_bits uint32 [K][5][8] (the `valid` bit layout per field; NULL =
 * none).  Count mode (rows == NULL): counts int32 [K] = rows per stock-day (the caller
 * turns them into off [K+1]); else the rows are written at rows[off[i] ...].
 */
int mff_rows_from_panel(const float* open, const float* high, const float* low, const float* close,
                        const uint32_t* volume, const uint32_t* valid, int S, int D, const int32_t* sd,
                        const uint32_t* null_bits, int K, const int32_t* off, int32_t* counts, MffRow* rows,
                        void* stream);

/*
 * Multi-day frame semantics of the four factors whose reference windows run over('code')
 * only: liq_amihud_1min (CM:745-746 pct_change over code), corr_prvr (CM:855-867),
 * trade_bottom20retRatio (CM:1212-1216 volume.sum().over('code')) and
 * trade_bottom50retRatio (CM:1233-1241).  The reference driver calls cal_* per day file
 * (MinuteFrequentFactorCICC.py:22), where they are per-day; a cal_* handed a frame of
 * several dates reaches across them.  Given the panel of such a frame (days = the frame's
 * dates, rows of a code in (date, time) order) and stage 1's output rows, this call
 * overwrites the rows of those four factors (when present in factor_ids) with the frame
 * semantics: the first bar of a day compares with the code's last close of the previous
 * day, and the 14:40+ / 14:10+ volume share uses the code's total over the whole frame.
 * open may be NULL unless a trade_bottom* row is requested.  rs_sd / rs_off / rs_rows (the
 * panel's row set, K = 0 and NULLs when it has none) give the listed stock-days' rows: a
 * null volume is 0 for the Amihud sum (CM:743-744) and filtered out by volume != 0
 * (CM:855), a null close is forward-filled by pct_change (CM:745, 861), the tail windows
 * test each row's own time (CM:1212, 1233).
 */
int mff_stage1_frame(const float* open, const float* close, const uint32_t* volume,
                     const uint32_t* valid, int S, int D, const int32_t* rs_sd, const int32_t* rs_off,
                     const MffRow* rs_rows, int K, const int32_t* factor_ids /* host */, int nf,
                     double* val, uint8_t* state, void* stream);

/*
 * doc_pdf60..95 frame-wide rank (CM:1015-1017: `.rank()` over ALL rows of the day
 * frame, every code).  Device phases; each works on days [d0, d0+nd) of arrays laid
 * out over all D days.
 *   sort:     queries of R ranks, float64 [R][5][D][S_all] (NaN = none; each rank's
 *             [5][D][S_loc] padded to S_all with NaN)
 *             -> q_sorted uint64 [nd][M], M = R*5*S_all (total-order keys; any M: beyond
 *             32768 per day the sort finishes with global merge passes)
 *   count:    this rank's keys c_last/c_b (from stage 1's pdf_levels: one key per
 *             distinct close of a stock-day, weighted by its bar count) against q_sorted
 *             -> counts uint32 [nd][M] = 2 n_less + n_eq over local keys (the
 *             average rank n_less + (n_eq + 1) / 2 is linear in it)
 *   [R > 1: the caller sums `counts` over ranks (reduce-scatter to each day's owner, or
 *    an all-reduce), see INTEGRATION.md]
 *   finalize: own queries [5][D][S_loc] -> val/state rows pdf_rows[5] (host, -1 = skip),
 *             looking each query up in the day's sorted list and the summed counts
 *   origin_counts: day-owner side of the reduce-scatter exchange: the summed counts of
 *             the owned days at each query of q_all [R][5][D][S_all] (days [d0, d0+nd)),
 *             written in that origin layout -> out uint32 [R][5][nd][S_all] (0 for NaN);
 *             q_sorted / counts may be the deduplicated lists [nd][M] (M <= R*5*S_all,
 *             each day's distinct keys padded with ~0: the counts of a value sit at its
 *             first position);
 *             one all_to_all then hands every rank its own queries' counts
 *   finalize_own: own queries [5][D][S_loc] with their counts in the same layout
 *             (2 n_less + n_eq summed over ranks) -> val/state (rank (c + 1) / 2)
 *   rank_local: count + finalize in one pass, for a single rank (R = 1: no exchange)
 * workspace: mff_pdf_workspace_bytes(S_loc, R, nd) bytes of device scratch (sort).
 */
size_t mff_pdf_workspace_bytes(int S_loc, int R, int nd);
int mff_pdf_sort(const double* q_all, int R, int S_all, int D, int d0, int nd,
                 uint64_t* q_sorted, void* workspace, void* stream);
int mff_pdf_count(const void* pdf_levels, int S_loc, int D, int d0, int nd,
                  const uint64_t* q_sorted, int M, uint32_t* counts, void* workspace,
                  void* stream);
/* Frame-wide count (one cal_doc_pdf* call on a frame holding several dates: `.rank()`
 * at CM:1015-1017 ranks every row of every date).  The D days' queries are sorted as ONE
 * list (mff_pdf_sort with the [5][D][S] queries viewed as [5][1][D*S]); every day's level
 * keys are counted against it and their words 2 n_less + n_eq ADDED to counts uint32 [M]
 * (zeroed by the caller); mff_pdf_finalize with S_loc = D*S, D = 1 then writes the ranks.
 * Requires 240*S*D < 2^31 and M <= 2^24. */
int mff_pdf_count_frame(const void* pdf_levels, int S, int D, const uint64_t* q_sorted, int M,
                        uint32_t* counts, void* stream);
int mff_pdf_finalize(const double* q_local, const uint64_t* q_sorted,
                     const uint32_t* counts, int S_loc, int D, int d0, int nd, int M,
                     const int32_t* pdf_rows /* host, 5 entries, -1 = skip */,
                     double* val, uint8_t* state, void* stream);
int mff_pdf_origin_counts(const double* q_all, int R, int S_all, int D, int d0, int nd,
                          const uint64_t* q_sorted, const uint32_t* counts, int M, uint32_t* out,
                          void* stream);
int mff_pdf_finalize_own(const double* q_local, const uint32_t* own_counts, int S_loc, int D,
                         const int32_t* pdf_rows /* host, 5 entries, -1 = skip */, double* val,
                         uint8_t* state, void* stream);
int mff_pdf_rank_local(const void* pdf_levels, const double* q_local,
                       int S, int D, int d0, int nd, const uint64_t* q_sorted, int M,
                       const int32_t* pdf_rows /* host, 5 entries */, double* val,
                       uint8_t* state, void* stream);

/*
 * Stage 2: N-day rolling post-processing over present days, per stock.
 * Replaces: MinFreqFactor.cal_final_exposure(frequency=N, method, mode='days')
 * (MinuteFrequentFactorCICC.py:187-240).  rows = number of factor rows.
 * Any N >= 1, like the reference's `frequency: int` (MF:188-189, 205).
 */
int mff_stage2(const double* val, const uint8_t* state, int rows, int D, int S,
               int N, int method, double* out_val, uint8_t* out_state, void* stream);

/*
 * Calendar resampling, mode='calendar' of cal_final_exposure (MinuteFrequentFactorCICC.py:
 * 130-186; the reference raises there: group_by_dynamic without index_column, MF:145 —
 * this is the build's definition): per stock and calendar window p (days
 * [period_start[p], period_start[p+1]), period_start int32 [P+1] device, date-sorted),
 * over the window's rows: 'o' last value (null if the last row is null), 'm' mean,
 * 'std' std (ddof=1), 'z' (last - mean) / std; nulls skipped, NaN propagates.
 * Output [P][S]: ABSENT where the stock has no row in the window.
 */
int mff_calendar(const double* val, const uint8_t* state, const int32_t* period_start, int D,
                 int S, int P, int method, double* out_val, uint8_t* out_state, void* stream);

/*
 * Stage 3: per-day cross-sectional z-score (ddof=1) or average rank over stocks with
 * state VALUE and non-NaN value.  No single reference function; closest semantics
 * Factor.py:99-105 (coverage), :163-186 (per-date Pearson / Spearman), :285-291 (qcut).
 * z-score, multi-GPU: mff_xs_moments per rank -> all-gather [R][rows][D][3] ->
 * mff_xs_zscore.  rank: all-gather values/states [R][rows][D][S_all] (every rank's
 * columns padded to S_all with ABSENT) -> mff_xs_rank.
 */
int mff_xs_moments(const double* val, const uint8_t* state, int rows, int D, int S,
                   double* moments /* [rows][D][3]: n, mean, M2 */, void* stream);
int mff_xs_zscore(const double* val, const uint8_t* state, int rows, int D, int S,
                  const double* moments_all, int R, double* out_val,
                  uint8_t* out_state, void* stream);
/* Single-rank z in one pass (same result contract as moments + zscore with R = 1):
 * one workgroup per (row, day) holds the column in registers; S <= max_stocks(). */
int mff_xs_zscore_local(const double* val, const uint8_t* state, int rows, int D, int S,
                        double* out_val, uint8_t* out_state, void* stream);
int mff_xs_zscore_local_max_stocks(void);
/* Rank workspace layout, with nseg = rows * D, M = R * S_all, g = min(nseg, 2048):
 *   [0, sort)          the sorting kernel's buffers: sort = 256 bytes (unused) when
 *                      M <= 8192 (the sort runs in LDS), else g * 2 * M * 8 bytes (two u64
 *                      [M] ping-pong buffers per workgroup);
 *   [sort, sort + lst) the hand-over list, uint32 [1 + nseg]: word 0 = the number of
 *                      (row, day) segments the bucketed kernels handed to the sorting kernel
 *                      in this call, then their segment indices (row * D + day) in no
 *                      particular order; lst = 4 * (nseg + 1) rounded up to 256.
 * The list is written only when M <= 8192 and the bucketed kernels run (not under
 * MFF_XS_RANK_IMPL=sort); otherwise its bytes are left untouched.  The count is valid once
 * the call's stream work has completed. */
size_t mff_xs_rank_workspace_bytes(int rows, int D, int S_all, int R);
int mff_xs_rank(const double* val, const uint8_t* state, int rows, int D, int S_loc,
                const double* val_all, const uint8_t* state_all, int R, int S_all,
                double* out_val, uint8_t* out_state, void* workspace, void* stream);

/*
 * Cross-sectional preprocessing ahead of the IC / group tests: per-day MAD winsorisation,
 * industry / size neutralisation and standardisation of exposure rows [rows][D][S].  No
 * reference function (the reference tests raw exposures, Factor.py:127-350); this is the
 * build's definition.  One segment = one row on one day, over its S stocks.
 *   group int32 [D][S]: industry id in [0, G), anything else (-1) = none; NULL = no
 *     industries (one group: intercept only).  G <= max_groups().
 *   size / size_state [D][S]: the size covariate itself (normally ln market cap) and its
 *     state; NULL = no covariate.
 *   Usable set U: state VALUE and x finite; an industry, when group is given; size_state
 *     VALUE and size finite, when size is given.  n = |U|.
 *   1. winsor_k > 0: med = median of x over U (numpy.median: the mean of the two middle
 *      order statistics for even n), mad = median of |x - med|; mad > 0: x clipped to
 *      med -+ winsor_k * 1.4826 * mad; mad == 0: no clipping.
 *   2. e = the OLS residual of x on industry dummies + size by within-industry demeaning:
 *      x~ = x - mean_g(x), z~ = z - mean_g(z) over the industry's members of U,
 *      beta = sum(x~ z~) / sum(z~ z~) (0 when the denominator is 0), e = x~ - beta z~
 *      (e = x~ without a covariate).
 *   3. standardize != 0: e <- (e - mean(e)) / sd(e), ddof = 1.
 *   Degrees of freedom: k = non-empty industries among U (+ 1 with a covariate);
 *   n - k < 1, or n < 2 when standardising: every stock of U gets NULL.
 *   States: ABSENT stays ABSENT, NULL stays NULL, a VALUE NaN / +-inf passes through
 *   unchanged, a finite VALUE without industry or size becomes NULL, U gets VALUE (or NULL
 *   by the rule above).  The result is bit-identical from run to run (fixed summation
 *   orders, no floating-point atomics).
 * workspace: mff_xs_neutralize_workspace_bytes(D, S) bytes of device scratch, required
 * when group is given (the per-day industry order, built by the call itself).
 * Errors (negative, nothing launched): S > max_stocks(), G outside [1, max_groups()] with
 * group given, a negative size, size without size_state.
 */
int mff_xs_neutralize_max_stocks(void); /* 8192 */
int mff_xs_neutralize_max_groups(void); /* 256 */
size_t mff_xs_neutralize_workspace_bytes(int D, int S);
int mff_xs_neutralize(const double* val, const uint8_t* state, int rows, int D, int S,
                      const int32_t* group /* [D][S], -1 = none; NULL = no industries */, int G,
                      const double* size, const uint8_t* size_state /* [D][S]; NULL = no covariate */,
                      double winsor_k /* <= 0: off */, int standardize,
                      double* out_val, uint8_t* out_state, void* workspace, void* stream);

/*
 * Pairwise factor correlation: per day the rows x rows matrix of the cross-sectional
 * correlations of exposure rows [rows][D][S] (rows = F factors), and its mean over days.
 * No reference function (Factor.py never relates two factors); this is the build's
 * definition, restated in numpy by tests/xs_corr_ref.py.
 *   Usable entry u_i[d][s]: state VALUE and x finite (the usable set of mff_xs_neutralize;
 *     NaN and +-inf drop out of the pair like a null).
 *   Pair set P_ij(d) = {s : u_i and u_j}, n_ij = |P_ij|.
 *   corr_ij(d) = the Pearson correlation of (x_i, x_j) over P_ij(d), both means taken over
 *     P_ij(d) (pairwise-complete, as pandas.DataFrame.corr); NaN when n_ij < min_pairs
 *     (min_pairs >= 2) or when either side is constant on the pair set.
 *   Constant rule: with y = x - c_i, c_i the row's centre of that day (below), side i is
 *     constant on P_ij when var_i|j <= 1e-12 * Q_ij, Q_ij = sum_P y_i^2,
 *     var_i|j = Q_ij - (sum_P y_i)^2 / n_ij.  It catches an exactly constant pair set (whose
 *     one-pass variance is rounding residue, not 0); a non-constant one reaches it only when
 *     its spread is 1e-6 of its offset from the row mean, which f64 sums cannot resolve.
 *   The diagonal is exactly 1.0 where defined (NaN when n_ii < min_pairs or the row is
 *   constant), the matrix is bitwise symmetric (i <= j computed, then mirrored), values are
 *   clamped to [-1, 1], n (int32) is always written and exact, and the result is
 *   bit-identical from run to run (fixed summation orders, no floating-point atomics).
 *   Spearman = the same on rows replaced per day by their average ranks over their own
 *   usable set (mff_xs_rank after non-finite values are masked to NULL); the ranks are not
 *   recomputed inside each pair set.
 *   Numerics: no raw sum x, sum x^2.  Every row is centred per day by c_i(d), a value close
 *   to its mean over its usable set (the correlation is shift-invariant: any finite centre
 *   common to all shards gives the same result up to rounding); with m the 0/1 usable mask
 *     n_ij = sum_s m_i m_j,  A_ij = sum_s y_i m_j,  Q_ij = sum_s y_i^2 m_j,  P_ij = sum_s y_i y_j,
 *     cov_ij = P_ij - A_ij A_ji / n_ij,  var_i|j = Q_ij - A_ij^2 / n_ij,
 *     corr_ij = cov_ij / (sqrt(var_i|j) sqrt(var_j|i)).
 *   The four sums are f64 matrix-core products over the stock axis (v_mfma_f64_16x16x4_f64).
 * moments: per (row, day) n and sum of x over the usable set of the local S stocks
 *   -> [rows][D][2] (stock shards: all-gather, centre = sum of sums / sum of n).
 * sums: the four rows x rows planes of the local stocks -> sums [D][4][rows][rows] (n, A, Q,
 *   P; plane entry [i][j]); center [rows][D], or NULL: each row's own mean over the local
 *   usable set, computed by the call in `workspace` (mff_xs_corr_workspace_bytes bytes; may
 *   be NULL when center is given).
 * finalize: add the R shards' planes in rank order and apply the definition -> corr f64, n
 *   int32, both [D][rows][rows].
 * mean: per (i, j) the mean over days of the non-NaN corr entries, summed in day order
 *   -> mean f64 (NaN when there is none), days int32 (their count), both [rows][rows].
 * Errors (negative, nothing launched): rows < 1, rows > max_rows(), min_pairs < 2, a negative
 * size.  D == 0 or S == 0 is a success (empty result; all-zero planes, NaN corr, n = 0).
 */
int mff_xs_corr_max_rows(void); /* 1024 */
size_t mff_xs_corr_workspace_bytes(int rows, int D, int S);
int mff_xs_corr_moments(const double* val, const uint8_t* state, int rows, int D, int S,
                        double* moments, void* stream);
int mff_xs_corr_sums(const double* val, const uint8_t* state, int rows, int D, int S,
                     const double* center, double* sums, void* workspace, void* stream);
int mff_xs_corr_finalize(const double* sums_all /* [R][D][4][rows][rows] */, int R, int rows, int D,
                         int min_pairs, double* corr, int32_t* n, void* stream);
int mff_xs_corr_mean(const double* corr, int rows, int D, double* mean, int32_t* days, void* stream);

/*
 * Per-day multi-factor cross-sectional regression (Fama-MacBeth / pure factor returns):
 * per day the weighted least squares of a regressand on industry dummies and K exposure
 * rows, with t-statistics and R^2, and the time aggregate of the coefficients.  No reference
 * function (Factor.py never regresses); this is the build's definition,
 * restated in numpy by tests/xs_reg_ref.py.
 *   Inputs: x [K][D][S] (val f64, state u8), y [D][S] (val, state), optional weight /
 *   weight_state [D][S] (the WLS weight itself; NULL = all 1), optional group int32 [D][S]
 *   with ids in [0, G), anything else = none (NULL = no industries: one group, i.e. a plain
 *   intercept), min_obs.
 *   Usable set U of a day (listwise): every one of the K rows VALUE and finite, y VALUE and
 *     finite, the weight VALUE, finite and > 0 when weights are given, an industry when group
 *     is given.  n = |U| (int32) is always written and exact.
 *   Model: WLS of y on [dummies of the non-empty industries | x_1..x_K] by Frisch-Waugh: with
 *     the weighted means over U and g, x~ = x - mean_g(x), y~ = y - mean_g(y),
 *     M = sum_U w x~ x~^T (K x K), b = sum_U w x~ y~, T = sum_U w y~^2, beta solves M beta = b.
 *     M, b and T are accumulated on the centred values (f64 matrix-core products over the
 *     stock axis, v_mfma_f64_16x16x4_f64); raw second moments are never differenced.
 *   dof = n - K - G_ne, G_ne = the non-empty industries among U (1 without group).
 *     n < max(min_obs, 1) or dof < 1: status 1, beta, t and r2 of the day NaN.
 *   Singular rule (counting and fixed thresholds only): column j is constant within
 *     industries when M_jj <= 1e-20 * sum_U w x_j^2 (the raw second moment); otherwise M is
 *     scaled to a unit diagonal and factored by an unpivoted f64 Cholesky, a pivot <= 1e-10
 *     = collinear.  Either case: status 2, NaN outputs for the day.
 *   Constant regressand, by the same threshold: T <= 1e-20 * sum_U w y^2 is an exact fit,
 *     b and T count as 0 (beta = 0, RSS = 0, t NaN).
 *   Outputs per day: beta [D][K]; RSS = max(T - b^T beta, 0), sigma^2 = RSS / dof,
 *     se_j = sqrt(sigma^2 (M^-1)_jj), tstat [D][K] = beta_j / se_j (NaN when se_j == 0);
 *     r2 [D] = 1 - RSS / (T + sum_g W_g (ybar_g - ybar_w)^2), the denominator being
 *     sum_U w (y - ybar_w)^2 of the intercept-only model, NaN when it is <= 1e-20 * sum_U w y^2;
 *     n, dof, status int32 [D].
 *   Residual: e = y~ - x~^T beta [D][S]; state VALUE on U, NULL where y is VALUE but the
 *     stock is outside U and everywhere on a day with status != 0; ABSENT / NULL of y kept.
 *   Time aggregate per factor over the status-0 days, added in day order: agg [K][6] =
 *     (days, mean beta, std ddof = 1 (NaN when days < 2), t_fm = mean / (std / sqrt(days)), NaN
 *     when days < 2 or std == 0, mean |t|, share of |t| > 2 -- the last two over the status-0
 *     days whose t is not NaN, NaN when there is none); overall [2] = (mean r2 over the
 *     status-0 days with an r2, mean n over the status-0 days).
 *   The result is bit-identical from run to run (fixed summation orders: stock order inside
 *   an MFMA chain, wave order, plane order, day order; no floating-point atomics).
 * workspace: mff_xs_reg_workspace_bytes(K, D, S, G) bytes of device scratch shared by the
 *   calls of one regression (G = 0 without group): per-day scalars f64 [D][K + 5], the means
 *   table f64 [D][max(G, 1)][K + 1], the usable-set plane int32 [D][S] (the stock's industry,
 *   0 without group, inside U; -1 outside), each part 256-B aligned, in that order.
 * groups: the usable-set plane (into workspace) and the local group sums
 *   gsums f64 [nsplit][D][Ge + 1][K + 3], Ge = max(G, 1), one plane per run of the stocks (cut
 *   into nsplit runs of whole 32-stock tiles): row g < Ge = (n_g, W_g, sum w c for the K + 1
 *   columns: the x rows, then y), row Ge = (0, 0, the raw sum w c^2 of each column).
 * gram: adds the R planes of group sums [R][D][Ge + 1][K + 3] (shards x runs) in plane order
 *   into the means table and the per-day scalars (workspace), then the local Gram planes
 *   sum w c~ c~^T of the K + 1 columns -> gram f64 [nsplit][D][K + 1][K + 1], one workgroup per
 *   (day, run of the stocks).
 * solve: adds the P planes [P][D][K + 1][K + 1] (shards x splits) in plane order and applies
 *   the definition.  Needs the workspace gram filled.
 * residual: the residual of the local stocks from beta, status and the workspace.
 * mean: the time aggregate.
 * Errors (negative, nothing launched, nothing written): K < 1, K > max_factors(), G outside
 * [1, max_groups()] with group given (gram / residual: outside [0, max_groups()]), a negative
 * size, a weight without its state, min_obs < 0.  D == 0 or S == 0 is a success (empty
 * result; n = 0, status 1, NaN outputs).
 */
int mff_xs_reg_max_factors(void); /* 63: K + 1 columns fill one 64-row block */
int mff_xs_reg_max_groups(void);  /* 256 */
size_t mff_xs_reg_workspace_bytes(int K, int D, int S, int G);
int mff_xs_reg_groups(const double* x_val, const uint8_t* x_state, int K, int D, int S,
                      const double* y_val, const uint8_t* y_state, const double* weight,
                      const uint8_t* weight_state, const int32_t* group, int G, int nsplit,
                      double* gsums, void* workspace, void* stream);
int mff_xs_reg_gram(const double* x_val, int K, int D, int S, const double* y_val,
                    const double* weight, int G /* 0 = no industries */, const double* gsums_all, int R,
                    int nsplit, double* gram, void* workspace, void* stream);
int mff_xs_reg_solve(const double* gram_all, int P, int K, int D, int min_obs, double* beta,
                     double* tstat, double* r2, int32_t* n, int32_t* dof, int32_t* status,
                     void* workspace, void* stream);
int mff_xs_reg_residual(const double* x_val, int K, int D, int S, const double* y_val,
                        const uint8_t* y_state, int G, const double* beta, const int32_t* status,
                        double* out_val, uint8_t* out_state, void* workspace, void* stream);
int mff_xs_reg_mean(const double* beta, const double* tstat, const double* r2, const int32_t* n,
                    const int32_t* status, int K, int D, double* agg, double* overall, void* stream);

/*
 * Per-day factor orthogonalisation: the K exposure rows of a day are standardised over the
 * listwise usable set and mapped to K mutually uncorrelated unit-variance rows, symmetrically
 * (Loewdin) or by Gram-Schmidt in row order.  No reference function (Factor.py never combines
 * factors); this is the build's definition, restated in numpy by
 * tests/xs_orth_ref.py.
 *   Inputs: x [K][D][S] (val f64, state u8), 1 <= K <= 64; method 0 = symmetric, 1 =
 *   Gram-Schmidt in row order; min_obs >= 0.
 *   Usable set U of a day (listwise): every one of the K rows VALUE and finite.  n = |U|
 *     (int32) is always written and exact.
 *   Standardise: c_j = x_j - mean_U(x_j); M = sum_U c c^T (K x K), accumulated on the centred
 *     values (f64 matrix-core products over the stock axis, v_mfma_f64_16x16x4_f64; raw second
 *     moments are never differenced); sigma_j = sqrt(M_jj / (n - 1)), z_j = c_j / sigma_j;
 *     R_ij = M_ij / sqrt(M_ii M_jj) with the diagonal exactly 1.0, bitwise symmetric.
 *   Status: 1 when n < max(min_obs, K + 1); otherwise 2 (singular) when a column is constant
 *     on U (M_jj <= 1e-20 * sum_U x_j^2) or the smallest eigenvalue of R is <= 1e-10 (or the
 *     eigensolver has not converged in 30 sweeps); otherwise 0.  The eigenvalues of R are
 *     computed for both methods.
 *   Transform T [D][K][K], f_j = sum_k z_k T[k][j]:
 *     symmetric: R = V L V^T (cyclic two-sided Jacobi, round-robin pairing, a pair skipped
 *       when |a_pq| <= 2^-52 sqrt(|a_pp a_qq|), stop after the first sweep without a
 *       rotation), T = V L^-1/2 V^T, summed in a fixed k order, entries i <= j computed and
 *       mirrored: bitwise symmetric;
 *     Gram-Schmidt: R = L L^T by an unpivoted f64 Cholesky, T = L^-T: upper triangular with
 *       exact zeros below the diagonal; f_1 = z_1, f_K = the standardised OLS residual of x_K
 *       on an intercept and the rows before it.
 *     Either way the K output columns have, on U, mean 0, sample variance 1 (ddof = 1) and
 *     zero mutual sample covariance.
 *   Diagnostics per day: eig [D][K] = the eigenvalues of R ascending; keep [D][K] = (R T)_jj
 *     = corr_U(f_j, x_j) (symmetric: sum_k V_jk^2 sqrt(l_k); Gram-Schmidt: L_jj).  On a day
 *     with status != 0, T, eig and keep are NaN.
 *   Output [K][D][S] (val, state): ABSENT stays ABSENT, NULL stays NULL, a VALUE inside U is
 *     VALUE, a VALUE outside U (a finite value whose stock lacks another factor, a NaN / inf)
 *     becomes NULL, as does every VALUE of a day with status != 0; the value of a non-VALUE
 *     entry is 0.0.
 *   The result is bit-identical from run to run (fixed summation orders, a fixed rotation
 *   order, no floating-point atomics).
 * workspace: mff_xs_orth_workspace_bytes(K, D, S) bytes of device scratch shared by the calls
 *   of one orthogonalisation: per-day scalars f64 [D][2K + 1] = (n, the K means, the K raw
 *   sums of squares), T'[k][j] = T[k][j] / sigma_k f64 [D][K][K], the usable-set plane u8
 *   [D][S], each part 256-B aligned, in that order.
 * sums: the usable-set plane (into workspace) and sums f64 [nsplit][D][2K + 1] = (n, sum_U x_j,
 *   sum_U x_j^2), one plane per run of the stocks (nsplit runs of whole 32-stock tiles).
 * gram: adds the R planes of sums [R][D][2K + 1] (shards x runs) in plane order into the
 *   per-day scalars (workspace), then the local centred Gram planes
 *   gram f64 [nsplit][D][K][K], one workgroup per (day, run).
 * solve: adds the P planes [P][D][K][K] in plane order and applies the definition; leaves T'
 *   in the workspace.  Reads the per-day scalars (n, means, raw sums of squares) that
 *   mff_xs_orth_gram left in the workspace.
 * The four calls of one orthogonalisation share one workspace (same K, D, S) and run in the
 *   order sums -> gram -> solve -> apply on one stream: sums writes the usable-set plane, gram
 *   the per-day scalars, solve T'; each later call reads what the earlier ones wrote.  The
 *   workspace needs no initialisation.
 * apply: out[j] = sum_k T'[k][j] c_k for the local stocks, and the output states.
 * Errors (negative, nothing launched, nothing written): K < 1, K > max_factors(), method not
 * 0 / 1, a negative size, min_obs < 0, R / P / nsplit < 1.  D == 0 or S == 0 is a success
 * (empty result; n = 0, status 1, NaN diagnostics).
 */
int mff_xs_orth_max_factors(void); /* 64: the full 64-row block is exposures */
size_t mff_xs_orth_workspace_bytes(int K, int D, int S);
int mff_xs_orth_sums(const double* x_val, const uint8_t* x_state, int K, int D, int S, int nsplit,
                     double* sums, void* workspace, void* stream);
int mff_xs_orth_gram(const double* x_val, int K, int D, int S, const double* sums_all, int R,
                     int nsplit, double* gram, void* workspace, void* stream);
int mff_xs_orth_solve(const double* gram_all, int P, int K, int D, int method, int min_obs,
                      double* transform, double* eig, double* keep, int32_t* n, int32_t* status,
                      void* workspace, void* stream);
int mff_xs_orth_apply(const double* x_val, const uint8_t* x_state, int K, int D, int S,
                      const int32_t* status, double* out_val, uint8_t* out_state, void* workspace,
                      void* stream);

/*
 * Composite factor: K factors' exposures combined into one signal with equal, rolling-IC,
 * rolling-ICIR or max-ICIR weights.  No reference function (Factor.py never combines
 * factors); this is the build's definition, restated in numpy by
 * tests/xs_combine_ref.py.
 *   Inputs: x [K][D][S] (val f64, state u8), 1 <= K <= 64; y [Ky][D][S] (val, state), the
 *   forward return: Ky = 1 pairs every factor with row 0 (Pearson IC), Ky = K pairs row k with
 *   row k (rank IC: x and y are then the average ranks over the pair set, mff_ic_pairs +
 *   mff_xs_rank per factor), Ky = 0 with y NULL = no y (the pair moments are 0, every IC NaN).
 *   Below h = future_days >= 1, W = window >= 1, m = min_periods >= 1.
 * moments: one pass over x and y -> partial f64 [K][D][9] = (n_x, mean_x, M2_x, n_p, mean_xp,
 *   mean_yp, Cxx, Cyy, Cxy) of the local S stocks.
 *     z set (the first three): x VALUE and finite (the set of mff_xs_moments).
 *     pair set (the last six): x VALUE and not NaN, y VALUE (the rule of mff_ic_pairs); a
 *       non-finite x or y inside the pair set makes the date's IC NaN, as there.
 *     Centred moments, never raw power sums: per 512-stock chunk the values are shifted by the
 *       chunk's first included value (that value's finite part for the pairs), the mean taken,
 *       then the centred squares and products (the two passes of mff_ic_moments on registers);
 *       chunks are merged in stock order by the pairwise update n = na + nb, dl = mean_b - mean_a,
 *       M2 += M2_b + dl^2 na nb / n, mean += dl nb / n.  A constant set gives M2 = 0 exactly.
 *     Each stock tile of y is read once for all K factors of a day (Ky = 1); neither x nor y is
 *     read more than once.
 * finalize: merges the R shards' partials [R][K][D][9] by the same update in rank order and
 *   writes zmom f64 [K][D][3] = (n, mean, std with ddof = 1): std NaN when n < 2, a std of 0 is
 *   kept as 0 and means "z undefined"; ic f64 [K][D] = Cxy / sqrt(Cxx Cyy), NaN when
 *   n_p < max(2, min_obs) or the denominator is 0 (the rule of mff_ic_finalize);
 *   n_pairs int32 [K][D] = n_p, always written and exact.
 * weights: ic [K][D] -> weights f64 [D][K], count int32 [D][K], status int32 [D] (0 ok, 1 too
 *   little history, 2 singular or degenerate).  For date index d the window is
 *   E(d) = {e : max(0, d - h - W + 1) <= e <= d - h}, empty when d < h: only ICs whose return
 *   horizon has closed by d are used (no look-ahead).
 *     equal (0): w_raw[k] = 1; count 0, status 0; ic may be NULL.
 *     ic (1): c_k = the finite ic[k][e] in E(d); w_raw[k] = their mean when c_k >= m, else 0.
 *     icir (2): needs c_k >= max(m, 2) and a std (ddof = 1) finite and > 0: w_raw[k] = mean /
 *       std, else 0.  For ic and icir count[d][k] = c_k, and status 1 when no factor qualifies.
 *       Means and stds run in date order on values shifted by the window's first finite IC, so
 *       a constant IC series has std = 0 exactly.
 *     max_icir (3): L(d) = the dates of E(d) on which all K ICs are finite, c = |L| in every
 *       column of count.  Status 1 unless c >= max(m, 2) and, when shrink == 0, c >= K + 1.
 *       mu and Sigma (ddof = 1) over L; Sigma_s = (1 - shrink) Sigma + shrink diag(Sigma),
 *       0 <= shrink <= 1; w_raw = Sigma_s^-1 mu.  Pivot rule (that of mff_xs_orth_solve /
 *       mff_xs_reg_solve): a Sigma_ii that is not > 0 is status 2; otherwise Sigma_s is scaled
 *       to a unit diagonal, C_ij = (1 - shrink) Sigma_ij / sqrt(Sigma_ii Sigma_jj), factored by
 *       an unpivoted f64 Cholesky, and a pivot <= 1e-10 is status 2; C u = mu / sigma,
 *       w_raw = u / sigma.
 *     Then w = w_raw / sum_k |w_raw[k]|; a sum that is zero or not finite is status 2.  On
 *     status != 0 the weights row is NaN.  One wave per date.
 * apply: x, zmom, weights, status -> the composite [D][S] (val, state).
 *     z[k][d][s] = (x - mean) / std where x is VALUE and finite, n >= 2 and std > 0 (computed
 *       as (x - mean) * (1 / std)).
 *     P(d, s) = the k with z defined and weights[d][k] != 0.
 *     status[d] == 0 and |P| >= min_factors (1 <= min_factors <= K):
 *       val = sum_P w z / sum_P |w|, both sums in factor order, state VALUE: the weights are
 *       renormalised over the factors a stock actually has.
 *     Otherwise val = 0.0; state ABSENT when every x[k][d][s] is ABSENT, else NULL.
 *   The result is bit-identical from run to run (fixed summation orders: the lane tree of a
 *   chunk, chunk order, rank order, date order, factor order; no floating-point atomics).
 * Errors (negative, nothing launched, nothing written): K < 1, K > 64, a negative size, Ky not
 * 0 / 1 / K or not matching y, R < 1, min_obs < 0, method outside 0..3, future_days / window /
 * min_periods < 1, shrink outside [0, 1] (NaN included), min_factors outside [1, K].  D == 0 is
 * a success (nothing written); S == 0 is a success (moments: all-zero partials; apply: nothing
 * written).
 */
int mff_xs_comb_moments(const double* x_val, const uint8_t* x_state, int K, int D, int S,
                        const double* y_val, const uint8_t* y_state, int Ky, double* partial,
                        void* stream);
int mff_xs_comb_finalize(const double* partial_all /* [R][K][D][9] */, int R, int K, int D,
                         int min_obs, double* zmom, double* ic, int32_t* n_pairs, void* stream);
int mff_xs_comb_weights(const double* ic, int K, int D, int method, int future_days, int window,
                        int min_periods, double shrink, double* weights, int32_t* count,
                        int32_t* status, void* stream);
int mff_xs_comb_apply(const double* x_val, const uint8_t* x_state, int K, int D, int S,
                      const double* zmom, const double* weights, const int32_t* status,
                      int min_factors, double* out_val, uint8_t* out_state, void* stream);

/*
 * Factor IC / rank-IC test.  Replaces Factor.ic_test
 * (Factor.py:127-229).  Inputs are dense [D][S] (val, state) like stage 1's output rows.
 * mff_future_return: Factor.py:142-162 — per stock over its present days,
 *   fut = exp(sum of log(1 + pct) over the next N present days) - 1, NULL unless N such
 *   days exist with no null among them (rolling_sum min_samples=N, then shift(-N)).
 *   Any N >= 1 (Factor.py:149 takes any future_days).
 * mff_ic_pairs: the pair set of pl.corr (Factor.py:165-183): x VALUE and not NaN (the
 *   is_nan filter), y VALUE; writes [2][D][S] rows (x, y) with state VALUE on pairs, else
 *   ABSENT.  Feed them to mff_ic_moments (IC) or first to mff_xs_rank (rank IC).
 * mff_ic_moments: per day, the local pair moments partial [D][6] = (n, mean_x, mean_y,
 *   Cxx, Cyy, Cxy) over pairs whose two states are VALUE.
 * mff_ic_finalize: combine the R stock shards' partials [R][D][6] (all-gathered) and
 *   write ic [D] = Cxy / sqrt(Cxx Cyy), NaN when n < 2 or the denominator is 0.
 */
int mff_future_return(const double* pct, const uint8_t* state, int D, int S, int N,
                      double* out_val, uint8_t* out_state, void* stream);
int mff_ic_pairs(const double* x_val, const uint8_t* x_state, const double* y_val,
                 const uint8_t* y_state, int D, int S, double* pair_val, uint8_t* pair_state,
                 void* stream);
int mff_ic_moments(const double* pair_val, const uint8_t* pair_state, int D, int S,
                   double* partial, void* stream);
int mff_ic_finalize(const double* partial_all, int R, int D, double* ic, void* stream);

/*
 * Factor group back-test.  Replaces Factor.group_test
 * (Factor.py:231-350).  Exposure / pct_change / weight rows are dense [D][S] (val, state).
 * mff_bt_qcut: per date, G quantile groups of the non-null non-NaN exposures of all
 *   ranks (val_all/state_all [R][D][S_all], each rank's columns padded with ABSENT):
 *   pandas-qcut edges (linear quantiles, duplicate edges dropped) -> group int8 [D][S_loc]
 *   in 0..G-1, -1 = null.  workspace: mff_bt_qcut_workspace_bytes bytes.  G <= 63.
 * mff_bt_periods: per stock over the dates (period_of [D] int32, non-decreasing, every
 *   period 0..P-1 present): per period the return prod(1 + pct) - 1 over the exposure
 *   rows with non-null pct, and the group / weight of the previous period the stock held
 *   (shift(1).over('code')) -> p_ret f64, p_group int8 (-1 = null), p_weight f64 +
 *   p_weight_state u8, all [P][S].  weight / weight_state NULL = equal weights.
 * mff_bt_reduce: per (period, group) over local stocks -> partial [P][G][4] = (count,
 *   sum ret, sum w, sum w*ret).
 * mff_bt_finalize: sum the R ranks' partials [R][P][G][4] -> ret [P][G] = mean ret, or
 *   (weighted) sum w*ret / sum w (0 when sum w == 0); present [P][G] u8 = count > 0.
 */
size_t mff_bt_qcut_workspace_bytes(int D, int S_all, int R);
int mff_bt_qcut(const double* val, const uint8_t* state, int D, int S_loc, const double* val_all,
                const uint8_t* state_all, int R, int S_all, int G, int8_t* group, void* workspace,
                void* stream);
int mff_bt_periods(const uint8_t* x_state, const int8_t* group, const double* pct,
                   const uint8_t* pct_state, const double* weight, const uint8_t* weight_state,
                   const int32_t* period_of, int D, int S, int P, double* p_ret, int8_t* p_group,
                   double* p_weight, uint8_t* p_weight_state, void* stream);
int mff_bt_reduce(const double* p_ret, const int8_t* p_group, const double* p_weight,
                  const uint8_t* p_weight_state, int P, int S, int G, double* partial, void* stream);
int mff_bt_finalize(const double* partial_all, int R, int P, int G, int weighted, double* ret,
                    uint8_t* present, void* stream);

/*
 * Daily group portfolios: the drifting-weight value of the G quantile portfolios of K factors
 * per date, and the turnover of every rebalance.  The build's definition; it
 * extends Factor.group_test (Factor.py:231-350), which keeps one number per period.
 *
 * Inputs, dense like mff_bt_*: group int8 [K][D][S] from mff_bt_qcut (-1 = null, else 0..G-1),
 * x_state u8 [K][D][S]; pct (val, state) [D][S] and an optional weight (val, state) [D][S],
 * shared by the K factors; period_of int32 [D] on the device, non-decreasing, every period
 * 0..P-1 present.  1 <= G <= 63, K >= 1.
 *
 * Per factor k and stock s, exactly as mff_bt_periods walks:
 *   a date d is a row when x_state[k][d][s] != ABSENT; period p is held when it has a row; the
 *   signal of a held period is its last row's group and weight; prev(p) is the latest held
 *   period before p (the stock's own, possibly earlier than p - 1: shift(1).over('code')).
 *   m(p) = the group of prev(p)'s signal when p is held and prev(p) exists, else -1.
 *   u(p) = 1.0 without a weight plane; with one, the weight of prev(p)'s signal when that is
 *     VALUE, finite and > 0, else 0.0.  A member with u = 0 still counts as a member.  Stored
 *     as 0.0 where m(p) = -1.
 *   c(d), d in period p: 1.0 multiplied in date order by pct[d'] + 1.0 over the rows d' <= d of
 *     p whose pct state is VALUE; cend(p) = c on the last date of p (1.0 when p is not held).
 *   Bit for bit, m(p) is mff_bt_periods' p_group and cend(p) - 1.0 its p_ret.
 * Per (k, p, g), over the stocks with m(p) = g:
 *   n = their count, U = sum u; A(d) = sum u c(d) for every date d of p, A_end = A(last date).
 *   V(d) = A(d) / U when U > 0, else 1.0 (cash); V before the first date of a period is 1.0.
 *   ret[k][d][g] = V(d) / V(d-) - 1 (0 when U is not > 0); count[k][p][g] = n, the cell is
 *   present when n > 0.  A NaN, infinite or -1 pct is not special-cased: IEEE arithmetic carries
 *   it until the period ends.
 * Turnover, p >= 1:
 *   t_s = u_s(p) / U(p) when m_s(p) = g and U(p) > 0, else 0;
 *   b_s = u_s(p-1) cend_s(p-1) / A_end(p-1) when m_s(p-1) = g and U(p-1) > 0, else 0;
 *   traded[k][p][g] = sum_s |t_s - b_s|; traded[k][0][g] = 0.  Both sides of a trade count, in
 *   units of portfolio value: built from cash = 1, a complete swap = 2.
 *
 * mff_pf_signal: m int8, u f64, cend f64, all [K][P][S_loc].
 * mff_pf_sums: the daily pass over the local stocks -> a_partial f64 [K][D][G] = A and
 *   nu_partial f64 [K][P][G][2] = (n, U).  One workgroup per (period, factor) walks the stocks
 *   in tiles of 256; each stock-day is read once (x_state 1 byte per factor, pct and its state
 *   once per tile) and added to the LDS bin of its group; no loop over the groups.
 * mff_pf_finalize: sums the R shards' partials [R][K][D][G] and [R][K][P][G][2] in rank order
 *   -> ret f64 [K][D][G], count int32 [K][P][G], tot f64 [K][P][G][2] = (U, A_end).
 * mff_pf_traded: from the local m, u, cend and the merged tot -> partial f64 [K][P][G].
 * mff_pf_traded_finalize: sums the R shards' partials [R][K][P][G] in rank order -> traded.
 * Every output element is written.  No floating-point atomics: the summation order (stocks
 * j, j + J, ... of a tile per bin, tiles in order, the J bins in order, ranks in order) depends on
 * the shapes alone, so two runs are bit-identical.
 * Errors (negative, nothing launched, nothing written): K < 1 or > 65535, a negative size, P
 * outside [0, min(D, 65535)] or 0 with D > 0, G outside [1, 63], R < 1, weight without
 * weight_state, a NULL buffer.  D == 0 or S == 0 is a success with nothing launched and nothing written (the partials
 * of a shard without stocks are zeros the caller provides).
 */
int mff_pf_signal(const uint8_t* x_state, const int8_t* group, const double* pct,
                  const uint8_t* pct_state, const double* weight, const uint8_t* weight_state,
                  const int32_t* period_of, int K, int D, int S, int P, int8_t* m, double* u,
                  double* cend, void* stream);
int mff_pf_sums(const uint8_t* x_state, const double* pct, const uint8_t* pct_state,
                const int32_t* period_of, const int8_t* m, const double* u, int K, int D, int S,
                int P, int G, double* a_partial, double* nu_partial, void* stream);
int mff_pf_finalize(const double* a_all, const double* nu_all, const int32_t* period_of, int R,
                    int K, int D, int P, int G, double* ret, int32_t* count, double* tot,
                    void* stream);
int mff_pf_traded(const int8_t* m, const double* u, const double* cend, const double* tot, int K,
                  int P, int S, int G, double* partial, void* stream);
int mff_pf_traded_finalize(const double* partial_all, int R, int K, int P, int G, double* traded,
                           void* stream);

#ifdef __cplusplus
}
#endif
#endif /* MFF_H */
