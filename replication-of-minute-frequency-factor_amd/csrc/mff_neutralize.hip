// mff_neutralize.hip — per-day cross-sectional preprocessing of factor exposures:
// MAD winsorisation, industry / size neutralisation, standardisation.
//
// Build definition (no reference function; include/mff.h states it in full).  Over the
// usable stocks U of one (factor, day) column -- state VALUE, x finite, an industry when
// industries are given, a finite VALUE size when a size covariate is given:
//   1. med = median(x), mad = median(|x - med|) (numpy.median: mean of the two middle
//      order statistics); mad > 0: x clipped to med -+ winsor_k * 1.4826 * mad
//   2. e = OLS residual of x on industry dummies + size, by within-industry demeaning
//      (Frisch-Waugh): x~ = x - mean_g(x), z~ = z - mean_g(z), beta = S(x~ z~) / S(z~ z~)
//   3. e <- (e - mean(e)) / sd(e), ddof = 1
// n - k < 1 (k = non-empty industries + 1 with a size covariate) -> NULL.
//
// k_xs_neutralize: one workgroup per (row, day) -- 256 threads up to 1,024 stocks, 1,024
// threads above with at most 5 (8 beyond 5,120 stocks) values per thread, the shape of
// k_xs_rank_day -- the column in registers, element t + T i of thread t, read once and
// written once (the day's side inputs, shared by its rows, are re-read from the cache
// where a copy in registers would cost occupancy).
//  * Median / MAD: exact radix select on the total-order keys (ord64, -0 as +0), 12-bit
//    digits from the top through a 4,096-bin LDS histogram (the first pass takes sign and
//    exponent whole, the second the top of the mantissa: two passes for most columns).
//    Both middle order statistics are found in the same passes: while they fall into one
//    bin the prefix grows; once they part, the lower one is the largest key of its bin and
//    the upper one the smallest key of the next non-empty bin, so one min / max reduction
//    ends the search (as it does when the bin holds only the targets).
//  * Industry sums are bit-identical from run to run: k_nz_order builds once per day (all
//    rows of a day share the industries) a counting-sort position of every stock by
//    industry (stock order kept inside an industry) and the size covariate in that order.
//    The column is scattered to LDS at those positions, each industry is then a contiguous
//    run; every wave takes its share of the positions into registers and sums its part of
//    each run per lane in position order + a fixed DPP butterfly, and the parts of a run
//    that spans waves add up in wave order.  Integer LDS atomics only (the histogram); no
//    floating-point atomics anywhere.
#include "../../include/mff.h"
#include "mff_internal.h"
#include "mff_wave.h"

namespace mff {

constexpr int NZ_THREADS = 256;                      // k_nz_order; k_xs_neutralize up to 1,024 stocks
constexpr int NZ_BIG = 1024;                         // k_xs_neutralize's threads above
constexpr int NZ_MAX_WAVES = NZ_BIG / 64;
constexpr int NZ_MAX_S = 8192;                       // stocks per day
constexpr int NZ_MAX_G = 256;                        // industries
constexpr int NZ_NONE = NZ_MAX_G;                    // bucket of the stocks without one (sorted last)
constexpr int NZ_CHUNKS = 64;                        // k_nz_order: stock chunks counted apart

// per-day workspace: size covariate in industry order f64 [S], positions u16 [S],
// run starts u16 [NZ_MAX_G + 2]; every part 256-B aligned
__host__ __device__ inline size_t nz_align(size_t b) { return (b + 255) & ~(size_t)255; }
__host__ __device__ inline size_t nz_pos_off(int S) { return nz_align((size_t)S * 8); }
__host__ __device__ inline size_t nz_start_off(int S) { return nz_pos_off(S) + nz_align((size_t)S * 2); }
__host__ __device__ inline size_t nz_day_bytes(int S) { return nz_start_off(S) + nz_align((NZ_MAX_G + 2) * 2); }

// exclusive scan of one u32 per thread over the T-thread block; *total = the sum.  Does
// not end synced: the callers pass a barrier before wsum is written again.
template <int T>
__device__ __forceinline__ uint32_t nz_scan(uint32_t x, uint32_t* wsum, uint32_t* total) {
  const int lane = lane_id(), wave = (int)threadIdx.x >> 6;
  const uint32_t incl = wscan_dpp(x);
  if (lane == 63) wsum[wave] = incl;
  __syncthreads();
  uint32_t off = incl - x, tot = 0u;
#pragma unroll
  for (int w = 0; w < T / 64; ++w) {
    off += w < wave ? wsum[w] : 0u;
    tot += wsum[w];
  }
  *total = tot;
  return off;
}

// Per day: sorted position of every stock by industry bucket (ids outside [0, G) -> the
// last bucket), stock order kept inside a bucket -- a counting sort with per-chunk counts,
// no atomics, so the order never depends on timing.
__global__ __launch_bounds__(NZ_THREADS) void k_nz_order(const int32_t* group, int G, const double* size, int S,
                                                         char* ws) {
  __shared__ uint16_t gl[NZ_MAX_S];                      // bucket of stock s, then its position
  __shared__ uint16_t tab[(NZ_MAX_G + 1) * NZ_CHUNKS];   // [bucket][chunk] count, then offset in the bucket
  __shared__ uint16_t tot[NZ_MAX_G + 1];
  __shared__ uint16_t start[NZ_MAX_G + 2];
  __shared__ uint32_t wsum[NZ_THREADS / 64];
  const int tid = (int)threadIdx.x;
  const size_t day = blockIdx.x;
  const int32_t* g = group + day * S;
  char* wd = ws + day * nz_day_bytes(S);
  double* zs = reinterpret_cast<double*>(wd);
  uint16_t* pos = reinterpret_cast<uint16_t*>(wd + nz_pos_off(S));
  uint16_t* gstart = reinterpret_cast<uint16_t*>(wd + nz_start_off(S));
  for (int s = tid; s < S; s += NZ_THREADS) {
    const int32_t gi = g[s];
    gl[s] = (uint16_t)((gi >= 0 && gi < G) ? gi : NZ_NONE);
  }
  for (int i = tid; i < (NZ_MAX_G + 1) * NZ_CHUNKS; i += NZ_THREADS) tab[i] = 0;
  __syncthreads();
  const int chunk = (S + NZ_CHUNKS - 1) / NZ_CHUNKS;
  const int c0 = min(S, tid * chunk), c1 = min(S, c0 + chunk);
  if (tid < NZ_CHUNKS)
    for (int s = c0; s < c1; ++s) ++tab[(int)gl[s] * NZ_CHUNKS + tid];  // column tid is this thread's own
  __syncthreads();
  for (int b = tid; b <= NZ_MAX_G; b += NZ_THREADS) {
    uint32_t run = 0u;
    for (int c = 0; c < NZ_CHUNKS; ++c) {
      const uint32_t n = tab[b * NZ_CHUNKS + c];
      tab[b * NZ_CHUNKS + c] = (uint16_t)run;
      run += n;
    }
    tot[b] = (uint16_t)run;
  }
  __syncthreads();
  {
    uint32_t all;
    const uint32_t off = nz_scan<NZ_THREADS>(tot[tid], wsum, &all);  // buckets 0 .. 255
    start[tid] = (uint16_t)off;
    if (tid == 0) {
      start[NZ_MAX_G] = (uint16_t)all;  // the stocks without an industry
      start[NZ_MAX_G + 1] = (uint16_t)S;
    }
  }
  __syncthreads();
  if (tid < NZ_CHUNKS)
    for (int s = c0; s < c1; ++s) {
      const int b = gl[s];
      gl[s] = (uint16_t)(start[b] + tab[b * NZ_CHUNKS + tid]++);
    }
  __syncthreads();
  for (int s = tid; s < S; s += NZ_THREADS) {
    const uint16_t p = gl[s];  // < S: a permutation of 0 .. S-1
    pos[s] = p;
    if (size) zs[p] = size[day * S + s];
  }
  for (int b = tid; b < NZ_MAX_G + 2; b += NZ_THREADS) gstart[b] = start[b];
}

// sum / min / max over groups of NW (4 or 16) neighbouring lanes by the in-row DPP butterfly
// of wsum(): every lane of a group ends with the same bits
template <int NW>
__device__ __forceinline__ double nz_rowsum(double x) {
  x += dpp_in_row<0xB1>(x);
  x += dpp_in_row<0x4E>(x);
  if constexpr (NW == 16) {
    x += dpp_in_row<0x141>(x);
    x += dpp_in_row<0x140>(x);
  }
  return x;
}

// block sums of N doubles per thread, every thread gets the totals (fixed order: DPP
// butterfly inside the wave, then the wave totals, one per lane, by the same butterfly:
// a thread reads one total, not all of them -- 16 waves x N doubles in flight cost more
// registers than the column itself); ends synced
template <int T, int N>
__device__ __forceinline__ void nz_bsum(double (&v)[N], double* red) {
  constexpr int NW = T / 64;
  static_assert(NW == 4 || NW == 16, "wave totals in a quad or a DPP row");
  const int wave = (int)threadIdx.x >> 6, lane = lane_id();
#pragma unroll
  for (int k = 0; k < N; ++k) v[k] = wsum(v[k]);
  if (lane == 0) {
#pragma unroll
    for (int k = 0; k < N; ++k) red[wave * N + k] = v[k];
  }
  __syncthreads();
#pragma unroll
  for (int k = 0; k < N; ++k) v[k] = nz_rowsum<NW>(red[(lane & (NW - 1)) * N + k]);
  __syncthreads();
}

// block min of mn and max of mx (u64 keys); ends synced
template <int T>
__device__ __forceinline__ void nz_bminmax(uint64_t& mn, uint64_t& mx, uint64_t* red) {
  constexpr int NW = T / 64;
  const int wave = (int)threadIdx.x >> 6, lane = lane_id();
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const uint64_t a = (uint64_t)__shfl_xor((long long)mn, o, 64);
    const uint64_t b = (uint64_t)__shfl_xor((long long)mx, o, 64);
    mn = a < mn ? a : mn;
    mx = b > mx ? b : mx;
  }
  if (lane == 0) {
    red[wave] = mn;
    red[NW + wave] = mx;
  }
  __syncthreads();
  mn = red[lane & (NW - 1)];  // one wave's result per lane, then over NW neighbouring lanes
  mx = red[NW + (lane & (NW - 1))];
#pragma unroll
  for (int o = NW / 2; o > 0; o >>= 1) {
    const uint64_t a = (uint64_t)__shfl_xor((long long)mn, o, 64);
    const uint64_t b = (uint64_t)__shfl_xor((long long)mx, o, 64);
    mn = a < mn ? a : mn;
    mx = b > mx ? b : mx;
  }
  __syncthreads();
}

constexpr int NZ_DB = 12;                         // digit bits of the radix select
constexpr int NZ_BINS = 1 << NZ_DB;               // 4096 bins: sign + exponent in the first pass

struct NzShared {
  double red[NZ_MAX_WAVES * 3];
  uint64_t red64[NZ_MAX_WAVES * 2];
  uint32_t wsum[NZ_MAX_WAVES];
  uint32_t sel[6];  // bin, rank inside it, its count: of the lower, then the upper middle key
};

// The two middle order statistics (0-based ranks (n - 1) / 2 and n / 2) of the keys
// key(i) of the elements in `use` (n of them over the block, n >= 1): lo <= hi.
// hist: NZ_BINS LDS counters (any content on entry).
template <int T, int PER, typename KeyF>
__device__ __forceinline__ void nz_middle(KeyF key, uint32_t use, uint32_t n, uint32_t* hist, NzShared& sh,
                                          uint64_t& lo, uint64_t& hi) {
  constexpr int NZ_BPT = NZ_BINS / T;  // bins per thread in the scan
  const int tid = (int)threadIdx.x;
  uint64_t kk[PER];
#pragma unroll
  for (int i = 0; i < PER; ++i) kk[i] = key(i);
  uint32_t act = use;  // the elements whose key has the prefix found so far
  uint32_t ka = (n - 1u) >> 1, kb = n >> 1, cnt = n;  // ranks among them; how many
  uint32_t m_min = 0u, m_max = 0u;
  bool split = false;
#pragma unroll
  for (int q = 0; q < NZ_BPT; ++q) hist[tid + q * T] = 0u;
  __syncthreads();
#pragma unroll 1
  for (int top = 64; top > 0;) {
    if (ka == 0u && kb == cnt - 1u) break;  // only the targets are left (block-uniform)
    const int low = top > NZ_DB ? top - NZ_DB : 0;
    const uint32_t mask = (1u << (top - low)) - 1u;
#pragma unroll
    for (int i = 0; i < PER; ++i)
      if ((act >> i) & 1u) atomicAdd(&hist[(uint32_t)(kk[i] >> low) & mask], 1u);
    __syncthreads();
    // thread t scans bins NZ_BPT t .. NZ_BPT t + NZ_BPT - 1 (and clears them: they are read
    // by this thread only, and the next pass adds after two more barriers)
    uint32_t h[NZ_BPT], c = 0u;
#pragma unroll
    for (int q = 0; q < NZ_BPT; ++q) {
      h[q] = hist[tid * NZ_BPT + q];
      hist[tid * NZ_BPT + q] = 0u;
      c += h[q];
    }
    uint32_t all;
    uint32_t run = nz_scan<T>(c, sh.wsum, &all);
#pragma unroll
    for (int q = 0; q < NZ_BPT; ++q) {
      const uint32_t nxt = run + h[q];
      if (ka >= run && ka < nxt) {
        sh.sel[0] = (uint32_t)(tid * NZ_BPT + q);
        sh.sel[1] = ka - run;
        sh.sel[2] = h[q];
      }
      if (kb >= run && kb < nxt) {
        sh.sel[3] = (uint32_t)(tid * NZ_BPT + q);
        sh.sel[4] = kb - run;
        sh.sel[5] = h[q];
      }
      run = nxt;
    }
    __syncthreads();
    const uint32_t ba = sh.sel[0], bb = sh.sel[3];
    uint32_t ma = 0u, mb = 0u;
#pragma unroll
    for (int i = 0; i < PER; ++i) {
      const uint32_t d = (uint32_t)(kk[i] >> low) & mask;
      ma |= (uint32_t)(d == ba) << i;
      mb |= (uint32_t)(d == bb) << i;
    }
    ma &= act;
    mb &= act;
    if (ba != bb) {  // the lower key is the largest of its bin, the upper the smallest of its own
      split = true;
      m_max = ma;
      m_min = mb;
      break;
    }
    act = ma;
    ka = sh.sel[1];
    kb = sh.sel[4];
    cnt = sh.sel[2];
    top = low;
    // sel is written again after the next pass's first barrier: every thread has read it
  }
  if (!split) m_min = m_max = act;  // one or two keys, or every key equal
  uint64_t mn = ~0ull, mx = 0ull;
#pragma unroll
  for (int i = 0; i < PER; ++i) {
    if ((m_min >> i) & 1u) mn = kk[i] < mn ? kk[i] : mn;
    if ((m_max >> i) & 1u) mx = kk[i] > mx ? kk[i] : mx;
  }
  nz_bminmax<T>(mn, mx, sh.red64);
  lo = split ? mx : mn;
  hi = split ? mn : mx;
}

__device__ __forceinline__ double nz_median(uint64_t lo, uint64_t hi) {
  const double a = unord64(lo), b = unord64(hi);
  return lo == hi ? a : (a + b) * 0.5;
}

template <int T, int PER>
__global__ __launch_bounds__(T) void k_xs_neutralize(const double* val, const uint8_t* state, int rows,
                                                              int D, int S, const int32_t* group, int G,
                                                              const double* size, const uint8_t* size_state,
                                                              double winsor_k, int standardize, double* out_val,
                                                              uint8_t* out_state, const char* ws) {
  // one buffer, two lives: the select's histogram, then the column in industry order
  constexpr int NW = T / 64;
  constexpr int BUF = PER * T * 8 > NZ_BINS * 4 ? PER * T * 8 : NZ_BINS * 4;
  __shared__ __attribute__((aligned(16))) unsigned char buf[BUF];
  // count, sum x, sum z: of an industry inside one wave's positions; of the run a wave
  // shares with the waves before it (head) / after it (tail)
  __shared__ double full[NZ_MAX_G * 3], head[NW * 3], tail[NW * 3];
  __shared__ double xbar[NZ_MAX_G], zbar[NZ_MAX_G];  // industry means
  __shared__ uint16_t gst[NZ_MAX_G + 2];             // the day's run starts
  __shared__ NzShared sh;
  double* xs = reinterpret_cast<double*>(buf);
  uint32_t* hist = reinterpret_cast<uint32_t*>(buf);
  const int tid = (int)threadIdx.x, lane = lane_id();
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  // the rows of one day run side by side: they share the day's industries, sizes and order
  const int day = (int)(blockIdx.x / (unsigned)rows), row = (int)(blockIdx.x - (unsigned)day * (unsigned)rows);
  const size_t base = ((size_t)row * D + day) * S, dbase = (size_t)day * S;
  const double* v = val + base;
  const uint8_t* st = state + base;
  const bool has_g = group != nullptr, has_z = size != nullptr;
  // the day's side inputs through wave-uniform pointers (scalar base + the thread's 32-bit offset)
  const int32_t* gd = has_g ? group + dbase : nullptr;
  const double* zd = has_z ? size + dbase : nullptr;
  const uint8_t* zsd = has_z ? size_state + dbase : nullptr;
  double x[PER];
  uint32_t stv = 0u, stn = 0u, fin = 0u, use = 0u;  // state VALUE; state NULL; VALUE and finite; in U
#pragma unroll
  for (int i = 0; i < PER; ++i) {
    const int s = tid + i * T;
    const bool in = s < S;
    x[i] = in ? v[s] : 0.0;
    const uint8_t sx = in ? st[s] : (uint8_t)MFF_STATE_ABSENT;
    const bool f = sx == MFF_STATE_VALUE && __builtin_isfinite(x[i]);
    bool ok = f;
    if (has_g) {
      const int32_t gi = in ? gd[s] : -1;
      ok = ok && gi >= 0 && gi < G;
    }
    if (has_z) {  // only whether it is usable: the value is read again where it is needed
      const double zz = in ? zd[s] : 0.0;
      const uint8_t sz = in ? zsd[s] : (uint8_t)MFF_STATE_ABSENT;
      ok = ok && sz == MFF_STATE_VALUE && __builtin_isfinite(zz);
    }
    stv |= (uint32_t)(sx == MFF_STATE_VALUE) << i;
    stn |= (uint32_t)(sx == MFF_STATE_NULL) << i;
    fin |= (uint32_t)f << i;
    use |= (uint32_t)ok << i;
  }
  double n;
  {
    double c[1] = {(double)__builtin_popcount(use)};
    nz_bsum<T>(c, sh.red);
    n = c[0];
  }
  // 1. winsorise
  if (winsor_k > 0.0 && n > 0.0) {
    uint64_t lo, hi;
    nz_middle<T, PER>([&](int i) { return ord64(x[i]); }, use, (uint32_t)n, hist, sh, lo, hi);
    const double med = nz_median(lo, hi);
    nz_middle<T, PER>([&](int i) { return ord64(fabs(x[i] - med)); }, use, (uint32_t)n, hist, sh, lo, hi);
    const double mad = nz_median(lo, hi);
    if (mad > 0.0) {
      const double w = (winsor_k * 1.4826) * mad;
      const double cl = med - w, ch = med + w;
#pragma unroll
      for (int i = 0; i < PER; ++i)
        if ((use >> i) & 1u) x[i] = fmin(fmax(x[i], cl), ch);
    }
  }
  // 2. neutralise: x[i] <- x~, z[i] <- z~, then the slope over all of U.  The size
  // covariate of the usable stocks comes into registers only now (the selects above need
  // the registers; the day's sizes are shared by all rows, so this read hits the cache).
  double sxz, szz, k;  // S(x~ z~), S(z~ z~), regressors
  double z[PER];
  if (!has_g) {
#pragma unroll
    for (int i = 0; i < PER; ++i) z[i] = (has_z && ((use >> i) & 1u)) ? zd[tid + i * T] : 0.0;
    double a[2] = {0.0, 0.0};
#pragma unroll
    for (int i = 0; i < PER; ++i) {
      if ((use >> i) & 1u) {
        a[0] += x[i];
        a[1] += z[i];
      }
    }
    nz_bsum<T>(a, sh.red);
    const double xm = n > 0.0 ? a[0] / n : 0.0, zm = n > 0.0 ? a[1] / n : 0.0;
    double b[2] = {0.0, 0.0};
#pragma unroll
    for (int i = 0; i < PER; ++i) {
      if ((use >> i) & 1u) {
        x[i] -= xm;
        z[i] -= zm;
        b[0] += x[i] * z[i];
        b[1] += z[i] * z[i];
      }
    }
    nz_bsum<T>(b, sh.red);
    sxz = b[0];
    szz = b[1];
    k = (n > 0.0 ? 1.0 : 0.0) + (has_z ? 1.0 : 0.0);
  } else {
    const char* wd = ws + (size_t)day * nz_day_bytes(S);
    const double* zs = reinterpret_cast<const double*>(wd);
    const uint16_t* pos = reinterpret_cast<const uint16_t*>(wd + nz_pos_off(S));
    const uint16_t* gstart = reinterpret_cast<const uint16_t*>(wd + nz_start_off(S));
    const double nanv = qnan();
#pragma unroll
    for (int i = 0; i < PER; ++i) {
      const int s = tid + i * T;
      if (s < S) xs[pos[s]] = ((use >> i) & 1u) ? x[i] : nanv;  // pos[s] < S <= PER * T
    }
    // Wave w owns the sorted positions [w Q, (w + 1) Q), Q = 64 PER, lane-strided in
    // registers (the size covariate comes in that order from the workspace, coalesced,
    // every load in flight at once).  An industry is a run of positions: its sums over the
    // wave's part are per-lane sums in position order + the wave butterfly, and the parts
    // of a run that spans waves add up in wave order -- one fixed order for every sum.
    constexpr int Q = 64 * PER;
    const int c0 = wave * Q, c1 = min(S, c0 + Q);
    for (int i = tid; i < NZ_MAX_G + 2; i += T) gst[i] = gstart[i];
    double zv[PER];
#pragma unroll
    for (int kq = 0; kq < PER; ++kq) {
      const int j = c0 + lane + 64 * kq;
      zv[kq] = has_z ? zs[min(j, S - 1)] : 0.0;
    }
    __syncthreads();
    double xv[PER];
#pragma unroll
    for (int kq = 0; kq < PER; ++kq) {
      const int j = c0 + lane + 64 * kq;
      xv[kq] = j < c1 ? xs[j] : nanv;
    }
    // the industries whose run meets this wave's positions: g_lo and on, while they start below c1
    int g_lo = G;
#pragma unroll
    for (int m = 3; m >= 0; --m) {
      const int g = lane + 64 * m;
      const uint64_t bm = __ballot(g < G && (int)gst[g + 1] > c0);
      if (bm) g_lo = 64 * m + (int)__builtin_ctzll(bm);
    }
#pragma unroll 1
    for (int g = g_lo; g < G; ++g) {
      const int r0 = __builtin_amdgcn_readfirstlane((int)gst[g]), r1 = __builtin_amdgcn_readfirstlane((int)gst[g + 1]);
      if (r0 >= c1) break;
      if (r0 == r1) continue;
      const int a = max(r0, c0), b = min(r1, c1);
      uint32_t c = 0u;
      double sx = 0.0, sz = 0.0;
#pragma unroll
      for (int kq = 0; kq < PER; ++kq) {
        const int blk = c0 + 64 * kq;
        if (blk < b && blk + 64 > a) {  // wave-uniform
          const int j = blk + lane;
          const bool ok = j >= a && j < b && xv[kq] == xv[kq];
          c += ok ? 1u : 0u;
          sx += ok ? xv[kq] : 0.0;
          sz += ok ? zv[kq] : 0.0;
        }
      }
      c = wsum_u32(c);
      sx = wsum(sx);
      sz = wsum(sz);
      if (lane == 0) {
        double* pp = (r0 >= c0 && r1 <= c1) ? full + g * 3 : r0 < c0 ? head + wave * 3 : tail + wave * 3;
        pp[0] = (double)c;
        pp[1] = sx;
        pp[2] = sz;
      }
    }
    __syncthreads();
    double ne = 0.0;  // this thread's industry has a member in U
    if (tid < G) {
      const int r0 = gst[tid], r1 = gst[tid + 1];
      double c = 0.0, sx = 0.0, sz = 0.0;
      if (r0 < r1) {
        const int w0 = r0 / Q, w1 = (r1 - 1) / Q;  // < NW: r1 <= S <= NW Q
        const double* pp = w0 == w1 ? full + tid * 3 : tail + w0 * 3;
        c = pp[0];
        sx = pp[1];
        sz = pp[2];
        for (int w = w0 + 1; w <= w1; ++w) {  // the run's parts in wave order
          c += head[w * 3 + 0];
          sx += head[w * 3 + 1];
          sz += head[w * 3 + 2];
        }
      }
      ne = c > 0.0 ? 1.0 : 0.0;
      xbar[tid] = c > 0.0 ? sx / c : 0.0;
      zbar[tid] = c > 0.0 ? sz / c : 0.0;
    }
    double acc[3] = {0.0, 0.0, ne};
    {
      double one[1] = {ne};
      nz_bsum<T>(one, sh.red);  // (its barriers publish xbar / zbar)
      acc[2] = one[0];
    }
#pragma unroll 1
    for (int g = g_lo; g < G; ++g) {
      const int r0 = __builtin_amdgcn_readfirstlane((int)gst[g]), r1 = __builtin_amdgcn_readfirstlane((int)gst[g + 1]);
      if (r0 >= c1) break;
      if (r0 == r1) continue;
      const int a = max(r0, c0), b = min(r1, c1);
      const double xm = xbar[g], zm = zbar[g];
#pragma unroll
      for (int kq = 0; kq < PER; ++kq) {
        const int blk = c0 + 64 * kq;
        if (blk < b && blk + 64 > a) {  // wave-uniform
          const int j = blk + lane;
          if (j >= a && j < b && xv[kq] == xv[kq]) {
            const double xt = xv[kq] - xm, zt = zv[kq] - zm;
            xv[kq] = xt;
            acc[0] += xt * zt;
            acc[1] += zt * zt;
          }
        }
      }
    }
#pragma unroll
    for (int kq = 0; kq < PER; ++kq) {
      const int j = c0 + lane + 64 * kq;
      if (j < c1) xs[j] = xv[kq];
    }
    {
      double two[2] = {acc[0], acc[1]};
      nz_bsum<T>(two, sh.red);  // (its first barrier closes the write-back of x~)
      sxz = two[0];
      szz = two[1];
    }
    k = acc[2] + (has_z ? 1.0 : 0.0);
#pragma unroll
    for (int i = 0; i < PER; ++i) {
      z[i] = 0.0;
      if ((use >> i) & 1u) {
        const int s = tid + i * T;
        x[i] = xs[pos[s]];
        if (has_z) z[i] = zd[s] - zbar[gd[s]];  // the id of a usable stock is in [0, G)
      }
    }
  }
  const double beta = (has_z && szz > 0.0) ? sxz / szz : 0.0;
  if (has_z) {
#pragma unroll
    for (int i = 0; i < PER; ++i)
      if ((use >> i) & 1u) x[i] -= beta * z[i];
  }
  // 3. standardise
  bool null_all = n - k < 1.0;
  double mean = 0.0, sd = 1.0;
  if (standardize) {
    null_all = null_all || n < 2.0;
    double a[1] = {0.0};
#pragma unroll
    for (int i = 0; i < PER; ++i)
      if ((use >> i) & 1u) a[0] += x[i];
    nz_bsum<T>(a, sh.red);
    mean = n > 0.0 ? a[0] / n : 0.0;
    double b[1] = {0.0};
#pragma unroll
    for (int i = 0; i < PER; ++i) {
      if ((use >> i) & 1u) {
        const double dl = x[i] - mean;
        b[0] += dl * dl;
      }
    }
    nz_bsum<T>(b, sh.red);
    sd = sqrt(b[0] / (n - 1.0));
  }
  double* ov = out_val + base;
  uint8_t* os = out_state + base;
#pragma unroll
  for (int i = 0; i < PER; ++i) {
    const int s = tid + i * T;
    if (s >= S) break;
    const bool u = (use >> i) & 1u, vl = (stv >> i) & 1u, f = (fin >> i) & 1u;
    double r = 0.0;
    uint8_t so;
    if (u) {
      so = null_all ? MFF_STATE_NULL : MFF_STATE_VALUE;
      if (!null_all) r = standardize ? (x[i] - mean) / sd : x[i];
    } else if (vl) {
      so = f ? MFF_STATE_NULL : MFF_STATE_VALUE;  // finite without industry / size: NULL; NaN, inf pass
      if (!f) r = x[i];
    } else {
      so = ((stn >> i) & 1u) ? MFF_STATE_NULL : MFF_STATE_ABSENT;
    }
    ov[s] = r;
    os[s] = so;
  }
}

}  // namespace mff

using namespace mff;

extern "C" {

int mff_xs_neutralize_max_stocks(void) { return NZ_MAX_S; }
int mff_xs_neutralize_max_groups(void) { return NZ_MAX_G; }

size_t mff_xs_neutralize_workspace_bytes(int D, int S) {
  if (D <= 0 || S <= 0) return 0;
  return (size_t)D * nz_day_bytes(S);
}

int mff_xs_neutralize(const double* val, const uint8_t* state, int rows, int D, int S, const int32_t* group,
                      int G, const double* size, const uint8_t* size_state, double winsor_k, int standardize,
                      double* out_val, uint8_t* out_state, void* workspace, void* stream) {
  clear_error();
  MFF_REQUIRE(rows >= 0 && D >= 0 && S >= 0, "mff_xs_neutralize: bad sizes rows=%d D=%d S=%d", rows, D, S);
  MFF_REQUIRE(S <= NZ_MAX_S, "mff_xs_neutralize: S=%d above the %d stocks one workgroup holds", S, NZ_MAX_S);
  MFF_REQUIRE(!group || (G >= 1 && G <= NZ_MAX_G), "mff_xs_neutralize: G=%d outside [1, %d]", G, NZ_MAX_G);
  MFF_REQUIRE(!size || size_state, "mff_xs_neutralize: size given without size_state");
  if (rows == 0 || D == 0 || S == 0) return 0;
  MFF_REQUIRE(val && state && out_val && out_state, "mff_xs_neutralize: NULL buffer");
  MFF_REQUIRE(!group || workspace, "mff_xs_neutralize: industries given without a workspace");
  const long long nseg = (long long)rows * D;
  MFF_REQUIRE(nseg < (1ll << 31), "mff_xs_neutralize: too many segments");
  hipStream_t st = as_stream(stream);
  if (group) {
    hipLaunchKernelGGL(k_nz_order, dim3((unsigned)D), dim3(NZ_THREADS), 0, st, group, G, size, S,
                       reinterpret_cast<char*>(workspace));
    MFF_LAUNCH_CHECK();
  }
  // 256 threads x 4 values up to 1,024 stocks; above, 1,024 threads x 5 (x 8 beyond 5,120)
  auto kern = S <= 4 * NZ_THREADS ? k_xs_neutralize<NZ_THREADS, 4>
            : S <= 5 * NZ_BIG ? k_xs_neutralize<NZ_BIG, 5> : k_xs_neutralize<NZ_BIG, NZ_MAX_S / NZ_BIG>;
  hipLaunchKernelGGL(kern, dim3((unsigned)nseg), dim3(S <= 4 * NZ_THREADS ? NZ_THREADS : NZ_BIG), 0, st, val, state, rows, D, S, group, G, size,
                     size_state, winsor_k, standardize, out_val, out_state,
                     reinterpret_cast<const char*>(workspace));
  MFF_LAUNCH_CHECK();
  return 0;
}

}  // extern "C"
