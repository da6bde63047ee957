// mff_pf.hip — daily group portfolios on the GPU: drifting-weight value of the G quantile
// portfolios of K factors per date, and the turnover of every rebalance (the definition is
// on the declarations in include/mff.h).
//
//   k_pf_signal_rows / k_pf_signal_shift   the walk of k_bt_periods (mff_bt.hip) in two steps:
//                 thread = (stock, period, factor) walks the dates of its period alone -- the
//                 growth cend, the last row's group and sanitised weight -- so the D dates are
//                 spread over P times as many threads; then thread = (stock, factor) moves
//                 group and weight one held period on (the membership m and the raw weight u).
//   k_pf_sums     the daily pass, one workgroup per (period, factor).  A stock's group is
//                 fixed inside a period, so the block walks the stocks in tiles of 256 (thread =
//                 stock, the running growth c in a register), stages u*c of 16 dates in LDS and
//                 adds the tile into LDS bins acc[date][j][group]: thread (date, j) takes the
//                 stocks j, j + J, ... of the tile in order -- every stock is visited once, the
//                 bin is picked by its group (no loop over the groups), and nothing is atomic.
//                 After the last tile the J partial bins of a (date, group) are summed in order.
//                 A period longer than the LDS bins hold is cut into chunks; a later chunk
//                 re-walks the period's earlier dates to rebuild c.
//   k_pf_rows     the same binning with periods as rows: (n, U) per (period, group), and the
//                 traded sums |t - b| (a stock adds to its new group and, when it moved, to its
//                 old one).
//   k_pf_finalize / k_pf_traded_finalize   the R shards' partials summed in rank order.
// The summation order is a function of the shapes alone: two runs are bit-identical.
#include "../../include/mff.h"
#include "mff_internal.h"

namespace mff {

constexpr int PF_MAXG = 63;
constexpr int PF_TS = 256;           // stocks of a tile = threads of a block
constexpr int PF_TD = 16;            // rows (dates or periods) of a tile
constexpr int PF_ACC = 2560;         // f64 bins of a block (20 KiB)
constexpr int PF_MAXK = 65535;       // gridDim.y / z: factors, and periods

// bins per (row, group): the largest power of two J <= 16 with nacc * PF_TD * J * G <= PF_ACC
static int pf_split(int G, int nacc) {
  int J = 16;
  while (J > 1 && nacc * PF_TD * J * G > PF_ACC) J >>= 1;
  return J;
}
// dates of a chunk of the daily pass: a multiple of PF_TD
static int pf_chunk(int G, int J) { return PF_ACC / (J * G) / PF_TD * PF_TD; }

// first index of period_of [D] (non-decreasing) holding a value >= p
__device__ __forceinline__ int pf_lower(const int32_t* period_of, int D, int p) {
  int lo = 0, hi = D;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (period_of[mid] < p) lo = mid + 1; else hi = mid;
  }
  return lo;
}

// one staged tile into the bins: acc[(row0 + i) * J + j][g] += val[i][t] over the stocks
// t = j, j + J, ... whose gid[i][t] = g in 0..G-1 (anything else: no bin).  Thread r = i * J + j
// owns its bins: no races.
__device__ __forceinline__ void pf_bin_add(const double* val, const int8_t* gid, double* acc, int row0, int J,
                                           int G) {
  const int r = threadIdx.x;
  if (r >= PF_TD * J) return;
  const int j = r % J, i = r / J;
  double* a = acc + ((size_t)(row0 + i) * J + j) * G;
  for (int t = j; t < PF_TS; t += J) {
    const int g = gid[i * PF_TS + t];
    if ((unsigned)g < (unsigned)G) a[g] += val[i * PF_TS + t];
  }
}

// the J bins of (row, g) in order
__device__ __forceinline__ double pf_bin_sum(const double* acc, int row, int g, int J, int G) {
  double x = 0.0;
  for (int j = 0; j < J; ++j) x += acc[((size_t)row * J + j) * G + g];
  return x;
}

// thread = (stock, period, factor): the period's own signal.  cend is final; m and u hold the
// period's last row's group (-1 null, -2: the period is not held) and sanitised weight until
// k_pf_signal_shift moves them one held period on.
__global__ __launch_bounds__(PF_TS) void k_pf_signal_rows(const uint8_t* x_state, const int8_t* group,
                                                           const double* pct, const uint8_t* pct_state,
                                                           const double* w, const uint8_t* w_state,
                                                           const int32_t* period_of, int D, int S, int P,
                                                           int8_t* m, double* u, double* cend) {
  const int s = blockIdx.x * PF_TS + threadIdx.x;
  if (s >= S) return;
  const int p = blockIdx.y;
  const size_t k = blockIdx.z;
  x_state += k * D * S;
  group += k * D * S;
  const int d0 = pf_lower(period_of, D, p), d1 = pf_lower(period_of, D, p + 1);
  bool held = false;
  double prod = 1.0, u_last = 1.0;
  int8_t g_last = -1;
  for (int d = d0; d < d1; ++d) {  // the walk of k_bt_periods inside one period
    const size_t i = (size_t)d * S + s;
    if (x_state[i] == MFF_STATE_ABSENT) continue;
    held = true;
    if (pct_state[i] == MFF_STATE_VALUE) prod *= pct[i] + 1.0;
    g_last = group[i];
    if (w) {
      const double x = w[i];
      u_last = (w_state[i] == MFF_STATE_VALUE && x > 0.0 && x < __builtin_inf()) ? x : 0.0;
    }
  }
  const size_t o = (k * P + p) * S + s;
  m[o] = held ? (g_last < 0 ? (int8_t)-1 : g_last) : (int8_t)-2;
  u[o] = u_last;
  cend[o] = held ? prod : 1.0;
}

// thread = (stock, factor) over the periods, in place: shift(1).over('code') on the held periods
__global__ __launch_bounds__(PF_TS) void k_pf_signal_shift(int S, int P, int8_t* m, double* u) {
  const int s = blockIdx.x * PF_TS + threadIdx.x;
  if (s >= S) return;
  const size_t k = blockIdx.y;
  int8_t g_prev = -1;
  double u_prev = 0.0;
  for (int p = 0; p < P; ++p) {
    const size_t o = (k * P + p) * S + s;
    const int8_t g_last = m[o];
    const double u_last = u[o];
    const bool held = g_last != -2;
    const int8_t mm = held ? g_prev : (int8_t)-1;
    m[o] = mm;
    u[o] = mm >= 0 ? u_prev : 0.0;
    if (held) { g_prev = g_last; u_prev = u_last; }
  }
}

__global__ __launch_bounds__(PF_TS) void k_pf_sums(const uint8_t* x_state, const double* pct,
                                                    const uint8_t* pct_state, const int32_t* period_of,
                                                    const int8_t* m, const double* u, int D, int S, int P, int G,
                                                    int J, int LC, double* A) {
  __shared__ double s_val[PF_TD * PF_TS];
  __shared__ int8_t s_gid[PF_TD * PF_TS];
  __shared__ double s_acc[PF_ACC];
  const int p = blockIdx.x, tid = threadIdx.x;
  const size_t k = blockIdx.y;
  x_state += k * D * S;
  m += (k * P + p) * S;
  u += (k * P + p) * S;
  const int d0 = pf_lower(period_of, D, p), d1 = pf_lower(period_of, D, p + 1);
  for (int c0 = d0; c0 < d1; c0 += LC) {
    const int nc = min(LC, d1 - c0);
    for (int e = tid; e < nc * J * G; e += PF_TS) s_acc[e] = 0.0;
    __syncthreads();
    for (int sb = 0; sb < S; sb += PF_TS) {
      const int s = sb + tid;
      int g = -1;
      double wt = 0.0, c = 1.0;
      if (s < S) g = m[s];
      if (g >= 0) {
        wt = u[s];
        for (int d = d0; d < c0; ++d) {  // a later chunk: the growth up to its first date
          const size_t o = (size_t)d * S + s;
          if (x_state[o] != MFF_STATE_ABSENT && pct_state[o] == MFF_STATE_VALUE) c *= pct[o] + 1.0;
        }
      }
      for (int t0 = 0; t0 < nc; t0 += PF_TD) {
#pragma unroll 4
        for (int i = 0; i < PF_TD; ++i) {
          const int d = c0 + t0 + i;
          const bool on = g >= 0 && t0 + i < nc;
          if (on) {
            const size_t o = (size_t)d * S + s;
            if (x_state[o] != MFF_STATE_ABSENT && pct_state[o] == MFF_STATE_VALUE) c *= pct[o] + 1.0;
            s_val[i * PF_TS + tid] = wt * c;
          }
          s_gid[i * PF_TS + tid] = on ? (int8_t)g : (int8_t)-1;
        }
        __syncthreads();
        pf_bin_add(s_val, s_gid, s_acc, t0, J, G);
        __syncthreads();
      }
    }
    for (int e = tid; e < nc * G; e += PF_TS) {
      const int i = e / G, g = e % G;
      A[(k * D + c0 + i) * G + g] = pf_bin_sum(s_acc, i, g, J, G);
    }
    __syncthreads();
  }
}

// the pair `which` (0, 1) of (row p, stock s): a value and the bin it goes to (-1: none).
// MODE 0: (1, m) and (u, m).  MODE 1: |t - b| (or t) to the new group, b to the old group
// of a stock that moved.
template <int MODE>
__device__ __forceinline__ void pf_pair(const int8_t* m, const double* u, const double* cend, const double* tot,
                                        size_t k, int p, int s, int P, int S, int G, int which, int& g,
                                        double& v) {
#pragma clang fp contract(off)
  const size_t o = (k * P + p) * S + s;
  g = -1;
  v = 0.0;
  if (MODE == 0) {
    g = m[o];
    v = which == 0 ? 1.0 : u[o];
    return;
  }
  if (p < 1) return;
  const size_t ob = o - S;
  int gt = m[o], gb = m[ob];
  if (gt >= G) gt = -1;  // not a group of this cut: no bin, no total
  if (gb >= G) gb = -1;
  double t = 0.0, b = 0.0;
  if (gt >= 0 && which == 0) {
    const double U = tot[((k * P + p) * G + gt) * 2];
    if (U > 0.0) t = u[o] / U;
  }
  if (gb >= 0) {
    const double* q = tot + ((k * P + p - 1) * G + gb) * 2;
    if (q[0] > 0.0) b = u[ob] * cend[ob] / q[1];
  }
  if (which == 0) {
    g = gt;
    v = fabs(t - (gb == gt ? b : 0.0));
  } else {
    g = gb != gt ? gb : -1;
    v = fabs(0.0 - b);
  }
}

// MODE 0: out [K][P][G][2] = (n, U).  MODE 1: out [K][P][G] = sum |t - b| (period 0: 0).
template <int MODE>
__global__ __launch_bounds__(PF_TS) void k_pf_rows(const int8_t* m, const double* u, const double* cend,
                                                    const double* tot, int P, int S, int G, int J,
                                                    double* out) {
  __shared__ double s_val[PF_TD * PF_TS];
  __shared__ int8_t s_gid[PF_TD * PF_TS];
  __shared__ double s_acc[PF_ACC];
  const int p0 = blockIdx.x * PF_TD, tid = threadIdx.x;
  const size_t k = blockIdx.y;
  const int nr = min(PF_TD, P - p0);
  double* acc1 = s_acc + PF_TD * J * G;  // MODE 0: the U bins
  for (int e = tid; e < (MODE == 0 ? 2 : 1) * PF_TD * J * G; e += PF_TS) s_acc[e] = 0.0;
  __syncthreads();
  for (int sb = 0; sb < S; sb += PF_TS) {
    const int s = sb + tid;
#pragma unroll 1
    for (int which = 0; which < 2; ++which) {
#pragma unroll 1
      for (int i = 0; i < PF_TD; ++i) {
        int g = -1;
        double v = 0.0;
        if (i < nr && s < S) pf_pair<MODE>(m, u, cend, tot, k, p0 + i, s, P, S, G, which, g, v);
        s_val[i * PF_TS + tid] = v;
        s_gid[i * PF_TS + tid] = (int8_t)g;
      }
      __syncthreads();
      pf_bin_add(s_val, s_gid, (MODE == 0 && which == 1) ? acc1 : s_acc, 0, J, G);
      __syncthreads();
    }
  }
  for (int e = tid; e < nr * G; e += PF_TS) {
    const int i = e / G, g = e % G;
    const size_t o = (k * P + p0 + i) * G + g;
    if (MODE == 0) {
      out[o * 2] = pf_bin_sum(s_acc, i, g, J, G);
      out[o * 2 + 1] = pf_bin_sum(acc1, i, g, J, G);
    } else {
      out[o] = pf_bin_sum(s_acc, i, g, J, G);
    }
  }
}

// thread per (k, d, g): the shards' A and (n, U) in rank order -> ret; the period's last date
// also writes count and tot = (U, A_end)
__global__ __launch_bounds__(256) void k_pf_finalize(const double* a_all, const double* nu_all,
                                                      const int32_t* period_of, int R, int K, int D, int P,
                                                      int G, double* ret, int32_t* count, double* tot) {
#pragma clang fp contract(off)
  const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= (size_t)K * D * G) return;
  const int g = (int)(e % G), d = (int)(e / G % D);
  const size_t k = e / G / D;
  const int p = period_of[d];
  const bool first = d == 0 || period_of[d - 1] != p;
  const bool last = d == D - 1 || period_of[d + 1] != p;
  double a = 0.0, ap = 0.0, n = 0.0, U = 0.0;
  for (int r = 0; r < R; ++r) {
    const double* ar = a_all + (size_t)r * K * D * G;
    const double* q = nu_all + (((size_t)r * K + k) * P * G + (size_t)p * G + g) * 2;
    a += ar[e];
    if (!first) ap += ar[e - G];
    n += q[0];
    U += q[1];
  }
  double x = 0.0;
  if (U > 0.0) {
    const double v = a / U, vp = first ? 1.0 : ap / U;
    x = v / vp - 1.0;
  }
  ret[e] = x;
  if (last) {
    const size_t o = (k * P + p) * G + g;
    count[o] = (int32_t)n;
    tot[o * 2] = U;
    tot[o * 2 + 1] = a;
  }
}

__global__ __launch_bounds__(256) void k_pf_traded_finalize(const double* part_all, int R, size_t N,
                                                             double* traded) {
  const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= N) return;
  double x = 0.0;
  for (int r = 0; r < R; ++r) x += part_all[(size_t)r * N + e];
  traded[e] = x;
}

}  // namespace mff

extern "C" {

#define PF_SIZES(fn)                                                                             \
  MFF_REQUIRE(K >= 1 && K <= PF_MAXK, fn ": K=%d outside [1, %d]", K, PF_MAXK);                  \
  MFF_REQUIRE(D >= 0, fn ": D=%d is negative", D);                                               \
  MFF_REQUIRE(S >= 0, fn ": S=%d is negative", S);                                               \
  MFF_REQUIRE(P >= 0 && P <= D && P <= PF_MAXK, fn ": P=%d outside [0, min(D=%d, %d)]", P, D,    \
              PF_MAXK);                                                                          \
  MFF_REQUIRE(D == 0 || P >= 1, fn ": P=%d with D=%d dates", P, D)
#define PF_ROWS(fn)                                                                              \
  MFF_REQUIRE(K >= 1 && K <= PF_MAXK, fn ": K=%d outside [1, %d]", K, PF_MAXK);                  \
  MFF_REQUIRE(P >= 0, fn ": P=%d is negative", P)
#define PF_GROUPS(fn) MFF_REQUIRE(G >= 1 && G <= PF_MAXG, fn ": G=%d outside [1, %d]", G, PF_MAXG)

int mff_pf_signal(const uint8_t* x_state, const int8_t* group, const double* pct, const uint8_t* pct_state,
                  const double* weight, const uint8_t* weight_state, const int32_t* period_of, int K, int D,
                  int S, int P, int8_t* m, double* u, double* cend, void* stream) {
  using namespace mff;
  clear_error();
  PF_SIZES("mff_pf_signal");
  MFF_REQUIRE((weight == nullptr) == (weight_state == nullptr),
              "mff_pf_signal: weight and weight_state go together");
  if (D == 0 || S == 0) return 0;
  MFF_REQUIRE(x_state && group && pct && pct_state && period_of && m && u && cend, "mff_pf_signal: NULL buffer");
  const int nb = (S + PF_TS - 1) / PF_TS;
  hipLaunchKernelGGL(k_pf_signal_rows, dim3(nb, P, K), dim3(PF_TS), 0, as_stream(stream), x_state, group, pct,
                     pct_state, weight, weight_state, period_of, D, S, P, m, u, cend);
  MFF_LAUNCH_CHECK();
  hipLaunchKernelGGL(k_pf_signal_shift, dim3(nb, K), dim3(PF_TS), 0, as_stream(stream), S, P, m, u);
  MFF_LAUNCH_CHECK();
  return 0;
}

int mff_pf_sums(const uint8_t* x_state, const double* pct, const uint8_t* pct_state, const int32_t* period_of,
                const int8_t* m, const double* u, int K, int D, int S, int P, int G, double* a_partial,
                double* nu_partial, void* stream) {
  using namespace mff;
  clear_error();
  PF_SIZES("mff_pf_sums");
  PF_GROUPS("mff_pf_sums");
  if (D == 0 || S == 0) return 0;
  MFF_REQUIRE(period_of && a_partial && nu_partial && x_state && pct && pct_state && m && u,
              "mff_pf_sums: NULL buffer");
  const int J = pf_split(G, 1);
  hipLaunchKernelGGL(k_pf_sums, dim3(P, K), dim3(PF_TS), 0, as_stream(stream), x_state, pct, pct_state,
                     period_of, m, u, D, S, P, G, J, pf_chunk(G, J), a_partial);
  MFF_LAUNCH_CHECK();
  hipLaunchKernelGGL(k_pf_rows<0>, dim3((P + PF_TD - 1) / PF_TD, K), dim3(PF_TS), 0, as_stream(stream), m, u,
                     (const double*)nullptr, (const double*)nullptr, P, S, G, pf_split(G, 2), nu_partial);
  MFF_LAUNCH_CHECK();
  return 0;
}

int mff_pf_finalize(const double* a_all, const double* nu_all, const int32_t* period_of, int R, int K, int D,
                    int P, int G, double* ret, int32_t* count, double* tot, void* stream) {
  using namespace mff;
  clear_error();
  const int S = 0;
  PF_SIZES("mff_pf_finalize");
  PF_GROUPS("mff_pf_finalize");
  MFF_REQUIRE(R >= 1, "mff_pf_finalize: R=%d shards", R);
  if (D == 0) return 0;
  MFF_REQUIRE(a_all && nu_all && period_of && ret && count && tot, "mff_pf_finalize: NULL buffer");
  const size_t N = (size_t)K * D * G;
  MFF_REQUIRE((N + 255) / 256 <= 0x7fffffffull, "mff_pf_finalize: K*D*G=%zu is too large", N);
  hipLaunchKernelGGL(k_pf_finalize, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, as_stream(stream), a_all,
                     nu_all, period_of, R, K, D, P, G, ret, count, tot);
  MFF_LAUNCH_CHECK();
  return 0;
}

int mff_pf_traded(const int8_t* m, const double* u, const double* cend, const double* tot, int K, int P, int S,
                  int G, double* partial, void* stream) {
  using namespace mff;
  clear_error();
  PF_ROWS("mff_pf_traded");
  MFF_REQUIRE(S >= 0, "mff_pf_traded: S=%d is negative", S);
  PF_GROUPS("mff_pf_traded");
  if (P == 0 || S == 0) return 0;
  MFF_REQUIRE(tot && partial && m && u && cend, "mff_pf_traded: NULL buffer");
  hipLaunchKernelGGL(k_pf_rows<1>, dim3((P + PF_TD - 1) / PF_TD, K), dim3(PF_TS), 0, as_stream(stream), m, u,
                     cend, tot, P, S, G, pf_split(G, 1), partial);
  MFF_LAUNCH_CHECK();
  return 0;
}

int mff_pf_traded_finalize(const double* partial_all, int R, int K, int P, int G, double* traded,
                           void* stream) {
  using namespace mff;
  clear_error();
  PF_ROWS("mff_pf_traded_finalize");
  PF_GROUPS("mff_pf_traded_finalize");
  MFF_REQUIRE(R >= 1, "mff_pf_traded_finalize: R=%d shards", R);
  if (P == 0) return 0;
  MFF_REQUIRE(partial_all && traded, "mff_pf_traded_finalize: NULL buffer");
  const size_t N = (size_t)K * P * G;
  hipLaunchKernelGGL(k_pf_traded_finalize, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, as_stream(stream),
                     partial_all, R, N, traded);
  MFF_LAUNCH_CHECK();
  return 0;
}

}  // extern "C"
