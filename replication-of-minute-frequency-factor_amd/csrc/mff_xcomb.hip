// mff_xcomb.hip — composite factor from rolling IC / ICIR / max-ICIR weights (include/mff.h,
// mff_xs_comb_*): per (factor, date) the z-score moments and the IC against the
// forward return in one pass over the K exposure rows, trailing-window weights per date from
// the IC history, and the weighted sum of the per-date z-scores over the factors a stock has.
//
//   k_comb_moments   one workgroup per day, 512-stock chunks.  The chunk of y (values + states)
//                  is staged once in LDS for all K factors (Ky = 1); wave w takes the factors
//                  w, w + 4, ...: eight stocks per lane in registers, so the chunk's moments are
//                  the two passes of k_ic_moments / k_xs_moments without a second read (shift by
//                  the first included value, mean, centred squares and products; the counts are
//                  ballot popcounts), then the chunk is merged into the factor's running
//                  (n, mean, M2 | n, mean_x, mean_y, Cxx, Cyy, Cxy) by the pairwise update, in
//                  chunk order.  x and y are read once.
//   k_comb_finalize  thread per (factor, day): the R shards' partials merged in rank order ->
//                  (n, mean, std), ic, n_pairs.
//   k_comb_weights   one wave per date, lane = factor: the window's IC means / stds per lane in
//                  date order; max_icir: the listwise dates by ballot, the covariance rows in
//                  registers (lane i owns row i; the date's deviations are broadcast through
//                  LDS), unit-diagonal scaling, shrinkage of the off-diagonal, chol_lower
//                  (mff_gram.h) and the two triangular solves column by column; sum |w| by the
//                  fixed-order wave sum.
//   k_comb_apply     per (day, 1024-stock chunk): (w, mean, 1 / std) of the day's K factors in
//                  LDS, four stocks per thread, factors in row order; streaming: 9 B read per
//                  (factor, stock-day), 9 B written per stock-day.
// Every sum has one fixed order (lane tree of wsum, chunk order, rank order, date order, factor
// order), so results are bit-identical from run to run.
#include <hip/hip_runtime.h>

#include "../../include/mff.h"
#include "mff_gram.h"
#include "mff_internal.h"
#include "mff_wave.h"

namespace mff {

constexpr int COMB_MAX_K = 64;
constexpr int COMB_THREADS = 256;
constexpr int COMB_WAVES = COMB_THREADS / WAVE;
constexpr int COMB_P = 8;                  // stocks per lane and chunk
constexpr int COMB_CHUNK = WAVE * COMB_P;    // stocks per chunk of the moments pass (512)
constexpr int COMB_NP = 9;                 // entries of a partial
constexpr int COMB_AP = 4;                 // stocks per thread of the apply pass
constexpr int COMB_AP_STOCKS = COMB_THREADS * COMB_AP;  // 1024
static_assert(COMB_MAX_K <= GR_B, "k_comb_weights keeps its matrix with chol_lower's row stride");

// b merged into a: (n, mean, M2)
__device__ __forceinline__ void comb_merge3(double* a, double nb, double mb, double m2b) {
  if (nb == 0.0) return;
  if (a[0] == 0.0) {
    a[0] = nb; a[1] = mb; a[2] = m2b;
    return;
  }
  const double nt = a[0] + nb, dl = mb - a[1], w = a[0] * nb / nt;
  a[2] += m2b + dl * dl * w;
  a[1] += dl * nb / nt;
  a[0] = nt;
}
// b merged into a: (n, mean_x, mean_y, Cxx, Cyy, Cxy) (k_ic_finalize's update)
__device__ __forceinline__ void comb_merge6(double* a, double nb, double mxb, double myb, double cxxb, double cyyb,
                                          double cxyb) {
  if (nb == 0.0) return;
  if (a[0] == 0.0) {
    a[0] = nb; a[1] = mxb; a[2] = myb; a[3] = cxxb; a[4] = cyyb; a[5] = cxyb;
    return;
  }
  const double nt = a[0] + nb, dx = mxb - a[1], dy = myb - a[2], w = a[0] * nb / nt;
  a[3] += cxxb + dx * dx * w;
  a[4] += cyyb + dy * dy * w;
  a[5] += cxyb + dx * dy * w;
  a[1] += dx * nb / nt;
  a[2] += dy * nb / nt;
  a[0] = nt;
}

// partial [K][D][9]; Ky: 0 = no y (the pair moments are 0), 1 = row 0 for every factor, K = row k
__global__ __launch_bounds__(COMB_THREADS) void k_comb_moments(const double* __restrict__ xv,
                                                               const uint8_t* __restrict__ xs, int K, int D, int S,
                                                               const double* __restrict__ yv,
                                                               const uint8_t* __restrict__ ys, int Ky,
                                                               double* __restrict__ part) {
  __shared__ double ty[COMB_CHUNK];
  __shared__ uint8_t tys[COMB_CHUNK];
  __shared__ double acc[COMB_MAX_K][COMB_NP];
  const int d = blockIdx.x, t = threadIdx.x, lane = t & (WAVE - 1), w = t / WAVE;
  if (lane == 0)
    for (int k = w; k < K; k += COMB_WAVES)
#pragma unroll
      for (int j = 0; j < COMB_NP; ++j) acc[k][j] = 0.0;
  for (int c0 = 0; c0 < S; c0 += COMB_CHUNK) {
    if (Ky == 1) {
      __syncthreads();  // the previous chunk's reads are done
      for (int i = t; i < COMB_CHUNK; i += COMB_THREADS) {
        const int s = c0 + i;
        const bool in = s < S;
        ty[i] = in ? yv[(size_t)d * S + s] : 0.0;
        tys[i] = in ? ys[(size_t)d * S + s] : (uint8_t)MFF_STATE_ABSENT;
      }
      __syncthreads();
    }
    for (int k = w; k < K; k += COMB_WAVES) {
      const size_t row = ((size_t)k * D + d) * (size_t)S;
      double x[COMB_P], y[COMB_P];
      bool zin[COMB_P], pin[COMB_P];
#pragma unroll
      for (int i = 0; i < COMB_P; ++i) {
        const int s = c0 + i * WAVE + lane;
        const bool in = s < S;
        x[i] = in ? xv[row + s] : 0.0;
        const uint8_t sx = in ? xs[row + s] : (uint8_t)MFF_STATE_ABSENT;
        uint8_t sy = MFF_STATE_ABSENT;
        y[i] = 0.0;
        if (Ky == 1) {
          y[i] = ty[i * WAVE + lane];
          sy = tys[i * WAVE + lane];
        } else if (Ky != 0 && in) {
          y[i] = yv[row + s];
          sy = ys[row + s];
        }
        zin[i] = sx == MFF_STATE_VALUE && __builtin_isfinite(x[i]);
        pin[i] = sx == MFF_STATE_VALUE && !__builtin_isnan(x[i]) && sy == MFF_STATE_VALUE;
      }
      // counts and the first included entry in stock order (slot i holds stocks c0 + 64 i ..)
      int nz = 0, np = 0;
      double x0 = 0.0, px0 = 0.0, py0 = 0.0;
#pragma unroll
      for (int i = 0; i < COMB_P; ++i) {
        const uint64_t bz = __ballot(zin[i]), bp = __ballot(pin[i]);
        if (bz && nz == 0) x0 = rdlane(x[i], __builtin_ctzll(bz));
        if (bp && np == 0) {
          const int l0 = __builtin_ctzll(bp);
          const double cx = rdlane(x[i], l0), cy = rdlane(y[i], l0);
          px0 = __builtin_isfinite(cx) ? cx : 0.0;
          py0 = __builtin_isfinite(cy) ? cy : 0.0;
        }
        nz += __popcll(bz);
        np += __popcll(bp);
      }
      if (nz == 0 && np == 0) continue;  // (wave-uniform)
      double s1 = 0.0, s1x = 0.0, s1y = 0.0;
#pragma unroll
      for (int i = 0; i < COMB_P; ++i) {
        if (zin[i]) s1 += x[i] - x0;
        if (pin[i]) {
          s1x += x[i] - px0;
          s1y += y[i] - py0;
        }
      }
      s1 = wsum(s1);
      s1x = wsum(s1x);
      s1y = wsum(s1y);
      const double mz = nz ? x0 + s1 / (double)nz : 0.0;
      const double mx = np ? px0 + s1x / (double)np : 0.0, my = np ? py0 + s1y / (double)np : 0.0;
      double m2 = 0.0, cxx = 0.0, cyy = 0.0, cxy = 0.0;
#pragma unroll
      for (int i = 0; i < COMB_P; ++i) {
        if (zin[i]) {
          const double dl = x[i] - mz;
          m2 += dl * dl;
        }
        if (pin[i]) {
          const double dx = x[i] - mx, dy = y[i] - my;
          cxx += dx * dx;
          cyy += dy * dy;
          cxy += dx * dy;
        }
      }
      m2 = wsum(m2);
      cxx = wsum(cxx);
      cyy = wsum(cyy);
      cxy = wsum(cxy);
      if (lane == 0) {  // (this wave alone touches acc[k])
        comb_merge3(&acc[k][0], (double)nz, mz, m2);
        comb_merge6(&acc[k][3], (double)np, mx, my, cxx, cyy, cxy);
      }
    }
  }
  if (lane == 0)
    for (int k = w; k < K; k += COMB_WAVES) {
      double* p = part + ((size_t)k * D + d) * COMB_NP;
#pragma unroll
      for (int j = 0; j < COMB_NP; ++j) p[j] = acc[k][j];
    }
}

__global__ __launch_bounds__(COMB_THREADS) void k_comb_finalize(const double* __restrict__ parts, int R, int K, int D,
                                                                int min_obs, double* __restrict__ zmom,
                                                                double* __restrict__ ic,
                                                                int32_t* __restrict__ npairs) {
  const size_t nseg = (size_t)K * D;
  const size_t e = (size_t)blockIdx.x * COMB_THREADS + threadIdx.x;
  if (e >= nseg) return;
  double z[3] = {0.0, 0.0, 0.0}, c[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  for (int r = 0; r < R; ++r) {  // rank order
    const double* p = parts + ((size_t)r * nseg + e) * COMB_NP;
    comb_merge3(z, p[0], p[1], p[2]);
    comb_merge6(c, p[3], p[4], p[5], p[6], p[7], p[8]);
  }
  zmom[e * 3 + 0] = z[0];
  zmom[e * 3 + 1] = z[1];
  zmom[e * 3 + 2] = z[0] < 2.0 ? qnan() : sqrt(z[2] / (z[0] - 1.0));
  const double need = (double)(min_obs > 2 ? min_obs : 2);
  const double den = sqrt(c[3] * c[4]);
  ic[e] = (c[0] < need || den == 0.0) ? qnan() : c[5] / den;
  npairs[e] = (int32_t)c[0];
}

// one wave per date, lane = factor
__global__ __launch_bounds__(WAVE) void k_comb_weights(const double* __restrict__ ic, int K, int D, int method, int h,
                                                       int W, int m, double shrink, double* __restrict__ weights,
                                                       int32_t* __restrict__ count, int32_t* __restrict__ status) {
  __shared__ double A[COMB_MAX_K * GR_LS];
  __shared__ double bc[COMB_MAX_K];  // a date's deviations / a solve's broadcast value
  __shared__ double dg[COMB_MAX_K];
  const int d = blockIdx.x, k = threadIdx.x;
  const bool mine = k < K;
  const uint64_t full = ~0ull;
  // E(d) = [lo, hi], empty when hi < 0
  const long long hi = (long long)d - h;
  const long long lo = hi - W + 1 > 0 ? hi - W + 1 : 0;
  const double* row = ic + (size_t)(mine ? k : 0) * D;
  double wraw = 0.0;
  int cnt = 0, stat = 0;
  if (method == 0) {
    wraw = mine ? 1.0 : 0.0;
  } else if (method <= 2) {
    bool ok = false;
    if (mine) {
      double v0 = 0.0, s = 0.0;
      for (long long e = lo; e <= hi; ++e) {
        const double v = row[e];
        if (!__builtin_isfinite(v)) continue;
        if (cnt == 0) v0 = v;
        s += v - v0;
        ++cnt;
      }
      const double mean = cnt ? v0 + s / (double)cnt : 0.0;
      if (method == 1) {
        ok = cnt >= m;
        wraw = ok ? mean : 0.0;
      } else {
        double m2 = 0.0;
        for (long long e = lo; e <= hi; ++e) {
          const double v = row[e];
          if (__builtin_isfinite(v)) m2 += (v - mean) * (v - mean);
        }
        const double sd = cnt >= 2 ? sqrt(m2 / (double)(cnt - 1)) : qnan();
        ok = cnt >= (m > 2 ? m : 2) && __builtin_isfinite(sd) && sd > 0.0;
        wraw = ok ? mean / sd : 0.0;
      }
    }
    if (__ballot(ok) == 0) stat = 1;
  } else {
    // the listwise dates L(d): every one of the K ICs finite
    double v0 = 0.0, s = 0.0;
    for (long long e = lo; e <= hi; ++e) {
      const double v = mine ? row[e] : 0.0;
      if (__ballot(__builtin_isfinite(v)) != full) continue;
      if (cnt == 0) v0 = v;
      s += v - v0;
      ++cnt;
    }
    int need = m > 2 ? m : 2;
    if (shrink == 0.0 && need < K + 1) need = K + 1;
    if (cnt < need) stat = 1;
    if (stat == 0) {
      const double mu = v0 + s / (double)cnt;
      double a[COMB_MAX_K];
#pragma unroll
      for (int j = 0; j < COMB_MAX_K; ++j) a[j] = 0.0;
      for (long long e = lo; e <= hi; ++e) {  // lane i: row i of sum_L dev dev^T, date order
        const double v = mine ? row[e] : 0.0;
        if (__ballot(__builtin_isfinite(v)) != full) continue;
        const double dv = mine ? v - mu : 0.0;
        __syncthreads();  // the previous date's reads are done
        bc[k] = dv;
        __syncthreads();
#pragma unroll
        for (int j = 0; j < COMB_MAX_K; ++j) a[j] += dv * bc[j];
      }
#pragma unroll
      for (int j = 0; j < COMB_MAX_K; ++j) A[k * GR_LS + j] = a[j];
      __syncthreads();
      const double mkk = A[k * GR_LS + k];
      dg[k] = mkk;
      if (__ballot(mine && !(mkk > 0.0)) != 0) stat = 2;  // a constant IC series (or not finite)
      __syncthreads();
      if (stat == 0) {
        // unit diagonal, the off-diagonal shrunk: (1 - shrink) M_ij / sqrt(M_ii M_jj)
        if (mine)
          for (int j = 0; j < K; ++j)
            A[k * GR_LS + j] = j == k ? 1.0 : (1.0 - shrink) * (A[k * GR_LS + j] / sqrt(mkk * dg[j]));
        __syncthreads();
        if (!chol_lower(A, K, k, CHOL_PIVOT_MIN)) stat = 2;  // row t on lane t
      }
      if (stat == 0) {
        const double sig = sqrt(mkk / (double)(cnt - 1));
        double b = mine ? mu / sig : 0.0;
        for (int j = 0; j < K; ++j) {  // L u = b, column by column
          if (k == j) {
            b /= A[j * GR_LS + j];
            bc[j] = b;
          }
          __syncthreads();
          if (k > j && mine) b -= A[k * GR_LS + j] * bc[j];
          __syncthreads();
        }
        for (int j = K - 1; j >= 0; --j) {  // L^T v = u
          if (k == j) {
            b /= A[j * GR_LS + j];
            bc[j] = b;
          }
          __syncthreads();
          if (k < j) b -= A[j * GR_LS + k] * bc[j];
          __syncthreads();
        }
        wraw = mine ? b / sig : 0.0;
      }
    }
  }
  const double norm = wsum(mine ? fabs(wraw) : 0.0);
  if (stat == 0 && !(norm > 0.0 && __builtin_isfinite(norm))) stat = 2;
  if (mine) {
    weights[(size_t)d * K + k] = stat == 0 ? wraw / norm : qnan();
    count[(size_t)d * K + k] = cnt;
  }
  if (k == 0) status[d] = stat;
}

__global__ __launch_bounds__(COMB_THREADS) void k_comb_apply(const double* __restrict__ xv,
                                                             const uint8_t* __restrict__ xs, int K, int D, int S,
                                                             const double* __restrict__ zmom,
                                                             const double* __restrict__ weights,
                                                             const int32_t* __restrict__ status, int min_factors,
                                                             double* __restrict__ ov, uint8_t* __restrict__ os) {
  __shared__ double sw[COMB_MAX_K], sm[COMB_MAX_K], si[COMB_MAX_K];
  const int d = blockIdx.x, t = threadIdx.x;
  const int s0 = blockIdx.y * COMB_AP_STOCKS + t;
  const bool ok = status[d] == 0;
  if (t < K) {
    const double* z = zmom + ((size_t)t * D + d) * 3;
    const double wk = weights[(size_t)d * K + t], sd = z[2];
    const bool use = ok && z[0] >= 2.0 && sd > 0.0 && wk != 0.0;
    sw[t] = use ? wk : 0.0;
    sm[t] = z[1];
    si[t] = use ? 1.0 / sd : 0.0;
  }
  __syncthreads();
  double num[COMB_AP], den[COMB_AP];
  int cnt[COMB_AP];
  bool any[COMB_AP];
#pragma unroll
  for (int i = 0; i < COMB_AP; ++i) {
    num[i] = den[i] = 0.0;
    cnt[i] = 0;
    any[i] = false;
  }
  for (int k = 0; k < K; ++k) {  // factor order
    const size_t row = ((size_t)k * D + d) * (size_t)S;
    const double wk = sw[k], mean = sm[k], istd = si[k];
    uint8_t st[COMB_AP];
    double x[COMB_AP];
#pragma unroll
    for (int i = 0; i < COMB_AP; ++i) {
      const int s = s0 + i * COMB_THREADS;
      st[i] = s < S ? xs[row + s] : (uint8_t)MFF_STATE_ABSENT;
      x[i] = (ok && s < S) ? xv[row + s] : 0.0;
    }
#pragma unroll
    for (int i = 0; i < COMB_AP; ++i) {
      any[i] = any[i] || st[i] != MFF_STATE_ABSENT;
      if (wk != 0.0 && st[i] == MFF_STATE_VALUE && __builtin_isfinite(x[i])) {
        num[i] += wk * ((x[i] - mean) * istd);
        den[i] += fabs(wk);
        ++cnt[i];
      }
    }
  }
#pragma unroll
  for (int i = 0; i < COMB_AP; ++i) {
    const int s = s0 + i * COMB_THREADS;
    if (s >= S) continue;
    const bool val = ok && cnt[i] >= min_factors;
    ov[(size_t)d * S + s] = val ? num[i] / den[i] : 0.0;
    os[(size_t)d * S + s] = val ? (uint8_t)MFF_STATE_VALUE : (any[i] ? (uint8_t)MFF_STATE_NULL : (uint8_t)MFF_STATE_ABSENT);
  }
}

static int comb_check(const char* what, int K, int D, int S) { return xs_check(what, K, COMB_MAX_K, D, S); }

}  // namespace mff

using namespace mff;

extern "C" {

int mff_xs_comb_moments(const double* x_val, const uint8_t* x_state, int K, int D, int S, const double* y_val,
                        const uint8_t* y_state, int Ky, double* partial, void* stream) {
  clear_error();
  if (int rc = comb_check("mff_xs_comb_moments", K, D, S)) return rc;
  MFF_REQUIRE(Ky == 0 || Ky == 1 || Ky == K, "mff_xs_comb_moments: Ky=%d is not 0, 1 or K=%d", Ky, K);
  if (D == 0) return 0;
  // (an empty stock axis has no buffers to speak of)
  MFF_REQUIRE(S == 0 || ((Ky == 0) == (y_val == nullptr) && (y_val == nullptr) == (y_state == nullptr)),
              "mff_xs_comb_moments: Ky=%d does not match y_val / y_state (Ky = 0 means no y)", Ky);
  MFF_REQUIRE(partial && (S == 0 || (x_val && x_state)), "mff_xs_comb_moments: NULL buffer");
  hipLaunchKernelGGL(k_comb_moments, dim3((unsigned)D), dim3(COMB_THREADS), 0, as_stream(stream), x_val, x_state, K, D,
                     S, y_val, y_state, Ky, partial);
  MFF_LAUNCH_CHECK();
  return 0;
}

int mff_xs_comb_finalize(const double* partial_all, int R, int K, int D, int min_obs, double* zmom, double* ic,
                         int32_t* n_pairs, void* stream) {
  clear_error();
  if (int rc = comb_check("mff_xs_comb_finalize", K, D, 0)) return rc;
  MFF_REQUIRE(R >= 1, "mff_xs_comb_finalize: R=%d shards", R);
  MFF_REQUIRE(min_obs >= 0, "mff_xs_comb_finalize: min_obs=%d below 0", min_obs);
  if (D == 0) return 0;
  MFF_REQUIRE(partial_all && zmom && ic && n_pairs, "mff_xs_comb_finalize: NULL buffer");
  const size_t nseg = (size_t)K * D;
  hipLaunchKernelGGL(k_comb_finalize, dim3((unsigned)((nseg + COMB_THREADS - 1) / COMB_THREADS)), dim3(COMB_THREADS), 0,
                     as_stream(stream), partial_all, R, K, D, min_obs, zmom, ic, n_pairs);
  MFF_LAUNCH_CHECK();
  return 0;
}

int mff_xs_comb_weights(const double* ic, int K, int D, int method, int future_days, int window, int min_periods,
                        double shrink, double* weights, int32_t* count, int32_t* status, void* stream) {
  clear_error();
  if (int rc = comb_check("mff_xs_comb_weights", K, D, 0)) return rc;
  MFF_REQUIRE(method >= 0 && method <= 3, "mff_xs_comb_weights: method=%d (0 equal, 1 ic, 2 icir, 3 max_icir)",
              method);
  MFF_REQUIRE(future_days >= 1, "mff_xs_comb_weights: future_days=%d below 1", future_days);
  MFF_REQUIRE(window >= 1, "mff_xs_comb_weights: window=%d below 1", window);
  MFF_REQUIRE(min_periods >= 1, "mff_xs_comb_weights: min_periods=%d below 1", min_periods);
  MFF_REQUIRE(shrink >= 0.0 && shrink <= 1.0, "mff_xs_comb_weights: shrink=%g outside [0, 1]", shrink);
  if (D == 0) return 0;
  MFF_REQUIRE(weights && count && status && (ic || method == 0), "mff_xs_comb_weights: NULL buffer");
  hipLaunchKernelGGL(k_comb_weights, dim3((unsigned)D), dim3(WAVE), 0, as_stream(stream), ic, K, D, method,
                     future_days, window, min_periods, shrink, weights, count, status);
  MFF_LAUNCH_CHECK();
  return 0;
}

int mff_xs_comb_apply(const double* x_val, const uint8_t* x_state, int K, int D, int S, const double* zmom,
                      const double* weights, const int32_t* status, int min_factors, double* out_val,
                      uint8_t* out_state, void* stream) {
  clear_error();
  if (int rc = comb_check("mff_xs_comb_apply", K, D, S)) return rc;
  MFF_REQUIRE(min_factors >= 1 && min_factors <= K, "mff_xs_comb_apply: min_factors=%d outside [1, K=%d]",
              min_factors, K);
  if (D == 0 || S == 0) return 0;
  MFF_REQUIRE(x_val && x_state && zmom && weights && status && out_val && out_state, "mff_xs_comb_apply: NULL buffer");
  hipLaunchKernelGGL(k_comb_apply, dim3((unsigned)D, (unsigned)((S + COMB_AP_STOCKS - 1) / COMB_AP_STOCKS)),
                     dim3(COMB_THREADS), 0, as_stream(stream), x_val, x_state, K, D, S, zmom, weights, status,
                     min_factors, out_val, out_state);
  MFF_LAUNCH_CHECK();
  return 0;
}

}  // extern "C"
