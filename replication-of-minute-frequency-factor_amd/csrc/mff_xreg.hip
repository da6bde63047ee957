// mff_xreg.hip — per-day multi-factor cross-sectional regression (include/mff.h,
// mff_xs_reg_*): weighted least squares of the regressand on industry
// dummies and K exposure rows, solved by Frisch-Waugh on the within-industry centred values.
//
//   k_xr_mask    listwise usable set -> ugrp [D][S]: the stock's industry (0 without
//                industries) inside U, -1 outside.  One plane carries the mask of every column.
//   k_xr_groups_col  (up to 64 industries) per (day, stock run): n_g, W_g, sum w c per industry
//                and the raw sum w c^2: 32-stock tiles through LDS, one thread per column walking
//                each tile in stock order into its own column of an LDS table.
//   k_xr_groups  (more industries) the same per (day, 16 virtual columns, stock run).  A wave
//                walks the stocks in 64-stock chunks; inside a chunk it
//                visits the industries present in lane order of their first member, sums the
//                members' values by the fixed DPP butterfly of wsum() and adds the chunk's
//                total to its own LDS table in chunk order: no atomics, one order.
//   k_xr_means   the R shards' group sums added in rank order -> the means table and the
//                per-day scalars (n, non-empty industries, the between-industry part of the
//                r2 denominator, the raw second moments).
//   k_xr_gram    one workgroup per (day, stock split): sum w c~ c~^T of the C = K + 1 columns
//                (c~ is 0 outside U): gram_block (mff_gram.h) with the weight operand.
//   k_xr_solve   one wave per day: the planes of the shards / splits added in plane order, the
//                singular rule, unit-diagonal scaling, chol_lower (mff_gram.h), the two
//                triangular solves and diag(M^-1) from chol_inv_column.
//   k_xr_residual, k_xr_mean: elementwise / per-factor day loops.
// Every sum has one fixed order, so results are bit-identical from run to run.
#include <hip/hip_runtime.h>

#include "../../include/mff.h"
#include "mff_gram.h"
#include "mff_internal.h"
#include "mff_wave.h"

namespace mff {

constexpr int XR_MAX_K = 63;
constexpr int XR_MAX_G = 256;
constexpr int XR_GC = 4;            // virtual columns per wave in k_xr_groups
constexpr double XR_CONST_REL = 1e-20;
constexpr int XR_AGG = 6;

__host__ __device__ inline size_t xr_align(size_t b) { return (b + 255) & ~(size_t)255; }
// workspace: dayinfo f64 [D][C + 4] | means f64 [D][Ge][C] | ugrp i32 [D][S]
__host__ __device__ inline size_t xr_means_off(int K, int D) { return xr_align((size_t)D * (K + 5) * 8); }
__host__ __device__ inline size_t xr_ugrp_off(int K, int D, int Ge) {
  return xr_means_off(K, D) + xr_align((size_t)D * Ge * (K + 1) * 8);
}
__host__ __device__ inline size_t xr_ws_bytes(int K, int D, int S, int Ge) {
  return xr_ugrp_off(K, D, Ge) + xr_align((size_t)D * S * 4);
}

__global__ __launch_bounds__(256) void k_xr_mask(const double* __restrict__ xv, const uint8_t* __restrict__ xs, int K,
                                                 int D, int S, const double* __restrict__ yv,
                                                 const uint8_t* __restrict__ ys, const double* __restrict__ wv,
                                                 const uint8_t* __restrict__ wst, const int32_t* __restrict__ group,
                                                 int G, int32_t* __restrict__ ugrp) {
  const int d = blockIdx.x;
  const int s = (int)blockIdx.y * 256 + (int)threadIdx.x;
  if (s >= S) return;
  const size_t ds = (size_t)d * S + s;
  bool u = xs_usable(yv[ds], ys[ds]);
  if (wv) {
    const double w = wv[ds];
    u = u && xs_usable(w, wst[ds]) && w > 0.0;
  }
  int32_t g = 0;
  if (group) {
    g = group[ds];
    u = u && g >= 0 && g < G;
  }
  for (int k = 0; k < K; ++k) {
    const size_t off = ((size_t)k * D + d) * (size_t)S + s;
    u = u && xs_usable(xv[off], xs[off]);
  }
  ugrp[ds] = u ? g : -1;
}

// gsums [D][Ge + 1][C + 2]: row g = (n_g, W_g, sum w c_0 .. c_{C-1}); row Ge = (0, 0, sum w c^2).
// Virtual column v: v < K row v, v == K the regressand, v == C ones (W_g), v == C + 1 the count.
__global__ __launch_bounds__(256) void k_xr_groups(const double* __restrict__ xv, int K, int D, int S,
                                                   const double* __restrict__ yv, const double* __restrict__ wv,
                                                   const int32_t* __restrict__ ugrp, int Ge, int split_stocks,
                                                   double* __restrict__ gsums) {
  __shared__ double tab[4][XR_MAX_G * XR_GC];
  const int sbeg = (int)min((long long)blockIdx.z * split_stocks, (long long)S);
  const int send = (int)min((long long)sbeg + split_stocks, (long long)S);
  const int d = blockIdx.x, t = threadIdx.x, w = t >> 6, l = t & 63;
  const int C = K + 1, CV = C + 2;
  const int v0 = ((int)blockIdx.y * 4 + w) * XR_GC;
  double* tb = tab[w];
  for (int i = l; i < Ge * XR_GC; i += WAVE) tb[i] = 0.0;
  __syncthreads();
  double sq[XR_GC];
#pragma unroll
  for (int k = 0; k < XR_GC; ++k) sq[k] = 0.0;
  if (v0 < CV) {  // (wave-uniform)
    for (int s0 = sbeg; s0 < send; s0 += WAVE) {
      const int s = s0 + l;
      const size_t ds = (size_t)d * S + (s < send ? s : 0);
      const int g = s < send ? ugrp[ds] : -1;
      const double wt = (g >= 0 && wv) ? wv[ds] : 1.0;
      double val[XR_GC];
#pragma unroll
      for (int k = 0; k < XR_GC; ++k) {
        const int v = v0 + k;
        double x = 0.0;
        if (g >= 0 && v < CV) {
          if (v < K)
            x = xv[((size_t)v * D + d) * (size_t)S + s];
          else if (v == K)
            x = yv[ds];
          else
            x = 1.0;
          if (v < C) sq[k] += wt * x * x;
          if (v <= C) x *= wt;
        }
        val[k] = x;
      }
      uint64_t rem = __ballot(g >= 0);
      while (rem) {
        const int src = __builtin_amdgcn_readfirstlane((int)__builtin_ctzll(rem));
        const int g0 = __builtin_amdgcn_readlane(g, src);
        const bool sel = g == g0;
#pragma unroll
        for (int k = 0; k < XR_GC; ++k) {
          const double sum = wsum(sel ? val[k] : 0.0);
          if (l == 0) tb[g0 * XR_GC + k] += sum;
        }
        rem &= ~__ballot(sel);
      }
    }
  }
#pragma unroll
  for (int k = 0; k < XR_GC; ++k) sq[k] = wsum(sq[k]);
  __syncthreads();
  if (v0 >= CV) return;
  double* out = gsums + ((size_t)blockIdx.z * D + d) * (Ge + 1) * CV;
  for (int i = l; i < Ge * XR_GC; i += WAVE) {
    const int g = i / XR_GC, v = v0 + i % XR_GC;
    if (v >= CV) continue;
    const int col = v < C ? 2 + v : (v == C ? 1 : 0);
    out[(size_t)g * CV + col] = tb[i];
  }
  if (l < XR_GC && v0 + l < CV) {
    const int v = v0 + l;
    const int col = v < C ? 2 + v : (v == C ? 1 : 0);
    const double q = l == 0 ? sq[0] : l == 1 ? sq[1] : l == 2 ? sq[2] : sq[3];
    out[(size_t)Ge * CV + col] = v < C ? q : 0.0;
  }
}

// The same sums for Ge <= XR_COL_G industries.  A 32-stock tile of the K + 1 columns goes
// through LDS with the coalesced loader shape of k_xr_gram (the next tile's values in registers
// meanwhile; row stride 33 doubles: the column walk below reads 32 distinct banks); then one
// thread per virtual column walks the tile's stocks in stock order and adds into its own column
// of an LDS table [Ge][C + 2] -- no reduction across lanes at all, one order.
constexpr int XR_COL_G = 64;
constexpr int XR_COL_T = 256;
constexpr int XR_COL_STR = GR_KT + 1;
__global__ __launch_bounds__(XR_COL_T) void k_xr_groups_col(const double* __restrict__ xv, int K, int D, int S,
                                                            const double* __restrict__ yv,
                                                            const double* __restrict__ wv,
                                                            const int32_t* __restrict__ ugrp, int Ge, int split_stocks,
                                                            double* __restrict__ gsums) {
  __shared__ double tab[XR_COL_G * (XR_MAX_K + 3)];
  __shared__ double tile[GR_B * XR_COL_STR];
  __shared__ double wl[GR_KT];
  __shared__ int gl[GR_KT];
  const int d = blockIdx.x, p = blockIdx.y, t = threadIdx.x;
  const int C = K + 1, CV = C + 2;
  const int sbeg = (int)min((long long)p * split_stocks, (long long)S);
  const int send = (int)min((long long)sbeg + split_stocks, (long long)S);
  for (int i = t; i < Ge * CV; i += XR_COL_T) tab[i] = 0.0;
  const int ls = t & (GR_KT - 1), r0 = t / GR_KT;
  double cv[GR_NR], wt = 0.0, sq = 0.0;
  int g = -1;
  auto load = [&](int k0) {
    const int s = k0 + ls;
    const size_t ds = (size_t)d * S + (s < send ? s : 0);
    g = s < send ? ugrp[ds] : -1;
    wt = g >= 0 ? (wv ? wv[ds] : 1.0) : 0.0;
#pragma unroll
    for (int i = 0; i < GR_NR; ++i) {
      const int r = r0 + GR_RS * i;
      cv[i] = (g >= 0 && r <= K) ? (r < K ? xv[((size_t)r * D + d) * (size_t)S + s] : yv[ds]) : 0.0;
    }
  };
  if (sbeg < send) load(sbeg);
  for (int k0 = sbeg; k0 < send; k0 += GR_KT) {
    __syncthreads();  // the previous tile's walk is done (first pass: tab is zeroed)
#pragma unroll
    for (int i = 0; i < GR_NR; ++i) tile[(r0 + GR_RS * i) * XR_COL_STR + ls] = cv[i];
    if (t < GR_KT) {
      wl[ls] = wt;
      gl[ls] = g;
    }
    __syncthreads();
    if (k0 + GR_KT < send) load(k0 + GR_KT);
    if (t < CV) {
#pragma unroll 8
      for (int s = 0; s < GR_KT; ++s) {
        const int gs = gl[s];
        if (gs < 0) continue;  // (uniform over the block)
        const double x = t < C ? tile[t * XR_COL_STR + s] : 1.0;
        const double wx = wl[s] * x;
        tab[gs * CV + t] += t <= C ? wx : 1.0;
        sq += wx * x;
      }
    }
  }
  __syncthreads();
  double* out = gsums + ((size_t)p * D + d) * (Ge + 1) * CV;
  for (int i = t; i < Ge * CV; i += XR_COL_T) {
    const int gi = i / CV, v = i - gi * CV;
    out[(size_t)gi * CV + (v < C ? 2 + v : (v == C ? 1 : 0))] = tab[i];
  }
  if (t < CV) out[(size_t)Ge * CV + (t < C ? 2 + t : (t == C ? 1 : 0))] = t < C ? sq : 0.0;
}

// dayinfo [D][C + 4] = (n, non-empty industries, sum_g W_g (ybar_g - ybar_w)^2, W, raw sum w c^2 ...)
__global__ __launch_bounds__(256) void k_xr_means(const double* __restrict__ gs_all, int R, int K, int D, int Ge,
                                                  int nogroup, double* __restrict__ means, double* __restrict__ dayinfo) {
  const int d = blockIdx.x, t = threadIdx.x, l = t & 63;
  const int C = K + 1, CV = C + 2;
  const size_t rstride = (size_t)D * (Ge + 1) * CV;
  const double* g0 = gs_all + (size_t)d * (Ge + 1) * CV;
  for (int e = t; e < Ge * C; e += 256) {
    const int g = e / C, c = e - g * C;
    double ng = 0.0, W = 0.0, sum = 0.0;
    for (int r = 0; r < R; ++r) {  // rank order
      const double* p = g0 + (size_t)r * rstride + (size_t)g * CV;
      ng += p[0];
      W += p[1];
      sum += p[2 + c];
    }
    means[((size_t)d * Ge + g) * C + c] = ng > 0.0 ? sum / W : 0.0;
  }
  double* info = dayinfo + (size_t)d * (C + 4);
  for (int c = t; c < C; c += 256) {
    double q = 0.0;
    for (int r = 0; r < R; ++r) q += g0[(size_t)r * rstride + (size_t)Ge * CV + 2 + c];
    info[4 + c] = q;
  }
  if (t >= WAVE) return;  // wave 0: the per-day scalars, lanes over the industries
  double n = 0.0, gne = 0.0, Wt = 0.0, Sy = 0.0;
  for (int g = l; g < Ge; g += WAVE) {
    double ng = 0.0, W = 0.0, sy = 0.0;
    for (int r = 0; r < R; ++r) {
      const double* p = g0 + (size_t)r * rstride + (size_t)g * CV;
      ng += p[0];
      W += p[1];
      sy += p[2 + K];
    }
    if (ng > 0.0) {
      n += ng;
      gne += 1.0;
      Wt += W;
      Sy += sy;
    }
  }
  n = wsum(n);
  gne = wsum(gne);
  Wt = wsum(Wt);
  Sy = wsum(Sy);
  const double ybar = Wt > 0.0 ? Sy / Wt : 0.0;
  double bt = 0.0;
  for (int g = l; g < Ge; g += WAVE) {
    double ng = 0.0, W = 0.0, sy = 0.0;
    for (int r = 0; r < R; ++r) {
      const double* p = g0 + (size_t)r * rstride + (size_t)g * CV;
      ng += p[0];
      W += p[1];
      sy += p[2 + K];
    }
    if (ng > 0.0) {
      const double dlt = sy / W - ybar;
      bt += W * dlt * dlt;
    }
  }
  bt = wsum(bt);
  if (l == 0) {
    info[0] = n;
    info[1] = nogroup ? 1.0 : gne;  // (1 without industries, also for an empty U)
    info[2] = bt;
    info[3] = Wt;
  }
}

// this thread's part of a [64 columns][GR_KT stocks] tile: stock t % GR_KT, columns t / GR_KT + 8 i,
// already centred (0 outside U, beyond `send` and in the padding columns); wt = the stock's weight
__device__ __forceinline__ void xr_load(const double* __restrict__ xv, const double* __restrict__ yv,
                                        const double* __restrict__ wv, const int32_t* __restrict__ ugrp,
                                        const double* __restrict__ means, int K, int D, int d, int S, int send,
                                        int Ge, int k0, double (&cv)[GR_NR], double& wt) {
  const int s = k0 + (int)(threadIdx.x & (GR_KT - 1));
  const bool in = s < send;
  const size_t ds = (size_t)d * S + (in ? s : 0);
  const int g = in ? ugrp[ds] : -1;
  wt = g >= 0 ? (wv ? wv[ds] : 1.0) : 0.0;
  const double* mg = means + ((size_t)d * Ge + (g >= 0 ? g : 0)) * (K + 1);
#pragma unroll
  for (int i = 0; i < GR_NR; ++i) {
    const int r = (int)(threadIdx.x / GR_KT) + GR_RS * i;
    double v = 0.0;
    if (g >= 0 && r <= K) v = (r < K ? xv[((size_t)r * D + d) * (size_t)S + s] : yv[ds]) - mg[r];
    cv[i] = v;
  }
}

// gram [P][D][C][C], plane of split p at p * D + d
__global__ __launch_bounds__(GR_THREADS) void k_xr_gram(const double* __restrict__ xv, const double* __restrict__ yv,
                                                        const double* __restrict__ wv,
                                                        const int32_t* __restrict__ ugrp,
                                                        const double* __restrict__ means, int K, int D, int S, int Ge,
                                                        int split_stocks, double* __restrict__ gram) {
  __shared__ double tile[GR_B * GR_STR];
  __shared__ double wts[GR_KT];
  __shared__ double red[GR_NT * 256];
  const int d = blockIdx.x, p = blockIdx.y;
  const int C = K + 1;
  const int sbeg = (int)min((long long)p * split_stocks, (long long)S);
  const int send = (int)min((long long)sbeg + split_stocks, (long long)S);
  gram_block<true>(
      C, sbeg, send,
      [&](int k0, double(&cv)[GR_NR], double& wt) {
        xr_load(xv, yv, wv, ugrp, means, K, D, d, S, send, Ge, k0, cv, wt);
      },
      tile, wts, red, gram + ((size_t)p * D + d) * (size_t)C * C);
}

__global__ __launch_bounds__(WAVE) void k_xr_solve(const double* __restrict__ gram_all, int P, int K, int D,
                                                   int min_obs, const double* __restrict__ dayinfo,
                                                   double* __restrict__ beta, double* __restrict__ tstat,
                                                   double* __restrict__ r2, int32_t* __restrict__ nout,
                                                   int32_t* __restrict__ dofout, int32_t* __restrict__ status) {
  __shared__ double A[GR_B * GR_LS];
  __shared__ double bb[GR_B];
  __shared__ double sc[GR_B];
  __shared__ int flag;
  const int d = blockIdx.x, t = threadIdx.x;
  const int C = K + 1;
  const size_t plane = (size_t)C * C;
  const double* info = dayinfo + (size_t)d * (C + 4);
  const double nd = info[0], gne = info[1], between = info[2];
  const int n = (int)nd, dof = n - K - (int)gne;
  int stat = (n < (min_obs > 1 ? min_obs : 1) || dof < 1) ? 1 : 0;
  if (t == 0) flag = 0;
  if (stat == 0) {
    for (int e = t; e < (int)plane; e += WAVE) {
      double s = 0.0;
      for (int p = 0; p < P; ++p) s += gram_all[((size_t)p * D + d) * plane + e];  // plane order
      const int i = e / C, j = e - i * C;
      if (j < K && i < K) A[i * GR_LS + j] = s;
      if (j == K) bb[i] = s;  // bb[K] = T
    }
  }
  __syncthreads();
  double T = 0.0, rawy = 0.0;
  if (stat == 0) {
    T = bb[K];
    rawy = info[4 + K];
    if (t < K) {
      const double mjj = A[t * GR_LS + t];
      if (!(mjj > XR_CONST_REL * info[4 + t])) flag = 1;  // constant within industries (or not finite)
      sc[t] = 1.0 / sqrt(mjj);
    }
  }
  __syncthreads();
  if (stat == 0 && flag) stat = 2;
  const bool yconst = !(T > XR_CONST_REL * rawy);  // the regressand itself: an exact fit, beta = 0
  if (stat == 0) {
    for (int e = t; e < K * K; e += WAVE) {
      const int i = e / K, j = e - i * K;
      A[i * GR_LS + j] *= sc[i] * sc[j];
    }
    if (t < K) bb[t] = yconst ? 0.0 : bb[t] * sc[t];
    __syncthreads();
    if (!chol_lower(A, K, t, CHOL_PIVOT_MIN)) stat = 2;
  }
  double bj = qnan(), tj = qnan(), r2v = qnan();
  if (stat == 0) {
    // L z = b, then L^T beta~ = z, both in bb
    for (int k = 0; k < K; ++k) {
      const double zk = bb[k] / A[k * GR_LS + k];
      __syncthreads();
      if (t == k) bb[k] = zk;
      if (t > k && t < K) bb[t] -= A[t * GR_LS + k] * zk;
      __syncthreads();
    }
    double zz = t < K ? bb[t] * bb[t] : 0.0;  // b^T beta = z^T z
    const double btb = wsum(zz);
    for (int k = K - 1; k >= 0; --k) {
      const double xk = bb[k] / A[k * GR_LS + k];
      __syncthreads();
      if (t == k) bb[k] = xk;
      if (t < k) bb[t] -= A[k * GR_LS + t] * xk;
      __syncthreads();
    }
    const double inv = chol_inv_column(A, K, t);  // (M~^-1)_tt
    const double Tz = yconst ? 0.0 : T;
    double rss = Tz - btb;
    if (!(rss > 0.0)) rss = 0.0;
    const double sigma2 = rss / (double)dof;
    if (t < K) {
      bj = bb[t] * sc[t];
      const double se = sqrt(sigma2 * inv * sc[t] * sc[t]);
      tj = se == 0.0 ? qnan() : bj / se;
    }
    const double den = Tz + between;
    r2v = den > XR_CONST_REL * rawy ? 1.0 - rss / den : qnan();
  }
  if (t < K) {
    beta[(size_t)d * K + t] = bj;
    tstat[(size_t)d * K + t] = tj;
  }
  if (t == 0) {
    r2[d] = r2v;
    nout[d] = n;
    dofout[d] = dof;
    status[d] = stat;
  }
}

__global__ __launch_bounds__(256) void k_xr_residual(const double* __restrict__ xv, int K, int D, int S,
                                                     const double* __restrict__ yv, const uint8_t* __restrict__ ys,
                                                     const int32_t* __restrict__ ugrp,
                                                     const double* __restrict__ means, int Ge,
                                                     const double* __restrict__ beta,
                                                     const int32_t* __restrict__ status, double* __restrict__ ov,
                                                     uint8_t* __restrict__ os) {
  const int d = blockIdx.x;
  const int s = (int)blockIdx.y * 256 + (int)threadIdx.x;
  if (s >= S) return;
  const size_t ds = (size_t)d * S + s;
  const uint8_t st = ys[ds];
  const int g = ugrp[ds];
  double e = 0.0;
  uint8_t so = st == MFF_STATE_VALUE ? (uint8_t)MFF_STATE_NULL : st;
  if (st == MFF_STATE_VALUE && g >= 0 && status[d] == 0) {
    const double* mg = means + ((size_t)d * Ge + g) * (K + 1);
    e = yv[ds] - mg[K];
    for (int k = 0; k < K; ++k) e -= (xv[((size_t)k * D + d) * (size_t)S + s] - mg[k]) * beta[(size_t)d * K + k];
    so = MFF_STATE_VALUE;
  }
  ov[ds] = e;
  os[ds] = so;
}

// agg [K][6] = (days, mean, std, t_fm, mean |t|, share |t| > 2) over the status-0 days in day
// order (the two t columns over those with a t); overall [2] = (mean r2 over the status-0 days
// with an r2, mean n over the status-0 days).  Thread j < K: factor j; thread K: overall.
__global__ __launch_bounds__(WAVE) void k_xr_mean(const double* __restrict__ beta, const double* __restrict__ tstat,
                                                  const double* __restrict__ r2, const int32_t* __restrict__ n,
                                                  const int32_t* __restrict__ status, int K, int D,
                                                  double* __restrict__ agg, double* __restrict__ overall) {
  const int j = threadIdx.x;
  if (j > K) return;
  if (j == K) {
    double sr = 0.0, sn = 0.0;
    int cr = 0, cn = 0;
    for (int d = 0; d < D; ++d) {
      if (status[d] != 0) continue;
      const double v = r2[d];
      if (v == v) {
        sr += v;
        ++cr;
      }
      sn += (double)n[d];
      ++cn;
    }
    overall[0] = cr > 0 ? sr / cr : qnan();
    overall[1] = cn > 0 ? sn / cn : qnan();
    return;
  }
  double sb = 0.0, sa = 0.0;
  int days = 0, ct = 0, big = 0;
  for (int d0 = 0; d0 < D; d0 += 8) {  // eight days in flight, added in day order
    double b[8], tv[8];
    int ok[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      const bool in = d0 + k < D;
      ok[k] = in && status[in ? d0 + k : 0] == 0;
      b[k] = in ? beta[(size_t)(d0 + k) * K + j] : 0.0;
      tv[k] = in ? tstat[(size_t)(d0 + k) * K + j] : qnan();
    }
#pragma unroll
    for (int k = 0; k < 8; ++k)
      if (ok[k]) {
        sb += b[k];
        ++days;
        if (tv[k] == tv[k]) {
          const double a = fabs(tv[k]);
          sa += a;
          ++ct;
          big += a > 2.0 ? 1 : 0;
        }
      }
  }
  const double mean = days > 0 ? sb / days : qnan();
  double ss = 0.0;
  for (int d0 = 0; d0 < D; d0 += 8) {
    double b[8];
    int ok[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      const bool in = d0 + k < D;
      ok[k] = in && status[in ? d0 + k : 0] == 0;
      b[k] = in ? beta[(size_t)(d0 + k) * K + j] : 0.0;
    }
#pragma unroll
    for (int k = 0; k < 8; ++k)
      if (ok[k]) ss += (b[k] - mean) * (b[k] - mean);
  }
  const double sd = days > 1 ? sqrt(ss / (days - 1)) : qnan();
  double* o = agg + (size_t)j * XR_AGG;
  o[0] = (double)days;
  o[1] = mean;
  o[2] = sd;
  o[3] = (days < 2 || sd == 0.0) ? qnan() : mean / (sd / sqrt((double)days));
  o[4] = ct > 0 ? sa / ct : qnan();
  o[5] = ct > 0 ? (double)big / ct : qnan();
}

static int xr_check(const char* what, int K, int D, int S, int G) {
  if (int rc = xs_check(what, K, XR_MAX_K, D, S)) return rc;
  MFF_REQUIRE(G >= 0 && G <= XR_MAX_G, "%s: G=%d outside [1, %d]", what, G, XR_MAX_G);
  return 0;
}

}  // namespace mff

using namespace mff;

extern "C" {

int mff_xs_reg_max_factors(void) { return XR_MAX_K; }
int mff_xs_reg_max_groups(void) { return XR_MAX_G; }

size_t mff_xs_reg_workspace_bytes(int K, int D, int S, int G) {
  if (K < 1 || D <= 0 || S < 0 || G < 0) return 0;
  return xr_ws_bytes(K, D, S, G > 0 ? G : 1);
}

int mff_xs_reg_groups(const double* x_val, const uint8_t* x_state, int K, int D, int S, const double* y_val,
                      const uint8_t* y_state, const double* weight, const uint8_t* weight_state,
                      const int32_t* group, int G, int nsplit, double* gsums, void* workspace, void* stream) {
  clear_error();
  if (int rc = xr_check("mff_xs_reg_groups", K, D, S, group ? G : 0)) return rc;
  MFF_REQUIRE(nsplit >= 1 && nsplit <= 65535, "mff_xs_reg_groups: nsplit=%d", nsplit);
  MFF_REQUIRE(!group || G >= 1, "mff_xs_reg_groups: G=%d outside [1, %d]", G, XR_MAX_G);
  MFF_REQUIRE((weight == nullptr) == (weight_state == nullptr), "mff_xs_reg_groups: weight without its state");
  if (D == 0) return 0;
  MFF_REQUIRE(gsums && workspace && (S == 0 || (x_val && x_state && y_val && y_state)),
              "mff_xs_reg_groups: NULL buffer");
  const int Ge = group ? G : 1;
  hipStream_t st = as_stream(stream);
  int32_t* ugrp = reinterpret_cast<int32_t*>(reinterpret_cast<char*>(workspace) + xr_ugrp_off(K, D, Ge));
  if (S > 0) {
    hipLaunchKernelGGL(k_xr_mask, dim3((unsigned)D, (unsigned)((S + 255) / 256)), dim3(256), 0, st, x_val, x_state, K,
                       D, S, y_val, y_state, weight, weight_state, group, G, ugrp);
    MFF_LAUNCH_CHECK();
  }
  const int CV = K + 3;
  const int split_stocks = xs_split_stocks(S, nsplit);
  if (Ge <= XR_COL_G)
    hipLaunchKernelGGL(k_xr_groups_col, dim3((unsigned)D, (unsigned)nsplit), dim3(XR_COL_T), 0, st, x_val, K, D, S, y_val,
                       weight, ugrp, Ge, split_stocks, gsums);
  else
    hipLaunchKernelGGL(k_xr_groups, dim3((unsigned)D, (unsigned)((CV + 4 * XR_GC - 1) / (4 * XR_GC)), (unsigned)nsplit),
                       dim3(256), 0, st, x_val, K, D, S, y_val, weight, ugrp, Ge, split_stocks, gsums);
  MFF_LAUNCH_CHECK();
  return 0;
}

int mff_xs_reg_gram(const double* x_val, int K, int D, int S, const double* y_val, const double* weight, int G,
                    const double* gsums_all, int R, int nsplit, double* gram, void* workspace, void* stream) {
  clear_error();
  if (int rc = xr_check("mff_xs_reg_gram", K, D, S, G)) return rc;
  MFF_REQUIRE(R >= 1 && nsplit >= 1 && nsplit <= 65535, "mff_xs_reg_gram: R=%d nsplit=%d", R, nsplit);
  if (D == 0) return 0;
  MFF_REQUIRE(gsums_all && gram && workspace && (S == 0 || (x_val && y_val)), "mff_xs_reg_gram: NULL buffer");
  const int Ge = G > 0 ? G : 1;
  hipStream_t st = as_stream(stream);
  char* ws = reinterpret_cast<char*>(workspace);
  double* dayinfo = reinterpret_cast<double*>(ws);
  double* means = reinterpret_cast<double*>(ws + xr_means_off(K, D));
  const int32_t* ugrp = reinterpret_cast<const int32_t*>(ws + xr_ugrp_off(K, D, Ge));
  hipLaunchKernelGGL(k_xr_means, dim3((unsigned)D), dim3(256), 0, st, gsums_all, R, K, D, Ge,
                     G > 0 ? 0 : 1, means, dayinfo);
  MFF_LAUNCH_CHECK();
  hipLaunchKernelGGL(k_xr_gram, dim3((unsigned)D, (unsigned)nsplit), dim3(GR_THREADS), 0, st, x_val, y_val, weight,
                     ugrp, means, K, D, S, Ge, xs_split_stocks(S, nsplit), gram);
  MFF_LAUNCH_CHECK();
  return 0;
}

int mff_xs_reg_solve(const double* gram_all, int P, int K, int D, int min_obs, double* beta, double* tstat, double* r2,
                     int32_t* n, int32_t* dof, int32_t* status, void* workspace, void* stream) {
  clear_error();
  if (int rc = xr_check("mff_xs_reg_solve", K, D, 0, 0)) return rc;
  MFF_REQUIRE(P >= 1, "mff_xs_reg_solve: P=%d planes", P);
  MFF_REQUIRE(min_obs >= 0, "mff_xs_reg_solve: min_obs=%d below 0", min_obs);
  if (D == 0) return 0;
  MFF_REQUIRE(gram_all && beta && tstat && r2 && n && dof && status && workspace, "mff_xs_reg_solve: NULL buffer");
  hipLaunchKernelGGL(k_xr_solve, dim3((unsigned)D), dim3(WAVE), 0, as_stream(stream), gram_all, P, K, D, min_obs,
                     reinterpret_cast<const double*>(workspace), beta, tstat, r2, n, dof, status);
  MFF_LAUNCH_CHECK();
  return 0;
}

int mff_xs_reg_residual(const double* x_val, int K, int D, int S, const double* y_val, const uint8_t* y_state, int G,
                        const double* beta, const int32_t* status, double* out_val, uint8_t* out_state,
                        void* workspace, void* stream) {
  clear_error();
  if (int rc = xr_check("mff_xs_reg_residual", K, D, S, G)) return rc;
  if (D == 0 || S == 0) return 0;
  MFF_REQUIRE(x_val && y_val && y_state && beta && status && out_val && out_state && workspace,
              "mff_xs_reg_residual: NULL buffer");
  const int Ge = G > 0 ? G : 1;
  char* ws = reinterpret_cast<char*>(workspace);
  hipLaunchKernelGGL(k_xr_residual, dim3((unsigned)D, (unsigned)((S + 255) / 256)), dim3(256), 0, as_stream(stream),
                     x_val, K, D, S, y_val, y_state, reinterpret_cast<const int32_t*>(ws + xr_ugrp_off(K, D, Ge)),
                     reinterpret_cast<const double*>(ws + xr_means_off(K, D)), Ge, beta, status, out_val, out_state);
  MFF_LAUNCH_CHECK();
  return 0;
}

int mff_xs_reg_mean(const double* beta, const double* tstat, const double* r2, const int32_t* n,
                    const int32_t* status, int K, int D, double* agg, double* overall, void* stream) {
  clear_error();
  if (int rc = xr_check("mff_xs_reg_mean", K, D, 0, 0)) return rc;
  MFF_REQUIRE(agg && overall && (D == 0 || (beta && tstat && r2 && n && status)), "mff_xs_reg_mean: NULL buffer");
  hipLaunchKernelGGL(k_xr_mean, dim3(1), dim3(WAVE), 0, as_stream(stream), beta, tstat, r2, n, status, K, D, agg,
                     overall);
  MFF_LAUNCH_CHECK();
  return 0;
}

}  // extern "C"
