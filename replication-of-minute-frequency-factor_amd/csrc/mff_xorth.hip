// mff_xorth.hip — per-day factor orthogonalisation (include/mff.h, mff_xs_orth_*; DESIGN.md
// §12): the K exposure rows of a day are standardised over the listwise usable set and
// mapped to K uncorrelated unit-variance rows, either symmetrically (Loewdin, R^-1/2) or by
// Gram-Schmidt in row order (the inverse Cholesky factor).
//
//   k_xo_sums   one workgroup per (day, stock run): the listwise mask plane u8 [D][S] and the
//               run's (n, sum x_j, sum x_j^2) over U.  32-stock tiles, eight rows per thread;
//               the eight row groups of a stock agree on its mask through LDS; every thread
//               adds its own (row, stock lane) in tile order, the 32 lanes of a row are added
//               in lane order at the end.  Values and states are read once.
//   k_xo_means  the R planes of sums added in plane order -> per-day (n, means, raw squares).
//   k_xo_gram   sum c c^T of the K centred rows: gram_block (mff_gram.h) without the weight
//               operand.
//   k_xo_solve  one workgroup per day: planes added in plane order, R with a unit diagonal,
//               cyclic two-sided Jacobi in LDS (round-robin pairing, up to 32 disjoint
//               rotations per step: (c, s) by one thread per pair, then columns, then rows, a
//               wave per pair and a lane per row), eigenvalue sort, the singular rule, T and
//               keep; for Gram-Schmidt (no eigenvectors kept) chol_lower / chol_inv_column
//               (mff_gram.h) on a second copy of R.
//   k_xo_apply  per (day, 512-stock chunk): out[j][s] = sum_k T'[k][j] c[k][s] as f64 MFMA,
//               factors on the M side (a wave owns 16 output rows and keeps its T' fragments
//               in registers), stocks on the N side (an accumulator row stores 16 consecutive
//               stocks); the states follow the listwise rule.
// Every sum has one fixed order and the rotation order is fixed, so results are bit-identical
// from run to run.
#include <hip/hip_runtime.h>

#include "../../include/mff.h"
#include "mff_gram.h"
#include "mff_internal.h"
#include "mff_wave.h"

namespace mff {

constexpr int XO_MAX_K = 64;
constexpr int XO_SWEEPS = 30;
constexpr int XO_PW = GR_B / 2 / (GR_THREADS / WAVE);  // Jacobi pairs per wave and step (8)
constexpr int XO_AP_STOCKS = 512;   // stocks per workgroup of the apply pass
constexpr double XO_CONST_REL = 1e-20;
constexpr double XO_EIG_MIN = 1e-10;  // the singular rule on the smallest eigenvalue
constexpr double XO_SKIP = 0x1p-52;

__host__ __device__ inline size_t xo_align(size_t b) { return (b + 255) & ~(size_t)255; }
// workspace: dayinfo f64 [D][2K + 1] | T' f64 [D][K][K] | mask u8 [D][S]
__host__ __device__ inline size_t xo_tp_off(int K, int D) { return xo_align((size_t)D * (2 * K + 1) * 8); }
__host__ __device__ inline size_t xo_mask_off(int K, int D) {
  return xo_tp_off(K, D) + xo_align((size_t)D * K * K * 8);
}
__host__ __device__ inline size_t xo_ws_bytes(int K, int D, int S) {
  return xo_mask_off(K, D) + xo_align((size_t)D * S);
}

// sums [nsplit][D][2K + 1] = (n, sum x_0 .. x_{K-1}, sum x_0^2 .. x_{K-1}^2) over U of the run
__global__ __launch_bounds__(GR_THREADS) void k_xo_sums(const double* __restrict__ xv, const uint8_t* __restrict__ xs,
                                                        int K, int D, int S, int split_stocks,
                                                        uint8_t* __restrict__ mask, double* __restrict__ sums) {
  __shared__ uint8_t okf[2][GR_RS][GR_KT];
  __shared__ double red[GR_B * (GR_KT + 1)];
  const int d = blockIdx.x, p = blockIdx.y, t = threadIdx.x;
  const int ls = t & (GR_KT - 1), r0 = t / GR_KT;
  const int sbeg = (int)min((long long)p * split_stocks, (long long)S);
  const int send = (int)min((long long)sbeg + split_stocks, (long long)S);
  double sm[GR_NR], sq[GR_NR], v[GR_NR], cnt = 0.0;
  bool fin = false;
#pragma unroll
  for (int i = 0; i < GR_NR; ++i) sm[i] = sq[i] = v[i] = 0.0;
  auto load = [&](int k0) {
    const int s = k0 + ls;
    fin = s < send;
#pragma unroll
    for (int i = 0; i < GR_NR; ++i) {
      const int r = r0 + GR_RS * i;
      v[i] = 0.0;
      if (s < send && r < K) {
        const size_t off = ((size_t)r * D + d) * (size_t)S + s;
        const double x = xv[off];
        const bool ok = xs_usable(x, xs[off]);
        fin = fin && ok;
        v[i] = ok ? x : 0.0;
      }
    }
  };
  if (sbeg < send) load(sbeg);
  int buf = 0;
  for (int k0 = sbeg; k0 < send; k0 += GR_KT, buf ^= 1) {
    double cur[GR_NR];
#pragma unroll
    for (int i = 0; i < GR_NR; ++i) cur[i] = v[i];
    okf[buf][r0][ls] = fin ? 1 : 0;
    __syncthreads();  // (the other buffer is still being read by the slowest threads of the previous tile)
    bool u = true;
#pragma unroll
    for (int j = 0; j < GR_RS; ++j) u = u && okf[buf][j][ls] != 0;
    if (k0 + GR_KT < send) load(k0 + GR_KT);
    if (u) {
#pragma unroll
      for (int i = 0; i < GR_NR; ++i) {
        sm[i] += cur[i];
        sq[i] += cur[i] * cur[i];
      }
    }
    if (r0 == 0) {
      const int s = k0 + ls;
      if (s < send) mask[(size_t)d * S + s] = u ? 1 : 0;
      cnt += u ? 1.0 : 0.0;
    }
  }
  double* out = sums + ((size_t)p * D + d) * (2 * K + 1);
  // the 32 stock lanes of a row, added in lane order
#pragma unroll
  for (int i = 0; i < GR_NR; ++i) red[(r0 + GR_RS * i) * (GR_KT + 1) + ls] = sm[i];
  __syncthreads();
  if (t < K) {
    double s = 0.0;
    for (int j = 0; j < GR_KT; ++j) s += red[t * (GR_KT + 1) + j];
    out[1 + t] = s;
  }
  __syncthreads();
#pragma unroll
  for (int i = 0; i < GR_NR; ++i) red[(r0 + GR_RS * i) * (GR_KT + 1) + ls] = sq[i];
  __syncthreads();
  if (t < K) {
    double s = 0.0;
    for (int j = 0; j < GR_KT; ++j) s += red[t * (GR_KT + 1) + j];
    out[1 + K + t] = s;
  }
  __syncthreads();
  if (r0 == 0) red[ls] = cnt;
  __syncthreads();
  if (t == 0) {
    double s = 0.0;
    for (int j = 0; j < GR_KT; ++j) s += red[j];
    out[0] = s;
  }
}

// dayinfo [D][2K + 1] = (n, mean_0 .. mean_{K-1}, raw sum x_j^2 ...)
__global__ __launch_bounds__(128) void k_xo_means(const double* __restrict__ sums_all, int R, int K, int D,
                                                  double* __restrict__ dayinfo) {
  const int d = blockIdx.x, W = 2 * K + 1;
  for (int t = threadIdx.x; t < W; t += blockDim.x) {  // (W = 129 entries at K = 64)
    double n = 0.0, s = 0.0;
    for (int r = 0; r < R; ++r) {  // plane order
      const double* p = sums_all + ((size_t)r * D + d) * W;
      n += p[0];
      s += p[t];
    }
    dayinfo[(size_t)d * W + t] = t == 0 ? n : (t <= K ? (n > 0.0 ? s / n : 0.0) : s);
  }
}

// this thread's part of a [64 rows][GR_KT stocks] tile: stock t % GR_KT, rows t / GR_KT + 8 i,
// centred (0 outside U, beyond `send` and in the padding rows)
__device__ __forceinline__ void xo_load(const double* __restrict__ xv, const uint8_t* __restrict__ mask,
                                        const double* __restrict__ mean, int K, int D, int d, int S, int send, int k0,
                                        double (&cv)[GR_NR]) {
  const int s = k0 + (int)(threadIdx.x & (GR_KT - 1));
  const bool u = s < send && mask[(size_t)d * S + s] != 0;
#pragma unroll
  for (int i = 0; i < GR_NR; ++i) {
    const int r = (int)(threadIdx.x / GR_KT) + GR_RS * i;
    cv[i] = (u && r < K) ? xv[((size_t)r * D + d) * (size_t)S + s] - mean[r] : 0.0;
  }
}

// gram [nsplit][D][K][K], plane of run p at p * D + d
__global__ __launch_bounds__(GR_THREADS) void k_xo_gram(const double* __restrict__ xv, const uint8_t* __restrict__ mask,
                                                        const double* __restrict__ dayinfo, int K, int D, int S,
                                                        int split_stocks, double* __restrict__ gram) {
  __shared__ double tile[GR_B * GR_STR];
  __shared__ double red[GR_NT * 256];
  const int d = blockIdx.x, p = blockIdx.y;
  const int sbeg = (int)min((long long)p * split_stocks, (long long)S);
  const int send = (int)min((long long)sbeg + split_stocks, (long long)S);
  const double* mean = dayinfo + (size_t)d * (2 * K + 1) + 1;
  gram_block<false>(
      K, sbeg, send, [&](int k0, double(&cv)[GR_NR], double&) { xo_load(xv, mask, mean, K, D, d, S, send, k0, cv); },
      tile, nullptr, red, gram + ((size_t)p * D + d) * (size_t)K * K);
}

// dst (row stride GR_LS) = the P planes of day d added in plane order
__device__ __forceinline__ void xo_sum_planes(const double* __restrict__ gram_all, int P, int K, int D, int d,
                                              double* dst) {
  const size_t plane = (size_t)K * K;
  for (int e = threadIdx.x; e < (int)plane; e += GR_THREADS) {
    double s = 0.0;
    for (int p = 0; p < P; ++p) s += gram_all[((size_t)p * D + d) * plane + e];
    const int i = e / K, j = e - i * K;
    dst[i * GR_LS + j] = s;
  }
}

// M -> R: unit diagonal, M_ij / sqrt(M_ii M_jj) elsewhere (bitwise symmetric: the planes are)
__device__ __forceinline__ void xo_to_corr(double* dst, const double* dg, int K) {
  for (int e = threadIdx.x; e < K * K; e += GR_THREADS) {
    const int i = e / K, j = e - i * K;
    dst[i * GR_LS + j] = i == j ? 1.0 : dst[i * GR_LS + j] / sqrt(dg[i] * dg[j]);
  }
}

__global__ __launch_bounds__(GR_THREADS) void k_xo_solve(const double* __restrict__ gram_all, int P, int K, int D,
                                                         int method, int min_obs, const double* __restrict__ dayinfo,
                                                         double* __restrict__ tprime, double* __restrict__ transform,
                                                         double* __restrict__ eig, double* __restrict__ keep,
                                                         int32_t* __restrict__ nout, int32_t* __restrict__ status) {
  __shared__ double A[GR_B * GR_LS];
  __shared__ double V[GR_B * GR_LS];
  __shared__ double dg[GR_B];   // M_jj
  __shared__ double lam[GR_B];  // eigenvalues in Jacobi order
  __shared__ double es[GR_B];   // ... ascending
  __shared__ double isq[GR_B];  // 1 / sqrt(lam)
  __shared__ double kp[GR_B];
  __shared__ double rc[GR_B / 2], rs[GR_B / 2];
  __shared__ int rp[GR_B / 2], rq[GR_B / 2];
  __shared__ int flag;
  const int d = blockIdx.x, t = threadIdx.x;
  const double* info = dayinfo + (size_t)d * (2 * K + 1);
  const int n = (int)info[0];
  int stat = n < (min_obs > K + 1 ? min_obs : K + 1) ? 1 : 0;
  if (t == 0) flag = 0;
  if (stat == 0) xo_sum_planes(gram_all, P, K, D, d, A);
  __syncthreads();
  if (stat == 0 && t < K) {
    const double mjj = A[t * GR_LS + t];
    if (!(mjj > XO_CONST_REL * info[1 + K + t])) flag = 1;  // constant on U (or not finite)
    dg[t] = mjj;
  }
  __syncthreads();
  if (stat == 0 && flag) stat = 2;
  if (stat == 0) {
    xo_to_corr(A, dg, K);
    for (int e = t; e < K * K; e += GR_THREADS) {
      const int i = e / K, j = e - i * K;
      V[i * GR_LS + j] = i == j ? 1.0 : 0.0;
    }
  }
  __syncthreads();

  if (stat == 0) {
    // cyclic two-sided Jacobi; round-robin over Kp indices (index Kp - 1 fixed, the others rotate).
    // A[l][p] and A[p][l] come from rotations applied in different orders, so A is symmetric only
    // to rounding during the sweeps: the upper entry A[p][q], p < q, alone drives (c, s) and the
    // skip test, and the eigenvalues are read off the diagonal.
    const int Kp = K + (K & 1), m = Kp / 2, ring = Kp - 1;
    const int w = t >> 6, l = t & 63;
    bool conv = false;
    for (int sweep = 0; sweep < XO_SWEEPS && !conv; ++sweep) {
      int rotated = 0;
      for (int r = 0; r < ring; ++r) {
        int rot = 0;
        if (t < m) {
          int p_ = t == 0 ? ring : (r + t) % ring;
          int q_ = t == 0 ? r : (r + ring - t) % ring;
          if (p_ > q_) {
            const int x = p_;
            p_ = q_;
            q_ = x;
          }
          double c = 1.0, s = 0.0;
          if (q_ < K) {
            const double apq = A[p_ * GR_LS + q_], app = A[p_ * GR_LS + p_], aqq = A[q_ * GR_LS + q_];
            if (fabs(apq) > XO_SKIP * sqrt(fabs(app * aqq))) {
              const double theta = (aqq - app) / (2.0 * apq);
              const double tt = copysign(1.0, theta) / (fabs(theta) + sqrt(theta * theta + 1.0));
              c = 1.0 / sqrt(tt * tt + 1.0);
              s = tt * c;
              rot = s != 0.0 ? 1 : 0;
            }
          }
          rp[t] = p_;
          rq[t] = q_;
          rc[t] = c;
          rs[t] = rot ? s : 0.0;
        }
        if (!__syncthreads_or(rot)) continue;
        rotated = 1;
        // a wave per pair, a lane per row / column; every load of a phase is issued before its
        // first store (the pairs of a step are disjoint), so the LDS round trips overlap
        double cc[XO_PW], ss[XO_PW], ap[XO_PW], aq[XO_PW], vp[XO_PW], vq[XO_PW];
        int pi[XO_PW], qi[XO_PW];
#pragma unroll
        for (int i = 0; i < XO_PW; ++i) {  // columns p, q of A and V
          const int pr = w + (GR_THREADS / WAVE) * i;
          ss[i] = (pr < m && l < K) ? rs[pr] : 0.0;
          cc[i] = pr < m ? rc[pr] : 1.0;
          pi[i] = pr < m ? rp[pr] : 0;
          qi[i] = pr < m ? rq[pr] : 0;
          if (ss[i] != 0.0) {
            ap[i] = A[l * GR_LS + pi[i]];
            aq[i] = A[l * GR_LS + qi[i]];
            if (method == 0) {  // (Gram-Schmidt needs the eigenvalues only)
              vp[i] = V[l * GR_LS + pi[i]];
              vq[i] = V[l * GR_LS + qi[i]];
            }
          }
        }
#pragma unroll
        for (int i = 0; i < XO_PW; ++i) {
          if (ss[i] != 0.0) {
            A[l * GR_LS + pi[i]] = cc[i] * ap[i] - ss[i] * aq[i];
            A[l * GR_LS + qi[i]] = ss[i] * ap[i] + cc[i] * aq[i];
            if (method == 0) {
              V[l * GR_LS + pi[i]] = cc[i] * vp[i] - ss[i] * vq[i];
              V[l * GR_LS + qi[i]] = ss[i] * vp[i] + cc[i] * vq[i];
            }
          }
        }
        __syncthreads();
#pragma unroll
        for (int i = 0; i < XO_PW; ++i) {  // rows p, q of A
          if (ss[i] != 0.0) {
            ap[i] = A[pi[i] * GR_LS + l];
            aq[i] = A[qi[i] * GR_LS + l];
          }
        }
#pragma unroll
        for (int i = 0; i < XO_PW; ++i) {  // ... the rotated entry is exactly 0
          if (ss[i] != 0.0) {
            A[pi[i] * GR_LS + l] = l == qi[i] ? 0.0 : cc[i] * ap[i] - ss[i] * aq[i];
            A[qi[i] * GR_LS + l] = l == pi[i] ? 0.0 : ss[i] * ap[i] + cc[i] * aq[i];
          }
        }
        __syncthreads();
      }
      conv = rotated == 0;
    }
    if (!conv) stat = 2;
  }

  if (stat == 0) {
    if (t < K) lam[t] = A[t * GR_LS + t];
    __syncthreads();
    if (t < K) {
      const double me = lam[t];
      int rank = 0;
      for (int j = 0; j < K; ++j) rank += (lam[j] < me || (lam[j] == me && j < t)) ? 1 : 0;
      es[rank] = me;
      isq[t] = 1.0 / sqrt(me);
    }
    __syncthreads();
    if (!(es[0] > XO_EIG_MIN)) stat = 2;
  }

  if (stat == 0 && method == 0) {
    if (t < K) {
      double s = 0.0;
      for (int k = 0; k < K; ++k) s += V[t * GR_LS + k] * V[t * GR_LS + k] * sqrt(lam[k]);
      kp[t] = s;
    }
    for (int e = t; e < K * K; e += GR_THREADS) {  // T = V diag(lam^-1/2) V^T, k order, mirrored
      const int i = e / K, j = e - i * K;
      if (i > j) continue;
      double s = 0.0;
      for (int k = 0; k < K; ++k) s += V[i * GR_LS + k] * V[j * GR_LS + k] * isq[k];
      A[i * GR_LS + j] = A[j * GR_LS + i] = s;
    }
  }
  if (stat == 0 && method == 1) {
    __syncthreads();
    xo_sum_planes(gram_all, P, K, D, d, V);
    __syncthreads();
    xo_to_corr(V, dg, K);
    __syncthreads();
    if (!chol_lower(V, K, t, CHOL_PIVOT_MIN)) stat = 2;
    if (stat == 0) {
      chol_inv_column(V, K, t);
      __syncthreads();
      if (t < K) kp[t] = V[t * GR_LS + t];
      for (int e = t; e < K * K; e += GR_THREADS) {  // T = L^-T
        const int i = e / K, j = e - i * K;
        A[i * GR_LS + j] = i < j ? V[i * GR_LS + j] : (i == j ? 1.0 / V[i * GR_LS + i] : 0.0);
      }
    }
  }
  __syncthreads();

  const double nm1 = (double)(n - 1);
  for (int e = t; e < K * K; e += GR_THREADS) {
    const int i = e / K, j = e - i * K;
    const double tv = stat == 0 ? A[i * GR_LS + j] : qnan();
    transform[(size_t)d * K * K + e] = tv;
    tprime[(size_t)d * K * K + e] = stat == 0 ? tv / sqrt(dg[i] / nm1) : 0.0;
  }
  if (t < K) {
    eig[(size_t)d * K + t] = stat == 0 ? es[t] : qnan();
    keep[(size_t)d * K + t] = stat == 0 ? kp[t] : qnan();
  }
  if (t == 0) {
    nout[d] = n;
    status[d] = stat;
  }
}

__global__ __launch_bounds__(GR_THREADS) void k_xo_apply(const double* __restrict__ xv, const uint8_t* __restrict__ xs,
                                                         const uint8_t* __restrict__ mask,
                                                         const double* __restrict__ dayinfo,
                                                         const double* __restrict__ tprime,
                                                         const int32_t* __restrict__ status, int K, int D, int S,
                                                         double* __restrict__ ov, uint8_t* __restrict__ os) {
  __shared__ double tile[GR_B * GR_STR];
  const int d = blockIdx.x;
  const int sbeg = (int)min((long long)blockIdx.y * XO_AP_STOCKS, (long long)S);
  const int send = (int)min((long long)sbeg + XO_AP_STOCKS, (long long)S);
  const int t = threadIdx.x, l = t & 63, w = t >> 6;
  const int r = l & 15, kq = l >> 4;
  const int ls = t & (GR_KT - 1), r0 = t / GR_KT;
  const bool ok = status[d] == 0;
  const int nt = (K + 15) / 16, nk = (K + 3) / 4;
  const double* mean = dayinfo + (size_t)d * (2 * K + 1) + 1;
  const double* tp = tprime + (size_t)d * K * K;
  // this wave's T' fragments: output rows 16 w .. 16 w + 15, every k step
  double af[GR_B / 4];
#pragma unroll
  for (int st = 0; st < GR_B / 4; ++st) {
    const int k = 4 * st + kq, j = 16 * w + r;
    af[st] = (ok && k < K && j < K) ? tp[(size_t)k * K + j] : 0.0;
  }
  double cv[GR_NR];
  uint8_t so[GR_NR];
  auto load = [&](int k0) {
    const int s = k0 + ls;
    const bool in = s < send;
    const bool u = in && ok && mask[(size_t)d * S + s] != 0;
#pragma unroll
    for (int i = 0; i < GR_NR; ++i) {
      const int rr = r0 + GR_RS * i;
      cv[i] = 0.0;
      so[i] = MFF_STATE_ABSENT;
      if (in && rr < K) {
        const size_t off = ((size_t)rr * D + d) * (size_t)S + s;
        const uint8_t st = xs[off];
        so[i] = st == MFF_STATE_VALUE ? (u ? (uint8_t)MFF_STATE_VALUE : (uint8_t)MFF_STATE_NULL) : st;
        if (u) cv[i] = xv[off] - mean[rr];
      }
    }
  };
  if (sbeg < send) load(sbeg);
  for (int k0 = sbeg; k0 < send; k0 += GR_KT) {
    __syncthreads();  // the previous tile's reads are done
#pragma unroll
    for (int i = 0; i < GR_NR; ++i) {
      const int rr = r0 + GR_RS * i;
      tile[rr * GR_STR + ls] = cv[i];
      if (rr < K && k0 + ls < send) os[((size_t)rr * D + d) * (size_t)S + k0 + ls] = so[i];
    }
    __syncthreads();
    if (k0 + GR_KT < send) load(k0 + GR_KT);
    if (w >= nt) continue;  // (wave-uniform: output rows beyond ceil(K / 16) tiles)
    v4d acc[2] = {v4d{0.0, 0.0, 0.0, 0.0}, v4d{0.0, 0.0, 0.0, 0.0}};
#pragma unroll
    for (int st = 0; st < GR_B / 4; ++st) {
      if (st < nk) {
        const double b0 = tile[(4 * st + kq) * GR_STR + r], b1 = tile[(4 * st + kq) * GR_STR + 16 + r];
        acc[0] = __builtin_amdgcn_mfma_f64_16x16x4f64(af[st], b0, acc[0], 0, 0, 0);
        acc[1] = __builtin_amdgcn_mfma_f64_16x16x4f64(af[st], b1, acc[1], 0, 0, 0);
      }
    }
#pragma unroll
    for (int h = 0; h < 2; ++h)
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int j = 16 * w + kq + 4 * q, s = k0 + 16 * h + r;
        if (j < K && s < send) ov[((size_t)j * D + d) * (size_t)S + s] = acc[h][q];
      }
  }
}

static int xo_check(const char* what, int K, int D, int S) { return xs_check(what, K, XO_MAX_K, D, S); }

}  // namespace mff

using namespace mff;

extern "C" {

int mff_xs_orth_max_factors(void) { return XO_MAX_K; }

size_t mff_xs_orth_workspace_bytes(int K, int D, int S) {
  if (K < 1 || D <= 0 || S < 0) return 0;
  return xo_ws_bytes(K, D, S);
}

int mff_xs_orth_sums(const double* x_val, const uint8_t* x_state, int K, int D, int S, int nsplit, double* sums,
                     void* workspace, void* stream) {
  clear_error();
  if (int rc = xo_check("mff_xs_orth_sums", K, D, S)) return rc;
  MFF_REQUIRE(nsplit >= 1 && nsplit <= 65535, "mff_xs_orth_sums: nsplit=%d", nsplit);
  if (D == 0) return 0;
  MFF_REQUIRE(sums && workspace && (S == 0 || (x_val && x_state)), "mff_xs_orth_sums: NULL buffer");
  uint8_t* mask = reinterpret_cast<uint8_t*>(workspace) + xo_mask_off(K, D);
  hipLaunchKernelGGL(k_xo_sums, dim3((unsigned)D, (unsigned)nsplit), dim3(GR_THREADS), 0, as_stream(stream), x_val,
                     x_state, K, D, S, xs_split_stocks(S, nsplit), mask, sums);
  MFF_LAUNCH_CHECK();
  return 0;
}

int mff_xs_orth_gram(const double* x_val, int K, int D, int S, const double* sums_all, int R, int nsplit, double* gram,
                     void* workspace, void* stream) {
  clear_error();
  if (int rc = xo_check("mff_xs_orth_gram", K, D, S)) return rc;
  MFF_REQUIRE(R >= 1 && nsplit >= 1 && nsplit <= 65535, "mff_xs_orth_gram: R=%d nsplit=%d", R, nsplit);
  if (D == 0) return 0;
  MFF_REQUIRE(sums_all && gram && workspace && (S == 0 || x_val), "mff_xs_orth_gram: NULL buffer");
  hipStream_t st = as_stream(stream);
  char* ws = reinterpret_cast<char*>(workspace);
  double* dayinfo = reinterpret_cast<double*>(ws);
  hipLaunchKernelGGL(k_xo_means, dim3((unsigned)D), dim3(128), 0, st, sums_all, R, K, D, dayinfo);
  MFF_LAUNCH_CHECK();
  hipLaunchKernelGGL(k_xo_gram, dim3((unsigned)D, (unsigned)nsplit), dim3(GR_THREADS), 0, st, x_val,
                     reinterpret_cast<const uint8_t*>(ws + xo_mask_off(K, D)), dayinfo, K, D, S,
                     xs_split_stocks(S, nsplit), gram);
  MFF_LAUNCH_CHECK();
  return 0;
}

int mff_xs_orth_solve(const double* gram_all, int P, int K, int D, int method, int min_obs, double* transform,
                      double* eig, double* keep, int32_t* n, int32_t* status, void* workspace, void* stream) {
  clear_error();
  if (int rc = xo_check("mff_xs_orth_solve", K, D, 0)) return rc;
  MFF_REQUIRE(P >= 1, "mff_xs_orth_solve: P=%d planes", P);
  MFF_REQUIRE(method == 0 || method == 1, "mff_xs_orth_solve: method=%d (0 symmetric, 1 Gram-Schmidt)", method);
  MFF_REQUIRE(min_obs >= 0, "mff_xs_orth_solve: min_obs=%d below 0", min_obs);
  if (D == 0) return 0;
  MFF_REQUIRE(gram_all && transform && eig && keep && n && status && workspace, "mff_xs_orth_solve: NULL buffer");
  char* ws = reinterpret_cast<char*>(workspace);
  hipLaunchKernelGGL(k_xo_solve, dim3((unsigned)D), dim3(GR_THREADS), 0, as_stream(stream), gram_all, P, K, D, method,
                     min_obs, reinterpret_cast<const double*>(ws), reinterpret_cast<double*>(ws + xo_tp_off(K, D)),
                     transform, eig, keep, n, status);
  MFF_LAUNCH_CHECK();
  return 0;
}

int mff_xs_orth_apply(const double* x_val, const uint8_t* x_state, int K, int D, int S, const int32_t* status,
                      double* out_val, uint8_t* out_state, void* workspace, void* stream) {
  clear_error();
  if (int rc = xo_check("mff_xs_orth_apply", K, D, S)) return rc;
  if (D == 0 || S == 0) return 0;
  MFF_REQUIRE(x_val && x_state && status && out_val && out_state && workspace, "mff_xs_orth_apply: NULL buffer");
  const char* ws = reinterpret_cast<const char*>(workspace);
  hipLaunchKernelGGL(k_xo_apply, dim3((unsigned)D, (unsigned)((S + XO_AP_STOCKS - 1) / XO_AP_STOCKS)),
                     dim3(GR_THREADS), 0, as_stream(stream), x_val, x_state,
                     reinterpret_cast<const uint8_t*>(ws + xo_mask_off(K, D)), reinterpret_cast<const double*>(ws),
                     reinterpret_cast<const double*>(ws + xo_tp_off(K, D)), status, K, D, S, out_val, out_state);
  MFF_LAUNCH_CHECK();
  return 0;
}

}  // extern "C"
