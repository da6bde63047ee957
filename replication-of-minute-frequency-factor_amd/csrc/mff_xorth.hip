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
//   k_xo_gram   the tile scheme of k_xr_gram (mff_xreg.hip) without the weight operand:
//               sum c c^T of the K centred rows on v_mfma_f64_16x16x4_f64, stride-34 LDS tile,
//               the next tile in registers before the MFMAs, lower block triangle, the four
//               waves' partial sums added in wave order, mirrored once.
//   k_xo_solve  one workgroup per day: planes added in plane order, R with a unit diagonal,
//               cyclic two-sided Jacobi in LDS (round-robin pairing, up to 32 disjoint
//               rotations per step: (c, s) by one thread per pair, then columns, then rows, a
//               wave per pair and a lane per row), eigenvalue sort, the singular rule, T and
//               keep; for Gram-Schmidt (no eigenvectors kept) the Cholesky / L^-1 of k_xr_solve
//               on a second copy of R.
//   k_xo_apply  per (day, 512-stock chunk): out[j][s] = sum_k T'[k][j] c[k][s] as f64 MFMA,
//               factors on the M side (a wave owns 16 output rows and keeps its T' fragments
//               in registers), stocks on the N side (an accumulator row stores 16 consecutive
//               stocks); the states follow the listwise rule.
// Every sum has one fixed order and the rotation order is fixed, so results are bit-identical
// from run to run.
#include <hip/hip_runtime.h>

#include "../../include/mff.h"
#include "mff_internal.h"
#include "mff_wave.h"

namespace mff {

constexpr int XO_MAX_K = 64;
constexpr int XO_B = 64;            // padded rows of the Gram block
constexpr int XO_KT = 32;           // stocks per LDS tile
constexpr int XO_STR = XO_KT + 2;   // row stride of the tile (doubles)
constexpr int XO_THREADS = 256;
constexpr int XO_NR = XO_B * XO_KT / XO_THREADS;  // rows per thread (8)
constexpr int XO_RS = XO_THREADS / XO_KT;         // row step (8)
constexpr int XO_NT = 10;           // tiles on or below the block diagonal
constexpr int XO_LS = XO_B + 1;     // row stride of the solve's matrices
constexpr int XO_SWEEPS = 30;
constexpr int XO_PW = XO_B / 2 / (XO_THREADS / WAVE);  // Jacobi pairs per wave and step (8)
constexpr int XO_AP_STOCKS = 512;   // stocks per workgroup of the apply pass
constexpr double XO_CONST_REL = 1e-20;
constexpr double XO_EIG_MIN = 1e-10;
constexpr double XO_SKIP = 0x1p-52;

typedef double xo_v4d __attribute__((ext_vector_type(4)));

__host__ __device__ inline size_t xo_align(size_t b) { return (b + 255) & ~(size_t)255; }
// workspace: dayinfo f64 [D][2K + 1] | T' f64 [D][K][K] | mask u8 [D][S]
__host__ __device__ inline size_t xo_tp_off(int K, int D) { return xo_align((size_t)D * (2 * K + 1) * 8); }
__host__ __device__ inline size_t xo_mask_off(int K, int D) {
  return xo_tp_off(K, D) + xo_align((size_t)D * K * K * 8);
}
__host__ __device__ inline size_t xo_ws_bytes(int K, int D, int S) {
  return xo_mask_off(K, D) + xo_align((size_t)D * S);
}

__device__ __forceinline__ bool xo_fin(double x, uint8_t s) { return s == MFF_STATE_VALUE && __builtin_isfinite(x); }

// sums [nsplit][D][2K + 1] = (n, sum x_0 .. x_{K-1}, sum x_0^2 .. x_{K-1}^2) over U of the run
__global__ __launch_bounds__(XO_THREADS) void k_xo_sums(const double* __restrict__ xv, const uint8_t* __restrict__ xs,
                                                        int K, int D, int S, int split_stocks,
                                                        uint8_t* __restrict__ mask, double* __restrict__ sums) {
  __shared__ uint8_t okf[2][XO_RS][XO_KT];
  __shared__ double red[XO_B * (XO_KT + 1)];
  const int d = blockIdx.x, p = blockIdx.y, t = threadIdx.x;
  const int ls = t & (XO_KT - 1), r0 = t / XO_KT;
  const int sbeg = (int)min((long long)p * split_stocks, (long long)S);
  const int send = (int)min((long long)sbeg + split_stocks, (long long)S);
  double sm[XO_NR], sq[XO_NR], v[XO_NR], cnt = 0.0;
  bool fin = false;
#pragma unroll
  for (int i = 0; i < XO_NR; ++i) sm[i] = sq[i] = v[i] = 0.0;
  auto load = [&](int k0) {
    const int s = k0 + ls;
    fin = s < send;
#pragma unroll
    for (int i = 0; i < XO_NR; ++i) {
      const int r = r0 + XO_RS * i;
      v[i] = 0.0;
      if (s < send && r < K) {
        const size_t off = ((size_t)r * D + d) * (size_t)S + s;
        const double x = xv[off];
        const bool ok = xo_fin(x, xs[off]);
        fin = fin && ok;
        v[i] = ok ? x : 0.0;
      }
    }
  };
  if (sbeg < send) load(sbeg);
  int buf = 0;
  for (int k0 = sbeg; k0 < send; k0 += XO_KT, buf ^= 1) {
    double cur[XO_NR];
#pragma unroll
    for (int i = 0; i < XO_NR; ++i) cur[i] = v[i];
    okf[buf][r0][ls] = fin ? 1 : 0;
    __syncthreads();  // (the other buffer is still being read by the slowest threads of the previous tile)
    bool u = true;
#pragma unroll
    for (int j = 0; j < XO_RS; ++j) u = u && okf[buf][j][ls] != 0;
    if (k0 + XO_KT < send) load(k0 + XO_KT);
    if (u) {
#pragma unroll
      for (int i = 0; i < XO_NR; ++i) {
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
  for (int i = 0; i < XO_NR; ++i) red[(r0 + XO_RS * i) * (XO_KT + 1) + ls] = sm[i];
  __syncthreads();
  if (t < K) {
    double s = 0.0;
    for (int j = 0; j < XO_KT; ++j) s += red[t * (XO_KT + 1) + j];
    out[1 + t] = s;
  }
  __syncthreads();
#pragma unroll
  for (int i = 0; i < XO_NR; ++i) red[(r0 + XO_RS * i) * (XO_KT + 1) + ls] = sq[i];
  __syncthreads();
  if (t < K) {
    double s = 0.0;
    for (int j = 0; j < XO_KT; ++j) s += red[t * (XO_KT + 1) + j];
    out[1 + K + t] = s;
  }
  __syncthreads();
  if (r0 == 0) red[ls] = cnt;
  __syncthreads();
  if (t == 0) {
    double s = 0.0;
    for (int j = 0; j < XO_KT; ++j) s += red[j];
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

// this thread's part of a [64 rows][XO_KT stocks] tile: stock t % XO_KT, rows t / XO_KT + 8 i,
// centred (0 outside U, beyond `send` and in the padding rows)
__device__ __forceinline__ void xo_load(const double* __restrict__ xv, const uint8_t* __restrict__ mask,
                                        const double* __restrict__ mean, int K, int D, int d, int S, int send, int k0,
                                        double (&cv)[XO_NR]) {
  const int s = k0 + (int)(threadIdx.x & (XO_KT - 1));
  const bool u = s < send && mask[(size_t)d * S + s] != 0;
#pragma unroll
  for (int i = 0; i < XO_NR; ++i) {
    const int r = (int)(threadIdx.x / XO_KT) + XO_RS * i;
    cv[i] = (u && r < K) ? xv[((size_t)r * D + d) * (size_t)S + s] - mean[r] : 0.0;
  }
}

// the 10 tiles (row, col) on or below the block diagonal
__host__ __device__ constexpr int xo_tr(int i) { return i < 1 ? 0 : i < 3 ? 1 : i < 6 ? 2 : 3; }
__host__ __device__ constexpr int xo_tc(int i) { return i < 1 ? 0 : i < 3 ? i - 1 : i < 6 ? i - 3 : i - 6; }

// gram [nsplit][D][K][K], plane of run p at p * D + d
__global__ __launch_bounds__(XO_THREADS) void k_xo_gram(const double* __restrict__ xv, const uint8_t* __restrict__ mask,
                                                        const double* __restrict__ dayinfo, int K, int D, int S,
                                                        int split_stocks, double* __restrict__ gram) {
  __shared__ double tile[XO_B * XO_STR];
  __shared__ double red[XO_NT * 256];
  const int d = blockIdx.x, p = blockIdx.y;
  const int t = threadIdx.x, l = t & 63, w = t >> 6;
  const int nt = (K + 15) / 16;
  const int sbeg = (int)min((long long)p * split_stocks, (long long)S);
  const int send = (int)min((long long)sbeg + split_stocks, (long long)S);
  const int r = l & 15, kq = l >> 4;
  const double* mean = dayinfo + (size_t)d * (2 * K + 1) + 1;
  double cv[XO_NR];
  xo_v4d acc[XO_NT];
#pragma unroll
  for (int i = 0; i < XO_NT; ++i) acc[i] = xo_v4d{0.0, 0.0, 0.0, 0.0};

  if (sbeg < send) xo_load(xv, mask, mean, K, D, d, S, send, sbeg, cv);
  for (int k0 = sbeg; k0 < send; k0 += XO_KT) {
    __syncthreads();  // the previous tile's reads are done
    {
      const int ls = t & (XO_KT - 1);
#pragma unroll
      for (int i = 0; i < XO_NR; ++i) tile[((t / XO_KT) + XO_RS * i) * XO_STR + ls] = cv[i];
    }
    __syncthreads();
    if (k0 + XO_KT < send) xo_load(xv, mask, mean, K, D, d, S, send, k0 + XO_KT, cv);
#pragma unroll
    for (int kk = 0; kk < 2; ++kk) {
      const int k = (2 * w + kk) * 4 + kq;
      double a[4];
#pragma unroll
      for (int c = 0; c < 4; ++c) a[c] = tile[(16 * c + r) * XO_STR + k];
#pragma unroll
      for (int i = 0; i < XO_NT; ++i)
        if (xo_tr(i) < nt) acc[i] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[xo_tr(i)], a[xo_tc(i)], acc[i], 0, 0, 0);
    }
  }

  for (int ww = 0; ww < 4; ++ww) {  // wave order
    if (w == ww) {
#pragma unroll
      for (int i = 0; i < XO_NT; ++i)
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          double* e = &red[i * 256 + q * 64 + l];
          *e = ww == 0 ? acc[i][q] : *e + acc[i][q];
        }
    }
    __syncthreads();
  }
  double* out = gram + ((size_t)p * D + d) * (size_t)K * K;
  for (int e = t; e < XO_NT * 256; e += XO_THREADS) {
    const int ti = e >> 8, q = (e >> 6) & 3, ll = e & 63;
    int tr = 0, tc = 0;
    for (int i = 0; i < XO_NT; ++i)
      if (i == ti) {
        tr = xo_tr(i);
        tc = xo_tc(i);
      }
    const int i = 16 * tr + (ll >> 4) + 4 * q, j = 16 * tc + (ll & 15);
    if (i >= K || j > i) continue;
    out[(size_t)i * K + j] = out[(size_t)j * K + i] = red[e];
  }
}

// dst (row stride XO_LS) = the P planes of day d added in plane order
__device__ __forceinline__ void xo_sum_planes(const double* __restrict__ gram_all, int P, int K, int D, int d,
                                              double* dst) {
  const size_t plane = (size_t)K * K;
  for (int e = threadIdx.x; e < (int)plane; e += XO_THREADS) {
    double s = 0.0;
    for (int p = 0; p < P; ++p) s += gram_all[((size_t)p * D + d) * plane + e];
    const int i = e / K, j = e - i * K;
    dst[i * XO_LS + j] = s;
  }
}

// M -> R: unit diagonal, M_ij / sqrt(M_ii M_jj) elsewhere (bitwise symmetric: the planes are)
__device__ __forceinline__ void xo_to_corr(double* dst, const double* dg, int K) {
  for (int e = threadIdx.x; e < K * K; e += XO_THREADS) {
    const int i = e / K, j = e - i * K;
    dst[i * XO_LS + j] = i == j ? 1.0 : dst[i * XO_LS + j] / sqrt(dg[i] * dg[j]);
  }
}

__global__ __launch_bounds__(XO_THREADS) void k_xo_solve(const double* __restrict__ gram_all, int P, int K, int D,
                                                         int method, int min_obs, const double* __restrict__ dayinfo,
                                                         double* __restrict__ tprime, double* __restrict__ transform,
                                                         double* __restrict__ eig, double* __restrict__ keep,
                                                         int32_t* __restrict__ nout, int32_t* __restrict__ status) {
  __shared__ double A[XO_B * XO_LS];
  __shared__ double V[XO_B * XO_LS];
  __shared__ double dg[XO_B];   // M_jj
  __shared__ double lam[XO_B];  // eigenvalues in Jacobi order
  __shared__ double es[XO_B];   // ... ascending
  __shared__ double isq[XO_B];  // 1 / sqrt(lam)
  __shared__ double kp[XO_B];
  __shared__ double rc[XO_B / 2], rs[XO_B / 2];
  __shared__ int rp[XO_B / 2], rq[XO_B / 2];
  __shared__ int flag;
  const int d = blockIdx.x, t = threadIdx.x;
  const double* info = dayinfo + (size_t)d * (2 * K + 1);
  const int n = (int)info[0];
  int stat = n < (min_obs > K + 1 ? min_obs : K + 1) ? 1 : 0;
  if (t == 0) flag = 0;
  if (stat == 0) xo_sum_planes(gram_all, P, K, D, d, A);
  __syncthreads();
  if (stat == 0 && t < K) {
    const double mjj = A[t * XO_LS + t];
    if (!(mjj > XO_CONST_REL * info[1 + K + t])) flag = 1;  // constant on U (or not finite)
    dg[t] = mjj;
  }
  __syncthreads();
  if (stat == 0 && flag) stat = 2;
  if (stat == 0) {
    xo_to_corr(A, dg, K);
    for (int e = t; e < K * K; e += XO_THREADS) {
      const int i = e / K, j = e - i * K;
      V[i * XO_LS + j] = i == j ? 1.0 : 0.0;
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
            const double apq = A[p_ * XO_LS + q_], app = A[p_ * XO_LS + p_], aqq = A[q_ * XO_LS + q_];
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
          const int pr = w + (XO_THREADS / WAVE) * i;
          ss[i] = (pr < m && l < K) ? rs[pr] : 0.0;
          cc[i] = pr < m ? rc[pr] : 1.0;
          pi[i] = pr < m ? rp[pr] : 0;
          qi[i] = pr < m ? rq[pr] : 0;
          if (ss[i] != 0.0) {
            ap[i] = A[l * XO_LS + pi[i]];
            aq[i] = A[l * XO_LS + qi[i]];
            if (method == 0) {  // (Gram-Schmidt needs the eigenvalues only)
              vp[i] = V[l * XO_LS + pi[i]];
              vq[i] = V[l * XO_LS + qi[i]];
            }
          }
        }
#pragma unroll
        for (int i = 0; i < XO_PW; ++i) {
          if (ss[i] != 0.0) {
            A[l * XO_LS + pi[i]] = cc[i] * ap[i] - ss[i] * aq[i];
            A[l * XO_LS + qi[i]] = ss[i] * ap[i] + cc[i] * aq[i];
            if (method == 0) {
              V[l * XO_LS + pi[i]] = cc[i] * vp[i] - ss[i] * vq[i];
              V[l * XO_LS + qi[i]] = ss[i] * vp[i] + cc[i] * vq[i];
            }
          }
        }
        __syncthreads();
#pragma unroll
        for (int i = 0; i < XO_PW; ++i) {  // rows p, q of A
          if (ss[i] != 0.0) {
            ap[i] = A[pi[i] * XO_LS + l];
            aq[i] = A[qi[i] * XO_LS + l];
          }
        }
#pragma unroll
        for (int i = 0; i < XO_PW; ++i) {  // ... the rotated entry is exactly 0
          if (ss[i] != 0.0) {
            A[pi[i] * XO_LS + l] = l == qi[i] ? 0.0 : cc[i] * ap[i] - ss[i] * aq[i];
            A[qi[i] * XO_LS + l] = l == pi[i] ? 0.0 : ss[i] * ap[i] + cc[i] * aq[i];
          }
        }
        __syncthreads();
      }
      conv = rotated == 0;
    }
    if (!conv) stat = 2;
  }

  if (stat == 0) {
    if (t < K) lam[t] = A[t * XO_LS + t];
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
      for (int k = 0; k < K; ++k) s += V[t * XO_LS + k] * V[t * XO_LS + k] * sqrt(lam[k]);
      kp[t] = s;
    }
    for (int e = t; e < K * K; e += XO_THREADS) {  // T = V diag(lam^-1/2) V^T, k order, mirrored
      const int i = e / K, j = e - i * K;
      if (i > j) continue;
      double s = 0.0;
      for (int k = 0; k < K; ++k) s += V[i * XO_LS + k] * V[j * XO_LS + k] * isq[k];
      A[i * XO_LS + j] = A[j * XO_LS + i] = s;
    }
  }
  if (stat == 0 && method == 1) {
    __syncthreads();
    xo_sum_planes(gram_all, P, K, D, d, V);
    __syncthreads();
    xo_to_corr(V, dg, K);
    __syncthreads();
    // unpivoted Cholesky, row t on thread t, L in the lower triangle (k_xr_solve)
    for (int k = 0; k < K; ++k) {
      const double piv = V[k * XO_LS + k];
      if (!(piv > XO_EIG_MIN)) {  // (uniform: every thread reads the same entry)
        stat = 2;
        break;
      }
      const double lkk = sqrt(piv);
      __syncthreads();
      if (t == k) V[k * XO_LS + k] = lkk;
      double lik = 0.0;
      if (t > k && t < K) {
        lik = V[t * XO_LS + k] / lkk;
        V[t * XO_LS + k] = lik;
      }
      __syncthreads();
      if (t > k && t < K)
        for (int j = k + 1; j <= t; ++j) V[t * XO_LS + j] -= lik * V[j * XO_LS + k];
      __syncthreads();
    }
    if (stat == 0) {
      // column t of L^-1 into row t of the upper triangle
      if (t < K) {
        const double vt = 1.0 / V[t * XO_LS + t];
        for (int i = t + 1; i < K; ++i) {
          double s = V[i * XO_LS + t] * vt;
          for (int k = t + 1; k < i; ++k) s += V[i * XO_LS + k] * V[t * XO_LS + k];
          V[t * XO_LS + i] = -s / V[i * XO_LS + i];
        }
      }
      __syncthreads();
      if (t < K) kp[t] = V[t * XO_LS + t];
      for (int e = t; e < K * K; e += XO_THREADS) {  // T = L^-T
        const int i = e / K, j = e - i * K;
        A[i * XO_LS + j] = i < j ? V[i * XO_LS + j] : (i == j ? 1.0 / V[i * XO_LS + i] : 0.0);
      }
    }
  }
  __syncthreads();

  const double nm1 = (double)(n - 1);
  for (int e = t; e < K * K; e += XO_THREADS) {
    const int i = e / K, j = e - i * K;
    const double tv = stat == 0 ? A[i * XO_LS + j] : qnan();
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

__global__ __launch_bounds__(XO_THREADS) void k_xo_apply(const double* __restrict__ xv, const uint8_t* __restrict__ xs,
                                                         const uint8_t* __restrict__ mask,
                                                         const double* __restrict__ dayinfo,
                                                         const double* __restrict__ tprime,
                                                         const int32_t* __restrict__ status, int K, int D, int S,
                                                         double* __restrict__ ov, uint8_t* __restrict__ os) {
  __shared__ double tile[XO_B * XO_STR];
  const int d = blockIdx.x;
  const int sbeg = (int)min((long long)blockIdx.y * XO_AP_STOCKS, (long long)S);
  const int send = (int)min((long long)sbeg + XO_AP_STOCKS, (long long)S);
  const int t = threadIdx.x, l = t & 63, w = t >> 6;
  const int r = l & 15, kq = l >> 4;
  const int ls = t & (XO_KT - 1), r0 = t / XO_KT;
  const bool ok = status[d] == 0;
  const int nt = (K + 15) / 16, nk = (K + 3) / 4;
  const double* mean = dayinfo + (size_t)d * (2 * K + 1) + 1;
  const double* tp = tprime + (size_t)d * K * K;
  // this wave's T' fragments: output rows 16 w .. 16 w + 15, every k step
  double af[XO_B / 4];
#pragma unroll
  for (int st = 0; st < XO_B / 4; ++st) {
    const int k = 4 * st + kq, j = 16 * w + r;
    af[st] = (ok && k < K && j < K) ? tp[(size_t)k * K + j] : 0.0;
  }
  double cv[XO_NR];
  uint8_t so[XO_NR];
  auto load = [&](int k0) {
    const int s = k0 + ls;
    const bool in = s < send;
    const bool u = in && ok && mask[(size_t)d * S + s] != 0;
#pragma unroll
    for (int i = 0; i < XO_NR; ++i) {
      const int rr = r0 + XO_RS * i;
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
  for (int k0 = sbeg; k0 < send; k0 += XO_KT) {
    __syncthreads();  // the previous tile's reads are done
#pragma unroll
    for (int i = 0; i < XO_NR; ++i) {
      const int rr = r0 + XO_RS * i;
      tile[rr * XO_STR + ls] = cv[i];
      if (rr < K && k0 + ls < send) os[((size_t)rr * D + d) * (size_t)S + k0 + ls] = so[i];
    }
    __syncthreads();
    if (k0 + XO_KT < send) load(k0 + XO_KT);
    if (w >= nt) continue;  // (wave-uniform: output rows beyond ceil(K / 16) tiles)
    xo_v4d acc[2] = {xo_v4d{0.0, 0.0, 0.0, 0.0}, xo_v4d{0.0, 0.0, 0.0, 0.0}};
#pragma unroll
    for (int st = 0; st < XO_B / 4; ++st) {
      if (st < nk) {
        const double b0 = tile[(4 * st + kq) * XO_STR + r], b1 = tile[(4 * st + kq) * XO_STR + 16 + r];
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

static int xo_check(const char* what, int K, int D, int S) {
  MFF_REQUIRE(K >= 1 && K <= XO_MAX_K, "%s: K=%d outside [1, %d]", what, K, XO_MAX_K);
  MFF_REQUIRE(D >= 0 && S >= 0, "%s: bad sizes D=%d S=%d", what, D, S);
  MFF_REQUIRE(S < (1 << 24) && (long long)D * S < (1ll << 40), "%s: panel too large", what);
  return 0;
}

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
  const int tiles = (S + XO_KT - 1) / XO_KT;
  const int split_stocks = max(1, (tiles + nsplit - 1) / nsplit) * XO_KT;
  uint8_t* mask = reinterpret_cast<uint8_t*>(workspace) + xo_mask_off(K, D);
  hipLaunchKernelGGL(k_xo_sums, dim3((unsigned)D, (unsigned)nsplit), dim3(XO_THREADS), 0, as_stream(stream), x_val,
                     x_state, K, D, S, split_stocks, mask, sums);
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
  const int tiles = (S + XO_KT - 1) / XO_KT;
  const int split_stocks = max(1, (tiles + nsplit - 1) / nsplit) * XO_KT;
  hipLaunchKernelGGL(k_xo_gram, dim3((unsigned)D, (unsigned)nsplit), dim3(XO_THREADS), 0, st, x_val,
                     reinterpret_cast<const uint8_t*>(ws + xo_mask_off(K, D)), dayinfo, K, D, S, split_stocks, gram);
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
  hipLaunchKernelGGL(k_xo_solve, dim3((unsigned)D), dim3(XO_THREADS), 0, as_stream(stream), gram_all, P, K, D, method,
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
                     dim3(XO_THREADS), 0, as_stream(stream), x_val, x_state,
                     reinterpret_cast<const uint8_t*>(ws + xo_mask_off(K, D)), reinterpret_cast<const double*>(ws),
                     reinterpret_cast<const double*>(ws + xo_tp_off(K, D)), status, K, D, S, out_val, out_state);
  MFF_LAUNCH_CHECK();
  return 0;
}

}  // extern "C"
