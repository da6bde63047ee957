// mff_gram.h — the per-day linear algebra shared by the cross-sectional kernels (mff_xreg.hip,
// mff_xorth.hip, mff_xcomb.hip; constants, typedef and predicate also mff_xcorr.hip):
//   gram_block       sum c c^T (or sum w c c^T) of up to 64 rows over a stock run on
//                    v_mfma_f64_16x16x4_f64, one 256-thread workgroup;
//   chol_lower       unpivoted Cholesky in LDS, row t on thread t;
//   chol_inv_column  column t of L^-1 into the unused upper triangle;
//   xs_check, xs_split_stocks  the host wrappers' size checks and stock runs.
// Every sum has one fixed order, so results are bit-identical from run to run.
#pragma once
#include <hip/hip_runtime.h>

#include "../../include/mff.h"
#include "mff_internal.h"

namespace mff {

typedef double v4d __attribute__((ext_vector_type(4)));

constexpr int GR_B = 64;            // padded rows of the Gram block
constexpr int GR_KT = 32;           // stocks per LDS tile
constexpr int GR_STR = GR_KT + 2;   // row stride of the tile (doubles; DESIGN.md §10: conflict-free)
constexpr int GR_THREADS = 256;
constexpr int GR_NR = GR_B * GR_KT / GR_THREADS;  // rows per thread (8)
constexpr int GR_RS = GR_THREADS / GR_KT;         // row step (8)
constexpr int GR_NT = 10;           // tiles on or below the block diagonal
constexpr int GR_LS = GR_B + 1;     // row stride of a solve's matrix
constexpr double CHOL_PIVOT_MIN = 1e-10;

// the 10 tiles (row, col) on or below the block diagonal
__host__ __device__ constexpr int gr_tr(int i) { return i < 1 ? 0 : i < 3 ? 1 : i < 6 ? 2 : 3; }
__host__ __device__ constexpr int gr_tc(int i) { return i < 1 ? 0 : i < 3 ? i - 1 : i < 6 ? i - 3 : i - 6; }

__device__ __forceinline__ bool xs_usable(double x, uint8_t s) { return s == MFF_STATE_VALUE && __builtin_isfinite(x); }

// out [C][C] = sum over the stocks [sbeg, send) of c c^T (WEIGHTED: w c c^T) of C <= 64 rows.
// load(k0, cv, wt) fills this thread's part of the [64 rows][GR_KT stocks] tile at k0: stock
// t % GR_KT, rows t / GR_KT + 8 i (0 where a row or a stock does not count), and the stock's
// weight if WEIGHTED.  The tile goes through LDS (tile [GR_B * GR_STR], wts [GR_KT] if WEIGHTED)
// while the next one is loaded into registers; the second operand w c is one multiply in
// registers.  The four waves split the k steps of a tile (stocks 8 w .. 8 w + 7), each holds the
// 10 tiles on or below the block diagonal (tile rows above ceil(C / 16) are skipped), and the
// four partial sums are added in wave order through red [GR_NT * 256], then mirrored.
template <bool WEIGHTED, typename Load>
__device__ __forceinline__ void gram_block(int C, int sbeg, int send, Load load, double* tile, double* wts,
                                           double* red, double* __restrict__ out) {
  const int t = threadIdx.x, l = t & 63, w = t >> 6;
  const int nt = (C + 15) / 16;
  const int r = l & 15, kq = l >> 4;
  double cv[GR_NR], wt;
  v4d acc[GR_NT];
#pragma unroll
  for (int i = 0; i < GR_NT; ++i) acc[i] = v4d{0.0, 0.0, 0.0, 0.0};

  if (sbeg < send) load(sbeg, cv, wt);
  for (int k0 = sbeg; k0 < send; k0 += GR_KT) {
    __syncthreads();  // the previous tile's reads are done
    {
      const int ls = t & (GR_KT - 1);
#pragma unroll
      for (int i = 0; i < GR_NR; ++i) tile[((t / GR_KT) + GR_RS * i) * GR_STR + ls] = cv[i];
      if (WEIGHTED && t < GR_KT) wts[ls] = wt;
    }
    __syncthreads();
    if (k0 + GR_KT < send) load(k0 + GR_KT, cv, wt);
#pragma unroll
    for (int kk = 0; kk < 2; ++kk) {
      const int k = (2 * w + kk) * 4 + kq;
      const double wk = WEIGHTED ? wts[k] : 1.0;
      double a[4], b[4];
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        a[c] = tile[(16 * c + r) * GR_STR + k];
        b[c] = WEIGHTED ? a[c] * wk : a[c];
      }
#pragma unroll
      for (int i = 0; i < GR_NT; ++i)
        if (gr_tr(i) < nt) acc[i] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[gr_tr(i)], b[gr_tc(i)], acc[i], 0, 0, 0);
    }
  }

  for (int ww = 0; ww < 4; ++ww) {  // wave order
    if (w == ww) {
#pragma unroll
      for (int i = 0; i < GR_NT; ++i)
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          double* e = &red[i * 256 + q * 64 + l];
          *e = ww == 0 ? acc[i][q] : *e + acc[i][q];
        }
    }
    __syncthreads();
  }
  for (int e = t; e < GR_NT * 256; e += GR_THREADS) {
    const int ti = e >> 8, q = (e >> 6) & 3, ll = e & 63;
    int tr = 0, tc = 0;
    for (int i = 0; i < GR_NT; ++i)
      if (i == ti) {
        tr = gr_tr(i);
        tc = gr_tc(i);
      }
    const int i = 16 * tr + (ll >> 4) + 4 * q, j = 16 * tc + (ll & 15);
    if (i >= C || j > i) continue;
    out[(size_t)i * C + j] = out[(size_t)j * C + i] = red[e];
  }
}

// Unpivoted Cholesky of the K x K matrix A (LDS, row stride GR_LS) in place, L in the lower
// triangle.  Called by every thread of the workgroup, row t on thread t; false at the first
// pivot that is not above piv_min (uniform: every thread reads the same entry, and leaves
// before that step's first barrier).
__device__ __forceinline__ bool chol_lower(double* A, int K, int t, double piv_min) {
  for (int k = 0; k < K; ++k) {
    const double piv = A[k * GR_LS + k];
    if (!(piv > piv_min)) return false;
    const double lkk = sqrt(piv);
    __syncthreads();
    if (t == k) A[k * GR_LS + k] = lkk;
    double lik = 0.0;
    if (t > k && t < K) {
      lik = A[t * GR_LS + k] / lkk;
      A[t * GR_LS + k] = lik;
    }
    __syncthreads();
    if (t > k && t < K)
      for (int j = k + 1; j <= t; ++j) A[t * GR_LS + j] -= lik * A[j * GR_LS + k];
    __syncthreads();
  }
  return true;
}

// Column t of L^-1 into row t of the upper triangle of A (its diagonal entry is 1 / L_tt and
// is not stored); returns the column's squared norm, (A^-1)_tt.  No barrier: thread t reads L
// and row t of the upper triangle only.
__device__ __forceinline__ double chol_inv_column(double* A, int K, int t) {
  double inv = 0.0;
  if (t < K) {
    const double vt = 1.0 / A[t * GR_LS + t];
    inv = vt * vt;
    for (int i = t + 1; i < K; ++i) {
      double s = A[i * GR_LS + t] * vt;
      for (int k = t + 1; k < i; ++k) s += A[i * GR_LS + k] * A[t * GR_LS + k];
      const double vi = -s / A[i * GR_LS + i];
      A[t * GR_LS + i] = vi;
      inv += vi * vi;
    }
  }
  return inv;
}

// stocks per run when S stocks are cut into nsplit runs of whole tiles
inline int xs_split_stocks(int S, int nsplit) {
  const int tiles = (S + GR_KT - 1) / GR_KT;
  const int per = (tiles + nsplit - 1) / nsplit;
  return (per > 1 ? per : 1) * GR_KT;
}

inline int xs_check(const char* what, int K, int Kmax, int D, int S) {
  MFF_REQUIRE(K >= 1 && K <= Kmax, "%s: K=%d outside [1, %d]", what, K, Kmax);
  MFF_REQUIRE(D >= 0 && S >= 0, "%s: bad sizes D=%d S=%d", what, D, S);
  MFF_REQUIRE(S < (1 << 24) && (long long)D * S < (1ll << 40), "%s: panel too large", what);
  return 0;
}

}  // namespace mff
