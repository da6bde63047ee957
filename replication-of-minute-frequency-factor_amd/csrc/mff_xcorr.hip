// mff_xcorr.hip — pairwise factor correlation: per day the F x F matrix of the
// pairwise-complete Pearson correlations of the exposure rows (include/mff.h, mff_xs_corr_*).
//
// The pairwise-complete sums of a day are four small GEMMs over the stock axis,
//   n = M M^T,  A = Y M^T,  Q = Y^2 M^T,  P = Y Y^T
// (Y: the rows centred per day and zeroed where unusable, M: the 0/1 usable mask), summed
// in f64 on the matrix cores: v_mfma_f64_16x16x4_f64, operands one f64 per lane
// (A[i = lane & 15][k = lane >> 4], B[k = lane >> 4][j = lane & 15]), results four f64 per
// lane at row (lane >> 4) + 4 * reg, column lane & 15.  n is a sum of exact 0/1 products of
// at most S terms, so it is exact in f64.
//
// k_xc_sums_diag / k_xc_sums_off: one 256-thread workgroup per (day, 64-row block I, 64-row
// block J).  A tile of GR_KT stocks of a block's rows goes through LDS as ONE f64 plane:
// y = x - centre where the entry is usable, NaN where it is not, so y, y^2 and the mask are
// derived in registers from one ds_read_b64 per operand.  The tile is row-major with a row
// stride of GR_KT + 2 doubles (68 dwords = 4 mod 64): the 32 lanes of one ds_read_b64 group
// (16 rows x 2 stocks) hit 32 distinct even banks, and the stores (32 consecutive stocks of
// a row) are conflict-free too.  The next tile's values and states are loaded into registers
// before the MFMAs of the current one.  Tile assignment: on the two kernels below.
// Every sum has one fixed order (the stock order inside the MFMA chain), so results are
// bit-identical from run to run; nothing is accumulated with atomics.
#include <hip/hip_runtime.h>

#include "../../include/mff.h"
#include "mff_gram.h"
#include "mff_internal.h"
#include "mff_wave.h"

namespace mff {

constexpr int XC_MAX_ROWS = 1024;
constexpr double XC_CONST_REL = 1e-12;  // the constant rule: var <= XC_CONST_REL * Q

// per (row, day): n and sum of x over the usable set -> [rows][D][2]; one wave per segment
__global__ __launch_bounds__(256) void k_xc_moments(const double* __restrict__ val, const uint8_t* __restrict__ state,
                                                    long long nseg, int S, double* __restrict__ moments) {
  const long long seg = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (seg >= nseg) return;
  const int l = lane_id();
  const double* v = val + (size_t)seg * S;
  const uint8_t* st = state + (size_t)seg * S;
  double sum = 0.0;
  uint32_t n = 0;
#pragma unroll 4
  for (int s = l; s < S; s += WAVE) {
    const double x = v[s];
    const bool u = xs_usable(x, st[s]);
    sum += u ? x : 0.0;
    n += u ? 1u : 0u;
  }
  sum = wsum(sum);
  n = wsum_u32(n);
  if (l == 0) {
    moments[2 * seg] = (double)n;
    moments[2 * seg + 1] = sum;
  }
}

// centre [rows][D] = sum / n of the local moments (0 for an empty segment)
__global__ __launch_bounds__(256) void k_xc_center(const double* __restrict__ moments, long long nseg,
                                                   double* __restrict__ center) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= nseg) return;
  const double n = moments[2 * i], s = moments[2 * i + 1];
  center[i] = n > 0.0 ? s / n : 0.0;
}

struct XcAcc {
  v4d A[4], Q[4], P[4], N[4];
};

template <bool SYM>
__device__ __forceinline__ void xc_tile_mma(const double* __restrict__ ti, const double* __restrict__ tj, int w, int l,
                                            XcAcc& acc) {
  const int r = l & 15, kq = l >> 4;
#pragma unroll
  for (int ks = 0; ks < GR_KT / 4; ++ks) {
    const int k = ks * 4 + kq;
    const double a = ti[(16 * w + r) * GR_STR + k];
    const bool ua = a == a;
    const double ya = ua ? a : 0.0, fa = ua ? 1.0 : 0.0, qa = ya * ya;
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      const double b = tj[(16 * c + r) * GR_STR + k];
      const bool ub = b == b;
      const double yb = ub ? b : 0.0, fb = ub ? 1.0 : 0.0;
      acc.A[c] = __builtin_amdgcn_mfma_f64_16x16x4f64(ya, fb, acc.A[c], 0, 0, 0);
      acc.Q[c] = __builtin_amdgcn_mfma_f64_16x16x4f64(qa, fb, acc.Q[c], 0, 0, 0);
      if (SYM) {
        acc.P[c] = __builtin_amdgcn_mfma_f64_16x16x4f64(ya, yb, acc.P[c], 0, 0, 0);
        acc.N[c] = __builtin_amdgcn_mfma_f64_16x16x4f64(fa, fb, acc.N[c], 0, 0, 0);
      }
    }
  }
}

// this thread's part of a [64 rows][GR_KT stocks] tile: stock t % GR_KT, rows t / GR_KT + 8 i
__device__ __forceinline__ void xc_load(const double* __restrict__ val, const uint8_t* __restrict__ state, int rows,
                                        int D, int S, int d, int row0, int k0, double (&xv)[GR_NR],
                                        uint8_t (&xs)[GR_NR]) {
  const int s = k0 + (int)(threadIdx.x & (GR_KT - 1));
#pragma unroll
  for (int i = 0; i < GR_NR; ++i) {
    const int g = row0 + (int)(threadIdx.x / GR_KT) + GR_RS * i;
    const bool ok = g < rows && s < S;
    const size_t off = ((size_t)g * D + d) * (size_t)S + s;
    xv[i] = ok ? val[off] : 0.0;
    xs[i] = ok ? state[off] : (uint8_t)MFF_STATE_ABSENT;
  }
}
// y = x - centre where usable, NaN where not (a padding row's centre is NaN)
__device__ __forceinline__ void xc_store(double* __restrict__ tile, const double* __restrict__ cen,
                                         const double (&xv)[GR_NR], const uint8_t (&xs)[GR_NR]) {
  const int ls = threadIdx.x & (GR_KT - 1);
#pragma unroll
  for (int i = 0; i < GR_NR; ++i) {
    const int r = (int)(threadIdx.x / GR_KT) + GR_RS * i;
    tile[r * GR_STR + ls] = xs_usable(xv[i], xs[i]) ? xv[i] - cen[r] : qnan();
  }
}

// Diagonal blocks (I == J), sums [D][4][rows][rows]: planes n, A, Q, P of the local stocks.
// One tile in LDS serves both operands.  Wave w owns tile row w of A and Q (8 tiles); P and n
// need only the 10 tiles on or below the diagonal each, and those 20 are split 5 per wave:
// waves 0 / 1 take P, waves 2 / 3 take n, of tile rows {0, 3} (1 + 4 tiles) and {1, 2}
// (2 + 3 tiles).  13 accumulator tiles per wave instead of 16, and two workgroups per CU.
__global__ __launch_bounds__(GR_THREADS, 2) void k_xc_sums_diag(const double* __restrict__ val,
                                                                const uint8_t* __restrict__ state, int rows, int D,
                                                                int S, const double* __restrict__ center,
                                                                double* __restrict__ sums) {
  __shared__ double tI[GR_B * GR_STR];
  __shared__ double cen[GR_B];
  const int d = blockIdx.x, bi = blockIdx.y;
  const int t = threadIdx.x, l = t & 63, w = t >> 6;
  if (t < GR_B) {
    const int g = bi * GR_B + t;
    cen[t] = g < rows ? center[(size_t)g * D + d] : qnan();
  }
  double xv[GR_NR];
  uint8_t xs[GR_NR];
  v4d A[4], Q[4], T[5];
#pragma unroll
  for (int c = 0; c < 4; ++c) A[c] = Q[c] = v4d{0.0, 0.0, 0.0, 0.0};
#pragma unroll
  for (int k = 0; k < 5; ++k) T[k] = v4d{0.0, 0.0, 0.0, 0.0};
  const bool g1 = (w & 1) != 0;  // tile rows {1, 2}, else {0, 3}
  const bool cnt = w >= 2;       // the n plane, else P
  const int r = l & 15, kq = l >> 4;

  if (S > 0) xc_load(val, state, rows, D, S, d, bi * GR_B, 0, xv, xs);
  for (int k0 = 0; k0 < S; k0 += GR_KT) {
    __syncthreads();  // the previous tile's reads are done (first pass: cen is written)
    xc_store(tI, cen, xv, xs);
    __syncthreads();
    if (k0 + GR_KT < S) xc_load(val, state, rows, D, S, d, bi * GR_B, k0 + GR_KT, xv, xs);
#pragma unroll
    for (int ks = 0; ks < GR_KT / 4; ++ks) {
      const int k = ks * 4 + kq;
      double y[4], f[4], z[4];
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        const double b = tI[(16 * c + r) * GR_STR + k];
        const bool u = b == b;
        y[c] = u ? b : 0.0;
        f[c] = u ? 1.0 : 0.0;
        z[c] = cnt ? f[c] : y[c];
      }
      const double yw = w == 0 ? y[0] : w == 1 ? y[1] : w == 2 ? y[2] : y[3];
      const double qw = yw * yw;
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        A[c] = __builtin_amdgcn_mfma_f64_16x16x4f64(yw, f[c], A[c], 0, 0, 0);
        Q[c] = __builtin_amdgcn_mfma_f64_16x16x4f64(qw, f[c], Q[c], 0, 0, 0);
      }
      // tiles (row, col): {0,3}: (0,0) (3,0) (3,1) (3,2) (3,3);  {1,2}: (1,0) (1,1) (2,0) (2,1) (2,2)
      const double a0 = g1 ? z[1] : z[0], a1 = g1 ? z[1] : z[3], a2 = g1 ? z[2] : z[3];
      const double b1 = g1 ? z[1] : z[0], b2 = g1 ? z[0] : z[1], b3 = g1 ? z[1] : z[2], b4 = g1 ? z[2] : z[3];
      T[0] = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, z[0], T[0], 0, 0, 0);
      T[1] = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, b1, T[1], 0, 0, 0);
      T[2] = __builtin_amdgcn_mfma_f64_16x16x4f64(a2, b2, T[2], 0, 0, 0);
      T[3] = __builtin_amdgcn_mfma_f64_16x16x4f64(a2, b3, T[3], 0, 0, 0);
      T[4] = __builtin_amdgcn_mfma_f64_16x16x4f64(a2, b4, T[4], 0, 0, 0);
    }
  }

  const size_t plane = (size_t)rows * rows;
  double* out = sums + (size_t)d * 4 * plane;
  const int base = bi * GR_B;
#pragma unroll
  for (int c = 0; c < 4; ++c) {
    const int j = base + 16 * c + r;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int i = base + 16 * w + kq + 4 * q;
      if (i >= rows || j >= rows) continue;
      out[plane + (size_t)i * rows + j] = A[c][q];
      out[2 * plane + (size_t)i * rows + j] = Q[c][q];
    }
  }
  double* sym = out + (cnt ? 0 : 3 * plane);
#pragma unroll
  for (int k = 0; k < 5; ++k) {
    const int tr = g1 ? (k < 2 ? 1 : 2) : (k < 1 ? 0 : 3);
    const int tc = g1 ? (k < 2 ? k : k - 2) : (k < 1 ? 0 : k - 1);
    const int j = base + 16 * tc + r;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int i = base + 16 * tr + kq + 4 * q;
      if (i >= rows || j > i) continue;  // (a diagonal tile's upper half comes from its mirror)
      sym[(size_t)i * rows + j] = sym[(size_t)j * rows + i] = T[k][q];
    }
  }
}

// Off-diagonal blocks (I != J): wave w owns tile row w of block I against the four tile
// columns of block J for every product, 16 accumulator tiles, one wave per SIMD.  J < I: all
// four planes, P and n written mirrored too; J > I: A and Q only.
__global__ __launch_bounds__(GR_THREADS) void k_xc_sums_off(const double* __restrict__ val,
                                                            const uint8_t* __restrict__ state, int rows, int D, int S,
                                                            const double* __restrict__ center,
                                                            double* __restrict__ sums) {
  __shared__ double tI[GR_B * GR_STR];
  __shared__ double tJ[GR_B * GR_STR];
  __shared__ double cen[2][GR_B];
  const int d = blockIdx.x;
  const int nb = (rows + GR_B - 1) / GR_B;
  const int bi = (int)blockIdx.y / (nb - 1), rj = (int)blockIdx.y % (nb - 1), bj = rj + (rj >= bi ? 1 : 0);
  const bool sym = bj < bi;
  const int t = threadIdx.x, l = t & 63, w = t >> 6;

  if (t < 2 * GR_B) {
    const int g = (t < GR_B ? bi : bj) * GR_B + (t & (GR_B - 1));
    cen[t / GR_B][t & (GR_B - 1)] = g < rows ? center[(size_t)g * D + d] : qnan();
  }
  double xvI[GR_NR], xvJ[GR_NR];
  uint8_t xsI[GR_NR], xsJ[GR_NR];
  XcAcc acc;
#pragma unroll
  for (int c = 0; c < 4; ++c) acc.A[c] = acc.Q[c] = acc.P[c] = acc.N[c] = v4d{0.0, 0.0, 0.0, 0.0};

  if (S > 0) {
    xc_load(val, state, rows, D, S, d, bi * GR_B, 0, xvI, xsI);
    xc_load(val, state, rows, D, S, d, bj * GR_B, 0, xvJ, xsJ);
  }
  for (int k0 = 0; k0 < S; k0 += GR_KT) {
    __syncthreads();  // the previous tile's reads are done (first pass: cen is written)
    xc_store(tI, cen[0], xvI, xsI);
    xc_store(tJ, cen[1], xvJ, xsJ);
    __syncthreads();
    if (k0 + GR_KT < S) {
      xc_load(val, state, rows, D, S, d, bi * GR_B, k0 + GR_KT, xvI, xsI);
      xc_load(val, state, rows, D, S, d, bj * GR_B, k0 + GR_KT, xvJ, xsJ);
    }
    if (sym)
      xc_tile_mma<true>(tI, tJ, w, l, acc);
    else
      xc_tile_mma<false>(tI, tJ, w, l, acc);
  }

  const size_t plane = (size_t)rows * rows;
  double* out = sums + (size_t)d * 4 * plane;
#pragma unroll
  for (int c = 0; c < 4; ++c) {
    const int j = bj * GR_B + 16 * c + (l & 15);
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int i = bi * GR_B + 16 * w + (l >> 4) + 4 * q;
      if (i >= rows || j >= rows) continue;
      const size_t ij = (size_t)i * rows + j, ji = (size_t)j * rows + i;
      out[plane + ij] = acc.A[c][q];
      out[2 * plane + ij] = acc.Q[c][q];
      if (sym) {
        out[ij] = out[ji] = acc.N[c][q];
        out[3 * plane + ij] = out[3 * plane + ji] = acc.P[c][q];
      }
    }
  }
}

// the definition on the summed planes; every (i, j) is computed from the pair (min, max),
// so the two mirror entries come from the same operations on the same inputs
__global__ __launch_bounds__(256) void k_xc_finalize(const double* __restrict__ sums_all, int R, int rows, int D,
                                                     int min_pairs, double* __restrict__ corr,
                                                     int32_t* __restrict__ nout) {
  const size_t plane = (size_t)rows * rows;
  const size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= (size_t)D * plane) return;
  const size_t d = idx / plane, e = idx - d * plane;
  const int i = (int)(e / rows), j = (int)(e - (size_t)i * rows);
  const int a = i < j ? i : j, b = i < j ? j : i;
  const size_t ab = (size_t)a * rows + b, ba = (size_t)b * rows + a;
  double n = 0.0, Aab = 0.0, Aba = 0.0, Qab = 0.0, Qba = 0.0, P = 0.0;
  for (int r = 0; r < R; ++r) {  // rank order
    const double* p = sums_all + ((size_t)r * D + d) * 4 * plane;
    n += p[ab];
    Aab += p[plane + ab];
    Aba += p[plane + ba];
    Qab += p[2 * plane + ab];
    Qba += p[2 * plane + ba];
    P += p[3 * plane + ab];
  }
  nout[idx] = (int32_t)n;
  double r = qnan();
  if (n >= (double)min_pairs) {
    const double va = Qab - Aab * Aab / n, vb = Qba - Aba * Aba / n;
    const bool ca = va <= XC_CONST_REL * Qab, cb = vb <= XC_CONST_REL * Qba;
    if (!ca && !cb) {
      if (a == b) {
        r = (va == va) ? 1.0 : va;  // (a non-finite sum stays NaN)
      } else {
        r = (P - Aab * Aba / n) / (sqrt(va) * sqrt(vb));
        if (r > 1.0) r = 1.0;
        if (r < -1.0) r = -1.0;
      }
    }
  }
  corr[idx] = r;
}

// mean over the days of the non-NaN entries, in day order
__global__ __launch_bounds__(256) void k_xc_mean(const double* __restrict__ corr, int rows, int D,
                                                 double* __restrict__ mean, int32_t* __restrict__ days) {
  const size_t plane = (size_t)rows * rows;
  const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= plane) return;
  double s = 0.0;
  int32_t c = 0;
  for (int d0 = 0; d0 < D; d0 += 8) {  // eight loads in flight, added in day order
    double v[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) v[k] = d0 + k < D ? corr[(size_t)(d0 + k) * plane + e] : qnan();
#pragma unroll
    for (int k = 0; k < 8; ++k)
      if (v[k] == v[k]) {
        s += v[k];
        ++c;
      }
  }
  mean[e] = c > 0 ? s / (double)c : qnan();
  days[e] = c;
}

static int xc_check_sizes(const char* what, int rows, int D, int S) {
  MFF_REQUIRE(rows >= 1 && D >= 0 && S >= 0, "%s: bad sizes rows=%d D=%d S=%d", what, rows, D, S);
  MFF_REQUIRE(rows <= XC_MAX_ROWS, "%s: rows=%d above the %d rows of one call", what, rows, XC_MAX_ROWS);
  MFF_REQUIRE((long long)rows * D < (1ll << 31), "%s: too many segments", what);
  return 0;
}

}  // namespace mff

using namespace mff;

extern "C" {

int mff_xs_corr_max_rows(void) { return XC_MAX_ROWS; }

size_t mff_xs_corr_workspace_bytes(int rows, int D, int S) {
  (void)S;
  if (rows <= 0 || D <= 0) return 0;
  return (size_t)rows * D * 3 * sizeof(double);  // local moments [rows][D][2] + centre [rows][D]
}

int mff_xs_corr_moments(const double* val, const uint8_t* state, int rows, int D, int S, double* moments,
                        void* stream) {
  clear_error();
  if (int rc = xc_check_sizes("mff_xs_corr_moments", rows, D, S)) return rc;
  if (D == 0) return 0;
  MFF_REQUIRE(moments && (S == 0 || (val && state)), "mff_xs_corr_moments: NULL buffer");
  const long long nseg = (long long)rows * D;
  hipLaunchKernelGGL(k_xc_moments, dim3((unsigned)((nseg + 3) / 4)), dim3(256), 0, as_stream(stream), val, state, nseg,
                     S, moments);
  MFF_LAUNCH_CHECK();
  return 0;
}

int mff_xs_corr_sums(const double* val, const uint8_t* state, int rows, int D, int S, const double* center,
                     double* sums, void* workspace, void* stream) {
  clear_error();
  if (int rc = xc_check_sizes("mff_xs_corr_sums", rows, D, S)) return rc;
  if (D == 0) return 0;
  MFF_REQUIRE(sums && (S == 0 || (val && state)), "mff_xs_corr_sums: NULL buffer");
  MFF_REQUIRE(center || workspace, "mff_xs_corr_sums: no centre and no workspace to compute it in");
  hipStream_t st = as_stream(stream);
  const long long nseg = (long long)rows * D;
  if (!center) {
    double* mom = reinterpret_cast<double*>(workspace);
    double* cen = mom + 2 * nseg;
    hipLaunchKernelGGL(k_xc_moments, dim3((unsigned)((nseg + 3) / 4)), dim3(256), 0, st, val, state, nseg, S, mom);
    MFF_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_xc_center, dim3((unsigned)((nseg + 255) / 256)), dim3(256), 0, st, mom, nseg, cen);
    MFF_LAUNCH_CHECK();
    center = cen;
  }
  const int nb = (rows + GR_B - 1) / GR_B;
  hipLaunchKernelGGL(k_xc_sums_diag, dim3((unsigned)D, (unsigned)nb), dim3(GR_THREADS), 0, st, val, state, rows, D, S,
                     center, sums);
  MFF_LAUNCH_CHECK();
  if (nb > 1) {
    hipLaunchKernelGGL(k_xc_sums_off, dim3((unsigned)D, (unsigned)(nb * (nb - 1))), dim3(GR_THREADS), 0, st, val, state,
                       rows, D, S, center, sums);
    MFF_LAUNCH_CHECK();
  }
  return 0;
}

int mff_xs_corr_finalize(const double* sums_all, int R, int rows, int D, int min_pairs, double* corr, int32_t* n,
                         void* stream) {
  clear_error();
  if (int rc = xc_check_sizes("mff_xs_corr_finalize", rows, D, 0)) return rc;
  MFF_REQUIRE(R >= 1, "mff_xs_corr_finalize: R=%d", R);
  MFF_REQUIRE(min_pairs >= 2, "mff_xs_corr_finalize: min_pairs=%d below 2", min_pairs);
  if (D == 0) return 0;
  MFF_REQUIRE(sums_all && corr && n, "mff_xs_corr_finalize: NULL buffer");
  const size_t total = (size_t)D * rows * rows;
  MFF_REQUIRE((total + 255) / 256 < (1ull << 31), "mff_xs_corr_finalize: too many entries");
  hipLaunchKernelGGL(k_xc_finalize, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, as_stream(stream), sums_all, R,
                     rows, D, min_pairs, corr, n);
  MFF_LAUNCH_CHECK();
  return 0;
}

int mff_xs_corr_mean(const double* corr, int rows, int D, double* mean, int32_t* days, void* stream) {
  clear_error();
  if (int rc = xc_check_sizes("mff_xs_corr_mean", rows, D, 0)) return rc;
  MFF_REQUIRE(mean && days && (D == 0 || corr), "mff_xs_corr_mean: NULL buffer");
  const size_t plane = (size_t)rows * rows;
  hipLaunchKernelGGL(k_xc_mean, dim3((unsigned)((plane + 255) / 256)), dim3(256), 0, as_stream(stream), corr, rows, D,
                     mean, days);
  MFF_LAUNCH_CHECK();
  return 0;
}

}  // extern "C"
