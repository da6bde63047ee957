// mff_dd.h — double-double (hi + lo, ~106-bit) running sums for the sliding windows of
// stage 2 and the future return (any window length N: one add and one remove per row
// instead of an O(N) recompute).  Error-free transforms only (TwoSum, TwoProd by fma):
// a value added and later removed with the same shift cancels to within 2^-106 of the
// largest partial sum, so window sums stay accurate however long the walk.
#pragma once
#include <hip/hip_runtime.h>

namespace mff {

struct DD {
  double hi, lo;
};

// s + e == a + b exactly (Knuth TwoSum; no multiplications, so fp-contraction cannot
// touch it)
__device__ __forceinline__ void two_sum(double a, double b, double& s, double& e) {
  s = a + b;
  const double bb = s - a;
  e = (a - (s - bb)) + (b - bb);
}
__device__ __forceinline__ DD dd_add(DD x, double y) {
  double s, e;
  two_sum(x.hi, y, s, e);
  e += x.lo;
  const double h = s + e;
  return DD{h, e - (h - s)};
}
__device__ __forceinline__ DD dd_add(DD x, DD y) {
  double s, e;
  two_sum(x.hi, y.hi, s, e);
  e += x.lo + y.lo;
  const double h = s + e;
  return DD{h, e - (h - s)};
}
// a * b exactly as a double-double.  The rounded product must stay the value that the fma
// measures.  hipcc contracts across inlined calls, and a product with several uses too: a
// consumer's add or subtract would see the exact product (one fma) while the low word is
// counted a second time, and a negated product (dd_neg, a value leaving a sliding sum) is
// rebuilt as a fresh contractable multiply even under `fp contract(off)`, so leaving values
// did not cancel the entering ones.  The empty asm makes p opaque: nothing can fuse it.
__device__ __forceinline__ DD two_prod(double a, double b) {
#pragma clang fp contract(off)
  double p = a * b;
  asm volatile("" : "+v"(p));
  return DD{p, fma(a, b, -p)};
}
__device__ __forceinline__ DD dd_neg(DD x) { return DD{-x.hi, -x.lo}; }
// x - c exactly (TwoSum): the shifted image of a value, whatever the distance to the shift
__device__ __forceinline__ DD dd_diff(double x, double c) {
  DD y;
  two_sum(x, -c, y.hi, y.lo);
  return y;
}
// y^2 for a double-double y (error ~2^-104 relative)
__device__ __forceinline__ DD dd_sq(DD y) {
#pragma clang fp contract(off)
  DD p = two_prod(y.hi, y.hi);
  p.lo += 2.0 * y.hi * y.lo;
  return p;
}
// x / n for a double-double x (error ~2^-104 relative): the remainder of the rounded
// quotient comes from one fma, exactly
__device__ __forceinline__ DD dd_div(DD x, double n) {
#pragma clang fp contract(off)
  const double q1 = x.hi / n;
  const double lo = (fma(-q1, n, x.hi) + x.lo) / n;
  const double h = q1 + lo;
  return DD{h, lo - (h - q1)};
}
// x^2 / n for a double-double x (error ~2^-104 relative)
__device__ __forceinline__ DD dd_sq_div(DD x, double n) { return dd_div(dd_sq(x), n); }

}  // namespace mff
