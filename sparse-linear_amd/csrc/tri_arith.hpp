// tri_arith.hpp — the value arithmetic shared by the sparse triangular solves (trisolve.hip) and the incomplete
// factorisation that feeds them (ilu0.hip): a Double or a packed Complex Double, Data.Complex's product and its scaled
// quotient, every real operation separately rounded (-ffp-contract=off).  Device code only; included by those two files.
#pragma once

#include <math.h>

#include "common.hpp"

namespace spl {
namespace {

// ---- values: a double, or a packed (re, im) pair moved with 16-byte loads and stores ------------------------------
template <int VW>
struct Val;
template <>
struct Val<1> {
  double re;
};
template <>
struct Val<2> {
  double re, im;
};

template <int VW>
__device__ inline Val<VW> load_val(const double *x, int64_t o);
template <>
__device__ inline Val<1> load_val<1>(const double *x, int64_t o) {
  return Val<1>{x[o]};
}
template <>
__device__ inline Val<2> load_val<2>(const double *x, int64_t o) {
  const double2 z = *reinterpret_cast<const double2 *>(x + 2 * o);  // 16-byte aligned: the ABI checks the base
  return Val<2>{z.x, z.y};
}
__device__ inline void store_val(double *x, int64_t o, Val<1> v) { x[o] = v.re; }
__device__ inline void store_val(double *x, int64_t o, Val<2> v) {
  *reinterpret_cast<double2 *>(x + 2 * o) = make_double2(v.re, v.im);
}

__device__ inline Val<1> mul(Val<1> a, Val<1> b) { return Val<1>{a.re * b.re}; }
__device__ inline Val<2> mul(Val<2> a, Val<2> b) {  // (a :+ b) * (c :+ d) = (a c - b d) :+ (a d + b c)
  const double ac = a.re * b.re, bd = a.im * b.im, ad = a.re * b.im, bc = a.im * b.re;
  return Val<2>{ac - bd, ad + bc};
}
__device__ inline Val<1> sub(Val<1> a, Val<1> b) { return Val<1>{a.re - b.re}; }
__device__ inline Val<2> sub(Val<2> a, Val<2> b) { return Val<2>{a.re - b.re, a.im - b.im}; }

// `exponent` of RealFloat as frexp gives it: 0 for 0, and 0 for what is no finite number
__device__ inline int frexp_exponent(double x) {
  if (x == 0.0 || !isfinite(x)) return 0;
  int e = 0;
  (void)frexp(x, &e);
  return e;
}
__device__ inline Val<1> quot(Val<1> a, Val<1> d) { return Val<1>{a.re / d.re}; }
// (x :+ y) / (x' :+ y') of Data.Complex: both parts of the divisor scaled by 2^-max(exponent)
__device__ inline Val<2> quot(Val<2> a, Val<2> d) {
  const int ex = frexp_exponent(d.re), ey = frexp_exponent(d.im);
  const int k = -(ex > ey ? ex : ey);
  const double x2 = ldexp(d.re, k), y2 = ldexp(d.im, k);
  const double p0 = d.re * x2, p1 = d.im * y2;
  const double den = p0 + p1;
  const double a0 = a.re * x2, a1 = a.im * y2, b0 = a.im * x2, b1 = a.re * y2;
  const double nr = a0 + a1, ni = b0 - b1;
  return Val<2>{nr / den, ni / den};
}

template <int G>
__device__ inline Val<1> from_lane(Val<1> v, int l) {
  return G == 1 ? v : Val<1>{__shfl(v.re, l, G)};
}
template <int G>
__device__ inline Val<2> from_lane(Val<2> v, int l) {
  return G == 1 ? v : Val<2>{__shfl(v.re, l, G), __shfl(v.im, l, G)};
}

}  // namespace
}  // namespace spl
