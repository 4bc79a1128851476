// Double-double arithmetic of the normal-equation refit (mtp_normal.hip, mtp_normal.cpp): a value is the unevaluated sum
// hi + lo of two fp64 numbers, about 106 bits.  One header for device and host: __host__ __device__ under hipcc, plain
// inline functions under g++.  The algorithms are the classical error-free transformations (Knuth's TwoSum, TwoProd through
// a fused multiply-add, Dekker / Hida-Li-Bailey for the compound operations).
//
// Floating-point contraction is switched OFF from here to the end of the translation unit that includes this header: with
// hipcc's default, hi + x * y becomes one fma, and the error term of TwoSum is then taken against a different sum and is
// silently wrong.  No fast-math, no 128-bit float type.
#ifndef MTP_DD_HPP
#define MTP_DD_HPP

#include <cmath>

#if defined(__clang__)
#pragma clang fp contract(off)
#elif defined(__GNUC__)
#pragma GCC optimize("fp-contract=off")
#else
#pragma STDC FP_CONTRACT OFF
#endif

#if defined(__HIPCC__)
#define MTP_DD_FN __host__ __device__ inline
#else
#define MTP_DD_FN inline
#endif

struct mtp_dd {
  double hi, lo;
};

// s + e = a + b exactly (six additions, no condition on the magnitudes)
MTP_DD_FN mtp_dd two_sum(double a, double b)
{
  const double s = a + b;
  const double bb = s - a;
  const double e = (a - (s - bb)) + (b - bb);
  return mtp_dd{s, e};
}

// p + e = a * b exactly (barring over- and underflow)
MTP_DD_FN mtp_dd two_prod(double a, double b)
{
  const double p = a * b;
  const double e = __builtin_fma(a, b, -p);
  return mtp_dd{p, e};
}

// acc + x * y, the accumulation step of the Gram kernel: 1 mul, 1 fma, 8 add.  hi carries the running sum, lo collects
// the exact product error and the exact error of the sum by plain additions; the pair is NOT renormalised (dd_normal does
// that once, when the partial sum leaves the registers).
MTP_DD_FN mtp_dd dd_mac(mtp_dd acc, double x, double y)
{
  const mtp_dd p = two_prod(x, y);
  const mtp_dd s = two_sum(acc.hi, p.hi);
  return mtp_dd{s.hi, acc.lo + (s.lo + p.lo)};
}

// the same value with |lo| <= ulp(hi) / 2
MTP_DD_FN mtp_dd dd_normal(mtp_dd a) { return two_sum(a.hi, a.lo); }

// a + b (the accurate variant; TwoSum throughout, so the inputs need not be normalised)
MTP_DD_FN mtp_dd dd_add(mtp_dd a, mtp_dd b)
{
  mtp_dd s = two_sum(a.hi, b.hi);
  const mtp_dd t = two_sum(a.lo, b.lo);
  s.lo += t.hi;
  s = two_sum(s.hi, s.lo);
  s.lo += t.lo;
  return two_sum(s.hi, s.lo);
}

MTP_DD_FN mtp_dd dd_neg(mtp_dd a) { return mtp_dd{-a.hi, -a.lo}; }
MTP_DD_FN mtp_dd dd_sub(mtp_dd a, mtp_dd b) { return dd_add(a, dd_neg(b)); }

// a * b for a double b
MTP_DD_FN mtp_dd dd_mul_d(mtp_dd a, double b)
{
  mtp_dd p = two_prod(a.hi, b);
  p.lo += a.lo * b;
  return two_sum(p.hi, p.lo);
}

MTP_DD_FN mtp_dd dd_mul(mtp_dd a, mtp_dd b)
{
  mtp_dd p = two_prod(a.hi, b.hi);
  p.lo += a.hi * b.lo + a.lo * b.hi;
  return two_sum(p.hi, p.lo);
}

// a / b: three quotient digits, each from the remainder of the one before
MTP_DD_FN mtp_dd dd_div(mtp_dd a, mtp_dd b)
{
  const double q1 = a.hi / b.hi;
  mtp_dd r = dd_sub(a, dd_mul_d(b, q1));
  const double q2 = r.hi / b.hi;
  r = dd_sub(r, dd_mul_d(b, q2));
  const double q3 = r.hi / b.hi;
  const mtp_dd q = two_sum(q1, q2);
  return dd_add(q, mtp_dd{q3, 0.0});
}

// sqrt(a) for a >= 0 (Karp's trick: one Newton step on the fp64 root); 0 for a == 0
MTP_DD_FN mtp_dd dd_sqrt(mtp_dd a)
{
  if (!(a.hi > 0.0)) return mtp_dd{a.hi == 0.0 ? 0.0 : NAN, 0.0};
  const double x = 1.0 / std::sqrt(a.hi);
  const double ax = a.hi * x;
  const mtp_dd d = dd_sub(a, two_prod(ax, ax));
  return two_sum(ax, d.hi * (x * 0.5));
}

MTP_DD_FN double dd_round(mtp_dd a) { return a.hi + a.lo; }

#endif
