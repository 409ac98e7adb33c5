// EXP and POW to within a rounding of the exact value, for the few places where a result of the reference is ill-conditioned in one of them
// (CDUSTARZ0: Z0 = ZREF / (EXP(XKAPPA U10 / USTAR) - 1) moves by ten roundings when CD = (...) U10**P2CD moves by one).  The host's mathematical
// library rounds these functions correctly at almost every argument; the device's are good to a rounding or two.  Double precision: the value
// is formed as an unevaluated sum of two doubles (Dekker / Knuth sums and products, about 100 bits) and rounded once.  Single precision: the
// double precision function, rounded once more.  Plain host-and-device code, so that a host program can hold it against the host's library.
#pragma once
#include <cmath>

#if defined(__HIPCC__)
#define DD_FN __host__ __device__ __forceinline__
#else
#define DD_FN inline
#endif

struct dd_t { double h, l; };

DD_FN dd_t dd_quick_sum(double a, double b) {
#pragma clang fp contract(off)
  const double s = a + b;
  return {s, b - (s - a)};
}
DD_FN dd_t dd_two_sum(double a, double b) {
#pragma clang fp contract(off)
  const double s = a + b, bb = s - a;
  return {s, (a - (s - bb)) + (b - bb)};
}
DD_FN dd_t dd_two_prod(double a, double b) {
#pragma clang fp contract(off)
  const double p = a * b;
  return {p, __builtin_fma(a, b, -p)};
}
DD_FN dd_t dd_add(dd_t a, dd_t b) {
#pragma clang fp contract(off)
  dd_t s = dd_two_sum(a.h, b.h);
  const dd_t t = dd_two_sum(a.l, b.l);
  s.l += t.h;
  s = dd_quick_sum(s.h, s.l);
  s.l += t.l;
  return dd_quick_sum(s.h, s.l);
}
DD_FN dd_t dd_mul(dd_t a, dd_t b) {
#pragma clang fp contract(off)
  dd_t p = dd_two_prod(a.h, b.h);
  p.l += a.h * b.l + a.l * b.h;
  return dd_quick_sum(p.h, p.l);
}
DD_FN dd_t dd_mul_d(dd_t a, double b) {
#pragma clang fp contract(off)
  dd_t p = dd_two_prod(a.h, b);
  p.l += a.l * b;
  return dd_quick_sum(p.h, p.l);
}

// EXP(a) - 1 is not what is returned: EXP(a), for |a| up to a few hundred
DD_FN dd_t dd_exp(dd_t a) {
#pragma clang fp contract(off)
  const dd_t LN2 = {6.931471805599452862e-01, 2.319046813846299558e-17};
  const double k = __builtin_rint(a.h * 1.4426950408889634);
  dd_t r = dd_add(a, dd_mul_d(LN2, -k));      // |r| <= 0.35
  r.h *= 0x1p-9; r.l *= 0x1p-9;               // |r| <= 6.8e-4: the series ends at r**8 / 8! < 1.2e-30
  const double t = r.h;
  const double tail = t * t * t * (1.0 / 6 + t * (1.0 / 24 + t * (1.0 / 120 + t * (1.0 / 720 + t * (1.0 / 5040 + t * (1.0 / 40320))))));
  dd_t s = dd_add(r, dd_mul_d(dd_mul(r, r), 0.5));      // s = EXP(r) - 1
  s = dd_add(s, dd_t{tail, 0.0});
  for (int i = 0; i < 9; i++) s = dd_add(dd_mul_d(s, 2.0), dd_mul(s, s));      // (1 + s)**2 - 1
  const dd_t e = dd_add(dd_t{1.0, 0.0}, s);
  const int ik = (int)k;
  return {__builtin_ldexp(e.h, ik), __builtin_ldexp(e.l, ik)};
}
// LOG(x), x > 0: one step of Newton on the library's logarithm
DD_FN dd_t dd_log(double x, double y0) {
#pragma clang fp contract(off)
  const dd_t t = dd_mul_d(dd_exp(dd_t{-y0, 0.0}), x);      // x EXP(-y0) = 1 + d, |d| about 1e-16: LOG(1 + d) = d - d**2 / 2 ...
  return dd_add(dd_t{y0, 0.0}, dd_add(t, dd_t{-1.0, 0.0}));
}

DD_FN double ref_exp(double x) { return dd_exp(dd_t{x, 0.0}).h; }
DD_FN double ref_pow(double x, double y) { return dd_exp(dd_mul_d(dd_log(x, log(x)), y)).h; }
DD_FN float ref_exp(float x) { return (float)exp((double)x); }
DD_FN float ref_pow(float x, float y) { return (float)pow((double)x, (double)y); }
