// kmc_structure.h — the two expressions of the structure factor that the
// device kernel (kmc_structure.hip) and the sequential host counterpart
// (kmc_host_structure_factor, kmc_host_observe.cpp) must evaluate bit for bit alike
// (include/kmc.h).  Doubles, no fused multiply-add
// (-ffp-contract=off), round_ / sin / cos of kmc_math.h.
#pragma once
#include <stdint.h>

#include "kmc_math.h"

namespace kmcs {

#define SK_MAX 64              // KMC_SK_MAX
#define SK_SCALE 1073741824.0  // 2^30: the fixed-point quantum of a term

// (cos, sin) of the axis phase 2π (m X mod B) / B of multiplier m >= 0,
// integer coordinate X (may be negative) and box B >= 1: the floor modulus,
// folded into [-B/2, B/2).  m <= 64 and |X| < 2^56: the product fits.
KMC_HD void axis_phase(int64_t m, int64_t X, int64_t B, double* c, double* s) {
  int64_t p = (m * X) % B;
  if (p < 0) p += B;
  if (2 * p >= B) p -= B;
  const double t = (double)p / (double)B;
  const double a = 6.283185307179586 * t;
  *c = kmcm::cos(a);
  *s = kmcm::sin(a);
}

// (int64) round_(v) for |v| < 2^31 - 1, through int32: the conversion truncates
// as round_'s trunc does, the fraction v - trunc(v) is exact, and half a unit or
// more of it moves the result one away from zero.  One conversion each way, a
// difference and two compares instead of round_'s 64-bit selects.
KMC_HD int64_t round_small(double v) {
  int32_t i = (int32_t)v;
  const double f = v - (double)i;
  i += (int32_t)(f >= 0.5) - (int32_t)(f <= -0.5);
  return (int64_t)i;
}

// One protein's fixed-point term at (h, k) from its axis phases ((cy, sy) of
// |k|, neg = k < 0).  |re|, |im| <= 1 + a few ulp, so the scaled products lie
// within [-2^30 - 1, 2^30 + 1] and round_small is the (int64) round_ of
// include/kmc.h.
KMC_HD void term(double cx, double sx, double cy, double sy, bool neg, int64_t* tc, int64_t* ts) {
  if (neg) sy = -sy;
  const double re = cx * cy - sx * sy;
  const double im = sx * cy + cx * sy;
  *tc = round_small(re * SK_SCALE);
  *ts = round_small(im * SK_SCALE);
}

}  // namespace kmcs
