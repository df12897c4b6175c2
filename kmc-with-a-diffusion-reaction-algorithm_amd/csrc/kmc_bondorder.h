// kmc_bondorder.h — the expressions of the bond-orientational order that the
// device kernels (kmc_bondorder.hip) and the sequential host counterparts
// (kmc_host_bond_order / kmc_host_bond_order_corr, kmc_host_observe.cpp) must evaluate
// bit for bit alike (include/kmc.h): the periodic displacement,
// the cell of the integer grid, the term, the normalisation and the two bin
// rules.  Doubles, no fused multiply-add (-ffp-contract=off), round_ / atan2 /
// sin / cos of kmc_math.h; every decision is an integer comparison.
#pragma once
#include <stdint.h>

#include "kmc_math.h"
#include "kmc_structure.h"  // round_small

namespace kmcb {

#define BO_MAX_FOLD 12         // KMC_BO_MAX_FOLD
#define BO_NN_ROWS 16          // KMC_BO_NN_ROWS
#define BO_HIST_BINS 1024      // most |psi| bins of the histogram
#define BO_CORR_BINS 4096      // most distance bins of the correlation
#define BO_NN_MAX 65535        // most neighbours of one protein
#define BO_NC_MAX 2048         // cells per axis of the grids (wider cells stay correct)
#define BO_BOX_MAX (1ll << 31) // BX, BY below it: |DX| < 2^30, D2 < 2^61
#define BO_SCALE 1073741824.0  // 2^30: the fixed-point quantum of a term

// X mod B in [0, B), the floor modulus (X may be negative), B >= 1
KMC_HD int64_t wrap(int64_t X, int64_t B) {
  X %= B;
  if (X < 0) X += B;
  return X;
}

// the periodic displacement d = X_j - X_i folded into [-B/2, B/2)
KMC_HD int64_t fold(int64_t d, int64_t B) {
  d = wrap(d, B);
  if (2 * d >= B) d -= B;
  return d;
}

// cell of the wrapped coordinate Xm in [0, B) on an axis of nc cells: < nc, and
// two points within B / nc of each other (periodically) lie in the same or in
// adjacent cells — in integers, no float margin.  Xm < 2^31, nc <= 2048.
KMC_HD int cell_of(int64_t Xm, int nc, int64_t B) { return (int)(Xm * nc / B); }

// one ordered pair's fixed-point term: |cos|, |sin| <= 1, so the scaled values
// lie within [-2^30, 2^30] and round_small is the (int64) round_ of kmc.h
KMC_HD void term(int n, int64_t DX, int64_t DY, int64_t* tc, int64_t* ts) {
  const double th = kmcm::atan2((double)DY, (double)DX);
  const double a = (double)n * th;
  *tc = kmcs::round_small(kmcm::cos(a) * BO_SCALE);
  *ts = kmcs::round_small(kmcm::sin(a) * BO_SCALE);
}

// pc (or ps) of a protein's sum C over N >= 1 neighbours: |C| <= N 2^30 and
// N <= 65535, so both operands are exact doubles and |result| <= 2^15
KMC_HD int64_t normalise(int64_t C, int64_t N) { return kmcs::round_small((double)C / ((double)N * 32768.0)); }

// bin of m = pc^2 + ps^2 (<= 2^31): #{k in 1..nbins-1 : k^2 2^30 <= nbins^2 m}.
// The square root only guesses; the integer comparisons decide.  nbins <= 1024:
// both sides stay below 2^52.
KMC_HD int mag_bin(int64_t m, int nbins) {
  const int64_t rhs = (int64_t)nbins * nbins * m;
  int b = (int)((double)nbins * kmcm::sqrt_((double)m) / 32768.0);
  b = b < 0 ? 0 : b > nbins - 1 ? nbins - 1 : b;
  while (b < nbins - 1 && (((int64_t)(b + 1) * (b + 1)) << 30) <= rhs) ++b;
  while (b > 0 && (((int64_t)b * b) << 30) > rhs) --b;
  return b;
}

// edge m of the correlation's distance bins in integer coordinates
KMC_HD int64_t corr_edge(int m, double dr) { return (int64_t)kmcm::round_(((double)m * dr) * 1024.0); }

// k = #{m in 1..nbins : E2[m] <= D2} for the non-decreasing squared edges
// E2[0..nbins] (E2[0] = 0), walked from the guess k
KMC_HD int corr_bin(const int64_t* E2, int nbins, int64_t D2, int k) {
  k = k < 0 ? 0 : k > nbins ? nbins : k;
  while (k < nbins && E2[k + 1] <= D2) ++k;
  while (k > 0 && E2[k] > D2) --k;
  return k;
}

}  // namespace kmcb
