// kmc_pairdyn.h — the expressions of the pair-dynamics layer that the device
// kernels (kmc_pairdyn.hip) and the sequential host counterpart
// (kmc_host_pd_*, kmc_host_observe.cpp) must evaluate alike (include/kmc.h, DESIGN.md
// §20): the fold into the box, the search grid's cell, the bin of a squared
// distance against the squared integer edges, the validity of a displacement
// and the two terms of the displacement correlation.  Integers throughout: no
// square root and no double decides anything after the configuration's edges
// were rounded.
//
// The self table of part A is the FOLDED self part: the bin of the minimum
// image of fold(U_i) - fold(X0_i), which is the bin of the true displacement
// U_i - X0_i while |u| < box / 2 on both axes and of one of its periodic
// images beyond that.
#pragma once
#include <stdint.h>

#include "kmc_lagcorr.h"  // kmcl::min_image, LAG_DISP_MAX

namespace kmcp {

#define PD_MAX_BINS 256   // KMC_PD_MAX_BINS
#define PD_NC_MAX 2048    // cells per axis of the search grid (wider cells stay correct)
#define PD_JUMPED 1       // KMC_PD_JUMPED: the sticky bit of flags[i]
#define PD_CU_WORDS 6     // 64-bit words of a kmc_pd_cell: n_pairs, n_valid, dot (2), sq (2)

// the floor modulus of X into [0, B), B >= 1
KMC_HD int64_t fold(int64_t X, int64_t B) {
  int64_t m = X % B;
  if (m < 0) m += B;
  return m;
}

// the search grid's cell of a folded coordinate along one axis: below nc
KMC_HD int cell(int64_t fx, int nc, int64_t B) { return (int)(fx * nc / B); }

// d2 of a minimum-image displacement: |D| <= B / 2 < 2^30 on each axis, so below 2^61
KMC_HD uint64_t d2(int64_t Dx, int64_t Dy) { return (uint64_t)(Dx * Dx) + (uint64_t)(Dy * Dy); }

// k = #{m in 1..nbins : E2[m] <= d2}, E2 the squared edges (strictly increasing); k == nbins: not counted
KMC_HD int bin(const uint64_t* E2, int nbins, uint64_t q) {
  int lo = 0, hi = nbins;  // E2[lo] <= q (E2[0] = 0) and E2[m] > q for every m > hi
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (E2[mid] <= q)
      lo = mid;
    else
      hi = mid - 1;
  }
  return lo;
}

KMC_HD bool valid(int flags, int64_t ux, int64_t uy, int64_t F) {
  const int64_t ax = ux < 0 ? -ux : ux, ay = uy < 0 ? -uy : uy;
  return !(flags & PD_JUMPED) && ax < F && ay < F;
}

// the terms of a valid pair, |u| < F <= 2^24 on every axis: |dot| < 2^49, sq < 2^50
KMC_HD int64_t dot(int64_t uix, int64_t uiy, int64_t ujx, int64_t ujy) { return uix * ujx + uiy * ujy; }
KMC_HD int64_t sq(int64_t uix, int64_t uiy, int64_t ujx, int64_t ujy) {
  return uix * uix + uiy * uiy + ujx * ujx + ujy * ujy;
}

// ordered kind of part A, unordered kind of part B (species 0: receptor, 1: ligand)
KMC_HD int kind_a(int si, int sj) { return 2 * si + sj; }
KMC_HD int kind_b(int si, int sj) { return si + sj; }

// the half shell of part B: the cell itself, then (+1, 0), (-1, +1), (0, +1), (+1, +1)
KMC_HD void half_shell(int q, int* ox, int* oy) {
  *ox = q == 0 ? 0 : q == 1 ? 1 : q - 3;
  *oy = q < 2 ? 0 : 1;
}

struct Grid {
  int64_t BX, BY, J, F;
  int ncx, ncy, nbins;
};

// The configuration's bounds (include/kmc.h), on the host for both sides: what
// is wrong with it, or nullptr after max_jump and max_disp were resolved as
// kmcl::check resolves them, the integer box, J, F, the edges E[0..nbins] and
// the grid computed.  (A NaN fails both comparisons of a pair.)
inline const char* check(int every, int nbins, double r_max, double box_x, double box_y, double* max_jump,
                         double* max_disp, Grid* G, int64_t* E) {
  if (every < 1) return "pd: every >= 1";
  if (nbins < 1 || nbins > PD_MAX_BINS) return "pd: 1 <= nbins <= 256";
  if (!(r_max > 0.0) || !(r_max <= 1e9)) return "pd: r_max > 0 (and a number)";
  const double half = 0.5 * (box_x < box_y ? box_x : box_y);
  if (!(*max_jump <= 0.0) && !(*max_jump <= half)) return "pd: max_jump above half the box (or not a number)";
  if (!(*max_disp <= 0.0) && !(*max_disp <= LAG_DISP_MAX)) return "pd: max_disp above 16384 (or not a number)";
  if (*max_jump <= 0.0) *max_jump = 0.5 * half;
  if (*max_disp <= 0.0) *max_disp = LAG_DISP_MAX;
  if (!(box_x * 1024.0 < 2147483648.0) || !(box_y * 1024.0 < 2147483648.0)) return "pd: a box of 2^21 A or more";
  G->BX = (int64_t)kmcm::round_(box_x * 1024.0);
  G->BY = (int64_t)kmcm::round_(box_y * 1024.0);
  if (!(G->BX >= 1 && G->BY >= 1)) return "pd: a box below the coordinate quantum";
  G->J = (int64_t)kmcm::round_(*max_jump * 1024.0);
  G->F = (int64_t)kmcm::round_(*max_disp * 1024.0);
  G->nbins = nbins;
  const double dr = r_max / nbins;
  for (int m = 0; m <= nbins; ++m) {
    E[m] = (int64_t)kmcm::round_(m * dr * 1024.0);
    if (m > 0 && !(E[m] > E[m - 1])) return "pd: bin edges that do not increase (a bin below the coordinate quantum)";
  }
  const int64_t fx = G->BX / E[nbins], fy = G->BY / E[nbins];
  if (fx < 3 || fy < 3) return "pd: r_max above a third of the box (fewer than 3 cells along an axis)";
  G->ncx = (int)(fx < PD_NC_MAX ? fx : PD_NC_MAX);
  G->ncy = (int)(fy < PD_NC_MAX ? fy : PD_NC_MAX);
  return nullptr;
}

}  // namespace kmcp
