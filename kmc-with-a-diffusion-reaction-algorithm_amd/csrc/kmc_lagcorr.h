// kmc_lagcorr.h — the expressions of the multi-origin lag correlator that the
// device kernels (kmc_lagcorr.hip) and the sequential host counterpart
// (kmc_host_lag_*, kmc_host_observe.cpp) must evaluate alike (include/kmc.h, DESIGN.md
// §18): the integer minimum image, the firing schedule with its slot and row
// index, and the pair term.  Integers throughout; the only doubles are the
// cosines of F_s, rounded to fixed point term by term (kmc_structure.h).
#pragma once
#include <stdint.h>

#include "kmc_structure.h"  // axis_phase, round_small

namespace kmcl {

#define LAG_MAX_LEVELS 20      // KMC_LAG_MAX_LEVELS
#define LAG_MAX_SLOTS 16       // KMC_LAG_MAX_SLOTS
#define LAG_MAX_Q 4            // KMC_LAG_MAX_Q
#define LAG_CLASSES 5          // KMC_LAG_CLASSES
#define LAG_MAX_ROWS 168       // KMC_LAG_MAX_ROWS = 16 + 19 * 8
#define LAG_DISP_MAX 16384.0   // Å: the largest max_disp, F <= 2^24
#define LAG_SPLIT 25           // q = a 2^25 + b
#define LAG_SCALE 1073741824.0 // 2^30: the fixed-point quantum of a cosine

// the integer minimum image of a difference d in a box B >= 1: the floor
// modulus, folded into [-B/2, B/2) as kmcs::axis_phase folds its phase
KMC_HD int64_t min_image(int64_t d, int64_t B) {
  int64_t m = d % B;
  if (m < 0) m += B;
  if (2 * m >= B) m -= B;
  return m;
}

// §11's five classes from the links as the tracker names them
KMC_HD int cls(bool receptor, const int32_t l[3]) {
  if (receptor) return l[0] != 0 ? 2 : l[2] != 0 ? 1 : 0;
  return (l[0] | l[1] | l[2]) != 0 ? 4 : 3;
}

KMC_HD int rows(int L, int P) { return P + (L - 1) * (P / 2); }

// level l fires at update n when n mod 2^l == 0
KMC_HD bool fires(int64_t n, int l) { return (n & (((int64_t)1 << l) - 1)) == 0; }

// the first j of level l: the smaller j of a level above 0 repeat lags the level below holds
KMC_HD int j_first(int l, int P) { return l == 0 ? 1 : P / 2 + 1; }

KMC_HD int row_of(int l, int j, int P) { return l == 0 ? j - 1 : P + (l - 1) * (P / 2) + (j - P / 2 - 1); }

// one (level, j) pair of an update: the ring entry l * P + slot that holds the
// origin, the table row and the update n_k at which that origin was stored
struct Task {
  int32_t ring, row, nk;
};

// the tasks of update n >= 1, at most rows(L, P); every loop is bounded by L and P
KMC_HD int tasks(int64_t n, int L, int P, Task* out) {
  int cnt = 0;
  for (int l = 0; l < L; ++l) {
    if (!fires(n, l)) break;  // (a level that does not fire stops every level above it)
    const int64_t t = n >> l;
    for (int j = j_first(l, P); j <= P && j <= t; ++j) {
      out[cnt].ring = l * P + (int)((t - j) % P);
      out[cnt].row = row_of(l, j, P);
      out[cnt].nk = (int32_t)(n - ((int64_t)j << l));
      ++cnt;
    }
  }
  return cnt;
}

// the ring entry level l stores the new origin in after update n fired it
KMC_HD int store_ring(int64_t n, int l, int P) { return l * P + (int)((n >> l) % P); }

// far: the pair counts in n_far and nowhere else
KMC_HD bool far(int64_t Dx, int64_t Dy, int64_t F) {
  const int64_t ax = Dx < 0 ? -Dx : Dx, ay = Dy < 0 ? -Dy : Dy;
  return ax >= F || ay >= F;
}

// q = Dx² + Dy² of a pair that is not far: below 2^49 (F <= 2^24)
KMC_HD uint64_t sq(int64_t Dx, int64_t Dy) { return (uint64_t)(Dx * Dx) + (uint64_t)(Dy * Dy); }

// q = a 2^25 + b, a < 2^24, b < 2^25: a² < 2^48, ab < 2^49 and b² < 2^50 are
// summed apart in 64-bit words, and q² = a² 2^50 + ab 2^26 + b² (m4)
KMC_HD void split(uint64_t q, uint64_t* a2, uint64_t* ab, uint64_t* b2) {
  const uint64_t a = q >> LAG_SPLIT, b = q & (((uint64_t)1 << LAG_SPLIT) - 1);
  *a2 = a * a;
  *ab = a * b;
  *b2 = b * b;
}
KMC_HD unsigned __int128 m4(uint64_t a2, uint64_t ab, uint64_t b2) {
  return ((unsigned __int128)a2 << (2 * LAG_SPLIT)) + ((unsigned __int128)ab << (LAG_SPLIT + 1)) + b2;
}

// the F_s term of multiplier h: both axes' cosines in fixed point (|.| <= 2^31 + 2)
KMC_HD int64_t fs_term(int h, int64_t Dx, int64_t Dy, int64_t BX, int64_t BY) {
  double cx, cy, s;
  kmcs::axis_phase(h, Dx, BX, &cx, &s);
  kmcs::axis_phase(h, Dy, BY, &cy, &s);
  return kmcs::round_small(cx * LAG_SCALE) + kmcs::round_small(cy * LAG_SCALE);
}

// The configuration's bounds (include/kmc.h), on the host for both sides: what
// is wrong with it, or nullptr after max_jump and max_disp were resolved and
// J, F and the integer box computed.  (A NaN fails both comparisons of a pair.)
inline const char* check(int every, int levels, int slots, int nq, const int32_t* h, double box_x, double box_y,
                         double* max_jump, double* max_disp, int64_t* J, int64_t* F, int64_t* BX, int64_t* BY) {
  if (every < 1) return "lag: every >= 1";
  if (levels < 1 || levels > LAG_MAX_LEVELS) return "lag: 1 <= levels <= 20";
  if (slots < 2 || slots > LAG_MAX_SLOTS || slots % 2) return "lag: slots even, 2 <= slots <= 16";
  if (nq < 0 || nq > LAG_MAX_Q) return "lag: 0 <= nq <= 4";
  for (int k = 0; k < nq; ++k)
    if (h[k] < 1 || h[k] > 64) return "lag: 1 <= h[k] <= 64";
  const double half = 0.5 * (box_x < box_y ? box_x : box_y);
  if (!(*max_jump <= 0.0) && !(*max_jump <= half)) return "lag: max_jump above half the box (or not a number)";
  if (!(*max_disp <= 0.0) && !(*max_disp <= LAG_DISP_MAX)) return "lag: max_disp above 16384 (or not a number)";
  if (*max_jump <= 0.0) *max_jump = 0.5 * half;
  if (*max_disp <= 0.0) *max_disp = LAG_DISP_MAX;
  *BX = (int64_t)kmcm::round_(box_x * 1024.0);
  *BY = (int64_t)kmcm::round_(box_y * 1024.0);
  if (!(*BX >= 1 && *BY >= 1)) return "lag: a box below the coordinate quantum";
  *J = (int64_t)kmcm::round_(*max_jump * 1024.0);
  *F = (int64_t)kmcm::round_(*max_disp * 1024.0);
  return nullptr;
}

}  // namespace kmcl
