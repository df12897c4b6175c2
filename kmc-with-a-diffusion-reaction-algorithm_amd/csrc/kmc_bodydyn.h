// kmc_bodydyn.h — the expressions of the body-dynamics layer that the device
// kernels (kmc_bodydyn.hip) and the sequential host counterpart
// (kmc_host_bd_*, kmc_host_observe.cpp) must evaluate alike (include/kmc.h, DESIGN.md
// §21): the per-member terms of a body's sums, the root correction that turns
// them into C and S, the verdict on a body and the three rotation terms.
// Integers throughout; the only doubles are atan2 and cos of the rotation
// angle, kmc_math.h's, rounded to fixed point body by body.
//
// The member sums are taken modulo 2^64 (unsigned arithmetic): they are exact
// wherever they are used — a VALID body for Su, a body that rotation applies to
// for C and S, see the bounds in include/kmc.h — and merely well defined
// elsewhere.
#pragma once
#include <stdint.h>

#include "kmc_lagcorr.h"  // kmcl::min_image, LAG_DISP_MAX

#define BD_MAX_SIZE 255   // KMC_BD_MAX_SIZE
#define BD_ROT_MAX 1023   // KMC_BD_ROT_MAX
#define BD_JUMPED 1       // KMC_BD_JUMPED
#define BD_CHANGED 2      // KMC_BD_CHANGED
#define BD_FAR 4          // in a body's OR of flags only: a member with |u| >= F
#define BD_WIDE 4         // KMC_BD_WIDE, beside the two spanning bits
#define BD_WIDE_AT ((int64_t)1 << 24)
#define BD_CELL_WORDS 16  // 64-bit words of a kmc_bd_cell
#define BD_SCALE_C 1073741824.0  // 2^30: the fixed-point quantum of a cosine
#define BD_SCALE_P 16777216.0    // 2^24: that of the angle
// the words of a kmc_bd_cell
enum { BD_W_BODIES, BD_W_SIZE, BD_W_PRISTINE, BD_W_INTACT, BD_W_GROWN, BD_W_BROKEN, BD_W_VALID, BD_W_ROT, BD_W_NULL,
       BD_W_SKIPPED, BD_W_C1, BD_W_C2, BD_W_M2, BD_W_PHI2 = 14 };
enum { BD_INTACT, BD_GROWN, BD_BROKEN };
enum { BD_IS_PRISTINE = 1, BD_IS_VALID = 2, BD_IS_ROT = 4 };

namespace kmcb {

KMC_HD bool wide(int64_t dx, int64_t dy) {
  const int64_t ax = dx < 0 ? -dx : dx, ay = dy < 0 ? -dy : dy;
  return ax >= BD_WIDE_AT || ay >= BD_WIDE_AT;
}

// what a member adds to its body's OR
KMC_HD int member_bits(int flags, int64_t ux, int64_t uy, int64_t F) {
  const int64_t ax = ux < 0 ? -ux : ux, ay = uy < 0 ? -uy : uy;
  return (flags & (BD_JUMPED | BD_CHANGED)) | (ax >= F || ay >= F ? BD_FAR : 0);
}

// the member terms D0 . u and D0 x u, modulo 2^64
KMC_HD uint64_t dot(int64_t ax, int64_t ay, int64_t bx, int64_t by) {
  return (uint64_t)ax * (uint64_t)bx + (uint64_t)ay * (uint64_t)by;
}
KMC_HD uint64_t cross(int64_t ax, int64_t ay, int64_t bx, int64_t by) {
  return (uint64_t)ax * (uint64_t)by - (uint64_t)ay * (uint64_t)bx;
}

// The sums of one body: n members, its static bits, ΣD0 and Σ|D0|², the
// member sums of a sample, the OR of member_bits, the smallest and the largest
// current label (0-based) with the size of the smallest one's component, and
// the root's displacement.
struct Sums {
  int n, bits, orbits, lmin, lmax, cur_size;
  uint64_t sd0x, sd0y, sd2, sux, suy, sdu, scu;
  int64_t urx, ury;
};

struct Verdict {
  int status, is;
  int64_t sux, suy, C, S;  // su when VALID, C and S when the rot bit is set, else 0
};

// C = Σ|D0|² + Σ D0.u − (ΣD0).u_r and S = Σ D0×u − (ΣD0)×u_r: the definition's
// Σ D0.D and Σ D0×D with D = D0 + u − u_r multiplied out (D0 × D0 = 0)
KMC_HD Verdict verdict(const Sums& b) {
  Verdict v = {0, 0, 0, 0, 0, 0};
  v.status = b.lmin != b.lmax ? BD_BROKEN : b.cur_size == b.n ? BD_INTACT : BD_GROWN;
  if (b.orbits & (BD_JUMPED | BD_CHANGED)) return v;
  v.is |= BD_IS_PRISTINE;
  if (b.orbits & BD_FAR) return v;
  v.is |= BD_IS_VALID;
  v.sux = (int64_t)b.sux;
  v.suy = (int64_t)b.suy;
  if (b.n < 2 || b.n > BD_ROT_MAX || b.bits) return v;
  v.is |= BD_IS_ROT;
  v.C = (int64_t)(b.sd2 + b.sdu - dot((int64_t)b.sd0x, (int64_t)b.sd0y, b.urx, b.ury));
  v.S = (int64_t)(b.scu - cross((int64_t)b.sd0x, (int64_t)b.sd0y, b.urx, b.ury));
  return v;
}

// the rotation terms of C, S not both zero: |c1|, |c2| <= 2^30, |p| < 2^26
KMC_HD void rot_terms(int64_t C, int64_t S, int64_t* c1, int64_t* c2, int64_t* p) {
  const double phi = kmcm::atan2((double)S, (double)C);
  *c1 = (int64_t)kmcm::round_(kmcm::cos(phi) * BD_SCALE_C);
  *c2 = (int64_t)kmcm::round_(kmcm::cos(2.0 * phi) * BD_SCALE_C);
  *p = (int64_t)kmcm::round_(phi * BD_SCALE_P);
}

// T = Su.x² + Su.y² of a VALID body: |Su| < 2^55
KMC_HD unsigned __int128 trans_term(int64_t sux, int64_t suy) {
  return (unsigned __int128)((__int128)sux * sux) + (unsigned __int128)((__int128)suy * suy);
}

// The configuration's bounds (include/kmc.h), on the host for both sides: what
// is wrong with it, or nullptr after max_jump and max_disp were resolved as
// kmcl::check resolves them and J, F and the integer box computed.
inline const char* check(int every, int max_size, double box_x, double box_y, double* max_jump, double* max_disp,
                         int64_t* J, int64_t* F, int64_t* BX, int64_t* BY) {
  if (every < 1) return "bd: every >= 1";
  if (max_size < 2 || max_size > BD_MAX_SIZE) return "bd: 2 <= max_size <= 255";
  const double half = 0.5 * (box_x < box_y ? box_x : box_y);
  if (!(*max_jump <= 0.0) && !(*max_jump <= half)) return "bd: max_jump above half the box (or not a number)";
  if (!(*max_disp <= 0.0) && !(*max_disp <= LAG_DISP_MAX)) return "bd: max_disp above 16384 (or not a number)";
  if (*max_jump <= 0.0) *max_jump = 0.5 * half;
  if (*max_disp <= 0.0) *max_disp = LAG_DISP_MAX;
  if (!(box_x * 1024.0 < 2147483648.0) || !(box_y * 1024.0 < 2147483648.0)) return "bd: a box of 2^21 A or more";
  *BX = (int64_t)kmcm::round_(box_x * 1024.0);
  *BY = (int64_t)kmcm::round_(box_y * 1024.0);
  if (!(*BX >= 1 && *BY >= 1)) return "bd: a box below the coordinate quantum";
  *J = (int64_t)kmcm::round_(*max_jump * 1024.0);
  *F = (int64_t)kmcm::round_(*max_disp * 1024.0);
  return nullptr;
}

}  // namespace kmcb
