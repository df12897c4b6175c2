// kmc_encounter.h — the expressions of the encounter layer that the device
// kernels (kmc_encounter.hip) and the sequential host counterparts
// (kmc_host_reach_census, kmc_host_enc_*, kmc_host_observe.cpp) must evaluate alike
// (include/kmc.h): the engine's reaction gates restated on the
// committed state — the squared site distance, the two angles in gettheta's
// expression order (main.cpp:2329-2366) over kmcm::sqrt_ / kmcm::acos — the bin
// rules of the census, and one receptor's slot transition at an update.  Both
// sides compile this text with -ffp-contract=off.
#pragma once
#include <math.h>
#include <stdint.h>

#include "kmc_kinetics.h"  // kmck::bin: the bin rule of every duration
#include "kmc_math.h"      // KMC_HD, kmcm::

namespace kmce {

#define ENC_SLOTS 4     // KMC_ENC_SLOTS
#define ENC_BINS 256    // KMC_ENC_BINS (kmck::bin's)
#define ENC_HISTS 9     // KMC_ENC_HISTS
#define ENC_ROWS_UPD 8  // rows 0..7 are accumulated by the updates, row 8 is filled by a sample
#define ENC_REACT 2     // react_hist rows: slots that ended bound / otherwise
#define ENC_ACC_ROWS (ENC_ROWS_UPD + ENC_REACT)  // what an update adds into: the eight rows, then react_hist
#define ENC_MAX_ND 64   // KMC_REACH_MAX_ND
#define ENC_MAX_NA 36   // KMC_REACH_MAX_NA
#define ENC_CHANNELS 3

enum : int { CH_RL = 0, CH_MONO = 1, CH_CX = 2 };

// histogram rows
enum : int {
  ROW_BOUND = 0,           // the encounter ended in the bond
  ROW_SEPARATED = 1,       // the pair left reach
  ROW_LOST_RECEPTOR = 2,   // the receptor bound another site
  ROW_LOST_SITE = 3,       // the ligand site was taken by another receptor
  ROW_CENSORED_ENDED = 4,  // open at begin, ended otherwise than in the bond
  ROW_GEM_REBOUND = 5,     // geminate: the pair bound again
  ROW_GEM_ESCAPED = 6,     // geminate: the pair left reach
  ROW_GEM_LOST = 7,        // geminate: the receptor or the site was taken
  ROW_ALIVE = 8            // ages of the open, non-censored slots
};

// bits of a slot
enum : uint8_t { F_CENSORED = 1, F_GEMINATE = 2, F_REACTIVE = 4, F_WAS_REACTIVE = 8 };

// counters of one begin / update
enum : int {
  C_FROM_ENCOUNTER = 0, C_DIRECT, C_OPENED, C_ENDED, C_OVERFLOW, C_OCC_REACH, C_OCC_REACTIVE, C_OCC_FREE, ENC_NCNT
};
#define ENC_NEV 5  // the first five accumulate since begin, the occupancies are of the last look

// ---------------------------------------------------------------- gates
KMC_HD double d2(double dx, double dy, double dz) { return dx * dx + dy * dy + dz * dz; }

// gettheta (p1 is the origin at every call site)
KMC_HD double theta(double p0x, double p0y, double p0z, double p2x, double p2y, double p2z) {
  double lx0 = 0.0 - p0x, ly0 = 0.0 - p0y, lz0 = 0.0 - p0z;
  double lr0 = kmcm::sqrt_(lx0 * lx0 + ly0 * ly0 + lz0 * lz0);
  double lx1 = p2x - 0.0, ly1 = p2y - 0.0, lz1 = p2z - 0.0;
  double lr1 = kmcm::sqrt_(lx1 * lx1 + ly1 * ly1 + lz1 * lz1);
  double conv = 180 / 3.14159;
  double doth1 = -(lx1 * lx0 + ly0 * ly1 + lz0 * lz1);
  double doth2 = doth1 / (lr1 * lr0);
  if (doth2 > 1) doth2 = 1;
  if (doth2 < -1) doth2 = -1;
  return kmcm::acos(doth2) * conv;
}

struct V3 {
  double x, y, z;
};

// the R–L angles (main.cpp:1889-1911): r31, r32, r34 the receptor's beads
// [3][1], [3][2], [3][4]; lk1, lk2 the ligand's [k][1], [k][2]; l11, l12 its
// [1][1], [1][2].  What the gates compare: |theta_pd| and |theta_ot - 180|.
KMC_HD void rl_angles(const V3& r31, const V3& r32, const V3& r34, const V3& lk1, const V3& lk2, const V3& l11,
                      const V3& l12, double* pd, double* ot) {
  const double t_ot =
      theta(r31.x - r32.x, r31.y - r32.y, r31.z - r32.z, lk1.x - lk2.x, lk1.y - lk2.y, lk1.z - lk2.z);
  const double t_pd =
      theta(r31.x - r34.x, r31.y - r34.y, r31.z - r34.z, l11.x - l12.x, l11.y - l12.y, l11.z - l12.z);
  *pd = kmcm::fabs_(t_pd);
  *ot = kmcm::fabs_(t_ot - 180);
}

// the cis angle (main.cpp:1966-1981): beads [3][1], [3][3] of the lower (a) and the higher (b) receptor
KMC_HD double cis_angle(const V3& a31, const V3& a33, const V3& b31, const V3& b33) {
  return kmcm::fabs_(
      theta(a31.x - a33.x, a31.y - a33.y, a31.z - a33.z, b31.x - b33.x, b31.y - b33.y, b31.z - b33.z) - 180);
}

// ---------------------------------------------------------------- bins of the census
// squared edges of a channel: E2[m] = (cutoff m / nd)^2, m = 1..nd-1 (E2[0] = 0 is not compared)
inline void edges(double cutoff, int nd, double* E2) {
  E2[0] = 0.0;
  for (int m = 1; m < nd; ++m) {
    const double e = cutoff * m / nd;
    E2[m] = e * e;
  }
}
KMC_HD int dist_bin(const double* E2, int nd, double q) {
  int k = 0;
  for (int m = 1; m < nd; ++m) k += E2[m] <= q ? 1 : 0;
  return k;
}
// x in degrees, >= 0 (not a number: the last bin)
KMC_HD int ang_bin(double x, int na) {
  if (!(x >= 0.0)) return na - 1;
  const double v = x * (na / 180.0);
  return v >= (double)na ? na - 1 : (int)v;
}

// ---------------------------------------------------------------- the recorder
KMC_HD int32_t key_of(int32_t b, int32_t k) { return b << 2 | (k - 2); }  // ligand b = 1..n_b, site k = 2..4

// one receptor's record
struct Slots {
  int32_t lig, site;  // the link at the last update: reference index n_a + b and site, 0: none
  int32_t key[ENC_SLOTS];  // ascending, 0: empty (the empty ones last)
  int64_t since[ENC_SLOTS];
  int32_t nreact[ENC_SLOTS];
  uint8_t flags[ENC_SLOTS];
};

// one receptor's current look: its link and the in-reach triples, cut to the `cap` smallest keys
struct Cur {
  int32_t lig, site;
  int32_t n, total;
  int32_t key[ENC_SLOTS];
  uint8_t react[ENC_SLOTS];
};

KMC_HD void cur_clear(Cur& c, int32_t lig, int32_t site) {
  c.lig = lig;
  c.site = site;
  c.n = c.total = 0;
  for (int s = 0; s < ENC_SLOTS; ++s) {
    c.key[s] = 0;
    c.react[s] = 0;
  }
}

// one more in-reach triple: kept if it is among the cap smallest keys so far (any order of arrival gives the same set)
KMC_HD void cur_add(Cur& c, int cap, int32_t key, bool react) {
  c.total += 1;
  int32_t k = key;
  uint8_t r = react ? 1 : 0;
#pragma unroll
  for (int s = 0; s < ENC_SLOTS; ++s) {
    if (s >= cap) break;
    if (s >= c.n) {
      c.key[s] = k;
      c.react[s] = r;
      c.n += 1;
      return;
    }
    if (k < c.key[s]) {
      const int32_t tk = c.key[s];
      const uint8_t tr = c.react[s];
      c.key[s] = k;
      c.react[s] = r;
      k = tk;
      r = tr;
    }
  }
}

// the histogram entries of one update of one receptor: at most one per old slot
struct Events {
  int n;
  int row[ENC_SLOTS];
  int64_t val[ENC_SLOTS];
  int rrow[ENC_SLOTS];  // react_hist row: 0 bound, 1 otherwise
  int32_t rval[ENC_SLOTS];
};

KMC_HD void occupancy(const Cur& c, int32_t cnt[ENC_NCNT]) {
  cnt[C_OVERFLOW] += c.total - c.n;
  cnt[C_OCC_REACH] += c.n;
  for (int s = 0; s < ENC_SLOTS; ++s) cnt[C_OCC_REACTIVE] += s < c.n && c.react[s] ? 1 : 0;
  cnt[C_OCC_FREE] += c.lig == 0 ? 1 : 0;
}

// begin: the current set becomes the slots, left-censored
KMC_HD void begin(int64_t t, const Cur& c, Slots& r, int32_t cnt[ENC_NCNT]) {
  r.lig = c.lig;
  r.site = c.site;
  for (int s = 0; s < ENC_SLOTS; ++s) {
    const bool on = s < c.n;
    r.key[s] = on ? c.key[s] : 0;
    r.since[s] = on ? t : 0;
    r.nreact[s] = on && c.react[s] ? 1 : 0;
    r.flags[s] = (uint8_t)(on ? F_CENSORED | (c.react[s] ? F_REACTIVE | F_WAS_REACTIVE : 0) : 0);
  }
  occupancy(c, cnt);
}

// update of one receptor at step t, in the order of include/kmc.h.  occ[s]:
// the ligand site of old slot s is occupied now.  na: n_a (a link names the
// ligand by its reference index n_a + b).
KMC_HD void transition(int64_t t, int32_t na, const Cur& c, const bool occ[ENC_SLOTS], Slots& r, Events& ev,
                       int32_t cnt[ENC_NCNT]) {
  ev.n = 0;
  const bool born = c.lig != 0 && (c.lig != r.lig || c.site != r.site);
  const int32_t bkey = born ? key_of(c.lig - na, c.site) : 0;
  const int32_t gkey = r.lig != 0 ? key_of(r.lig - na, r.site) : 0;  // the bond of the last look
  bool from_encounter = false;
  for (int s = 0; s < ENC_SLOTS; ++s) {
    const int32_t k = r.key[s];
    if (k == 0) continue;
    int row;
    bool bound = false;
    if (born && k == bkey) {
      bound = from_encounter = true;
      row = r.flags[s] & F_GEMINATE ? ROW_GEM_REBOUND : ROW_BOUND;
    } else {
      bool kept = false;
      for (int q = 0; q < ENC_SLOTS; ++q) kept = kept || (q < c.n && c.key[q] == k);
      if (kept) continue;
      const int outcome = c.lig != 0 ? ROW_LOST_RECEPTOR : occ[s] ? ROW_LOST_SITE : ROW_SEPARATED;
      row = r.flags[s] & F_CENSORED   ? ROW_CENSORED_ENDED
            : r.flags[s] & F_GEMINATE ? (outcome == ROW_SEPARATED ? ROW_GEM_ESCAPED : ROW_GEM_LOST)
                                      : outcome;
    }
    ev.row[ev.n] = row;
    ev.val[ev.n] = t - r.since[s];
    ev.rrow[ev.n] = bound ? 0 : 1;
    ev.rval[ev.n] = r.nreact[s];
    ev.n += 1;
    cnt[C_ENDED] += 1;
  }
  if (born) cnt[from_encounter ? C_FROM_ENCOUNTER : C_DIRECT] += 1;
  Slots w;
  w.lig = c.lig;
  w.site = c.site;
  for (int q = 0; q < ENC_SLOTS; ++q) {
    w.key[q] = 0;
    w.since[q] = 0;
    w.nreact[q] = 0;
    w.flags[q] = 0;
    if (q >= c.n) continue;
    const int32_t k = c.key[q];
    const uint8_t now = (uint8_t)(c.react[q] ? F_REACTIVE | F_WAS_REACTIVE : 0);
    int o = -1;
    for (int s = 0; s < ENC_SLOTS; ++s)
      if (r.key[s] == k) o = s;
    w.key[q] = k;
    if (o >= 0) {  // the slot continues
      w.since[q] = r.since[o];
      w.nreact[q] = r.nreact[o] + (c.react[q] ? 1 : 0);
      w.flags[q] = (uint8_t)((r.flags[o] & (F_CENSORED | F_GEMINATE | F_WAS_REACTIVE)) | now);
    } else {  // a new encounter; geminate when the bond to this very site ended at this update
      w.since[q] = t;
      w.nreact[q] = c.react[q] ? 1 : 0;
      w.flags[q] = (uint8_t)((k == gkey ? F_GEMINATE : 0) | now);
      cnt[C_OPENED] += 1;
    }
  }
  r = w;
  occupancy(c, cnt);
}

// smallest T with sqrt(T) >= c, so that  sqrt(s) < c  <=>  s < T  (the engine's thresholds)
inline double sqrt_threshold(double c) {
  double t = c * c;
  while (sqrt(t) >= c) t = nextafter(t, 0.0);
  while (sqrt(t) < c) t = nextafter(t, INFINITY);
  return t;
}

}  // namespace kmce
