// kmc_kinetics.h — the expressions of the bond kinetics recorder that the
// device kernels (kmc_kinetics.hip) and the sequential host counterparts
// (kmc_host_kin_*, kmc_host_observe.cpp) must evaluate alike (include/kmc.h, DESIGN.md
// §15): the bin rule of every lifetime and waiting time, and one receptor's
// transition at an update.  Integers only.
#pragma once
#include <stdint.h>

#include "kmc_math.h"  // KMC_HD

namespace kmck {

#define KIN_BINS 256   // KMC_KIN_BINS
#define KIN_HISTS 9    // KMC_KIN_HISTS
#define KIN_ROWS_UPD 7 // rows 0..6 are accumulated by the updates, 7 and 8 filled by a sample

// histogram rows
enum : int {
  KIN_ROW_RL = 0,        // lifetimes of R–L bonds born after begin
  KIN_ROW_RL_CENS = 1,   // ... of R–L bonds that existed at begin (left-censored)
  KIN_ROW_CIS_MONO = 2,  // cis bonds born after begin, mono at their last look
  KIN_ROW_CIS_CX = 3,    // ... complex at their last look
  KIN_ROW_CIS_CENS = 4,  // cis bonds that existed at begin
  KIN_ROW_REBIND_SAME = 5,   // waiting time until the receptor took its last ligand back
  KIN_ROW_REBIND_OTHER = 6,  // ... until it took another one
  KIN_ROW_RL_ALIVE = 7,  // ages of the living, non-censored R–L bonds
  KIN_ROW_CIS_ALIVE = 8  // ... cis bonds (at their lower member)
};

// bits of a receptor's record
enum : uint8_t { KIN_RL_CENS = 1, KIN_CIS_CENS = 2, KIN_CX = 4 };

// event and occupancy bits of one transition: bit k counts in counter k.
// 0..6 are the event counters in kmc_kin_out's order, 7..9 the occupancy.
enum : int {
  KIN_EV_RL_ON = 0, KIN_EV_RL_OFF, KIN_EV_RL_SWAP, KIN_EV_CIS_ON, KIN_EV_CIS_OFF_MONO, KIN_EV_CIS_OFF_CX,
  KIN_EV_CIS_SWAP, KIN_OCC_RL, KIN_OCC_MONO, KIN_OCC_CX, KIN_NCNT
};
#define KIN_NEV 7

// bin of a lifetime or waiting time v >= 0: exact below 16, then eight bins per
// octave; v >= 2^34 clamps into the last bin
KMC_HD int bin(int64_t v) {
  if (v < 16) return v < 0 ? 0 : (int)v;
  const int e = 63 - __builtin_clzll((unsigned long long)v);
  const int b = 16 + 8 * (e - 4) + (int)((v >> (e - 3)) & 7);
  return b < KIN_BINS - 1 ? b : KIN_BINS - 1;
}

// one receptor's record, in registers
struct Rec {
  int32_t rl_lig, rl_site, cis_with, last_lig;
  int64_t rl_since, cis_since, free_since;
  uint8_t bits;
};

// the receptor's current links as reference indices (0: none), and whether it
// or its cis partner holds a ligand
struct Cur {
  int32_t lig, site, cis;
  bool cx;
};

// the occupancy bits of receptor i (1-based) in state c
KMC_HD uint32_t occupancy(int32_t i, const Cur& c) {
  uint32_t m = 0;
  if (c.lig != 0) m |= 1u << KIN_OCC_RL;
  if (c.cis != 0 && i < c.cis) m |= 1u << (c.cx ? KIN_OCC_CX : KIN_OCC_MONO);
  return m;
}

// begin: the current links become the record
KMC_HD uint32_t begin(int32_t i, int64_t t, const Cur& c, Rec& r) {
  r.rl_lig = c.lig;
  r.rl_site = c.site;
  r.cis_with = c.cis;
  r.last_lig = 0;
  r.rl_since = r.cis_since = r.free_since = t;
  r.bits = (uint8_t)((c.lig != 0 ? KIN_RL_CENS : 0) | (c.cis != 0 ? KIN_CIS_CENS : 0) | (c.cis != 0 && c.cx ? KIN_CX : 0));
  return occupancy(i, c);
}

// update of receptor i (1-based) at step t, in the order of include/kmc.h.
// Returns the event and occupancy bits; at most three histogram entries
// (row[k], value[k]), k < *nh, are produced.
KMC_HD uint32_t transition(int32_t i, int64_t t, const Cur& c, Rec& r, int row[3], int64_t value[3], int* nh) {
  uint32_t m = 0;
  int n = 0;
  const bool rl_differs = c.lig != r.rl_lig || c.site != r.rl_site;
  if (r.rl_lig != 0 && rl_differs) {  // R–L ended
    row[n] = r.bits & KIN_RL_CENS ? KIN_ROW_RL_CENS : KIN_ROW_RL;
    value[n++] = t - r.rl_since;
    m |= 1u << KIN_EV_RL_OFF;
    r.last_lig = r.rl_lig;
    r.free_since = t;
    if (c.lig != 0) m |= 1u << KIN_EV_RL_SWAP;
  }
  if (c.lig != 0 && rl_differs) {  // R–L born
    m |= 1u << KIN_EV_RL_ON;
    if (r.last_lig != 0) {
      row[n] = c.lig == r.last_lig ? KIN_ROW_REBIND_SAME : KIN_ROW_REBIND_OTHER;
      value[n++] = t - r.free_since;
    }
    r.rl_since = t;
    r.bits &= (uint8_t)~KIN_RL_CENS;
  }
  const int32_t old = r.cis_with;
  if (old != 0 && i < old && c.cis != old) {  // cis ended (recorded at the lower member)
    const bool cx = r.bits & KIN_CX;
    row[n] = r.bits & KIN_CIS_CENS ? KIN_ROW_CIS_CENS : cx ? KIN_ROW_CIS_CX : KIN_ROW_CIS_MONO;
    value[n++] = t - r.cis_since;
    m |= 1u << (cx ? KIN_EV_CIS_OFF_CX : KIN_EV_CIS_OFF_MONO);
    if (c.cis != 0) m |= 1u << KIN_EV_CIS_SWAP;
  }
  if (c.cis != 0 && c.cis != old) {  // cis born
    r.cis_since = t;
    r.bits &= (uint8_t)~KIN_CIS_CENS;
    if (i < c.cis) m |= 1u << KIN_EV_CIS_ON;
  }
  r.rl_lig = c.lig;
  r.rl_site = c.site;
  r.cis_with = c.cis;
  r.bits = (uint8_t)((r.bits & ~KIN_CX) | (c.cis != 0 && c.cx ? KIN_CX : 0));
  *nh = n;
  return m | occupancy(i, c);
}

// what a sample reads off a record at step t_last: the row (7, 8) entries and
// the censored-alive flags.  bit 0: an R–L age, bit 1: a cis age, bit 2 / 3:
// a left-censored R–L / cis bond still alive
KMC_HD uint32_t alive(int32_t i, const Rec& r) {
  uint32_t m = 0;
  if (r.rl_lig != 0) m |= r.bits & KIN_RL_CENS ? 4u : 1u;
  if (r.cis_with != 0 && i < r.cis_with) m |= r.bits & KIN_CIS_CENS ? 8u : 2u;
  return m;
}

}  // namespace kmck
