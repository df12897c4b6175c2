// kmc_rings.h — what the device kernels (kmc_rings.hip) and the sequential
// host counterparts (kmc_host_network / kmc_host_rings, kmc_host_observe.cpp) of the
// ligand network's ring statistics must evaluate alike (include/kmc.h,
// DESIGN.md §17): the hop over a ligand's three sites with its validity
// checks, the order of the bridge ends, the site a ring leaves free and the
// chord rule.  Integers only; no position is read.
//
// The state's int arrays have one layout on both sides (a_int [5][na]: st2 st3
// nei2 nei4 nei3; b_int [8][nb]: st1..4 nei1..4); a link is an index + 1 (0:
// none) of the side's own numbering — slots on the device, reference indices on
// the host — so the same functions serve both.
#pragma once
#include <stdint.h>

#include "kmc_math.h"  // KMC_HD

namespace kmcr {

#define RG_MAX 12  // KMC_RING_MAX: the longest ring counted

// the three hops of ligand b, stage by stage (all three chains advance together: the loads of a stage are independent)
struct Hops {
  int32_t r[3];   // the receptor on site e + 2 (link, 0: the site is free)
  int32_t r2[3];  // its cis partner (link, 0: none)
  int32_t l[3];   // the partner's ligand as a 1-based LIGAND number (0: none — a half bridge when r2 != 0)
  int32_t s2[3];  // the site of l the partner sits on (2..4; 0 when l == 0)
  bool bad;       // a link of the wrong kind or an asymmetric bridge: nothing was read through it
};

// Follows the chains of ligand b (0-based within the ligands, b < nb).  Every
// link is range-checked before it is used as an index, and every bond is
// checked from its other side:
//   r  = nei[b][s]   a receptor in [0, na]; when != 0 its nei2 is b, its nei4 is s;
//   r' = nei3[r]     a receptor in [0, na], r' != r; when != 0 its nei3 is r;
//   l  = nei2[r']    0 or a ligand in (na, na + nb]; when != 0 s' = nei4[r'] is in 2..4 and nei[l][s'] is r'.
// With these the hop from (l, s') returns (b, s): the bridges are symmetric.
KMC_HD void hops(const int32_t* a_int, const int32_t* b_int, int na, int nb, int b, Hops& h) {
  const size_t NA = (size_t)na, NB = (size_t)nb;
  h.bad = false;
#pragma unroll
  for (int e = 0; e < 3; ++e) {
    h.r[e] = b_int[(size_t)(5 + e) * NB + b];  // nei[e + 2] of ligand b < nb
    if (h.r[e] < 0 || h.r[e] > na) h.bad = true, h.r[e] = 0;
    h.r2[e] = h.l[e] = h.s2[e] = 0;
  }
#pragma unroll
  for (int e = 0; e < 3; ++e) {
    if (h.r[e] == 0) continue;
    const size_t i = (size_t)h.r[e] - 1;  // < na
    const int32_t own = a_int[2 * NA + i], site = a_int[3 * NA + i], cis = a_int[4 * NA + i];
    if (own != na + b + 1 || site != e + 2 || cis < 0 || cis > na || cis == h.r[e]) h.bad = true;
    else h.r2[e] = cis;
  }
#pragma unroll
  for (int e = 0; e < 3; ++e) {
    if (h.r2[e] == 0) continue;
    const size_t i = (size_t)h.r2[e] - 1;  // < na
    const int32_t lig = a_int[2 * NA + i], site = a_int[3 * NA + i], back = a_int[4 * NA + i];
    if (back != h.r[e] || (lig != 0 && (lig <= na || lig > na + nb || site < 2 || site > 4))) h.bad = true;
    else if (lig != 0) h.l[e] = lig - na, h.s2[e] = site;
  }
#pragma unroll
  for (int e = 0; e < 3; ++e) {
    if (h.l[e] == 0) continue;
    if (b_int[(size_t)(3 + h.s2[e]) * NB + (size_t)(h.l[e] - 1)] != h.r2[e]) {  // nei[s'] of ligand l - 1 < nb
      h.bad = true;
      h.l[e] = h.s2[e] = 0;
    }
  }
}

// a receptor's two links: nei2 is 0 or a ligand in (na, na + nb], nei3 is 0 or another receptor in [1, na]
KMC_HD bool receptor_links_ok(int32_t nei2, int32_t nei3, int self_link, int na, int nb) {
  return (nei2 == 0 || (nei2 > na && nei2 <= na + nb)) && nei3 >= 0 && nei3 <= na && nei3 != self_link;
}

// index of a receptor in rec[4]
KMC_HD int rec_bin(int32_t nei2, int32_t nei3) { return (nei2 != 0) + 2 * (nei3 != 0); }

// of a bridge's two ends (b, s) and (l, s') the first one counts the bridge: a loop (l == b) once, at its lower site
KMC_HD bool first_end(int b, int s, int l, int s2) { return b < l || (b == l && s < s2); }

// the site a ring's ligand does not use on the ring (the sites are 2, 3 and 4)
KMC_HD int off_site(int in, int out) { return 9 - in - out; }

// The chord rule.  v[0..L) are the ring's ligands and off[i] the ligand
// bridged to v[i]'s off-ring site (0: none; both 1-based in one numbering): the
// ring is chordless when no off[i] is one of its own ligands.  At most L^2
// compares.  (A loop takes two sites of its ligand, so off[i] is never v[i].)
template <typename V, typename O>
KMC_HD bool chordless(int L, V v, O off) {
  for (int i = 0; i < L; ++i) {
    const int32_t o = off(i);
    if (o == 0) continue;
    for (int j = 0; j < L; ++j)
      if (v(j) == o) return false;
  }
  return true;
}

}  // namespace kmcr
