// kmc_host_state.h — what the host code shares about a kmc_state_view (host
// only: no device file includes it).  The layout of the view is stated here
// once: the bead index, a reader of the links, the status words and the bead
// (1,1) positions, and the three small tools every sequential counterpart of
// kmc_host_observe.cpp is built from (a component walk, a counting sort, the
// kmc_i128 arithmetic).
#pragma once
#include <cstddef>
#include <cstdint>
#include <vector>

#include "../../include/kmc.h"
#include "kmc_math.h"

namespace kmch_host {

// coordinate c of bead (j, k) of receptor / ligand i in ra / rb (j, k 1-based)
inline size_t RA(int na, int j, int k, int c, int i) { return (size_t)((((j - 1) * 4 + (k - 1)) * 3) + c) * na + i; }
inline size_t RB(int nb, int j, int k, int c, int i) { return (size_t)((((j - 1) * 2 + (k - 1)) * 3) + c) * nb + i; }

// A state view read by reference index q: 0 .. na - 1 the receptors, na .. n - 1
// the ligands.  Every word comes back as stored; the range policy is the
// caller's (as with the device's prot_links).
struct StateReader {
  const kmc_params* p;
  const kmc_state_view* v;
  int na, nb, n;
  StateReader(const kmc_params* p_, const kmc_state_view* v_)
      : p(p_), v(v_), na(p_ ? p_->n_a : 0), nb(p_ ? p_->n_b : 0), n(na + nb) {}
  bool ok(bool need_positions) const {
    return p && v && v->a_int && v->b_int && (!need_positions || (v->ra && v->rb)) && na >= 0 && nb >= 0;
  }
  // receptor i: status2, status3, nei2 (its ligand), nei4 (that ligand's site), nei3 (its cis partner)
  int32_t status2(int i) const { return v->a_int[0 * (size_t)na + i]; }
  int32_t status3(int i) const { return v->a_int[1 * (size_t)na + i]; }
  int32_t nei2(int i) const { return v->a_int[2 * (size_t)na + i]; }
  int32_t nei4(int i) const { return v->a_int[3 * (size_t)na + i]; }
  int32_t nei3(int i) const { return v->a_int[4 * (size_t)na + i]; }
  // ligand b: the status and the receptor of site k = 2..4
  int32_t site_status(int b, int k) const { return v->b_int[(size_t)(k - 1) * nb + b]; }
  int32_t site_nei(int b, int k) const { return v->b_int[(size_t)(4 + k - 1) * nb + b]; }
  // q's bond links (1-based reference numbers, 0: none): nei2, nei3 of a receptor, nei2..4 of a ligand
  int links(int q, int32_t nei[3]) const {
    if (q < na) {
      nei[0] = nei2(q);
      nei[1] = nei3(q);
      return 2;
    }
    for (int k = 2; k <= 4; ++k) nei[k - 2] = site_nei(q - na, k);
    return 3;
  }
  bool bound(int q) const {
    int32_t nei[3];
    const int m = links(q, nei);
    bool any = false;
    for (int e = 0; e < m; ++e) any = any || nei[e] != 0;
    return any;
  }
  // bead (1,1): coordinate c in A, and in units of 2^-10 A
  double pos(int q, int c) const { return q < na ? v->ra[RA(na, 1, 1, c, q)] : v->rb[RB(nb, 1, 1, c, q - na)]; }
  int64_t ipos(int q, int c) const { return (int64_t)kmcm::round_(pos(q, c) * 1024.0); }
  // the box along x (c = 0) or y (1) in units of 2^-10 A; box_q is the rounded double to test before the cast
  double box_q(int c) const { return kmcm::round_((c ? p->box_y : p->box_x) * 1024.0); }
  int64_t ibox(int c) const { return (int64_t)box_q(c); }
};

// The components of a graph on vertices 0 .. n - 1: a breadth-first walk from
// every vertex not yet labelled, in index order, so a walk's start r is its
// component's smallest member and label[] = r + 1 for all of it.
//   each(q, f):       calls f(j) for q's neighbours j in stored order; false stops the walk
//   reached(q, j):    j was first reached, from q
//   done(r, members): r's component is complete, members in the order they were reached (r first)
// Returns -1, or the vertex whose each() said false (label[] is then partial).
template <typename Each, typename Reached, typename Done>
int walk_components(int n, std::vector<int32_t>& label, Each each, Reached reached, Done done) {
  label.assign((size_t)n, 0);
  std::vector<int32_t> queue;
  queue.reserve((size_t)n);
  for (int r = 0; r < n; ++r) {
    if (label[(size_t)r]) continue;
    queue.clear();
    queue.push_back(r);
    label[(size_t)r] = r + 1;
    for (size_t h = 0; h < queue.size(); ++h) {
      const int q = queue[h];
      const bool ok = each(q, [&](int j) {
        if (label[(size_t)j]) return;
        label[(size_t)j] = r + 1;
        reached(q, j);
        queue.push_back(j);
      });
      if (!ok) return q;
    }
    done(r, queue);
  }
  return -1;
}

// Items 0 .. n - 1 sorted by key[t] in 0 .. nkeys - 1, stable in input order:
// key k holds item[start[k] .. start[k + 1]).
inline void counting_sort(const int32_t* key, size_t n, size_t nkeys, std::vector<int32_t>& start,
                          std::vector<int32_t>& item) {
  start.assign(nkeys + 1, 0);
  item.resize(n);
  for (size_t t = 0; t < n; ++t) start[(size_t)key[t] + 1] += 1;
  for (size_t k = 0; k < nkeys; ++k) start[k + 1] += start[k];
  std::vector<int32_t> fill(start.begin(), start.end() - 1);
  for (size_t t = 0; t < n; ++t) item[(size_t)fill[(size_t)key[t]]++] = (int32_t)t;
}

// f(c) for the 3 x 3 block of cells around cell (cx, cy) of a periodic ncx x ncy grid, row by row
template <typename F>
void block3x3(int cx, int cy, int ncx, int ncy, F f) {
  for (int oy = -1; oy <= 1; ++oy)
    for (int ox = -1; ox <= 1; ++ox) f((size_t)((cy + oy + ncy) % ncy) * ncx + (cx + ox + ncx) % ncx);
}

// kmc_i128 := x, and kmc_i128 += x (modulo 2^128)
inline void put(kmc_i128* w, __int128 x) {
  w->lo = (uint64_t)(unsigned __int128)x;
  w->hi = (int64_t)(x >> 64);
}
inline void add(kmc_i128* w, __int128 x) {
  const unsigned __int128 u = ((unsigned __int128)(uint64_t)w->hi << 64 | w->lo) + (unsigned __int128)x;
  w->lo = (uint64_t)u;
  w->hi = (int64_t)(uint64_t)(u >> 64);
}

}  // namespace kmch_host
