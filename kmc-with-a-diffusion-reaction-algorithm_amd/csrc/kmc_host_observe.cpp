// kmc_host_observe.cpp — the sequential counterparts (kmc_host_*) of the
// read-only layers, in kmc_observe.hip's order: what the GPU tests compare
// each layer's device result with, bit for bit.  Every function reads as its
// definition in include/kmc.h; the expressions both sides must evaluate alike
// are the layers' headers' (kmc_bondorder.h, kmc_kinetics.h, ...), the state
// view's layout, the component walk, the counting sort and the 128-bit sums
// are kmc_host_state.h's.  The error string is kmc_io.cpp's
// (kmc_host_last_error); that file does not depend on this one.
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <string>
#include <utility>
#include <vector>

#include "../../include/kmc.h"
#include "kmc_bodydyn.h"
#include "kmc_bondorder.h"
#include "kmc_coag.h"
#include "kmc_encounter.h"
#include "kmc_host.h"
#include "kmc_host_state.h"
#include "kmc_kinetics.h"
#include "kmc_lagcorr.h"
#include "kmc_math.h"
#include "kmc_orient.h"
#include "kmc_pairdyn.h"
#include "kmc_proximity.h"
#include "kmc_rings.h"
#include "kmc_structure.h"

namespace {

using kmch_host::RA;
using kmch_host::RB;
using kmch_host::StateReader;
using kmch_host::add;
using kmch_host::block3x3;
using kmch_host::counting_sort;
using kmch_host::put;
using kmch_host::walk_components;

int fail(int code, const std::string& msg) {
  kmch_host::set_error(msg);
  return code;
}

// f(j) for every bond link of q that is set (j 0-based), in stored order; false at one that leaves 1..n
template <typename F>
bool bond_links(const StateReader& s, int q, F f) {
  int32_t nei[3];
  const int m = s.links(q, nei);
  for (int e = 0; e < m; ++e) {
    if (nei[e] == 0) continue;
    if (nei[e] < 1 || nei[e] > s.n) return false;
    f(nei[e] - 1);
  }
  return true;
}

// protein i's integer position and links as the trackers (lag, rot, pd, bd) name them: a link outside 1..n reads 0
void tracked(const StateReader& s, int i, int64_t X[2], int32_t l[3]) {
  auto ref = [&](int32_t x) { return x >= 1 && x <= s.n ? x : 0; };
  for (int c = 0; c < 2; ++c) X[c] = s.ipos(i, c);
  if (i < s.na) {
    l[0] = ref(s.nei2(i));
    l[1] = s.nei4(i);
    l[2] = ref(s.nei3(i));
  } else {
    s.links(i, l);
    for (int k = 0; k < 3; ++k) l[k] = ref(l[k]);
  }
}

// the opening check of a recorder's begin (`cfg` counts) and update: one condition and one message per layer
int recorder_args(const StateReader& s, const char* layer, const char* arrays, bool begin, const void* cfg,
                  bool view_ok, const void* acc) {
  if (s.ok(true) && (!begin || cfg) && view_ok && acc) return KMC_OK;
  return fail(KMC_ERR_ARG, std::string(layer) + ": params, state, " + (begin ? "the configuration, " : "") +
                               "the view's " + arrays + " arrays and acc are needed");
}

int not_due(const char* layer, int64_t every) {
  return fail(KMC_ERR_ARG,
              std::string(layer) + ": an update is due " + std::to_string(every) + " steps after the last one");
}

// Bond order and prox: the set's integer coordinates, every protein's (C, S, N)
// and the counting-sorted periodic cell grid (kmcb::cell_of / wrap) the
// neighbours within a cutoff come from, so the cost is linear in the set.
struct BoHost {
  int n = 0;          // proteins of the species
  int64_t B[2] = {0, 0};
  std::vector<uint8_t> sel;
  std::vector<int64_t> X, Y, C, S;
  std::vector<int32_t> nn;
  int cell_x(int i, int ncx) const { return kmcb::cell_of(kmcb::wrap(X[i], B[0]), ncx, B[0]); }
  int cell_y(int i, int ncy) const { return kmcb::cell_of(kmcb::wrap(Y[i], B[1]), ncy, B[1]); }
};

// h->B from the box, which the integer grid takes from 2^-10 A to below 2^21 A; the message names `layer`
int bo_box(const StateReader& s, const char* layer, BoHost* h) {
  const double bx = s.box_q(0), by = s.box_q(1);
  if (!(bx >= 1.0) || !(by >= 1.0) || !(bx < (double)BO_BOX_MAX) || !(by < (double)BO_BOX_MAX))
    return fail(KMC_ERR_ARG, std::string(layer) + ": the box is below 2^-10 A or not below 2^21 A");
  h->B[0] = (int64_t)bx;
  h->B[1] = (int64_t)by;
  return KMC_OK;
}

struct BoCells {
  int ncx = 0, ncy = 0;
  std::vector<int32_t> start, item;  // cell c holds item[start[c] .. start[c + 1])
  // the cells are the box over `cut`, at most BO_NC_MAX along an axis
  void build(const BoHost& h, const std::vector<int32_t>& who, int64_t cut) {
    ncx = (int)std::min<int64_t>(h.B[0] / cut, BO_NC_MAX);
    ncy = (int)std::min<int64_t>(h.B[1] / cut, BO_NC_MAX);
    std::vector<int32_t> cell(who.size());
    for (size_t t = 0; t < who.size(); ++t) cell[t] = h.cell_y(who[t], ncy) * ncx + h.cell_x(who[t], ncx);
    counting_sort(cell.data(), who.size(), (size_t)ncx * ncy, start, item);
    for (int32_t& t : item) t = who[(size_t)t];
  }
  // f(j) for every item of the 3 x 3 cells around point i's cell (distinct cells: ncx, ncy >= 3)
  template <typename F>
  void around(const BoHost& h, int i, F f) const {
    block3x3(h.cell_x(i, ncx), h.cell_y(i, ncy), ncx, ncy, [&](size_t c) {
      for (int32_t t = start[c]; t < start[c + 1]; ++t) f(item[(size_t)t]);
    });
  }
};

}  // namespace

// (The kmc_host_* below take their C linkage from their declarations in include/kmc.h.)

// Components of the bond graph and their census (include/kmc.h), sequential:
// the walk's start is the component's smallest index — its label.
int kmc_host_census(const kmc_params* p, const kmc_state_view* v, int32_t* label, int32_t max_r, int32_t max_l,
                    int64_t* hist, kmc_census* out) {
  const StateReader s(p, v);
  if (!s.ok(false) || !out || max_r < 0 || max_l < 0)
    return fail(KMC_ERR_ARG, "census: params, state and out are needed, max_r and max_l >= 0");
  std::vector<int32_t> lab;
  std::memset(out, 0, sizeof *out);
  if (hist) std::fill(hist, hist + ((size_t)max_r + 1) * ((size_t)max_l + 1), (int64_t)0);
  const int bad = walk_components(
      s.n, lab, [&](int q, auto f) { return bond_links(s, q, f); }, [](int, int) {},
      [&](int r, const std::vector<int32_t>& members) {
        const int size = (int)members.size();
        int nr = 0;
        for (int q : members) nr += q < s.na;
        const int nl = size - nr;
        out->n_components += 1;
        if (nl >= 1 && size > 1) {
          out->n_complexes += 1;
          out->proteins_in_complexes += size;
        }
        if (nl == 0 && nr == 2) out->n_cis_dimers += 1;
        if (size > out->max_size) {  // (components come in label order: the first of a size keeps the tie)
          out->max_size = size;
          out->max_receptors = nr;
          out->max_ligands = nl;
          out->max_label = r + 1;
        }
        if (hist) hist[(size_t)std::min(nr, (int)max_r) * ((size_t)max_l + 1) + std::min(nl, (int)max_l)] += 1;
      });
  if (bad >= 0) return fail(KMC_ERR_STATE, "census: a bond link of protein " + std::to_string(bad + 1) + " leaves the state");
  if (label) std::copy(lab.begin(), lab.end(), label);
  return KMC_OK;
}

// Cluster geometry (include/kmc.h), sequential: the walk's start is the label,
// its image shift (0, 0), and a member takes its shift from the member that
// reached it; then every edge of the component is compared with the shifts
// (the spanning bits), and the moments are summed in 128-bit integers.
int kmc_host_cluster_geometry(const kmc_params* p, const kmc_state_view* v, int32_t* label, int32_t* shift,
                              uint8_t* span, int32_t max_size, kmc_geom_bin* table, kmc_geom* out) {
  const StateReader s(p, v);
  if (!s.ok(true) || !out || max_size < 2)
    return fail(KMC_ERR_ARG, "cluster geometry: params, state and out are needed, max_size >= 2");
  const int n = s.n;
  const double box[2] = {p->box_x, p->box_y};
  const int64_t B[2] = {s.ibox(0), s.ibox(1)};
  auto edge = [&](int i, int j, int c) { return -(int)kmcm::round_((s.pos(j, c) - s.pos(i, c)) / box[c]); };
  typedef __int128 i128;
  std::vector<int32_t> lab, sx((size_t)n, 0), sy((size_t)n, 0);
  std::vector<uint8_t> sp((size_t)n, 0);
  std::vector<i128> sum_m(table ? (size_t)max_size + 1 : 0, 0);
  std::memset(out, 0, sizeof *out);
  if (table) std::memset(table, 0, sizeof(kmc_geom_bin) * ((size_t)max_size + 1));
  const int bad = walk_components(
      n, lab, [&](int q, auto f) { return bond_links(s, q, f); },
      [&](int q, int j) {
        sx[j] = sx[q] + edge(q, j, 0);
        sy[j] = sy[q] + edge(q, j, 1);
      },
      [&](int r, const std::vector<int32_t>& members) {
        int bits = 0;
        for (int q : members)
          bond_links(s, q, [&](int j) {
            if (sx[j] - sx[q] != edge(q, j, 0)) bits |= KMC_SPAN_X;
            if (sy[j] - sy[q] != edge(q, j, 1)) bits |= KMC_SPAN_Y;
          });
        const int size = (int)members.size();
        if (size > out->largest_size) {  // (components come in label order: the first of a size keeps the tie)
          out->largest_size = size;
          out->largest_label = r + 1;
          out->largest_span = bits;
        }
        if (bits) {
          out->n_spanning += 1;
          out->n_span_x += (bits & KMC_SPAN_X) != 0;
          out->n_span_y += (bits & KMC_SPAN_Y) != 0;
          out->proteins_in_spanning += size;
          for (int q : members) {
            sp[q] = (uint8_t)bits;
            sx[q] = sy[q] = 0;
          }
          return;
        }
        if (size < 2) return;
        out->n_measured += 1;
        if (!table) return;
        int64_t s1[2] = {0, 0};
        i128 s2 = 0;
        for (int q : members)
          for (int c = 0; c < 2; ++c) {
            const int64_t d = (s.ipos(q, c) + (int64_t)(c ? sy[q] : sx[q]) * B[c]) - s.ipos(r, c);
            s1[c] += d;
            s2 += (i128)d * d;
          }
        const int k = std::min(size, (int)max_size);
        table[k].count += 1;
        table[k].sum_size += size;
        sum_m[k] += (i128)size * s2 - ((i128)s1[0] * s1[0] + (i128)s1[1] * s1[1]);
      });
  if (bad >= 0)
    return fail(KMC_ERR_STATE,
                "cluster geometry: a bond link of protein " + std::to_string(bad + 1) + " leaves the state");
  for (size_t k = 0; k < sum_m.size(); ++k) put(&table[k].sum_m, sum_m[k]);
  if (label) std::copy(lab.begin(), lab.end(), label);
  if (shift) {
    std::copy(sx.begin(), sx.end(), shift);
    std::copy(sy.begin(), sy.end(), shift + n);
  }
  if (span) std::copy(sp.begin(), sp.end(), span);
  return KMC_OK;
}

// Structure factor (include/kmc.h), sequential: per selected protein the axis
// tables of h = 0..hmax and |k| = 0..kmax, then one term per wave vector added
// to its species' sums.
int kmc_host_structure_factor(const kmc_params* p, const kmc_state_view* v, int32_t hmax, int32_t kmax,
                              int32_t select, int64_t* sums, int64_t n_sel[2]) {
  const StateReader s(p, v);
  if (!s.ok(true) || !sums || !n_sel || hmax < 0 || hmax > KMC_SK_MAX || kmax < 0 || kmax > KMC_SK_MAX ||
      (select != KMC_SK_ALL && select != KMC_SK_BOUND))
    return fail(KMC_ERR_ARG,
                "structure factor: params, state, sums and n_sel are needed, 0 <= hmax, kmax <= 64, select 0 or 1");
  const int64_t B[2] = {s.ibox(0), s.ibox(1)};
  if (B[0] < 1 || B[1] < 1) return fail(KMC_ERR_ARG, "structure factor: the box is below 2^-10 A");
  const int W = 2 * kmax + 1;
  const size_t nq = (size_t)(hmax + 1) * W;
  std::memset(sums, 0, sizeof(int64_t) * 4 * nq);
  n_sel[0] = n_sel[1] = 0;
  double cx[KMC_SK_MAX + 1], sx[KMC_SK_MAX + 1], cy[KMC_SK_MAX + 1], sy[KMC_SK_MAX + 1];
  for (int q = 0; q < s.n; ++q) {
    const int sp = q < s.na ? 0 : 1;
    if (select == KMC_SK_BOUND && !s.bound(q)) continue;
    n_sel[sp] += 1;
    const int64_t X = s.ipos(q, 0), Y = s.ipos(q, 1);
    for (int h = 0; h <= hmax; ++h) kmcs::axis_phase(h, X, B[0], &cx[h], &sx[h]);
    for (int k = 0; k <= kmax; ++k) kmcs::axis_phase(k, Y, B[1], &cy[k], &sy[k]);
    int64_t* C = sums + (size_t)(2 * sp) * nq;
    int64_t* S = sums + (size_t)(2 * sp + 1) * nq;
    for (int h = 0; h <= hmax; ++h)
      for (int k = -kmax; k <= kmax; ++k) {
        const int ak = k < 0 ? -k : k;
        int64_t tc, ts;
        kmcs::term(cx[h], sx[h], cy[ak], sy[ak], k < 0, &tc, &ts);
        C[(size_t)h * W + (k + kmax)] += tc;
        S[(size_t)h * W + (k + kmax)] += ts;
      }
  }
  return KMC_OK;
}

// Bond-orientational order (include/kmc.h), sequential.  The local pass leaves
// the set, its integer coordinates and every protein's (C, S, N) by the
// species' reference index.
namespace {

int bo_host_local(const kmc_params* p, const kmc_state_view* v, int32_t which, int32_t mode, int32_t fold,
                  double r_cut, int32_t select, BoHost* h) {
  const StateReader s(p, v);
  if (!s.ok(true) || (which != KMC_BO_A && which != KMC_BO_B) || (mode != KMC_BO_WITHIN && mode != KMC_BO_LINKED) ||
      fold < 1 || fold > KMC_BO_MAX_FOLD || (select != KMC_BO_ALL && select != KMC_BO_BOUND) ||
      (mode == KMC_BO_LINKED && which != KMC_BO_B))
    return fail(KMC_ERR_ARG,
                "bond order: params and state are needed, which 0 or 1, mode 0 or 1 (linked: ligands only), 1 <= fold <= 12, select 0 or 1");
  const int na = s.na, nb = s.nb, n = which == KMC_BO_A ? na : nb, first = which == KMC_BO_A ? 0 : na;
  if (const int rc = bo_box(s, "bond order", h)) return rc;
  h->n = n;
  int64_t RC = 0;
  if (mode == KMC_BO_WITHIN) {
    const double rc = r_cut > 0.0 && r_cut * 1024.0 < (double)BO_BOX_MAX ? kmcm::round_(r_cut * 1024.0) : 0.0;
    RC = (int64_t)rc;
    if (RC < 1 || h->B[0] / RC < 3 || h->B[1] / RC < 3)
      return fail(KMC_ERR_ARG,
                  "bond order: r_cut must be positive and at most a third of the box (3 cells along an axis)");
  }
  h->sel.assign((size_t)n, 1);
  h->X.resize((size_t)n);
  h->Y.resize((size_t)n);
  h->C.assign((size_t)n, 0);
  h->S.assign((size_t)n, 0);
  h->nn.assign((size_t)n, 0);
  std::vector<int32_t> who;
  for (int i = 0; i < n; ++i) {
    h->X[i] = s.ipos(first + i, 0);
    h->Y[i] = s.ipos(first + i, 1);
    if (select == KMC_BO_BOUND) h->sel[i] = s.bound(first + i);
    if (h->sel[i]) who.push_back(i);
  }
  auto add = [&](int i, int j) {
    const int64_t DX = kmcb::fold(h->X[j] - h->X[i], h->B[0]), DY = kmcb::fold(h->Y[j] - h->Y[i], h->B[1]);
    if (DX == 0 && DY == 0) return;
    int64_t tc, ts;
    kmcb::term(fold, DX, DY, &tc, &ts);
    h->C[i] += tc;
    h->S[i] += ts;
    h->nn[i] += 1;
  };
  if (mode == KMC_BO_WITHIN) {
    BoCells g;
    g.build(*h, who, RC);
    const int64_t RC2 = RC * RC;
    for (int i : who) {
      int64_t cnt = 0;
      g.around(*h, i, [&](int j) {
        const int64_t DX = kmcb::fold(h->X[j] - h->X[i], h->B[0]), DY = kmcb::fold(h->Y[j] - h->Y[i], h->B[1]);
        const int64_t D2 = DX * DX + DY * DY;
        if (D2 <= 0 || D2 > RC2) return;
        if (++cnt <= BO_NN_MAX) add(i, j);
      });
      if (cnt > BO_NN_MAX) return fail(KMC_ERR_CAPACITY, "bond order: a protein with more than 65535 neighbours");
    }
  } else {
    for (int b : who) {
      for (int j = 2; j <= 4; ++j) {
        const int r = s.site_nei(b, j);
        if (r == 0) continue;
        int r2 = 0, l = 0;
        bool ok = r >= 1 && r <= na;
        if (ok) {
          r2 = s.nei3(r - 1);
          ok = r2 >= 0 && r2 <= na;
        }
        if (ok && r2 != 0) {
          l = s.nei2(r2 - 1);
          ok = l == 0 || (l > na && l <= na + nb);
        }
        if (!ok)
          return fail(KMC_ERR_STATE,
                      "bond order: a link followed from ligand " + std::to_string(b + 1) + " leaves the state");
        if (r2 == 0 || l == 0) continue;
        const int b2 = l - 1 - na;
        if (b2 == b || !h->sel[b2]) continue;
        add(b, b2);
      }
    }
  }
  return KMC_OK;
}

}  // namespace

int kmc_host_bond_order(const kmc_params* p, const kmc_state_view* v, int32_t which, int32_t mode, int32_t fold,
                        double r_cut, int32_t select, int32_t nbins, int64_t* hist, kmc_bond_order_out* out,
                        int64_t* C, int64_t* S, int32_t* nn) {
  if (!out || nbins < 1 || nbins > BO_HIST_BINS)
    return fail(KMC_ERR_ARG, "bond order: out is needed, 1 <= nbins <= 1024");
  BoHost h;
  const int rc = bo_host_local(p, v, which, mode, fold, r_cut, select, &h);
  if (rc != KMC_OK) return rc;
  std::memset(out, 0, sizeof *out);
  if (hist) std::fill(hist, hist + (size_t)KMC_BO_NN_ROWS * nbins, (int64_t)0);
  for (int i = 0; i < h.n; ++i) {
    if (!h.sel[i]) continue;
    const int64_t N = h.nn[i];
    const int64_t pc = N ? kmcb::normalise(h.C[i], N) : 0, ps = N ? kmcb::normalise(h.S[i], N) : 0;
    const int64_t m = pc * pc + ps * ps;
    out->n_sel += 1;
    out->n_with += N > 0;
    out->sum_nn += N;
    out->sum_pc += pc;
    out->sum_ps += ps;
    out->sum_m += m;
    if (hist) hist[(size_t)std::min<int64_t>(N, KMC_BO_NN_ROWS - 1) * nbins + kmcb::mag_bin(m, nbins)] += 1;
  }
  if (C) std::copy(h.C.begin(), h.C.end(), C);
  if (S) std::copy(h.S.begin(), h.S.end(), S);
  if (nn) std::copy(h.nn.begin(), h.nn.end(), nn);
  return KMC_OK;
}

int kmc_host_bond_order_corr(const kmc_params* p, const kmc_state_view* v, int32_t which, int32_t mode,
                             int32_t fold, double r_cut, int32_t select, double r_max, int32_t nbins,
                             int64_t* corr) {
  if (!corr || nbins < 1 || nbins > BO_CORR_BINS || !(r_max > 0.0) || !std::isfinite(r_max))
    return fail(KMC_ERR_ARG, "bond order: corr is needed, r_max > 0, 1 <= nbins <= 4096");
  BoHost h;
  const int rc = bo_host_local(p, v, which, mode, fold, r_cut, select, &h);
  if (rc != KMC_OK) return rc;
  const double dr = r_max / nbins;
  std::vector<int64_t> E2((size_t)nbins + 1);
  const int64_t EN = r_max * 1024.0 < (double)BO_BOX_MAX ? kmcb::corr_edge(nbins, dr) : 0;
  if (EN < 1 || !(std::floor(p->box_x / r_max) >= 3.0) || !(std::floor(p->box_y / r_max) >= 3.0) || h.B[0] / EN < 3 ||
      h.B[1] / EN < 3)
    return fail(KMC_ERR_ARG,
                "bond order: r_max must be at least 2^-10 A and at most a third of the box (3 cells along an axis)");
  for (int m = 0; m <= nbins; ++m) {
    const int64_t e = kmcb::corr_edge(m, dr);
    E2[m] = e * e;
  }
  std::vector<int32_t> who;
  std::vector<int64_t> pc((size_t)h.n, 0), ps((size_t)h.n, 0);
  for (int i = 0; i < h.n; ++i) {
    if (!h.sel[i] || h.nn[i] == 0) continue;
    pc[i] = kmcb::normalise(h.C[i], h.nn[i]);
    ps[i] = kmcb::normalise(h.S[i], h.nn[i]);
    who.push_back(i);
  }
  std::fill(corr, corr + 2 * (size_t)nbins, (int64_t)0);
  BoCells g;
  g.build(h, who, EN);
  const double inv = 1.0 / (dr * 1024.0);
  for (int i : who)
    g.around(h, i, [&](int j) {
      if (j <= i) return;
      const int64_t DX = kmcb::fold(h.X[j] - h.X[i], h.B[0]), DY = kmcb::fold(h.Y[j] - h.Y[i], h.B[1]);
      const int64_t D2 = DX * DX + DY * DY;
      if (D2 >= E2[nbins]) return;
      const int k = kmcb::corr_bin(E2.data(), nbins, D2, (int)(std::sqrt((double)D2) * inv));
      if (k >= nbins) return;
      corr[k] += pc[i] * pc[j] + ps[i] * ps[j];
      corr[(size_t)nbins + k] += 1;
    });
  return KMC_OK;
}

// Bond kinetics (include/kmc.h): kmc_kin_*'s definitions on host
// state views, one receptor after the other; the transition and the bin rule
// are kmc_kinetics.h's, the ones the device evaluates.
namespace {

bool kin_view_ok(const kmc_kin_view* w) {
  return w && w->rl_lig && w->rl_site && w->rl_since && w->cis_with && w->cis_since && w->last_lig && w->free_since &&
         w->bits;
}

// receptor i's (0-based) current links, checked as the device checks them
bool kin_host_cur(const StateReader& s, int i, kmck::Cur* c) {
  const int na = s.na, n = s.n;
  const int32_t n2 = s.nei2(i), n4 = s.nei4(i), n3 = s.nei3(i);
  c->lig = c->site = c->cis = 0;
  c->cx = false;
  if (n2 != 0 && (n2 <= na || n2 > n)) return false;
  if (n3 != 0 && (n3 < 1 || n3 > na || n3 == i + 1)) return false;
  if (n4 < 0 || n4 > 4) return false;
  c->lig = n2;
  c->site = n4;
  c->cis = n3;
  c->cx = n3 != 0 && (n2 != 0 || s.nei2(n3 - 1) != 0);
  return true;
}

// the begin's and the update's arguments
int kin_args(const StateReader& s, const kmc_kin_view* view, const kmc_kin_out* acc, const int64_t* hist7) {
  if (s.ok(false) && kin_view_ok(view) && acc && hist7) return KMC_OK;
  return fail(KMC_ERR_ARG, "kinetics: params, state, the view's eight arrays, acc and hist are needed");
}

kmck::Rec kin_load(const kmc_kin_view* w, int i) {
  kmck::Rec r;
  r.rl_lig = w->rl_lig[i];
  r.rl_site = w->rl_site[i];
  r.cis_with = w->cis_with[i];
  r.last_lig = w->last_lig[i];
  r.rl_since = w->rl_since[i];
  r.cis_since = w->cis_since[i];
  r.free_since = w->free_since[i];
  r.bits = w->bits[i];
  return r;
}

void kin_store(const kmc_kin_view* w, int i, const kmck::Rec& r) {
  w->rl_lig[i] = r.rl_lig;
  w->rl_site[i] = r.rl_site;
  w->cis_with[i] = r.cis_with;
  w->last_lig[i] = r.last_lig;
  w->rl_since[i] = r.rl_since;
  w->cis_since[i] = r.cis_since;
  w->free_since[i] = r.free_since;
  w->bits[i] = r.bits;
}

void kin_set_occ(const kmc_params* p, kmc_kin_out* acc, const int64_t cnt[kmck::KIN_NCNT]) {
  acc->occ_rl = cnt[kmck::KIN_OCC_RL];
  acc->occ_mono = cnt[kmck::KIN_OCC_MONO];
  acc->occ_cx = cnt[kmck::KIN_OCC_CX];
  acc->occ_free_receptor = (int64_t)p->n_a - acc->occ_rl;
  acc->occ_free_site = 3 * (int64_t)p->n_b - acc->occ_rl;
}

}  // namespace

int kmc_host_kin_begin(const kmc_params* p, const kmc_state_view* v, const kmc_kin_view* view, kmc_kin_out* acc,
                       int64_t* hist7) {
  const StateReader s(p, v);
  if (const int rc = kin_args(s, view, acc, hist7)) return rc;
  int64_t cnt[kmck::KIN_NCNT] = {0};
  for (int i = 0; i < p->n_a; ++i) {
    kmck::Cur c;
    if (!kin_host_cur(s, i, &c)) return fail(KMC_ERR_STATE, "kinetics: a receptor's bond link leaves its range");
    kmck::Rec r;
    const uint32_t m = kmck::begin(i + 1, v->step, c, r);
    kin_store(view, i, r);
    for (int b = 0; b < kmck::KIN_NCNT; ++b) cnt[b] += m >> b & 1u;
  }
  std::memset(acc, 0, sizeof *acc);
  std::fill(hist7, hist7 + (size_t)KIN_ROWS_UPD * KIN_BINS, (int64_t)0);
  acc->origin_step = acc->last_step = v->step;
  kin_set_occ(p, acc, cnt);
  return KMC_OK;
}

int kmc_host_kin_update(const kmc_params* p, const kmc_state_view* v, const kmc_kin_view* view, kmc_kin_out* acc,
                        int64_t* hist7) {
  const StateReader s(p, v);
  if (const int rc = kin_args(s, view, acc, hist7)) return rc;
  for (int i = 0; i < p->n_a; ++i) {  // checked first: a failed call leaves the recorder as it was
    kmck::Cur c;
    if (!kin_host_cur(s, i, &c)) return fail(KMC_ERR_STATE, "kinetics: a receptor's bond link leaves its range");
  }
  const int64_t t = v->step, dt = t - acc->last_step;
  acc->exp_rl += dt * acc->occ_rl;
  acc->exp_mono += dt * acc->occ_mono;
  acc->exp_cx += dt * acc->occ_cx;
  acc->exp_free_receptor += dt * acc->occ_free_receptor;
  acc->exp_free_site += dt * acc->occ_free_site;
  int64_t cnt[kmck::KIN_NCNT] = {0};
  for (int i = 0; i < p->n_a; ++i) {
    kmck::Cur c;
    kin_host_cur(s, i, &c);
    kmck::Rec r = kin_load(view, i);
    int row[3], nh;
    int64_t val[3];
    const uint32_t m = kmck::transition(i + 1, t, c, r, row, val, &nh);
    for (int k = 0; k < nh; ++k) hist7[(size_t)row[k] * KIN_BINS + kmck::bin(val[k])] += 1;
    kin_store(view, i, r);
    for (int b = 0; b < kmck::KIN_NCNT; ++b) cnt[b] += m >> b & 1u;
  }
  acc->rl_on += cnt[kmck::KIN_EV_RL_ON];
  acc->rl_off += cnt[kmck::KIN_EV_RL_OFF];
  acc->rl_swap += cnt[kmck::KIN_EV_RL_SWAP];
  acc->cis_on += cnt[kmck::KIN_EV_CIS_ON];
  acc->cis_off_mono += cnt[kmck::KIN_EV_CIS_OFF_MONO];
  acc->cis_off_cx += cnt[kmck::KIN_EV_CIS_OFF_CX];
  acc->cis_swap += cnt[kmck::KIN_EV_CIS_SWAP];
  kin_set_occ(p, acc, cnt);
  acc->last_step = t;
  acc->n_updates += 1;
  return KMC_OK;
}

int kmc_host_kin_sample(const kmc_params* p, const kmc_kin_view* view, const kmc_kin_out* acc, const int64_t* hist7,
                        kmc_kin_out* out, int64_t* hist9) {
  if (!p || !kin_view_ok(view) || !acc || !hist7 || !out)
    return fail(KMC_ERR_ARG, "kinetics sample: params, the view's eight arrays, acc, hist and out are needed");
  const kmc_kin_out a = *acc;  // (out may be acc itself)
  *out = a;
  out->n_rl_censored_alive = out->n_cis_censored_alive = 0;
  if (hist9) {
    std::copy(hist7, hist7 + (size_t)KIN_ROWS_UPD * KIN_BINS, hist9);
    std::fill(hist9 + (size_t)KIN_ROWS_UPD * KIN_BINS, hist9 + (size_t)KIN_HISTS * KIN_BINS, (int64_t)0);
  }
  for (int i = 0; i < p->n_a; ++i) {
    const kmck::Rec r = kin_load(view, i);
    const uint32_t m = kmck::alive(i + 1, r);
    if (hist9 && (m & 1u)) hist9[(size_t)kmck::KIN_ROW_RL_ALIVE * KIN_BINS + kmck::bin(a.last_step - r.rl_since)] += 1;
    if (hist9 && (m & 2u)) hist9[(size_t)kmck::KIN_ROW_CIS_ALIVE * KIN_BINS + kmck::bin(a.last_step - r.cis_since)] += 1;
    out->n_rl_censored_alive += m >> 2 & 1u;
    out->n_cis_censored_alive += m >> 3 & 1u;
  }
  return KMC_OK;
}

// Cluster growth kinetics (include/kmc.h): kmc_cf_*'s
// definitions on host state views.  Where the device runs two lock-free
// union-finds, the partitions here come from breadth-first walks over an
// adjacency list (the walk's start, in index order, is the label); the filing
// rule is kmc_coag.h's, the one the device evaluates.
namespace {

typedef std::pair<int32_t, int32_t> CfEdge;

bool cf_view_ok(const kmc_cf_view* w) { return w && w->rl_lig && w->cis_with && w->prev_label; }

bool cf_tables_ok(const kmc_cf_tables* t) {
  return t && t->merge && t->frag && t->merge_kind && t->frag_kind && t->merge_pieces && t->frag_pieces &&
         t->merge_product && t->frag_parent && t->n_s && t->expo && t->expo2;
}

// receptor i's (0-based) current bonds, checked as the device checks them
bool cf_host_cur(const StateReader& s, int i, int32_t* lig, int32_t* cis) {
  const int na = s.na, n = s.n;
  const int32_t n2 = s.nei2(i), n3 = s.nei3(i);
  *lig = *cis = 0;
  if (n2 != 0 && (n2 <= na || n2 > n)) return false;
  if (n3 != 0 && (n3 < 1 || n3 > na || n3 == i + 1)) return false;
  *lig = n2;
  *cis = n3;
  return true;
}

// components of n vertices under `edges` (0-based ends): label[i] = the
// smallest member (0-based), cnt[label] = the packed (receptors, ligands)
void cf_walk(int n, int na, const std::vector<CfEdge>& edges, std::vector<int32_t>& label,
             std::vector<uint64_t>& cnt) {
  // the adjacency: every edge's two ends, sorted by the end they start from (edge order within a vertex)
  std::vector<int32_t> from(2 * edges.size()), to(2 * edges.size()), start, adj;
  for (size_t e = 0; e < edges.size(); ++e) {
    from[2 * e] = to[2 * e + 1] = edges[e].first;
    from[2 * e + 1] = to[2 * e] = edges[e].second;
  }
  counting_sort(from.data(), from.size(), (size_t)n, start, adj);
  for (int32_t& k : adj) k = to[(size_t)k];
  cnt.assign((size_t)n, 0);
  walk_components(
      n, label,
      [&](int q, auto f) {
        for (int32_t k = start[(size_t)q]; k < start[(size_t)q + 1]; ++k) f(adj[(size_t)k]);
        return true;
      },
      [](int, int) {},
      [&](int r, const std::vector<int32_t>& members) {
        for (int q : members) cnt[(size_t)r] += q < na ? 1ull : 1ull << 32;
      });
  for (int32_t& l : label) l -= 1;
}

// the look at `label` / `cnt` becomes the last one: n_s, n_clusters, max_cluster
void cf_host_look(int n, int S, const std::vector<int32_t>& label, const std::vector<uint64_t>& cnt, kmc_cf_out* acc,
                  int64_t* n_s) {
  std::fill(n_s, n_s + S + 1, (int64_t)0);
  acc->n_clusters = acc->max_cluster = 0;
  for (int i = 0; i < n; ++i) {
    if (label[(size_t)i] != i) continue;
    const int size = kmcc::size_of(cnt[(size_t)i]);
    n_s[kmcc::clamp_size(size, S)] += 1;
    acc->n_clusters += 1;
    if (size > acc->max_cluster) acc->max_cluster = size;
  }
}

}  // namespace

int kmc_host_cf_begin(const kmc_params* p, const kmc_state_view* v, int32_t max_size, const kmc_cf_view* view,
                      kmc_cf_out* acc, const kmc_cf_tables* t) {
  const StateReader s(p, v);
  if (!s.ok(false) || !cf_view_ok(view) || !acc || !cf_tables_ok(t) || max_size < CF_MIN_SIZE || max_size > CF_MAX_SIZE)
    return fail(KMC_ERR_ARG,
                "growth: params, state, the view's three arrays, acc and every table are needed, 2 <= max_size <= 63");
  const int na = s.na, n = s.n, S = max_size;
  std::vector<CfEdge> e1;
  for (int i = 0; i < na; ++i) {
    int32_t lig, cis;
    if (!cf_host_cur(s, i, &lig, &cis)) return fail(KMC_ERR_STATE, "growth: a receptor's bond link leaves its range");
    if (lig) e1.push_back(CfEdge(i, lig - 1));
    if (cis && i + 1 < cis) e1.push_back(CfEdge(i, cis - 1));
  }
  for (int i = 0; i < na; ++i) cf_host_cur(s, i, &view->rl_lig[i], &view->cis_with[i]);
  std::vector<int32_t> label;
  std::vector<uint64_t> cnt;
  cf_walk(n, na, e1, label, cnt);
  for (int i = 0; i < n; ++i) view->prev_label[i] = label[(size_t)i] + 1;
  const size_t n1 = (size_t)S + 1, n2 = n1 * n1;
  std::memset(acc, 0, sizeof *acc);
  std::fill(t->merge, t->merge + n2, (int64_t)0);
  std::fill(t->frag, t->frag + n2, (int64_t)0);
  std::fill(t->merge_kind, t->merge_kind + CF_KINDS * CF_KINDS, (int64_t)0);
  std::fill(t->frag_kind, t->frag_kind + CF_KINDS * CF_KINDS, (int64_t)0);
  std::fill(t->merge_pieces, t->merge_pieces + CF_PIECES, (int64_t)0);
  std::fill(t->frag_pieces, t->frag_pieces + CF_PIECES, (int64_t)0);
  std::fill(t->merge_product, t->merge_product + n1, (int64_t)0);
  std::fill(t->frag_parent, t->frag_parent + n1, (int64_t)0);
  std::fill(t->expo, t->expo + n1, (int64_t)0);
  std::memset(t->expo2, 0, sizeof(kmc_i128) * n2);
  acc->origin_step = acc->last_step = v->step;
  acc->max_size = S;
  cf_host_look(n, S, label, cnt, acc, t->n_s);
  return KMC_OK;
}

int kmc_host_cf_update(const kmc_params* p, const kmc_state_view* v, const kmc_cf_view* view, kmc_cf_out* acc,
                       const kmc_cf_tables* t) {
  const StateReader s(p, v);
  if (!s.ok(false) || !cf_view_ok(view) || !acc || !cf_tables_ok(t) || acc->max_size < CF_MIN_SIZE ||
      acc->max_size > CF_MAX_SIZE)
    return fail(KMC_ERR_ARG, "growth: params, state, the view's three arrays, a begun acc and every table are needed");
  const int na = s.na, n = s.n, S = (int)acc->max_size;
  if (v->step == acc->last_step) {  // the state of the last look: nothing to file
    acc->n_updates += 1;
    return KMC_OK;
  }
  // the current bonds E1 and the kept bonds K, with the bond counters of this update
  std::vector<CfEdge> e1, kept;
  int64_t ev[4] = {0, 0, 0, 0};  // formed_rl, formed_cis, broken_rl, broken_cis
  for (int i = 0; i < na; ++i) {  // checked first: a failed call leaves the recorder as it was
    int32_t lig, cis;
    if (!cf_host_cur(s, i, &lig, &cis)) return fail(KMC_ERR_STATE, "growth: a receptor's bond link leaves its range");
  }
  for (int i = 0; i < n; ++i) {
    const int32_t l = view->prev_label[i];
    if (l < 1 || l > i + 1 || view->prev_label[l - 1] != l)
      return fail(KMC_ERR_STATE,
                  "growth: the recorder's label of protein " + std::to_string(i + 1) + " is not its class' smallest member");
  }
  for (int i = 0; i < na; ++i) {
    int32_t lig, cis;
    cf_host_cur(s, i, &lig, &cis);
    const int32_t old_lig = view->rl_lig[i], old_cis = view->cis_with[i], me = i + 1;
    if (lig) e1.push_back(CfEdge(i, lig - 1));
    if (cis && me < cis) e1.push_back(CfEdge(i, cis - 1));
    if (lig != old_lig) {
      ev[0] += lig != 0;
      ev[2] += old_lig != 0;
    } else if (lig) {
      kept.push_back(CfEdge(i, lig - 1));
    }
    if (cis != old_cis) {
      ev[1] += cis != 0 && me < cis;
      ev[3] += old_cis != 0 && me < old_cis;
    } else if (cis && me < cis) {
      kept.push_back(CfEdge(i, cis - 1));
    }
    view->rl_lig[i] = lig;
    view->cis_with[i] = cis;
  }
  std::vector<int32_t> cur, core, prev((size_t)n);
  std::vector<uint64_t> cur_cnt, core_cnt, prev_cnt((size_t)n, 0);
  cf_walk(n, na, e1, cur, cur_cnt);
  cf_walk(n, na, kept, core, core_cnt);
  for (int i = 0; i < n; ++i) {
    prev[(size_t)i] = view->prev_label[i] - 1;
    prev_cnt[(size_t)prev[(size_t)i]] += i < na ? 1ull : 1ull << 32;
  }
  // cores per previous and per current cluster
  std::vector<int32_t> k0((size_t)n, 0), k1((size_t)n, 0);
  int64_t n_cores = 0;
  for (int i = 0; i < n; ++i)
    if (core[(size_t)i] == i) {
      k0[(size_t)prev[(size_t)i]] += 1;
      k1[(size_t)cur[(size_t)i]] += 1;
      n_cores += 1;
    }
  for (int i = 0; i < n; ++i) {
    if (core[(size_t)i] != i) continue;
    const int32_t pl = prev[(size_t)i], cl = cur[(size_t)i];
    kmcc::Filing f = kmcc::file(i, core_cnt[(size_t)i], pl, prev_cnt[(size_t)pl], k0[(size_t)pl], S);
    if (f.pieces >= 0) t->frag_pieces[f.pieces] += 1;
    if (f.whole >= 0) t->frag_parent[f.whole] += 1;
    if (f.pair >= 0) t->frag[f.pair] += 1;
    if (f.kinds >= 0) t->frag_kind[f.kinds] += 1;
    f = kmcc::file(i, core_cnt[(size_t)i], cl, cur_cnt[(size_t)cl], k1[(size_t)cl], S);
    if (f.pieces >= 0) t->merge_pieces[f.pieces] += 1;
    if (f.whole >= 0) t->merge_product[f.whole] += 1;
    if (f.pair >= 0) t->merge[f.pair] += 1;
    if (f.kinds >= 0) t->merge_kind[f.kinds] += 1;
  }
  // exposures of the interval that ended, from the previous look's n_s
  typedef __int128 i128;
  const int64_t dt = v->step - acc->last_step;
  for (int x = 1; x <= S; ++x) {
    const int64_t nx = t->n_s[x];
    t->expo[x] += dt * nx;
    for (int y = x; y <= S; ++y)
      add(&t->expo2[(size_t)x * (S + 1) + y], y == x ? (i128)dt * nx * (nx - 1) / 2 : (i128)dt * nx * t->n_s[y]);
  }
  const int64_t clusters_prev = acc->n_clusters;
  for (int i = 0; i < n; ++i) view->prev_label[i] = cur[(size_t)i] + 1;
  cf_host_look(n, S, cur, cur_cnt, acc, t->n_s);
  acc->formed_rl += ev[0];
  acc->formed_cis += ev[1];
  acc->broken_rl += ev[2];
  acc->broken_cis += ev[3];
  acc->n_cores = n_cores;
  acc->cycles_closed += ev[0] + ev[1] - (n_cores - acc->n_clusters);
  acc->cycles_opened += ev[2] + ev[3] - (n_cores - clusters_prev);
  acc->last_step = v->step;
  acc->n_updates += 1;
  return KMC_OK;
}

int kmc_host_cf_sample(const kmc_params* p, const kmc_cf_view* view, const kmc_cf_out* acc, const kmc_cf_tables* t,
                       kmc_cf_out* out, const kmc_cf_tables* to) {
  if (!p || !cf_view_ok(view) || !acc || !cf_tables_ok(t) || !out || acc->max_size < CF_MIN_SIZE ||
      acc->max_size > CF_MAX_SIZE)
    return fail(KMC_ERR_ARG,
                "growth sample: params, the view's three arrays, a begun acc, every table and out are needed");
  const kmc_cf_out a = *acc;  // (out may be acc itself)
  *out = a;
  if (!to) return KMC_OK;
  const size_t n1 = (size_t)a.max_size + 1, n2 = n1 * n1;
  auto copy = [](int64_t* dst, const int64_t* src, size_t n) {
    if (dst && dst != src) std::copy(src, src + n, dst);
  };
  copy(to->merge, t->merge, n2);
  copy(to->frag, t->frag, n2);
  copy(to->merge_kind, t->merge_kind, CF_KINDS * CF_KINDS);
  copy(to->frag_kind, t->frag_kind, CF_KINDS * CF_KINDS);
  copy(to->merge_pieces, t->merge_pieces, CF_PIECES);
  copy(to->frag_pieces, t->frag_pieces, CF_PIECES);
  copy(to->merge_product, t->merge_product, n1);
  copy(to->frag_parent, t->frag_parent, n1);
  copy(to->n_s, t->n_s, n1);
  copy(to->expo, t->expo, n1);
  if (to->expo2 && to->expo2 != t->expo2) std::copy(t->expo2, t->expo2 + n2, to->expo2);
  return KMC_OK;
}

// Ligand network and rings (include/kmc.h), sequential: the
// hops, their checks and the chord rule are kmc_rings.h's, the ones the device
// evaluates; the adjacency is by reference index, and a ring is counted from
// its smallest ligand by a recursive walk.
namespace {

struct RgHost {
  std::vector<int32_t> lig, site;  // [nb][3]: the hop's 1-based ligand number and site, 0: none
  int64_t hist[16];
  kmc_net_out out;
};

int rg_host_network(const kmc_params* p, const kmc_state_view* v, RgHost* g) {
  const StateReader s(p, v);
  if (!s.ok(false)) return fail(KMC_ERR_ARG, "rings: params and state are needed");
  const int na = s.na, nb = s.nb;
  g->lig.assign(3 * (size_t)nb, 0);
  g->site.assign(3 * (size_t)nb, 0);
  std::fill(g->hist, g->hist + 16, (int64_t)0);
  std::memset(&g->out, 0, sizeof g->out);
  for (int i = 0; i < na; ++i) {
    const int32_t v2 = s.nei2(i), v3 = s.nei3(i);
    bool ok = kmcr::receptor_links_ok(v2, v3, i + 1, na, nb);
    if (ok && v3 != 0) {
      const int32_t p2 = s.nei2(v3 - 1), p3 = s.nei3(v3 - 1);
      ok = p3 == i + 1;
      if (ok && v2 == 0 && p2 == 0 && i + 1 < v3) g->out.n_free_dimers += 1;
    }
    if (!ok)
      return fail(KMC_ERR_STATE,
                  "rings: a bond link of receptor " + std::to_string(i + 1) + " is of the wrong kind or not returned");
    g->out.rec[kmcr::rec_bin(v2, v3)] += 1;
  }
  std::vector<uint8_t> vertex((size_t)nb, 0);
  for (int b = 0; b < nb; ++b) {
    kmcr::Hops h;
    kmcr::hops(v->a_int, v->b_int, na, nb, b, h);
    if (h.bad)
      return fail(KMC_ERR_STATE,
                  "rings: a link followed from ligand " + std::to_string(b + 1) + " is of the wrong kind or the bridge is asymmetric");
    int occ = 0, ends = 0;
    for (int e = 0; e < 3; ++e) {
      occ += h.r[e] != 0;
      if (h.r2[e] != 0 && h.l[e] == 0) g->out.n_half += 1;
      if (h.l[e] == 0) continue;
      ++ends;
      g->lig[3 * (size_t)b + e] = h.l[e];
      g->site[3 * (size_t)b + e] = h.s2[e];
      if (kmcr::first_end(b + 1, e + 2, h.l[e], h.s2[e])) {
        g->out.n_bridges += 1;
        g->out.n_loops += h.l[e] == b + 1;
      }
    }
    g->hist[occ * 4 + ends] += 1;
    vertex[b] = ends >= 1;
    g->out.n_vertices += ends >= 1;
  }
  // the components of the whole bond graph (every link was checked above) that hold a bridge
  std::vector<int32_t> label;
  walk_components(
      s.n, label, [&](int q, auto f) { return bond_links(s, q, f); }, [](int, int) {},
      [&](int, const std::vector<int32_t>& members) {
        bool holds = false;
        for (int q : members) holds = holds || (q >= na && vertex[q - na]);
        g->out.n_net_components += holds;
      });
  g->out.cycle_rank = g->out.n_bridges - g->out.n_vertices + g->out.n_net_components;
  return KMC_OK;
}

// the walk of one (root, s_first < s_last): simple paths over ligands above the root, closed through s_last
struct RgWalk {
  const RgHost& g;
  int nb, max_len;
  int64_t* counts;   // [2][RG_MAX + 1]
  uint32_t* member;  // [2][nb] or null
  int root = 0, sb = 0;
  int32_t path[RG_MAX];
  int in[RG_MAX], out[RG_MAX];

  void close(int L) {
    auto vert = [&](int j) { return path[j]; };
    auto off = [&](int i) { return g.lig[3 * (size_t)(path[i] - 1) + kmcr::off_site(in[i], out[i]) - 2]; };
    const bool chordless = kmcr::chordless(L, vert, off);
    counts[L] += 1;
    if (chordless) counts[RG_MAX + 1 + L] += 1;
    if (!member) return;
    for (int i = 0; i < L; ++i) {
      member[path[i] - 1] |= 1u << L;
      if (chordless) member[(size_t)nb + path[i] - 1] |= 1u << L;
    }
  }
  // ligand v entered by site s at depth k < max_len (at most max_len - 1 levels of recursion)
  void visit(int32_t v, int s, int k) {
    path[k] = v;
    in[k] = s;
    for (int c = 2; c <= 4; ++c) {
      if (c == s) continue;
      const int32_t w = g.lig[3 * (size_t)(v - 1) + c - 2];
      const int ws = g.site[3 * (size_t)(v - 1) + c - 2];
      if (w == 0) continue;
      out[k] = c;
      if (w == root) {
        if (ws == sb) close(k + 1);
        continue;
      }
      if (w < root || k + 1 >= max_len) continue;
      bool seen = false;
      for (int j = 1; j <= k; ++j) seen = seen || path[j] == w;
      if (!seen) visit(w, ws, k + 1);
    }
  }
  void from(int32_t r, int sa, int sb_) {
    root = r;
    sb = sb_;
    path[0] = r;
    in[0] = sb_;
    out[0] = sa;
    const int32_t w = g.lig[3 * (size_t)(r - 1) + sa - 2];
    const int ws = g.site[3 * (size_t)(r - 1) + sa - 2];
    if (w == 0) return;
    if (w == r) {
      if (ws == sb) close(1);
      return;
    }
    if (w > r && max_len >= 2) visit(w, ws, 1);
  }
};

}  // namespace

int kmc_host_network(const kmc_params* p, const kmc_state_view* v, kmc_net_out* out, int64_t* lig_hist,
                     int32_t* adj_lig, int32_t* adj_site) {
  RgHost g;
  const int rc = rg_host_network(p, v, &g);
  if (rc != KMC_OK) return rc;
  if (out) *out = g.out;
  if (lig_hist) std::copy(g.hist, g.hist + 16, lig_hist);
  if (adj_lig) std::copy(g.lig.begin(), g.lig.end(), adj_lig);
  if (adj_site) std::copy(g.site.begin(), g.site.end(), adj_site);
  return KMC_OK;
}

int kmc_host_rings(const kmc_params* p, const kmc_state_view* v, int32_t max_len, int64_t* counts, uint32_t* member,
                   kmc_net_out* out) {
  if (!counts || max_len < 1 || max_len > RG_MAX)
    return fail(KMC_ERR_ARG, "rings: counts is needed, 1 <= max_len <= 12");
  RgHost g;
  const int rc = rg_host_network(p, v, &g);
  if (rc != KMC_OK) return rc;
  const int nb = p->n_b;
  std::fill(counts, counts + 2 * (RG_MAX + 1), (int64_t)0);
  if (member) std::fill(member, member + 2 * (size_t)nb, 0u);
  RgWalk w{g, nb, max_len, counts, member};
  for (int r = 1; r <= nb; ++r) {
    w.from(r, 2, 3);
    w.from(r, 2, 4);
    w.from(r, 3, 4);
  }
  if (out) *out = g.out;
  return KMC_OK;
}

// Lag correlator (include/kmc.h): kmc_lag_*'s definitions on
// host state views, one protein after the other and one task after the other;
// the schedule and the pair term are kmc_lagcorr.h's, the ones the device
// evaluates.  Every sum is taken whole, in __int128.
namespace {

bool lag_view_ok(const kmc_lag_view* w) {
  return w && w->prev && w->U && w->links && w->last_event && w->ring && w->table && w->n_pairs;
}

}  // namespace

int kmc_host_lag_begin(const kmc_params* p, const kmc_state_view* v, const kmc_lag_config* cfg,
                       const kmc_lag_view* view, kmc_lag_out* acc) {
  const StateReader s(p, v);
  if (const int rc = recorder_args(s, "lag", "seven", true, cfg, lag_view_ok(view), acc)) return rc;
  kmc_lag_config c = *cfg;
  for (int k = std::max(0, std::min(c.nq, LAG_MAX_Q)); k < LAG_MAX_Q; ++k) c.h[k] = 0;
  int64_t J, F, BX, BY;
  const char* bad =
      kmcl::check(c.every, c.levels, c.slots, c.nq, c.h, p->box_x, p->box_y, &c.max_jump, &c.max_disp, &J, &F, &BX, &BY);
  if (bad) return fail(KMC_ERR_ARG, bad);
  const size_t N = (size_t)p->n_a + (size_t)p->n_b;
  const int L = c.levels, P = c.slots, rows = kmcl::rows(L, P);
  for (size_t i = 0; i < N; ++i) {
    int64_t X[2];
    int32_t l[3];
    tracked(s, (int)i, X, l);
    for (int k = 0; k < 2; ++k) view->prev[2 * i + k] = view->U[2 * i + k] = X[k];
    for (int k = 0; k < 3; ++k) view->links[(size_t)k * N + i] = l[k];
    view->last_event[i] = 0;
    for (int lv = 0; lv < L; ++lv)
      for (int k = 0; k < 2; ++k) view->ring[((size_t)(lv * P) * N + i) * 2 + k] = X[k];
  }
  std::memset(view->table, 0, sizeof(kmc_lag_cell) * (size_t)rows * LAG_CLASSES);
  std::fill(view->n_pairs, view->n_pairs + rows, (int64_t)0);
  std::memset(acc, 0, sizeof *acc);
  acc->cfg = c;
  acc->J = J;
  acc->F = F;
  acc->BX = BX;
  acc->BY = BY;
  acc->origin_step = acc->last_step = v->step;
  acc->rows = rows;
  return KMC_OK;
}

int kmc_host_lag_update(const kmc_params* p, const kmc_state_view* v, const kmc_lag_view* view, kmc_lag_out* acc,
                        kmc_lag_info* info) {
  const StateReader s(p, v);
  if (const int rc = recorder_args(s, "lag", "seven", false, nullptr, lag_view_ok(view), acc)) return rc;
  if (v->step != acc->last_step + acc->cfg.every || acc->n_updates >= INT32_MAX) return not_due("lag", acc->cfg.every);
  const size_t N = (size_t)p->n_a + (size_t)p->n_b;
  const int L = acc->cfg.levels, P = acc->cfg.slots, nq = acc->cfg.nq;
  const int64_t n = acc->n_updates + 1;
  kmcl::Task tasks[LAG_MAX_ROWS];
  const int nt = kmcl::tasks(n, L, P, tasks);
  int64_t n_events = 0;
  for (size_t i = 0; i < N; ++i) {
    int64_t X[2], d[2];
    int32_t l[3];
    tracked(s, (int)i, X, l);
    d[0] = kmcl::min_image(X[0] - view->prev[2 * i], acc->BX);
    d[1] = kmcl::min_image(X[1] - view->prev[2 * i + 1], acc->BY);
    int64_t U[2];
    for (int k = 0; k < 2; ++k) {
      U[k] = view->U[2 * i + k] += d[k];
      view->prev[2 * i + k] = X[k];
    }
    bool ev = std::llabs(d[0]) >= acc->J || std::llabs(d[1]) >= acc->J;
    for (int k = 0; k < 3; ++k) {
      int32_t* q = &view->links[(size_t)k * N + i];
      ev = ev || *q != l[k];
      *q = l[k];
    }
    if (ev) {
      view->last_event[i] = (int32_t)n;
      ++n_events;
    }
    const int c = kmcl::cls(i < (size_t)p->n_a, l);
    for (int t = 0; t < nt; ++t) {
      const int64_t* O = &view->ring[((size_t)tasks[t].ring * N + i) * 2];
      const int64_t Dx = U[0] - O[0], Dy = U[1] - O[1];
      kmc_lag_cell* cell = &view->table[(size_t)tasks[t].row * LAG_CLASSES + c];
      if (kmcl::far(Dx, Dy, acc->F)) {
        cell->n_far += 1;
        continue;
      }
      const uint64_t q = kmcl::sq(Dx, Dy);
      cell->n_all += 1;
      add(&cell->m2_all, (__int128)q);
      if (view->last_event[i] > tasks[t].nk) continue;
      cell->n_clean += 1;
      add(&cell->m2_clean, (__int128)q);
      uint64_t a2, ab, b2;
      kmcl::split(q, &a2, &ab, &b2);
      add(&cell->m4_clean, (__int128)kmcl::m4(a2, ab, b2));
      for (int k = 0; k < nq; ++k)
        add(&cell->fs[k], (__int128)kmcl::fs_term(acc->cfg.h[k], Dx, Dy, acc->BX, acc->BY));
    }
    for (int lv = 0; lv < L && kmcl::fires(n, lv); ++lv)
      for (int k = 0; k < 2; ++k) view->ring[((size_t)kmcl::store_ring(n, lv, P) * N + i) * 2 + k] = U[k];
  }
  for (int t = 0; t < nt; ++t) view->n_pairs[tasks[t].row] += 1;
  acc->last_step = v->step;
  acc->n_updates = n;
  if (info) {
    info->n_updates = n;
    info->n_tasks = nt;
    info->n_events = n_events;
  }
  return KMC_OK;
}

int kmc_host_lag_sample(const kmc_params* p, const kmc_lag_view* view, const kmc_lag_out* acc, kmc_lag_out* out,
                        kmc_lag_cell* table, int64_t* n_pairs) {
  if (!p || !lag_view_ok(view) || !acc || !out)
    return fail(KMC_ERR_ARG, "lag sample: params, the view's seven arrays, acc and out are needed");
  const kmc_lag_out a = *acc;  // (out may be acc itself)
  *out = a;
  if (table && table != view->table) std::copy(view->table, view->table + (size_t)a.rows * LAG_CLASSES, table);
  if (n_pairs && n_pairs != view->n_pairs) std::copy(view->n_pairs, view->n_pairs + a.rows, n_pairs);
  return KMC_OK;
}

// Pair dynamics (include/kmc.h): kmc_pd_*'s definitions on host
// state views, one protein and one pair after the other; the fold, the cell,
// the bin, the validity and the terms are kmc_pairdyn.h's, the ones the device
// evaluates.  The sample sorts both point sets by cell (a counting sort of its
// own) and walks the 3 x 3 block for part A and the half shell for part B.
namespace {

bool pd_view_ok(const kmc_pd_view* w) { return w && w->prev && w->U && w->X0 && w->flags; }

// the configuration in acc resolved again: the grid and the edges (they were checked at begin)
const char* pd_grid(const kmc_params* p, const kmc_pd_out* acc, kmcp::Grid* G, int64_t* E) {
  double mj = acc->cfg.max_jump, md = acc->cfg.max_disp;
  return kmcp::check(acc->cfg.every, acc->cfg.nbins, acc->cfg.r_max, p->box_x, p->box_y, &mj, &md, G, E);
}

// points sorted by cell: start[ncell + 1], order[N] (the point indices of cell c are order[start[c] .. start[c + 1]))
struct PdCells {
  std::vector<int32_t> start, order, cx, cy;
  std::vector<int64_t> fx, fy;
  void build(const int64_t* X, size_t N, const kmcp::Grid& G) {
    cx.resize(N);
    cy.resize(N);
    fx.resize(N);
    fy.resize(N);
    std::vector<int32_t> cell(N);
    for (size_t i = 0; i < N; ++i) {
      fx[i] = kmcp::fold(X[2 * i], G.BX);
      fy[i] = kmcp::fold(X[2 * i + 1], G.BY);
      cx[i] = kmcp::cell(fx[i], G.ncx, G.BX);
      cy[i] = kmcp::cell(fy[i], G.ncy, G.BY);
      cell[i] = cy[i] * G.ncx + cx[i];
    }
    counting_sort(cell.data(), N, (size_t)G.ncx * G.ncy, start, order);
  }
};

}  // namespace

int kmc_host_pd_begin(const kmc_params* p, const kmc_state_view* v, const kmc_pd_config* cfg, const kmc_pd_view* view,
                      kmc_pd_out* acc) {
  const StateReader s(p, v);
  if (const int rc = recorder_args(s, "pd", "four", true, cfg, pd_view_ok(view), acc)) return rc;
  kmc_pd_config c = *cfg;
  kmcp::Grid G;
  int64_t E[PD_MAX_BINS + 1];
  const char* bad = kmcp::check(c.every, c.nbins, c.r_max, p->box_x, p->box_y, &c.max_jump, &c.max_disp, &G, E);
  if (bad) return fail(KMC_ERR_ARG, bad);
  const size_t N = (size_t)p->n_a + (size_t)p->n_b;
  for (size_t i = 0; i < N; ++i) {
    int64_t X[2];
    int32_t l[3];
    tracked(s, (int)i, X, l);
    for (int k = 0; k < 2; ++k) view->prev[2 * i + k] = view->U[2 * i + k] = view->X0[2 * i + k] = X[k];
    view->flags[i] = 0;
  }
  std::memset(acc, 0, sizeof *acc);
  acc->cfg = c;
  acc->J = G.J;
  acc->F = G.F;
  acc->BX = G.BX;
  acc->BY = G.BY;
  acc->ncx = G.ncx;
  acc->ncy = G.ncy;
  acc->origin_step = acc->last_step = v->step;
  return KMC_OK;
}

int kmc_host_pd_update(const kmc_params* p, const kmc_state_view* v, const kmc_pd_view* view, kmc_pd_out* acc,
                       kmc_pd_info* info) {
  const StateReader s(p, v);
  if (const int rc = recorder_args(s, "pd", "four", false, nullptr, pd_view_ok(view), acc)) return rc;
  if (v->step != acc->last_step + acc->cfg.every) return not_due("pd", acc->cfg.every);
  const size_t N = (size_t)p->n_a + (size_t)p->n_b;
  int64_t n_jumped = 0;
  for (size_t i = 0; i < N; ++i) {
    int64_t X[2];
    int32_t l[3];
    tracked(s, (int)i, X, l);
    const int64_t B[2] = {acc->BX, acc->BY};
    for (int k = 0; k < 2; ++k) {
      const int64_t d = kmcl::min_image(X[k] - view->prev[2 * i + k], B[k]);
      view->U[2 * i + k] += d;
      view->prev[2 * i + k] = X[k];
      if (std::llabs(d) >= acc->J) view->flags[i] |= PD_JUMPED;
    }
    n_jumped += view->flags[i] & PD_JUMPED;
  }
  acc->last_step = v->step;
  acc->n_updates += 1;
  if (info) {
    info->n_updates = acc->n_updates;
    info->n_jumped = n_jumped;
  }
  return KMC_OK;
}

int kmc_host_pd_sample(const kmc_params* p, const kmc_pd_view* view, const kmc_pd_out* acc, kmc_pd_out* out, int64_t* gd,
                       int64_t* gs, kmc_pd_cell* cu) {
  if (!p || !pd_view_ok(view) || !acc || !out)
    return fail(KMC_ERR_ARG, "pd sample: params, the view's four arrays, acc and out are needed");
  kmcp::Grid G;
  int64_t E[PD_MAX_BINS + 1];
  const char* bad = pd_grid(p, acc, &G, E);
  if (bad) return fail(KMC_ERR_ARG, bad);
  const kmc_pd_out a = *acc;  // (out may be acc itself)
  *out = a;
  if (!gd && !gs && !cu) return KMC_OK;
  const int nb = G.nbins, na = p->n_a;
  const size_t N = (size_t)p->n_a + (size_t)p->n_b;
  uint64_t E2[PD_MAX_BINS + 1];
  for (int m = 0; m <= nb; ++m) E2[m] = (uint64_t)E[m] * (uint64_t)E[m];
  if (gd) std::fill(gd, gd + 4 * (size_t)nb, (int64_t)0);
  if (gs) std::fill(gs, gs + 2 * (size_t)nb, (int64_t)0);
  if (cu) std::memset(cu, 0, sizeof(kmc_pd_cell) * 3 * (size_t)nb);
  PdCells o, w;
  o.build(view->X0, N, G);
  if (gd || gs) {
    w.build(view->U, N, G);
    for (size_t i = 0; i < N; ++i) {
      const int si = (int)i >= na;
      block3x3(o.cx[i], o.cy[i], G.ncx, G.ncy, [&](size_t jc) {
        for (int32_t t = w.start[jc]; t < w.start[jc + 1]; ++t) {
          const size_t j = (size_t)w.order[t];
          const int k = kmcp::bin(E2, nb, kmcp::d2(kmcl::min_image(w.fx[j] - o.fx[i], G.BX),
                                                   kmcl::min_image(w.fy[j] - o.fy[i], G.BY)));
          if (k >= nb) continue;
          if (i == j) {
            if (gs) gs[(size_t)si * nb + k] += 1;
          } else if (gd) {
            gd[(size_t)kmcp::kind_a(si, (int)j >= na) * nb + k] += 1;
          }
        }
      });
    }
  }
  if (cu) {
    for (int cy = 0; cy < G.ncy; ++cy)
      for (int cx = 0; cx < G.ncx; ++cx) {
        const size_t c = (size_t)cy * G.ncx + cx;
        for (int q = 0; q < 5; ++q) {
          int ox, oy;
          kmcp::half_shell(q, &ox, &oy);
          const size_t jc = (size_t)((cy + oy + G.ncy) % G.ncy) * G.ncx + (cx + ox + G.ncx) % G.ncx;
          for (int32_t ta = o.start[c]; ta < o.start[c + 1]; ++ta)
            for (int32_t tb = q == 0 ? ta + 1 : o.start[jc]; tb < o.start[jc + 1]; ++tb) {
              const size_t i = (size_t)o.order[ta], j = (size_t)o.order[tb];
              const int k = kmcp::bin(E2, nb, kmcp::d2(kmcl::min_image(o.fx[j] - o.fx[i], G.BX),
                                                       kmcl::min_image(o.fy[j] - o.fy[i], G.BY)));
              if (k >= nb) continue;
              kmc_pd_cell* cell = &cu[(size_t)kmcp::kind_b((int)i >= na, (int)j >= na) * nb + k];
              cell->n_pairs += 1;
              const int64_t uix = view->U[2 * i] - view->X0[2 * i], uiy = view->U[2 * i + 1] - view->X0[2 * i + 1];
              const int64_t ujx = view->U[2 * j] - view->X0[2 * j], ujy = view->U[2 * j + 1] - view->X0[2 * j + 1];
              if (!kmcp::valid(view->flags[i], uix, uiy, G.F) || !kmcp::valid(view->flags[j], ujx, ujy, G.F)) continue;
              cell->n_valid += 1;
              add(&cell->dot, (__int128)kmcp::dot(uix, uiy, ujx, ujy));
              add(&cell->sq, (__int128)kmcp::sq(uix, uiy, ujx, ujy));
            }
        }
      }
  }
  return KMC_OK;
}

// Body dynamics (include/kmc.h), sequential: the bodies are the components of
// kmc_host_cluster_geometry at the begin, with its image shifts; the
// per-protein step is the lag correlator's; the sample labels the current
// components (kmc_host_census) and walks each body's members in index order.
// C and S are summed as include/kmc.h defines them, member by member with D =
// D0 + u - u_r — not through the device's rearrangement; the verdict's bounds
// and the rotation terms are kmc_bodydyn.h's.
namespace {

bool bd_view_ok(const kmc_bd_view* w) {
  return w && w->prev && w->U && w->X0 && w->links && w->flags && w->label && w->D0 && w->bits;
}

// one row per body, in label order, from the view and the current state
int bd_host_rows(const kmc_params* p, const kmc_state_view* v, const kmc_bd_view* w, const kmc_bd_out* acc,
                 std::vector<kmc_bd_body>* rows) {
  const int na = p->n_a, n = p->n_a + p->n_b;
  std::vector<int32_t> cur((size_t)n), size((size_t)n + 1, 0);
  kmc_census census;
  const int rc = kmc_host_census(p, v, cur.data(), 0, 0, nullptr, &census);
  if (rc != KMC_OK) return rc;
  for (int i = 0; i < n; ++i) size[(size_t)cur[i]] += 1;
  // the members of every body, in index order: a counting sort by label
  std::vector<int32_t> start, order;
  counting_sort(w->label, (size_t)n, (size_t)n + 1, start, order);
  rows->clear();
  for (int r = 1; r <= n; ++r) {
    const int m = start[(size_t)r + 1] - start[r];
    if (!m) continue;
    const int32_t* mem = &order[(size_t)start[r]];
    kmc_bd_body b;
    std::memset(&b, 0, sizeof b);
    b.label = r;
    b.bits = w->bits[r - 1];
    int orbits = 0, lmin = n + 1, lmax = 0;
    for (int t = 0; t < m; ++t) {
      const size_t i = (size_t)mem[t];
      ((int)i < na ? b.n_r : b.n_l) += 1;
      orbits |= kmcb::member_bits(w->flags[i], w->U[2 * i] - w->X0[2 * i], w->U[2 * i + 1] - w->X0[2 * i + 1], acc->F);
      lmin = std::min(lmin, (int)cur[i]);
      lmax = std::max(lmax, (int)cur[i]);
    }
    b.cur_label = lmin;
    b.cur_size = size[(size_t)lmin];
    b.status = lmin != lmax ? KMC_BD_BROKEN : b.cur_size == m ? KMC_BD_INTACT : KMC_BD_GROWN;
    if (!(orbits & (BD_JUMPED | BD_CHANGED))) b.is |= KMC_BD_IS_PRISTINE;
    if (!orbits) {
      b.is |= KMC_BD_IS_VALID;
      const size_t q = (size_t)r - 1;
      const int64_t ur[2] = {w->U[2 * q] - w->X0[2 * q], w->U[2 * q + 1] - w->X0[2 * q + 1]};
      const bool rot = m >= 2 && m <= KMC_BD_ROT_MAX && !b.bits;
      for (int t = 0; t < m; ++t) {
        const size_t i = (size_t)mem[t];
        const int64_t u[2] = {w->U[2 * i] - w->X0[2 * i], w->U[2 * i + 1] - w->X0[2 * i + 1]};
        b.su[0] += u[0];
        b.su[1] += u[1];
        if (!rot) continue;
        const int64_t d0[2] = {w->D0[2 * i], w->D0[2 * i + 1]};
        const int64_t d[2] = {d0[0] + u[0] - ur[0], d0[1] + u[1] - ur[1]};
        b.C += d0[0] * d[0] + d0[1] * d[1];
        b.S += d0[0] * d[1] - d0[1] * d[0];
      }
      if (rot) b.is |= KMC_BD_IS_ROT;
    }
    rows->push_back(b);
  }
  return KMC_OK;
}

}  // namespace

int kmc_host_bd_begin(const kmc_params* p, const kmc_state_view* v, const kmc_bd_config* cfg, const kmc_bd_view* view,
                      kmc_bd_out* acc) {
  const StateReader s(p, v);
  if (const int rc = recorder_args(s, "bd", "eight", true, cfg, bd_view_ok(view), acc)) return rc;
  kmc_bd_config c = *cfg;
  int64_t J, F, BX, BY;
  const char* bad = kmcb::check(c.every, c.max_size, p->box_x, p->box_y, &c.max_jump, &c.max_disp, &J, &F, &BX, &BY);
  if (bad) return fail(KMC_ERR_ARG, bad);
  const size_t N = (size_t)p->n_a + (size_t)p->n_b;
  std::vector<int32_t> shift(2 * N + 1);
  kmc_geom geom;
  const int rc = kmc_host_cluster_geometry(p, v, view->label, shift.data(), view->bits, 2, nullptr, &geom);
  if (rc != KMC_OK) return rc;
  int64_t n_bodies = 0;
  for (size_t i = 0; i < N; ++i) {
    int64_t X[2];
    int32_t l[3];
    tracked(s, (int)i, X, l);
    for (int k = 0; k < 2; ++k) view->prev[2 * i + k] = view->U[2 * i + k] = view->X0[2 * i + k] = X[k];
    for (int k = 0; k < 3; ++k) view->links[(size_t)k * N + i] = l[k];
    view->flags[i] = 0;
    n_bodies += view->label[i] == (int32_t)i + 1;
  }
  for (size_t i = 0; i < N; ++i) {
    const size_t r = (size_t)view->label[i] - 1;
    view->D0[2 * i] = view->X0[2 * i] + (int64_t)shift[i] * BX - view->X0[2 * r];
    view->D0[2 * i + 1] = view->X0[2 * i + 1] + (int64_t)shift[N + i] * BY - view->X0[2 * r + 1];
  }
  // a body is WIDE by any of its members: the bit goes to all of them
  std::vector<uint8_t> wide(N, 0);
  for (size_t i = 0; i < N; ++i)
    if (kmcb::wide(view->D0[2 * i], view->D0[2 * i + 1])) wide[(size_t)view->label[i] - 1] = 1;
  for (size_t i = 0; i < N; ++i)
    if (wide[(size_t)view->label[i] - 1]) view->bits[i] |= KMC_BD_WIDE;
  std::memset(acc, 0, sizeof *acc);
  acc->cfg = c;
  acc->J = J;
  acc->F = F;
  acc->BX = BX;
  acc->BY = BY;
  acc->origin_step = acc->last_step = v->step;
  acc->n_bodies = n_bodies;
  return KMC_OK;
}

int kmc_host_bd_update(const kmc_params* p, const kmc_state_view* v, const kmc_bd_view* view, kmc_bd_out* acc,
                       kmc_bd_info* info) {
  const StateReader s(p, v);
  if (const int rc = recorder_args(s, "bd", "eight", false, nullptr, bd_view_ok(view), acc)) return rc;
  if (v->step != acc->last_step + acc->cfg.every) return not_due("bd", acc->cfg.every);
  const size_t N = (size_t)p->n_a + (size_t)p->n_b;
  const int64_t B[2] = {acc->BX, acc->BY};
  int64_t n_jumped = 0, n_changed = 0;
  for (size_t i = 0; i < N; ++i) {
    int64_t X[2];
    int32_t l[3];
    tracked(s, (int)i, X, l);
    int f = 0;
    for (int k = 0; k < 2; ++k) {
      const int64_t d = kmcl::min_image(X[k] - view->prev[2 * i + k], B[k]);
      view->U[2 * i + k] += d;
      view->prev[2 * i + k] = X[k];
      if (std::llabs(d) >= acc->J) f |= BD_JUMPED;
    }
    for (int k = 0; k < 3; ++k) {
      int32_t* q = &view->links[(size_t)k * N + i];
      if (*q != l[k]) f |= BD_CHANGED;
      *q = l[k];
    }
    const int fresh = f & ~view->flags[i];
    n_jumped += (fresh & BD_JUMPED) != 0;
    n_changed += (fresh & BD_CHANGED) != 0;
    view->flags[i] |= (uint8_t)f;
  }
  acc->last_step = v->step;
  acc->n_updates += 1;
  if (info) {
    info->n_updates = acc->n_updates;
    info->n_jumped = n_jumped;
    info->n_changed = n_changed;
  }
  return KMC_OK;
}

int kmc_host_bd_sample(const kmc_params* p, const kmc_state_view* v, const kmc_bd_view* view, const kmc_bd_out* acc,
                       kmc_bd_out* out, kmc_bd_cell* table) {
  if (!StateReader(p, v).ok(false) || !bd_view_ok(view) || !acc || !out)
    return fail(KMC_ERR_ARG, "bd sample: params, state, the view's eight arrays, acc and out are needed");
  if (v->step != acc->last_step)
    return fail(KMC_ERR_ARG, "bd sample: the state has moved on since the last update (an update is due first)");
  const kmc_bd_out a = *acc;  // (out may be acc itself)
  *out = a;
  if (!table) return KMC_OK;
  std::vector<kmc_bd_body> rows;
  const int rc = bd_host_rows(p, v, view, &a, &rows);
  if (rc != KMC_OK) return rc;
  const int ms = a.cfg.max_size;
  std::memset(table, 0, sizeof(kmc_bd_cell) * 2 * ((size_t)ms + 1));
  for (const kmc_bd_body& b : rows) {
    const int n = b.n_r + b.n_l;
    kmc_bd_cell* c = &table[(size_t)(b.n_l > 0) * (ms + 1) + std::min(n, ms)];
    c->n_bodies += 1;
    c->sum_size += n;
    (b.status == KMC_BD_INTACT ? c->n_intact : b.status == KMC_BD_GROWN ? c->n_grown : c->n_broken) += 1;
    if (b.is & KMC_BD_IS_PRISTINE) c->n_pristine += 1;
    if (!(b.is & KMC_BD_IS_VALID)) continue;
    c->n_valid += 1;
    add(&c->m2, (__int128)kmcb::trans_term(b.su[0], b.su[1]));
    if (!(b.is & KMC_BD_IS_ROT)) {
      if (n >= 2) c->n_rot_skipped += 1;
      continue;
    }
    if (b.C == 0 && b.S == 0) {
      c->n_rot_null += 1;
      continue;
    }
    int64_t c1, c2, ph;
    kmcb::rot_terms(b.C, b.S, &c1, &c2, &ph);
    c->n_rot += 1;
    c->c1 += c1;
    c->c2 += c2;
    add(&c->phi2, (__int128)(ph * ph));
  }
  return KMC_OK;
}

int kmc_host_bd_bodies(const kmc_params* p, const kmc_state_view* v, const kmc_bd_view* view, const kmc_bd_out* acc,
                       int32_t min_size, int64_t cap, kmc_bd_body* rows, int64_t* n) {
  if (!StateReader(p, v).ok(false) || !bd_view_ok(view) || !acc || !n || min_size < 1 || cap < 0 || (cap > 0 && !rows))
    return fail(KMC_ERR_ARG,
                "bd bodies: params, state, the view, acc and n are needed, min_size >= 1, cap >= 0, rows for cap > 0");
  if (v->step != acc->last_step)
    return fail(KMC_ERR_ARG, "bd bodies: the state has moved on since the last update (an update is due first)");
  std::vector<kmc_bd_body> all;
  const int rc = bd_host_rows(p, v, view, acc, &all);
  if (rc != KMC_OK) return rc;
  *n = 0;
  for (const kmc_bd_body& b : all)
    if (b.n_r + b.n_l >= min_size) {
      if (*n < cap) rows[*n] = b;
      *n += 1;
    }
  if (*n > cap)
    return fail(KMC_ERR_CAPACITY,
                "bd bodies: " + std::to_string(*n) + " bodies qualify, cap is " + std::to_string(cap));
  return KMC_OK;
}

// Orientation layer (include/kmc.h): kmc_rot_*'s and
// kmc_ligand_pose's definitions on host state views, one protein after the
// other; the vectors, the packing, the pair term and the bins are
// kmc_orient.h's, the ones the device evaluates.  Every sum is taken whole.
namespace {

bool rot_view_ok(const kmc_rot_view* w) {
  return w && w->vec && w->links && w->last_event && w->chi && w->ring && w->table && w->n_pairs;
}

// protein i's packed words, handedness and links; false for a bad protein.  Z, Nz as rot_vectors' (kmc_orient.hip)
bool rot_host_cur(const StateReader& s, int i, uint64_t w[2], int* chi, int32_t l[3], int64_t* Z, int64_t* Nz) {
  const kmc_state_view* v = s.v;
  const int na = s.na, nb = s.nb;
  int64_t X[2];
  tracked(s, i, X, l);
  *chi = 0;
  *Z = *Nz = 0;
  if (i < na) {
    const double b31[2] = {v->ra[RA(na, 3, 1, 0, i)], v->ra[RA(na, 3, 1, 1, i)]};
    const double b32[2] = {v->ra[RA(na, 3, 2, 0, i)], v->ra[RA(na, 3, 2, 1, i)]};
    const kmco::V3 h = kmco::heading(b31, b32);
    const bool ok = kmco::fits(h);
    w[0] = ok ? kmco::pack(h) : ROT_BAD;
    w[1] = 0;
    return ok;
  }
  const int b = i - na;
  double bead[4][3];
  const int jk[4][2] = {{1, 1}, {1, 2}, {2, 1}, {3, 1}};
  for (int m = 0; m < 4; ++m)
    for (int c = 0; c < 3; ++c) bead[m][c] = v->rb[RB(nb, jk[m][0], jk[m][1], c, b)];
  const kmco::Lig g = kmco::ligand(bead[0], bead[1], bead[2], bead[3]);
  const bool ok = kmco::fits(g);
  w[0] = ok ? kmco::pack(g.n) : ROT_BAD;
  w[1] = ok ? kmco::pack(g.a) : ROT_BAD;
  if (ok) *chi = kmco::chi(g.n, g.a, g.c);
  *Z = kmco::q(bead[0][2]);
  *Nz = g.n.z;
  return ok;
}

size_t rot_at(size_t i, int v, size_t na, size_t nb) { return i < na ? i : na + (size_t)v * nb + (i - na); }

}  // namespace

int kmc_host_rot_begin(const kmc_params* p, const kmc_state_view* v, const kmc_rot_config* cfg,
                       const kmc_rot_view* view, kmc_rot_out* acc) {
  const StateReader s(p, v);
  if (const int rc = recorder_args(s, "rot", "seven", true, cfg, rot_view_ok(view), acc)) return rc;
  const kmc_rot_config c = *cfg;
  const char* bad = kmco::check(c.every, c.levels, c.slots);
  if (bad) return fail(KMC_ERR_ARG, bad);
  const size_t na = (size_t)p->n_a, nb = (size_t)p->n_b, N = na + nb, W = na + 2 * nb;
  const int L = c.levels, P = c.slots, rows = kmcl::rows(L, P);
  for (size_t i = 0; i < N; ++i) {
    uint64_t w[2];
    int chi;
    int32_t l[3];
    int64_t Z, Nz;
    rot_host_cur(s, (int)i, w, &chi, l, &Z, &Nz);
    for (int k = 0; k < (i < na ? 1 : 2); ++k) {
      const size_t at = rot_at(i, k, na, nb);
      view->vec[at] = w[k];
      for (int lv = 0; lv < L; ++lv) view->ring[(size_t)(lv * P) * W + at] = w[k];
    }
    for (int k = 0; k < 3; ++k) view->links[(size_t)k * N + i] = l[k];
    view->last_event[i] = 0;
    view->chi[i] = (int8_t)chi;
  }
  std::memset(view->table, 0, sizeof(kmc_rot_cell) * (size_t)rows * LAG_CLASSES * ROT_VECS);
  std::fill(view->n_pairs, view->n_pairs + rows, (int64_t)0);
  std::memset(acc, 0, sizeof *acc);
  acc->cfg = c;
  acc->origin_step = acc->last_step = v->step;
  acc->rows = rows;
  return KMC_OK;
}

int kmc_host_rot_update(const kmc_params* p, const kmc_state_view* v, const kmc_rot_view* view, kmc_rot_out* acc,
                        kmc_rot_info* info) {
  const StateReader s(p, v);
  if (const int rc = recorder_args(s, "rot", "seven", false, nullptr, rot_view_ok(view), acc)) return rc;
  if (v->step != acc->last_step + acc->cfg.every || acc->n_updates >= INT32_MAX) return not_due("rot", acc->cfg.every);
  const size_t na = (size_t)p->n_a, nb = (size_t)p->n_b, N = na + nb, W = na + 2 * nb;
  const int L = acc->cfg.levels, P = acc->cfg.slots;
  const int64_t n = acc->n_updates + 1;
  kmcl::Task tasks[LAG_MAX_ROWS];
  const int nt = kmcl::tasks(n, L, P, tasks);
  int64_t n_events = 0, n_flips = 0, n_bad = 0;
  for (size_t i = 0; i < N; ++i) {
    uint64_t w[2];
    int chi;
    int32_t l[3];
    int64_t Z, Nz;
    const bool ok = rot_host_cur(s, (int)i, w, &chi, l, &Z, &Nz);
    const int nv = i < na ? 1 : 2;
    if (!ok) ++n_bad;
    const bool flip = view->chi[i] != (int8_t)chi;
    view->chi[i] = (int8_t)chi;
    bool ev = flip;
    for (int k = 0; k < 3; ++k) {
      int32_t* q = &view->links[(size_t)k * N + i];
      ev = ev || *q != l[k];
      *q = l[k];
    }
    if (flip) ++n_flips;
    if (ev) {
      view->last_event[i] = (int32_t)n;
      ++n_events;
    }
    const int c = kmcl::cls(i < na, l);
    for (int k = 0; k < nv; ++k) {
      const size_t at = rot_at(i, k, na, nb);
      view->vec[at] = w[k];
      const kmco::V3 u = kmco::unpack(w[k]);
      for (int t = 0; ok && t < nt; ++t) {
        const uint64_t o = view->ring[(size_t)tasks[t].ring * W + at];
        if (o & ROT_BAD) continue;
        const int64_t d = kmco::dot(u, kmco::unpack(o));
        kmc_rot_cell* cell = &view->table[((size_t)tasks[t].row * LAG_CLASSES + c) * ROT_VECS + k];
        cell->n_all += 1;
        add(&cell->s1_all, (__int128)d);
        if (view->last_event[i] > tasks[t].nk) continue;
        cell->n_clean += 1;
        add(&cell->s1_clean, (__int128)d);
        uint64_t a2, ab, b2;
        kmco::split(d, &a2, &ab, &b2);
        add(&cell->s2_clean, (__int128)kmco::sq(a2, ab, b2));
      }
      for (int lv = 0; lv < L && kmcl::fires(n, lv); ++lv) view->ring[(size_t)kmcl::store_ring(n, lv, P) * W + at] = w[k];
    }
  }
  for (int t = 0; t < nt; ++t) view->n_pairs[tasks[t].row] += 1;
  acc->last_step = v->step;
  acc->n_updates = n;
  if (info) {
    info->n_updates = n;
    info->n_tasks = nt;
    info->n_events = n_events;
    info->n_flips = n_flips;
    info->n_bad = n_bad;
  }
  return KMC_OK;
}

int kmc_host_rot_sample(const kmc_params* p, const kmc_rot_view* view, const kmc_rot_out* acc, kmc_rot_out* out,
                        kmc_rot_cell* table, int64_t* n_pairs) {
  if (!p || !rot_view_ok(view) || !acc || !out)
    return fail(KMC_ERR_ARG, "rot sample: params, the view's seven arrays, acc and out are needed");
  const kmc_rot_out a = *acc;  // (out may be acc itself)
  *out = a;
  if (table && table != view->table)
    std::copy(view->table, view->table + (size_t)a.rows * LAG_CLASSES * ROT_VECS, table);
  if (n_pairs && n_pairs != view->n_pairs) std::copy(view->n_pairs, view->n_pairs + a.rows, n_pairs);
  return KMC_OK;
}

int kmc_host_ligand_pose(const kmc_params* p, const kmc_state_view* v, int32_t nz, int32_t nc, int64_t* hist,
                         kmc_pose_out* out) {
  const StateReader s(p, v);
  if (!s.ok(true) || !out) return fail(KMC_ERR_ARG, "pose: params, state and out are needed");
  int64_t BZ, Lq;
  const char* bad = kmco::pose_check(nz, nc, p->box_z, p->rb_radius, &BZ, &Lq);
  if (bad) return fail(KMC_ERR_ARG, bad);
  if (hist) std::fill(hist, hist + (size_t)POSE_CLASSES * nz * nc, (int64_t)0);
  std::memset(out, 0, sizeof *out);
  for (int b = 0; b < p->n_b; ++b) {
    uint64_t w[2];
    int chi;
    int32_t l[3];
    int64_t Z, Nz;
    const bool ok = rot_host_cur(s, s.na + b, w, &chi, l, &Z, &Nz);
    const int k = (l[0] != 0) + (l[1] != 0) + (l[2] != 0);
    if (!ok) {
      out->n_bad += 1;
      continue;
    }
    if (chi > 0) out->chi_pos[k] += 1;
    if (chi < 0) out->chi_neg[k] += 1;
    if (hist) hist[((size_t)k * nz + kmco::pose_zbin(Z, BZ, nz)) * nc + kmco::pose_tbin(Nz, Lq, nc)] += 1;
  }
  return KMC_OK;
}

// Encounter statistics (include/kmc.h): kmc_reach_census' and
// kmc_enc_*'s definitions on host state views by brute force over all pairs;
// the gates, the bin rules and the slot transition are kmc_encounter.h's, the
// ones the device evaluates.
namespace {

struct EncHost {
  const StateReader s;
  const kmc_params* p;
  const int na, nb;
  double T_bond = 0.0, T_cis = 0.0;
  EncHost(const kmc_params* p_, const kmc_state_view* v) : s(p_, v), p(p_), na(s.na), nb(s.nb) {
    if (!ok()) return;
    T_bond = kmce::sqrt_threshold(p->bond_dist_cutoff);
    T_cis = kmce::sqrt_threshold(p->cis_dist_cutoff);
  }
  bool ok() const { return s.ok(true); }
  kmce::V3 a(int i, int j, int k) const {
    return kmce::V3{s.v->ra[RA(na, j, k, 0, i)], s.v->ra[RA(na, j, k, 1, i)], s.v->ra[RA(na, j, k, 2, i)]};
  }
  kmce::V3 b(int q, int j, int k) const {
    return kmce::V3{s.v->rb[RB(nb, j, k, 0, q)], s.v->rb[RB(nb, j, k, 1, q)], s.v->rb[RB(nb, j, k, 2, q)]};
  }
  int st2(int i) const { return s.status2(i); }
  int st3(int i) const { return s.status3(i); }
  int stb(int q, int k) const { return s.site_status(q, k); }
};

// the R–L triple (i, q, k), all 0-based but k: in reach (then *q2, *pd, *ot are set)
bool enc_host_rl(const EncHost& h, int i, int q, int k, double* q2, double* pd, double* ot) {
  const kmce::V3 s = h.a(i, 3, 2), t = h.b(q, k, 2);
  *q2 = kmce::d2(t.x - s.x, t.y - s.y, t.z - s.z);
  if (!(*q2 < h.T_bond)) return false;
  kmce::rl_angles(h.a(i, 3, 1), s, h.a(i, 3, 4), h.b(q, k, 1), t, h.b(q, 1, 1), h.b(q, 1, 2), pd, ot);
  return true;
}

bool enc_view_ok(const kmc_enc_view* w) { return w && w->lig && w->site && w->key && w->since && w->nreact && w->flags; }

// receptor i's (0-based) current look, checked as the device checks it
bool enc_host_cur(const EncHost& h, int i, int slots, kmce::Cur* c) {
  kmck::Cur l;
  bool ok = kin_host_cur(h.s, i, &l);
  if (ok && l.lig != 0 && (l.site < 2 || l.site > 4)) ok = false;
  kmce::cur_clear(*c, ok ? l.lig : 0, ok && l.lig != 0 ? l.site : 0);
  if (!ok) return false;
  if (h.st2(i) != 0) return true;
  for (int q = 0; q < h.nb; ++q)
    for (int k = 2; k <= 4; ++k) {
      if (h.stb(q, k) != 0) continue;
      double q2, pd, ot;
      if (!enc_host_rl(h, i, q, k, &q2, &pd, &ot)) continue;
      kmce::cur_add(*c, slots, kmce::key_of(q + 1, k), pd < h.p->bond_thetapd_cutoff && ot < h.p->bond_thetaot_cutoff);
    }
  return true;
}

kmce::Slots enc_load(const kmc_enc_view* w, int i) {
  kmce::Slots r;
  r.lig = w->lig[i];
  r.site = w->site[i];
  for (int s = 0; s < ENC_SLOTS; ++s) {
    r.key[s] = w->key[(size_t)i * ENC_SLOTS + s];
    r.since[s] = w->since[(size_t)i * ENC_SLOTS + s];
    r.nreact[s] = w->nreact[(size_t)i * ENC_SLOTS + s];
    r.flags[s] = w->flags[(size_t)i * ENC_SLOTS + s];
  }
  return r;
}

void enc_store(const kmc_enc_view* w, int i, const kmce::Slots& r) {
  w->lig[i] = r.lig;
  w->site[i] = r.site;
  for (int s = 0; s < ENC_SLOTS; ++s) {
    w->key[(size_t)i * ENC_SLOTS + s] = r.key[s];
    w->since[(size_t)i * ENC_SLOTS + s] = r.since[s];
    w->nreact[(size_t)i * ENC_SLOTS + s] = r.nreact[s];
    w->flags[(size_t)i * ENC_SLOTS + s] = r.flags[s];
  }
}

void enc_set_occ(kmc_enc_out* acc, const int64_t cnt[kmce::ENC_NCNT]) {
  acc->occ_reach = cnt[kmce::C_OCC_REACH];
  acc->occ_reactive = cnt[kmce::C_OCC_REACTIVE];
  acc->occ_free_receptor = cnt[kmce::C_OCC_FREE];
}

}  // namespace

int kmc_host_reach_census(const kmc_params* p, const kmc_state_view* v, int32_t nd, int32_t na, kmc_reach_out* out,
                          int64_t* hist_d, int64_t* hist_a_rl, int64_t* hist_a_cis) {
  const EncHost h(p, v);
  if (!h.ok() || !out)
    return fail(KMC_ERR_ARG, "reach census: params, the state's four arrays and out are needed");
  if (nd < 1 || nd > ENC_MAX_ND || na < 1 || na > ENC_MAX_NA)
    return fail(KMC_ERR_ARG, "reach census: 1 <= nd <= 64 and 1 <= na <= 36");
  double E2[ENC_CHANNELS][ENC_MAX_ND];
  kmce::edges(p->bond_dist_cutoff, nd, E2[kmce::CH_RL]);
  kmce::edges(p->cis_dist_cutoff, nd, E2[kmce::CH_MONO]);
  kmce::edges(p->cis_dist_cutoff, nd, E2[kmce::CH_CX]);
  std::memset(out, 0, sizeof *out);
  if (hist_d) std::fill(hist_d, hist_d + (size_t)ENC_CHANNELS * 2 * nd, (int64_t)0);
  if (hist_a_rl) std::fill(hist_a_rl, hist_a_rl + (size_t)na * na, (int64_t)0);
  if (hist_a_cis) std::fill(hist_a_cis, hist_a_cis + (size_t)2 * na, (int64_t)0);
  auto file = [&](int ch, bool react, double q2) {
    out->n_reach[ch] += 1;
    out->n_reactive[ch] += react ? 1 : 0;
    if (hist_d) hist_d[(size_t)(ch * 2 + (react ? 1 : 0)) * nd + kmce::dist_bin(E2[ch], nd, q2)] += 1;
  };
  std::vector<uint8_t> site_hit((size_t)3 * h.nb, 0);
  for (int q = 0; q < h.nb; ++q)
    for (int k = 2; k <= 4; ++k) out->rl_free_sites += h.stb(q, k) == 0 ? 1 : 0;
  for (int i = 0; i < h.na; ++i) {
    if (h.st2(i) != 0) continue;
    out->rl_free_receptors += 1;
    int64_t partners = 0;
    for (int q = 0; q < h.nb; ++q)
      for (int k = 2; k <= 4; ++k) {
        if (h.stb(q, k) != 0) continue;
        double q2, pd, ot;
        if (!enc_host_rl(h, i, q, k, &q2, &pd, &ot)) continue;
        file(kmce::CH_RL, pd < p->bond_thetapd_cutoff && ot < p->bond_thetaot_cutoff, q2);
        if (hist_a_rl) hist_a_rl[(size_t)kmce::ang_bin(pd, na) * na + kmce::ang_bin(ot, na)] += 1;
        site_hit[(size_t)3 * q + (k - 2)] = 1;
        partners += 1;
      }
    out->rl_receptors_in_reach += partners > 0 ? 1 : 0;
    out->rl_max_partners = std::max(out->rl_max_partners, partners);
  }
  for (uint8_t f : site_hit) out->rl_sites_in_reach += f;
  for (int i = 0; i < h.na; ++i) {
    if (h.st3(i) != 0) continue;
    for (int j = i + 1; j < h.na; ++j) {
      if (h.st3(j) != 0) continue;
      const kmce::V3 si = h.a(i, 3, 3), sj = h.a(j, 3, 3);
      const double q2 = kmce::d2(sj.x - si.x, sj.y - si.y, sj.z - si.z);
      if (!(q2 < h.T_cis)) continue;
      const double ot = kmce::cis_angle(h.a(i, 3, 1), si, h.a(j, 3, 1), sj);
      const int ch = h.st2(i) != 0 || h.st2(j) != 0 ? kmce::CH_CX : kmce::CH_MONO;
      file(ch, ot < p->cis_thetaot_cutoff, q2);
      if (hist_a_cis) hist_a_cis[(size_t)(ch - kmce::CH_MONO) * na + kmce::ang_bin(ot, na)] += 1;
    }
  }
  return KMC_OK;
}

int kmc_host_enc_begin(const kmc_params* p, const kmc_state_view* v, const kmc_enc_config* cfg,
                       const kmc_enc_view* view, kmc_enc_out* acc, int64_t* hist10) {
  const EncHost h(p, v);
  if (!h.ok() || !cfg || !enc_view_ok(view) || !acc || !hist10)
    return fail(KMC_ERR_ARG, "enc: params, state, the configuration, the view's six arrays, acc and hist are needed");
  if (cfg->every < 1) return fail(KMC_ERR_ARG, "enc: every >= 1");
  // debug: fewer slots are kept per receptor
  const char* e = getenv("KMC_DEBUG_ENC_SLOTS");
  const int slots = e && *e ? std::max(1, std::min(ENC_SLOTS, atoi(e))) : ENC_SLOTS;
  int64_t cnt[kmce::ENC_NCNT] = {0};
  std::vector<kmce::Slots> recs((size_t)h.na);
  for (int i = 0; i < h.na; ++i) {
    kmce::Cur c;
    if (!enc_host_cur(h, i, slots, &c)) return fail(KMC_ERR_STATE, "enc: a receptor's bond link leaves its range");
    int32_t m[kmce::ENC_NCNT] = {0};
    kmce::begin(v->step, c, recs[(size_t)i], m);
    for (int k = 0; k < kmce::ENC_NCNT; ++k) cnt[k] += m[k];
  }
  for (int i = 0; i < h.na; ++i) enc_store(view, i, recs[(size_t)i]);
  std::memset(acc, 0, sizeof *acc);
  std::fill(hist10, hist10 + (size_t)ENC_ACC_ROWS * ENC_BINS, (int64_t)0);
  acc->origin_step = acc->last_step = v->step;
  acc->n_overflow = cnt[kmce::C_OVERFLOW];
  acc->every = cfg->every;
  acc->slots = slots;
  enc_set_occ(acc, cnt);
  return KMC_OK;
}

int kmc_host_enc_update(const kmc_params* p, const kmc_state_view* v, const kmc_enc_view* view, kmc_enc_out* acc,
                        int64_t* hist10) {
  const EncHost h(p, v);
  if (!h.ok() || !enc_view_ok(view) || !acc || !hist10)
    return fail(KMC_ERR_ARG, "enc: params, state, the view's six arrays, acc and hist are needed");
  const int64_t t = v->step, dt = t - acc->last_step;
  if (dt == 0) {  // a second update at the same step moves only the count
    acc->n_updates += 1;
    return KMC_OK;
  }
  if (dt != acc->every)
    return not_due("enc", acc->every);
  const int slots = (int)acc->slots;
  std::vector<kmce::Cur> cur((size_t)h.na);
  for (int i = 0; i < h.na; ++i)  // checked first: a failed call leaves the recorder as it was
    if (!enc_host_cur(h, i, slots, &cur[(size_t)i]))
      return fail(KMC_ERR_STATE, "enc: a receptor's bond link leaves its range");
  acc->exp_reach += dt * acc->occ_reach;
  acc->exp_reactive += dt * acc->occ_reactive;
  acc->exp_free_receptor += dt * acc->occ_free_receptor;
  int64_t cnt[kmce::ENC_NCNT] = {0};
  for (int i = 0; i < h.na; ++i) {
    kmce::Slots r = enc_load(view, i);
    bool occ[ENC_SLOTS];
    for (int s = 0; s < ENC_SLOTS; ++s) {
      const int32_t k = r.key[s];
      const int q = (k >> 2) - 1;
      occ[s] = k != 0 && q >= 0 && q < h.nb && h.stb(q, 2 + (k & 3)) != 0;
    }
    kmce::Events ev;
    int32_t m[kmce::ENC_NCNT] = {0};
    kmce::transition(t, h.na, cur[(size_t)i], occ, r, ev, m);
    for (int k = 0; k < ev.n; ++k) {
      hist10[(size_t)ev.row[k] * ENC_BINS + kmck::bin(ev.val[k])] += 1;
      hist10[(size_t)(ENC_ROWS_UPD + ev.rrow[k]) * ENC_BINS + kmck::bin(ev.rval[k])] += 1;
    }
    enc_store(view, i, r);
    for (int k = 0; k < kmce::ENC_NCNT; ++k) cnt[k] += m[k];
  }
  acc->on_from_encounter += cnt[kmce::C_FROM_ENCOUNTER];
  acc->on_direct += cnt[kmce::C_DIRECT];
  acc->n_opened += cnt[kmce::C_OPENED];
  acc->n_ended += cnt[kmce::C_ENDED];
  acc->n_overflow += cnt[kmce::C_OVERFLOW];
  enc_set_occ(acc, cnt);
  acc->last_step = t;
  acc->n_updates += 1;
  return KMC_OK;
}

int kmc_host_enc_sample(const kmc_params* p, const kmc_enc_view* view, const kmc_enc_out* acc, const int64_t* hist10,
                        kmc_enc_out* out, int64_t* hist, int64_t* react_hist) {
  if (!p || !enc_view_ok(view) || !acc || !hist10 || !out)
    return fail(KMC_ERR_ARG, "enc sample: params, the view's six arrays, acc, hist10 and out are needed");
  const kmc_enc_out a = *acc;  // (out may be acc itself)
  *out = a;
  out->n_censored_alive = 0;
  if (hist) {
    std::copy(hist10, hist10 + (size_t)ENC_ROWS_UPD * ENC_BINS, hist);
    std::fill(hist + (size_t)ENC_ROWS_UPD * ENC_BINS, hist + (size_t)ENC_HISTS * ENC_BINS, (int64_t)0);
  }
  if (react_hist)
    std::copy(hist10 + (size_t)ENC_ROWS_UPD * ENC_BINS, hist10 + (size_t)ENC_ACC_ROWS * ENC_BINS, react_hist);
  for (int i = 0; i < p->n_a; ++i) {
    const kmce::Slots r = enc_load(view, i);
    for (int s = 0; s < ENC_SLOTS; ++s) {
      if (r.key[s] == 0) continue;
      if (r.flags[s] & kmce::F_CENSORED) out->n_censored_alive += 1;
      else if (hist) hist[(size_t)kmce::ROW_ALIVE * ENC_BINS + kmck::bin(a.last_step - r.since[s])] += 1;
    }
  }
  return KMC_OK;
}

// Proximity clusters (include/kmc.h), sequential on the bond
// order's cell grid (BoHost holds all n_a + n_b proteins by reference index):
// the neighbour counts, a union-find over the core pairs in index order, the
// border rule from each non-core's side, then the counts; c(i) is
// kmc_host_census' label.  The expressions are kmc_proximity.h's.
int kmc_host_prox_clusters(const kmc_params* p, const kmc_state_view* v, int32_t which, int32_t select,
                           const uint8_t* mask, double eps, int32_t min_pts, int32_t max_size, int32_t nbins,
                           kmc_prox_out* out, int64_t* size_hist, int64_t* nn_hist, int64_t* nnd_hist, int32_t* label,
                           int32_t* nn, uint8_t* kind) {
  const StateReader s(p, v);
  if (!s.ok(true) || !out || which < KMC_PX_A || which > KMC_PX_AB || (select != KMC_SK_ALL && select != KMC_SK_BOUND) ||
      min_pts < 1 || min_pts > PX_MIN_PTS_MAX || max_size < 1 || max_size > PX_MAX_SIZE || nbins < 1 ||
      nbins > PX_NND_BINS)
    return fail(KMC_ERR_ARG,
                "prox: params, state and out are needed, which 0..2, select 0 or 1, 1 <= min_pts <= 2^30, 1 <= max_size <= 65535, 1 <= nbins <= 4096");
  const int na = s.na, n = s.n;
  BoHost h;
  if (const int rc = bo_box(s, "prox", &h)) return rc;
  h.n = n;
  const int64_t EPS = eps > 0.0 && eps * 1024.0 < (double)BO_BOX_MAX ? (int64_t)kmcm::round_(eps * 1024.0) : 0;
  if (EPS < 1 || h.B[0] / EPS < 3 || h.B[1] / EPS < 3)
    return fail(KMC_ERR_ARG,
                "prox: eps must be at least 2^-10 A and at most a third of the box (3 cells along an axis)");
  std::vector<int32_t> c((size_t)n, 0);
  kmc_census census;
  const int rc = kmc_host_census(p, v, c.data(), 0, 0, nullptr, &census);
  if (rc != KMC_OK) return rc;
  h.sel.assign((size_t)n, 0);
  h.X.resize((size_t)n);
  h.Y.resize((size_t)n);
  std::vector<int32_t> who;
  for (int i = 0; i < n; ++i) {
    h.X[i] = s.ipos(i, 0);
    h.Y[i] = s.ipos(i, 1);
    bool sel = which != (i < na ? KMC_PX_B : KMC_PX_A) && (select == KMC_SK_ALL || s.bound(i));
    if (sel && mask) sel = mask[i] != 0;
    h.sel[i] = sel;
    if (sel) who.push_back(i);
  }
  BoCells g;
  g.build(h, who, EPS);
  const int64_t EPS2 = EPS * EPS;
  auto dist2 = [&](int i, int j) {
    const int64_t DX = kmcb::fold(h.X[j] - h.X[i], h.B[0]), DY = kmcb::fold(h.Y[j] - h.Y[i], h.B[1]);
    return DX * DX + DY * DY;
  };
  std::vector<int32_t> N((size_t)n, 0), lab((size_t)n, 0), parent((size_t)n);
  std::vector<int64_t> M((size_t)n, 0);
  std::vector<uint8_t> kd((size_t)n, 0);
  for (int i : who) {
    int64_t best = INT64_MAX;
    g.around(h, i, [&](int j) {
      if (j == i) return;
      const int64_t D2 = dist2(i, j);
      if (D2 > EPS2) return;
      N[i] += 1;
      best = std::min(best, D2);
    });
    M[i] = N[i] ? best : 0;
    kd[i] = kmcx::is_core(N[i], min_pts) ? 3 : 1;
  }
  for (int i = 0; i < n; ++i) parent[i] = i;
  auto find = [&](int x) {
    while (parent[x] != x) x = parent[x] = parent[parent[x]];
    return x;
  };
  std::memset(out, 0, sizeof *out);
  for (int i : who) {
    if (kd[i] != 3) continue;
    g.around(h, i, [&](int j) {
      if (j >= i || kd[j] != 3 || dist2(i, j) > EPS2) return;
      out->n_core_edges += 1;
      const int a = find(i), b = find(j);
      if (a != b) parent[std::max(a, b)] = std::min(a, b);
    });
  }
  for (int i : who)
    if (kd[i] == 3) lab[i] = find(i) + 1;
  for (int i : who) {
    if (kd[i] == 3 || N[i] == 0) continue;
    int64_t bestD = 0;
    int32_t bestR = -1;
    g.around(h, i, [&](int j) {
      if (j == i || kd[j] != 3) return;
      const int64_t D2 = dist2(i, j);
      if (D2 > EPS2 || !kmcx::nearer(D2, j, bestD, bestR)) return;
      bestD = D2;
      bestR = j;
    });
    if (bestR >= 0) {
      kd[i] = 2;
      lab[i] = lab[bestR];
    }
  }
  const double dr = eps / nbins;
  std::vector<int64_t> E2((size_t)nbins);
  for (int m = 0; m < nbins; ++m) {
    const int64_t e = kmcb::corr_edge(m, dr);
    E2[m] = e * e;
  }
  const double inv = 1.0 / (dr * 1024.0);
  if (size_hist) std::fill(size_hist, size_hist + (size_t)max_size + 1, (int64_t)0);
  if (nn_hist) std::fill(nn_hist, nn_hist + KMC_PX_NN_ROWS, (int64_t)0);
  if (nnd_hist) std::fill(nnd_hist, nnd_hist + nbins, (int64_t)0);
  // by root (a cluster's label - 1, a component's c - 1): members and the ranges purity is read from
  std::vector<int32_t> cnt((size_t)n, 0), cmin((size_t)n, INT32_MAX), cmax((size_t)n, -1), pmin((size_t)n, INT32_MAX),
      pmax((size_t)n, -1), bsel((size_t)n, 0);
  for (int i : who) {
    out->n_sel += 1;
    (kd[i] == 3 ? out->n_core : kd[i] == 2 ? out->n_border : out->n_noise) += 1;
    out->sum_nn += N[i];
    if (nn_hist) nn_hist[std::min<int32_t>(N[i], KMC_PX_NN_ROWS - 1)] += 1;
    if (N[i] == 0) out->n_alone += 1;
    else if (nnd_hist) nnd_hist[kmcx::nnd_bin(E2.data(), nbins, M[i], (int)(std::sqrt((double)M[i]) * inv))] += 1;
    const int ci = c[i] - 1, L = lab[i];
    bsel[ci] += 1;
    pmin[ci] = std::min(pmin[ci], L);
    pmax[ci] = std::max(pmax[ci], L);
    if (L > 0) {
      cnt[L - 1] += 1;
      cmin[L - 1] = std::min(cmin[L - 1], ci);
      cmax[L - 1] = std::max(cmax[L - 1], ci);
    }
  }
  for (int i = 0; i < n; ++i) {
    if (kd[i] == 3 && lab[i] == i + 1) {
      const int size = cnt[i];
      if (size_hist) size_hist[std::min(size, (int)max_size)] += 1;
      out->n_clusters += 1;
      if (size > out->max_size) {  // (roots come in label order: the first of a size keeps the tie)
        out->max_size = size;
        out->max_label = i + 1;
      }
      if (size >= 2) {
        out->n_multi += 1;
        if (cmin[i] == cmax[i]) {
          out->n_pure += 1;
          if (bsel[cmin[i]] == size) out->n_whole += 1;
        }
      }
    }
    if (bsel[i] >= 2) {
      out->n_bond_multi += 1;
      if (pmin[i] == pmax[i] && pmin[i] > 0) out->n_bond_kept += 1;
    }
  }
  if (label) std::copy(lab.begin(), lab.end(), label);
  if (nn) std::copy(N.begin(), N.end(), nn);
  if (kind) std::copy(kd.begin(), kd.end(), kind);
  return KMC_OK;
}
