// kmc_encounter.hip — encounter statistics over the committed state (DESIGN.md
// §22): which receptor sites and free ligand sites (and which pairs of cis
// sites) are within the engine's reaction distance, which of them also pass
// its orientation gates, and, for the R–L channel, a recorder that follows
// every such encounter from the update it opens to the one it ends in — the
// bond, a separation, or the loss of one side.  Like the other layers nothing
// here runs inside a step: the kernels are launched by kmc_reach_census /
// kmc_enc_* between kmc_step calls, read what kmc_get_state would return and
// write only the layer's own arrays.
//
// The pair walk is three-dimensional, fp64 and site to site.  The site points
// (x, y, z and an id word) are sorted by the cell of an xy grid whose side is
// at least the cutoff (count / bins_scan / scatter), the probing receptors
// likewise, and a WAVE takes a probe cell: it stages the cell's probes and a
// neighbour cell's points in an LDS region of its own (kmc_pairdyn.hip's
// walker) and its lanes take the staged pairs.  No periodic image is taken,
// as in the engine's gates: the 3 x 3 neighbourhood is clipped at the border,
// where the clamped cells hold every point outside [-box / 2, box / 2).
//   phase A  the distance test; the hits of a wave are compacted by ballot and
//            prefix into one list (one atomic per wave and round).  The list
//            has a capacity: the host reads the count, grows the list and
//            replays the walk when it was exceeded.
//   phase B  one lane a HIT: the remaining beads are gathered through the slot
//            maps and the two acos gates evaluated, so the rare expensive branch
//            does not run at 1/64 occupancy inside the walk.  The census bins
//            are privatised in LDS and flushed with 64-bit integer atomics.
//   slots    one thread a receptor: its hits (found through the per-receptor
//            counts' scan) are cut to the smallest keys in registers and the
//            slot transition of kmc_encounter.h applied.
// Every sum is an integer: any schedule gives the same bits.
//
// Included by kmc_engine.hip after kmc_bodydyn.hip (one translation unit, the
// library's flags); the expressions are kmc_encounter.h's, shared with
// kmc_host_reach_census / kmc_host_enc_* (kmc_host_observe.cpp); the host side of the
// calls is kmc_observe.hip §encounters.
#include "kmc_device.h"
#include "kmc_encounter.h"
#include "kmc_observe.h"

namespace kmcd {

#define ENC_T 256     // threads per workgroup
#define ENC_WAVES 4   // waves, and so probe cells, a workgroup takes at once
#define ENC_CHUNK 64  // points a wave stages per side (KMC_DEBUG_ENC_CHUNK lowers it)

typedef unsigned long long enc_u64;

struct alignas(16) EncPt {  // a site point
  double x, y, z;
  int32_t id;    // R–L probe: receptor (0-based reference index); R–L point: the key b << 2 | (k - 2);
                 // cis: receptor (0-based reference index)
  int32_t aux;   // cis: 1 when the receptor holds a ligand
};

struct alignas(8) EncHit {  // a pair within the cutoff
  double d2;
  int32_t a, b;  // the ids of the probe and of the point
  int32_t rank;  // R–L: the hit's place among its receptor's hits
  int32_t aux;   // cis: the pair's kind (CH_MONO, CH_CX)
};

struct EncGrid {
  int ncx, ncy;
  double x0, y0;  // the box's lower corner (-box / 2: main.cpp:329)
  double cs;      // cell side >= (1 + 2^-10) cutoff
};

// layout of the census tables (64-bit words)
#define ENC_TAB_D 0                                      // hist_d [3][2][nd]
#define ENC_TAB_ARL (ENC_CHANNELS * 2 * ENC_MAX_ND)      // hist_a_rl [na][na]
#define ENC_TAB_ACIS (ENC_TAB_ARL + ENC_MAX_NA * ENC_MAX_NA)  // hist_a_cis [2][na]
#define ENC_TAB_N (ENC_TAB_ACIS + 2 * ENC_MAX_NA)        // n_reach[3], n_reactive[3]
#define ENC_TAB_RL (ENC_TAB_N + 6)                       // free receptors, free sites, receptors / sites in reach
#define ENC_TAB_WORDS (ENC_TAB_RL + 4)

struct EncAcc {
  enc_u64 cnt[kmce::ENC_NCNT];  // the first ENC_NEV since begin, the rest of the last begin / update
  enc_u64 alive;                // of the last sample: censored slots still open
  unsigned int nhits;           // hits the last walk found (may exceed the list's capacity)
  unsigned int max_partners;    // census: the largest number of partners of one receptor
  unsigned int err;             // a slot or a link left its range in the last call
  unsigned int pad;
};

// the walk's scratch, shared by the census and the recorder; allocated at the first call, kept by the handle
struct EncW {
  EncPt *probe = nullptr, *point = nullptr;      // [NA], [max(3 NB, 1)] sorted by cell
  int32_t *pcell = nullptr, *prank = nullptr;    // [NA] cell (-1: not a probe) and rank of receptor i
  int32_t *tcell = nullptr, *trank = nullptr;    // [3 NB] of ligand site (b, k)
  int32_t *pcnt = nullptr, *pstart = nullptr, *tcnt = nullptr, *tstart = nullptr, *part = nullptr;  // [ncell + 1]
  int32_t *rcnt = nullptr, *rstart = nullptr, *rpart = nullptr;  // [NA + 1] hits per receptor and their scan
  EncHit* hits = nullptr;      // [hit_cap]
  int32_t* rhit = nullptr;     // [hit_cap] key << 1 | reactive, grouped by receptor
  uint8_t* site_flag = nullptr;  // [3 NB] the site has a partner in reach
  double* E2 = nullptr;        // [3][ENC_MAX_ND] squared edges per channel
  enc_u64* tab = nullptr;      // [ENC_TAB_WORDS]
  EncAcc* acc = nullptr;
  unsigned int hit_cap = 0;
  EncGrid G = {0, 0, 0.0, 0.0, 0.0};
};

// host side of the walk
struct EncWalk {
  EncW w;
  int chunk = ENC_CHUNK;  // KMC_DEBUG_ENC_CHUNK: smaller staged chunks (the chunked path at test size)
  hipEvent_t ev[4] = {nullptr, nullptr, nullptr, nullptr};  // after phase A and after phase B of the last call's
                                                            // (up to two) walks
  double ms[3] = {0.0, 0.0, 0.0};  // binning + phase A, phase B, the rest (kmc_enc_phase_ms)
};

struct Enc {  // the recorder's arrays, by the receptor's reference index
  int32_t *lig, *site;  // [NA]
  int4* key;            // [NA] the four keys
  longlong4* since;     // [NA]
  int4* nreact;         // [NA]
  uchar4* flags;        // [NA]
};

// host side: allocated by kmc_enc_begin, freed by kmc_enc_end
struct EncState {
  Recorder rec;
  Scratch scratch;
  Enc dev = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
  enc_u64* hist = nullptr;  // [ENC_ACC_ROWS + 1][ENC_BINS]: rows 0-7, react_hist's two, then row 8 of the last sample
  int32_t every = 1;
  int slots = ENC_SLOTS;    // KMC_DEBUG_ENC_SLOTS: fewer slots kept (the truncation at test size)
  int64_t occ[3] = {0, 0, 0};  // open slots, reactive slots, free receptors at the last update
  int64_t exp[3] = {0, 0, 0};  // exposures since begin
  int64_t ev[ENC_NEV] = {0, 0, 0, 0, 0};  // the event counters since begin
};

__device__ __forceinline__ int enc_cell1(double x, double cs, int nc) {
  const double q = x / cs;
  return !(q >= 0.0) ? 0 : q >= (double)nc ? nc - 1 : (int)q;
}
__device__ __forceinline__ int enc_cell(const EncGrid& G, double x, double y) {
  return enc_cell1(y - G.y0, G.cs, G.ncy) * G.ncx + enc_cell1(x - G.x0, G.cs, G.ncx);
}

__device__ __forceinline__ kmce::V3 enc_a(const Dev& d, int slot, int j, int k) {
  return kmce::V3{d.cur.A(slot, j, k, 0), d.cur.A(slot, j, k, 1), d.cur.A(slot, j, k, 2)};
}
__device__ __forceinline__ kmce::V3 enc_b(const Dev& d, int lb, int j, int k) {
  return kmce::V3{d.cur.B(lb, j, k, 0), d.cur.B(lb, j, k, 1), d.cur.B(lb, j, k, 2)};
}

// The site points of one thread's receptor (t < NA) and ligand site (t < 3 NB):
// CIS == false: the probe is bead [3][2] of a receptor with status[2] == 0, the
// point bead [k][2] of a ligand site with status[k] == 0; CIS == true: bead
// [3][3] of a receptor with status[3] == 0 is probe and point.  false: a slot
// left its range.
template <bool CIS>
__device__ __forceinline__ bool enc_probe(const KParams& P, const Dev& d, int i, EncPt* pt, bool* on) {
  const int NA = P.NA;
  const int slot = d.slot_of[i];
  *on = false;
  if ((unsigned)slot >= (unsigned)NA) return false;
  if ((CIS ? A_ST3(d, slot) : A_ST2(d, slot)) != 0) return true;
  const kmce::V3 v = enc_a(d, slot, 3, CIS ? 3 : 2);
  *pt = EncPt{v.x, v.y, v.z, i, CIS && A_ST2(d, slot) != 0 ? 1 : 0};
  *on = true;
  return true;
}
__device__ __forceinline__ bool enc_site(const KParams& P, const Dev& d, int t, EncPt* pt, bool* on) {
  const int NA = P.NA, NB = P.NB;
  const int b = t / 3, k = 2 + t % 3;
  const int slot = d.slot_of[NA + b];
  *on = false;
  if (slot < NA || slot >= P.N) return false;
  const int lb = slot - NA;
  if (B_ST(d, lb, k) != 0) return true;
  const kmce::V3 v = enc_b(d, lb, k, 2);
  *pt = EncPt{v.x, v.y, v.z, kmce::key_of(b + 1, k), 0};
  *on = true;
  return true;
}

// binning, first pass: cell and rank of every probe and point
template <bool CIS>
__global__ void __launch_bounds__(ENC_T) k_enc_count(KParams P, Dev d, EncW W) {
  const int t = blockIdx.x * ENC_T + threadIdx.x;
  bool bad = false;
  if (t < P.NA) {
    EncPt pt;
    bool on;
    bad = !enc_probe<CIS>(P, d, t, &pt, &on);
    int c = -1;
    if (on) {
      c = enc_cell(W.G, pt.x, pt.y);
      W.prank[t] = atomicAdd(&W.pcnt[c], 1);
    }
    W.pcell[t] = c;
  }
  if (!CIS && t < 3 * P.NB) {
    EncPt pt;
    bool on;
    bad = !enc_site(P, d, t, &pt, &on) || bad;
    int c = -1;
    if (on) {
      c = enc_cell(W.G, pt.x, pt.y);
      W.trank[t] = atomicAdd(&W.tcnt[c], 1);
    }
    W.tcell[t] = c;
  }
  if (bad) atomicOr(&W.acc->err, 1u);
}

// binning, second pass: the points into their cells
template <bool CIS>
__global__ void __launch_bounds__(ENC_T) k_enc_scatter(KParams P, Dev d, EncW W) {
  const int t = blockIdx.x * ENC_T + threadIdx.x;
  if (t < P.NA && W.pcell[t] >= 0) {
    EncPt pt;
    bool on;
    if (enc_probe<CIS>(P, d, t, &pt, &on) && on) W.probe[W.pstart[W.pcell[t]] + W.prank[t]] = pt;
  }
  if (!CIS && t < 3 * P.NB && W.tcell[t] >= 0) {
    EncPt pt;
    bool on;
    if (enc_site(P, d, t, &pt, &on) && on) W.point[W.tstart[W.tcell[t]] + W.trank[t]] = pt;
  }
}

// (kmc_pairdyn.hip's pd_wave_sync: what one wave wrote to its LDS region is read by its other lanes)
__device__ __forceinline__ void enc_wave_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// Phase A.  Wave w of workgroup b takes the probe cells (b * ENC_WAVES + w) +
// n * gridDim.x * ENC_WAVES.  Both sides are staged in chunks of `chunk`
// points, so any cell population is handled.  Every lane of the wave runs every
// round of the pair loop (the bound is uniform), so the ballot sees the whole
// wave.  CIS: the pair is taken where the probe's reference index is the
// lower one.
template <bool CIS>
__global__ void __launch_bounds__(ENC_T) k_enc_walk(EncW W, double T2, int chunk) {
  extern __shared__ __attribute__((aligned(16))) EncPt enc_lds[];  // [ENC_WAVES][2][chunk]
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  EncPt* si = enc_lds + (size_t)wave * 2 * chunk;
  EncPt* sj = si + chunk;
  const EncGrid G = W.G;
  const int ncell = G.ncx * G.ncy;
  const EncPt* __restrict__ ipts = W.probe;
  const EncPt* __restrict__ jpts = CIS ? W.probe : W.point;
  const int32_t* __restrict__ icst = W.pstart;
  const int32_t* __restrict__ jcst = CIS ? W.pstart : W.tstart;
  const unsigned int cap = W.hit_cap;
  for (int c = blockIdx.x * ENC_WAVES + wave; c < ncell; c += gridDim.x * ENC_WAVES) {
    const int i0 = icst[c], i1 = icst[c + 1];
    if (i0 == i1) continue;
    const int cx = c % G.ncx, cy = c / G.ncx;
    for (int q = 0; q < 9; ++q) {
      const int nx = cx + q % 3 - 1, ny = cy + q / 3 - 1;
      if (nx < 0 || nx >= G.ncx || ny < 0 || ny >= G.ncy) continue;  // no periodic image
      const int jc = ny * G.ncx + nx;
      const int j0 = jcst[jc], j1 = jcst[jc + 1];
      if (j0 == j1) continue;
      for (int ib = i0; ib < i1; ib += chunk) {
        const int ni = min(chunk, i1 - ib);
        for (int jb = j0; jb < j1; jb += chunk) {
          const int nj = min(chunk, j1 - jb);
          enc_wave_sync();  // the previous block's reads are done
          for (int t = lane; t < ni; t += 64) si[t] = ipts[ib + t];
          for (int t = lane; t < nj; t += 64) sj[t] = jpts[jb + t];
          enc_wave_sync();
          const int np = ni * nj;
          for (int e0 = 0; e0 < np; e0 += 64) {
            const int e = e0 + lane;
            bool hit = false;
            EncHit h = {0.0, 0, 0, 0, 0};
            if (e < np) {
              const int a = e / nj, b = e - a * nj;
              const EncPt pi = si[a], pj = sj[b];
              h.d2 = kmce::d2(pj.x - pi.x, pj.y - pi.y, pj.z - pi.z);
              h.a = pi.id;
              h.b = pj.id;
              h.aux = CIS ? (pi.aux | pj.aux ? kmce::CH_CX : kmce::CH_MONO) : 0;
              hit = h.d2 < T2 && (!CIS || pi.id < pj.id);
            }
            const enc_u64 m = __ballot(hit);
            if (m == 0ull) continue;
            unsigned int base = 0;
            if (lane == 0) base = atomicAdd(&W.acc->nhits, (unsigned int)__popcll(m));
            base = (unsigned int)__shfl((int)base, 0);
            if (hit) {
              if (!CIS) h.rank = atomicAdd(&W.rcnt[h.a], 1);
              const unsigned int at = base + (unsigned int)__popcll(m & ((1ull << lane) - 1ull));
              if (at < cap) W.hits[at] = h;  // (beyond: the host sees nhits > cap and replays)
            }
          }
        }
      }
    }
  }
}

// Phase B: one lane a hit.  The gates, the census bins (hist != 0) and, for the
// R–L channel, the hit's entry in its receptor's run of rhit and the site's
// flag.  Workgroups stride over the hits.
template <bool CIS>
__global__ void __launch_bounds__(ENC_T) k_enc_gates(KParams P, Dev d, EncW W, int nd, int na, int hist) {
  __shared__ uint32_t tab[ENC_TAB_N + 6];
  __shared__ double E2[ENC_CHANNELS * ENC_MAX_ND];
  const int NA = P.NA;
  if (hist) {
    for (int e = threadIdx.x; e < ENC_TAB_N + 6; e += ENC_T) tab[e] = 0u;
    for (int e = threadIdx.x; e < ENC_CHANNELS * ENC_MAX_ND; e += ENC_T) E2[e] = W.E2[e];
    __syncthreads();
  }
  const unsigned int n = min(W.acc->nhits, W.hit_cap);
  for (unsigned int h0 = blockIdx.x * ENC_T; h0 < n; h0 += gridDim.x * ENC_T) {
    const unsigned int hi = h0 + threadIdx.x;
    if (hi >= n) continue;
    const EncHit h = W.hits[hi];
    int ch, b0 = 0, b1 = 0;
    bool react;
    if (CIS) {
      const int sa = d.slot_of[h.a], sb = d.slot_of[h.b];  // (checked by k_enc_count)
      const double ot = kmce::cis_angle(enc_a(d, sa, 3, 1), enc_a(d, sa, 3, 3), enc_a(d, sb, 3, 1), enc_a(d, sb, 3, 3));
      react = ot < P.cis_theta_cut;
      ch = h.aux;
      if (hist) b0 = kmce::ang_bin(ot, na);
    } else {
      const int b = h.b >> 2, k = 2 + (h.b & 3);
      const int sa = d.slot_of[h.a], lb = d.slot_of[NA + b - 1] - NA;
      double pd, ot;
      kmce::rl_angles(enc_a(d, sa, 3, 1), enc_a(d, sa, 3, 2), enc_a(d, sa, 3, 4), enc_b(d, lb, k, 1), enc_b(d, lb, k, 2),
                      enc_b(d, lb, 1, 1), enc_b(d, lb, 1, 2), &pd, &ot);
      react = pd < P.thetapd_cut && ot < P.thetaot_cut;
      ch = kmce::CH_RL;
      W.rhit[W.rstart[h.a] + h.rank] = h.b << 1 | (react ? 1 : 0);
      W.site_flag[3 * (b - 1) + (k - 2)] = 1;
      if (hist) {
        b0 = kmce::ang_bin(pd, na);
        b1 = kmce::ang_bin(ot, na);
      }
    }
    if (hist) {
      atomicAdd(&tab[ENC_TAB_D + (ch * 2 + (react ? 1 : 0)) * nd + kmce::dist_bin(E2 + ch * ENC_MAX_ND, nd, h.d2)], 1u);
      if (CIS) atomicAdd(&tab[ENC_TAB_ACIS + (ch - kmce::CH_MONO) * na + b0], 1u);
      else atomicAdd(&tab[ENC_TAB_ARL + b0 * na + b1], 1u);
      atomicAdd(&tab[ENC_TAB_N + ch], 1u);
      if (react) atomicAdd(&tab[ENC_TAB_N + 3 + ch], 1u);
    }
  }
  if (hist) {
    __syncthreads();
    for (int e = threadIdx.x; e < ENC_TAB_N + 6; e += ENC_T)
      if (tab[e]) atomicAdd(&W.tab[e], (enc_u64)tab[e]);
  }
}

// the census' R–L summary: one thread a receptor and a ligand site
__global__ void __launch_bounds__(ENC_T) k_enc_census_fin(KParams P, EncW W) {
  const int t = blockIdx.x * ENC_T + threadIdx.x;
  const bool rec = t < P.NA, site = t < 3 * P.NB;
  const int n = rec ? W.rcnt[t] : 0;
  const enc_u64 v[4] = {__ballot(rec && W.pcell[t] >= 0), __ballot(site && W.tcell[t] >= 0), __ballot(n > 0),
                        __ballot(site && W.site_flag[t] != 0)};
  if ((threadIdx.x & 63) == 0)
    for (int k = 0; k < 4; ++k)
      if (v[k]) atomicAdd(&W.tab[ENC_TAB_RL + k], (enc_u64)__popcll(v[k]));
  if (n > 0) atomicMax(&W.acc->max_partners, (unsigned int)n);
}

// receptor i's current look: its link, checked as the kinetics recorder checks
// it (and the site of a bond in 2..4), and its hits cut to the `slots` smallest keys
__device__ __forceinline__ bool enc_cur(const KParams& P, const Dev& d, const EncW& W, int i, int slots,
                                        kmce::Cur& c) {
  int32_t lig, cis, site;
  bool cx;
  bool ok = receptor_bonds(P, d, i, lig, cis, &site, &cx);
  if (ok && lig != 0 && (site < 2 || site > 4)) ok = false;
  kmce::cur_clear(c, ok ? lig : 0, ok && lig != 0 ? site : 0);
  if (!ok) return false;
  const int h0 = W.rstart[i], h1 = W.rstart[i + 1];
  for (int h = h0; h < h1; ++h) {
    const int32_t w = W.rhit[h];
    kmce::cur_add(c, slots, w >> 1, w & 1);
  }
  return true;
}

__device__ __forceinline__ void enc_store(const Enc& E, int i, const kmce::Slots& r) {
  E.lig[i] = r.lig;
  E.site[i] = r.site;
  E.key[i] = make_int4(r.key[0], r.key[1], r.key[2], r.key[3]);
  E.since[i] = make_longlong4(r.since[0], r.since[1], r.since[2], r.since[3]);
  E.nreact[i] = make_int4(r.nreact[0], r.nreact[1], r.nreact[2], r.nreact[3]);
  E.flags[i] = make_uchar4(r.flags[0], r.flags[1], r.flags[2], r.flags[3]);
}
__device__ __forceinline__ void enc_load(const Enc& E, int i, kmce::Slots& r) {
  r.lig = E.lig[i];
  r.site = E.site[i];
  const int4 k = E.key[i], n = E.nreact[i];
  const longlong4 s = E.since[i];
  const uchar4 f = E.flags[i];
  r.key[0] = k.x, r.key[1] = k.y, r.key[2] = k.z, r.key[3] = k.w;
  r.since[0] = s.x, r.since[1] = s.y, r.since[2] = s.z, r.since[3] = s.w;
  r.nreact[0] = n.x, r.nreact[1] = n.y, r.nreact[2] = n.z, r.nreact[3] = n.w;
  r.flags[0] = f.x, r.flags[1] = f.y, r.flags[2] = f.z, r.flags[3] = f.w;
}

// The slot kernel: one thread a receptor, by reference index.  BEGIN: the
// current set becomes the record.  Otherwise the transition at step t; its
// histogram entries go into LDS rows (32-bit: a workgroup files at most 4 x 256
// x 2) flushed with one 64-bit atomic per non-empty bin, the counters through
// LDS with one atomic per workgroup and counter.
template <bool BEGIN>
__global__ void __launch_bounds__(ENC_T) k_enc_slots(KParams P, Dev d, EncW W, Enc E, int slots, long long t,
                                                    enc_u64* hist) {
  __shared__ uint32_t rows[BEGIN ? 1 : ENC_ACC_ROWS * ENC_BINS];
  __shared__ uint32_t cnts[kmce::ENC_NCNT];
  if (!BEGIN)
    for (int e = threadIdx.x; e < ENC_ACC_ROWS * ENC_BINS; e += ENC_T) rows[e] = 0u;
  if (threadIdx.x < kmce::ENC_NCNT) cnts[threadIdx.x] = 0u;
  __syncthreads();
  const int NA = P.NA, NB = P.NB;
  const int i = blockIdx.x * ENC_T + threadIdx.x;
  if (i < NA) {
    kmce::Cur c;
    int32_t cnt[kmce::ENC_NCNT];
    for (int k = 0; k < kmce::ENC_NCNT; ++k) cnt[k] = 0;
    if (!enc_cur(P, d, W, i, slots, c)) {
      atomicOr(&W.acc->err, 1u);  // (the call fails and drops the recorder)
    } else {
      kmce::Slots r;
      if (BEGIN) {
        kmce::begin(t, c, r, cnt);
      } else {
        enc_load(E, i, r);
        bool occ[ENC_SLOTS];
        for (int s = 0; s < ENC_SLOTS; ++s) {
          occ[s] = false;
          const int32_t k = r.key[s];
          if (k == 0) continue;
          const int b = k >> 2;  // (a key of this layer's own making: 1..NB)
          const int slot = d.slot_of[NA + b - 1];
          if (slot >= NA && slot < P.N) occ[s] = B_ST(d, slot - NA, 2 + (k & 3)) != 0;
        }
        kmce::Events ev;
        kmce::transition(t, NA, c, occ, r, ev, cnt);
        for (int k = 0; k < ENC_SLOTS; ++k)
          if (k < ev.n) {
            atomicAdd(&rows[ev.row[k] * ENC_BINS + kmck::bin(ev.val[k])], 1u);
            atomicAdd(&rows[(ENC_ROWS_UPD + ev.rrow[k]) * ENC_BINS + kmck::bin(ev.rval[k])], 1u);
          }
      }
      enc_store(E, i, r);
      for (int k = 0; k < kmce::ENC_NCNT; ++k)
        if (cnt[k]) atomicAdd(&cnts[k], (uint32_t)cnt[k]);
    }
  }
  __syncthreads();
  if (!BEGIN)
    for (int e = threadIdx.x; e < ENC_ACC_ROWS * ENC_BINS; e += ENC_T)
      if (rows[e]) atomicAdd(&hist[e], (enc_u64)rows[e]);
  if (threadIdx.x < kmce::ENC_NCNT && cnts[threadIdx.x]) atomicAdd(&W.acc->cnt[threadIdx.x], (enc_u64)cnts[threadIdx.x]);
}

// row 8: the ages of the open, non-censored slots as of the last update, and
// the censored ones still open.  Reads the recorder only.
__global__ void __launch_bounds__(ENC_T) k_enc_sample(int NA, Enc E, long long t_last, int nblk, enc_u64* row,
                                                     EncAcc* acc) {
  __shared__ uint32_t bins[ENC_BINS];
  __shared__ uint32_t cens;
  const int j = threadIdx.x;
  for (int b = j; b < ENC_BINS; b += ENC_T) bins[b] = 0u;
  if (j == 0) cens = 0u;
  __syncthreads();
  for (int blk = blockIdx.x; blk < nblk; blk += gridDim.x) {
    const int i = blk * ENC_T + j;
    if (i >= NA) continue;
    kmce::Slots r;
    enc_load(E, i, r);
    for (int s = 0; s < ENC_SLOTS; ++s) {
      if (r.key[s] == 0) continue;
      if (r.flags[s] & kmce::F_CENSORED) atomicAdd(&cens, 1u);
      else atomicAdd(&bins[kmck::bin(t_last - r.since[s])], 1u);
    }
  }
  __syncthreads();
  for (int b = j; b < ENC_BINS; b += ENC_T)
    if (bins[b]) atomicAdd(&row[b], (enc_u64)bins[b]);
  if (j == 0 && cens) atomicAdd(&acc->alive, (enc_u64)cens);
}

}  // namespace kmcd
