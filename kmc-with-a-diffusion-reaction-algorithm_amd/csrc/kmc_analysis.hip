// kmc_analysis.hip — read-only structure analysis of the committed state
// (DESIGN.md §10): connected components of the bond graph with the oligomer
// census, and lateral pair counts for g(r).  Nothing here runs inside a step or
// reads a step-internal table: the kernels see what kmc_get_state would return
// — the current beads (Dev::cur) and a_int / b_int, whose links are slot + 1 —
// and name proteins by their reference index through id_of.
//
// Included by kmc_engine.hip after kmc_kernels.hip (one translation unit, the
// library's flags: -ffp-contract=off keeps d2 below two roundings per product
// and sum, as the host reference computes it); the host side of the calls is
// kmc_observe.hip §analysis.
#include "kmc_device.h"
#include "kmc_observe.h"

namespace kmcd {

// ------------------------------------------------------------ bond links
// The readers of the committed state's protein links every later layer shares
// (here, not in kmc_device.h: Dev and its accessors are kmc_kernels.hip's).
// The <= 3 links of slot p as they are stored (slot + 1, 0: none): a receptor's
// nei2 and nei3 (l[2] = 0), a ligand's nei2..4.  Nothing is checked: every
// caller has a range policy of its own.
__device__ __forceinline__ void prot_links(const KParams& P, const Dev& d, int p, int32_t l[3]) {
  const int NA = P.NA, NB = P.NB;
  if (p < NA) {
    l[0] = A_NEI2(d, p);
    l[1] = A_NEI3(d, p);
    l[2] = 0;
  } else {
    for (int j = 2; j <= 4; ++j) l[j - 2] = B_NEI(d, p - NA, j);
  }
}

// The bonds of receptor i (0-based reference index) as reference indices + 1
// (0: none): its slot through slot_of, nei2 and nei3 there, range-checked, then
// translated through id_of and checked again.  With `site` / `cx` (the kinetics
// recorder's) nei4 is read and range-checked with the other two, and whether the
// cis pair is part of a complex is read at the partner's slot.  False when a
// slot or a link leaves its range: nothing is read through it then.
__device__ __forceinline__ bool receptor_bonds(const KParams& P, const Dev& d, int i, int32_t& lig, int32_t& cis,
                                               int32_t* site = nullptr, bool* cx = nullptr) {
  const int NA = P.NA, N = P.N;
  lig = cis = 0;
  const int slot = d.slot_of[i];
  if ((unsigned)slot >= (unsigned)NA) return false;
  const int32_t v2 = A_NEI2(d, slot), v4 = site ? A_NEI4(d, slot) : 0, v3 = A_NEI3(d, slot);
  if (v2 != 0 && (v2 <= NA || v2 > N)) return false;
  if (v3 != 0 && (v3 < 1 || v3 > NA)) return false;
  if (v4 < 0 || v4 > 4) return false;
  bool ok = true;
  if (site) *site = v4;
  if (v2 != 0) {
    lig = d.id_of[v2 - 1] + 1;
    ok = lig > NA && lig <= N;
  }
  if (v3 != 0) {
    cis = d.id_of[v3 - 1] + 1;
    if (cx) *cx = v2 != 0 || A_NEI2(d, v3 - 1) != 0;  // the partner's nei2 at the partner's slot
    ok = ok && cis >= 1 && cis <= NA && cis != i + 1;
  }
  return ok;
}

// device-side results of one analysis call
struct AnOut {
  unsigned long long n_components, n_complexes, proteins_in_complexes, n_cis_dimers;
  unsigned long long best;  // largest component: size << 32 | (0xffffffff − root): atomicMax → ties to the smallest label
  uint32_t err;             // 1: a find loop ran out of its bound or a link left [1, N]
  uint32_t pad;
};

#define AN_T 256           // threads per workgroup of every analysis kernel
#define AN_WG_MAX 2048     // workgroups of the grid-stride kernels (8 per CU)
#define AN_HIST_MAX 4096   // census bins / pair bins held in LDS
#define AN_CHUNK 512       // points per staged chunk of the pair kernel (KMC_DEBUG_PAIR_CHUNK lowers it)
#define AN_NC_MAX 2048     // cells per axis of the pair binning (wider cells stay correct)

// host side: scratch of the first analysis call, none before it
struct AnState {
  int32_t *parent = nullptr, *label = nullptr;
  unsigned long long *cnt = nullptr, *hist = nullptr;  // [N] packed member counts by root; [AN_HIST_MAX] bins
  AnOut* out = nullptr;
  int32_t *cell = nullptr, *rank = nullptr;  // [N] pair binning: cell and rank of each point
  CellBins bins;
  double2* pts = nullptr;   // [N] (x, y) sorted by cell
  double* edges = nullptr;  // [AN_HIST_MAX + 1] squared bin edges
  int chunk = AN_CHUNK;     // KMC_DEBUG_PAIR_CHUNK: smaller staged chunks (the chunked path at test size)
};

__device__ __forceinline__ int32_t an_ld(const int32_t* p) {
  return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ void an_st(int32_t* p, int32_t v) {
  __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// ------------------------------------------------------------ components
// Lock-free union-find over reference indices.  parent[x] <= x always (a root
// is hooked under a smaller root only), so every chain descends, ends within
// N links, and a tree's root is its smallest member: the component's label.

__global__ void __launch_bounds__(AN_T) k_an_init(int32_t* parent, unsigned long long* cnt, int N) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= N) return;
  parent[i] = i;
  cnt[i] = 0ull;
}

// root of x, halving the path on the way (a non-root never becomes a root
// again and only ever points at an ancestor, so the racing stores are benign)
__device__ __forceinline__ int an_find(int32_t* parent, int x, int N, uint32_t* err) {
  for (int it = 0; it <= N; ++it) {
    const int p = an_ld(&parent[x]);
    if (p == x) return x;
    const int g = an_ld(&parent[p]);
    if (g != p) an_st(&parent[x], g);
    x = g;
  }
  atomicOr(err, 1u);
  return -1;
}

__device__ __forceinline__ void an_unite(int32_t* parent, int a, int b, int N, uint32_t* err) {
  for (int it = 0; it <= N; ++it) {
    a = an_find(parent, a, N, err);
    b = an_find(parent, b, N, err);
    if (a < 0 || b < 0 || a == b) return;
    const int hi = a > b ? a : b, lo = a > b ? b : a;
    if (atomicCAS(&parent[hi], hi, lo) == hi) return;  // else: hi was hooked meanwhile, find again
  }
  atomicOr(err, 1u);
}

// one vertex (slot p) per thread: unite with its <= 3 neighbours
__global__ void __launch_bounds__(AN_T) k_an_hook(KParams P, Dev d, int32_t* parent, AnOut* out) {
  const int p = blockIdx.x * blockDim.x + threadIdx.x;
  const int N = P.N;
  if (p >= N) return;
  int32_t nb[3];
  prot_links(P, d, p, nb);
  const int me = d.id_of[p];
  for (int e = 0, n = p < P.NA ? 2 : 3; e < n; ++e) {
    if (nb[e] == 0) continue;
    if (nb[e] < 1 || nb[e] > N) {
      atomicOr(&out->err, 1u);
      continue;
    }
    an_unite(parent, me, d.id_of[nb[e] - 1], N, &out->err);
  }
}

// after the hooks every root is final: label[i] = its root, and the root's
// packed member counts (receptors low word, ligands high word)
__global__ void __launch_bounds__(AN_T) k_an_flatten(int32_t* parent, int32_t* label, int N, AnOut* out) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= N) return;
  int x = i;
  for (int it = 0; it <= N; ++it) {
    const int p = parent[x];
    if (p == x) {
      label[i] = x;
      return;
    }
    x = p;
  }
  label[i] = i;
  atomicOr(&out->err, 1u);
}

__global__ void __launch_bounds__(AN_T) k_an_count(const int32_t* __restrict__ label, unsigned long long* cnt, int NA,
                                                   int N) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= N) return;
  atomicAdd(&cnt[label[i]], i < NA ? 1ull : 1ull << 32);
}

// the roots' (receptors, ligands) histogram, clamped into the last row /
// column, and the summary.  Bins and sums are privatised in LDS; a workgroup
// flushes each non-empty bin with one 64-bit global atomic.
__global__ void __launch_bounds__(AN_T) k_an_census(const int32_t* __restrict__ label,
                                                    const unsigned long long* __restrict__ cnt, int N, int max_r,
                                                    int max_l, unsigned long long* hist, AnOut* out) {
  extern __shared__ __attribute__((aligned(16))) unsigned long long an_lds[];  // [nbin] bins, then 4 sums and the maximum
  const int nbin = hist ? (max_r + 1) * (max_l + 1) : 0;
  unsigned long long* sum = an_lds + nbin;
  for (int b = threadIdx.x; b < nbin + 5; b += AN_T) an_lds[b] = 0ull;
  __syncthreads();
  for (int i = blockIdx.x * AN_T + threadIdx.x; i < N; i += gridDim.x * AN_T) {
    if (label[i] != i) continue;
    const unsigned long long c = cnt[i];
    const int nr = (int)(uint32_t)c, nl = (int)(c >> 32), size = nr + nl;
    if (hist) atomicAdd(&an_lds[(size_t)min(nr, max_r) * (max_l + 1) + min(nl, max_l)], 1ull);
    atomicAdd(&sum[0], 1ull);
    if (nl >= 1 && size > 1) {
      atomicAdd(&sum[1], 1ull);
      atomicAdd(&sum[2], (unsigned long long)size);
    }
    if (nl == 0 && nr == 2) atomicAdd(&sum[3], 1ull);
    atomicMax(&sum[4], (unsigned long long)size << 32 | (0xffffffffu - (uint32_t)i));
  }
  __syncthreads();
  for (int b = threadIdx.x; b < nbin; b += AN_T)
    if (an_lds[b]) atomicAdd(&hist[b], an_lds[b]);
  if (threadIdx.x == 0) {
    if (sum[0]) atomicAdd(&out->n_components, sum[0]);
    if (sum[1]) atomicAdd(&out->n_complexes, sum[1]);
    if (sum[2]) atomicAdd(&out->proteins_in_complexes, sum[2]);
    if (sum[3]) atomicAdd(&out->n_cis_dimers, sum[3]);
    if (sum[4]) atomicMax(&out->best, sum[4]);
  }
}

// ------------------------------------------------------------ pair counts
// The analysis' own periodic binning: ncx × ncy cells of width box / nc >=
// r_max, per species set (set 0 = the i side, set 1 = the j side of AB).
struct AnGrid {
  int ncx, ncy;
  double box_x, box_y;
  int lo[2], hi[2];  // slot range [lo, hi) of each set
  int nsets;
};

__device__ __forceinline__ int an_cell(const AnGrid& G, double2 xy) {
  // members of a complex can lie slightly outside the box: reduce first
  const double x = xy.x - G.box_x * kmcm::round_(xy.x / G.box_x);
  const double y = xy.y - G.box_y * kmcm::round_(xy.y / G.box_y);
  int cx = (int)__builtin_floor((x + 0.5 * G.box_x) / (G.box_x / G.ncx));
  int cy = (int)__builtin_floor((y + 0.5 * G.box_y) / (G.box_y / G.ncy));
  cx = min(max(cx, 0), G.ncx - 1);
  cy = min(max(cy, 0), G.ncy - 1);
  return cy * G.ncx + cx;
}

__device__ __forceinline__ double2 an_xy(const KParams& P, const Dev& d, int p) {
  return p < P.NA ? d.cur.Axy(p, 1, 1) : d.cur.Bxy(p - P.NA, 1, 1);
}

// count: rank[t] = the point's position within its cell, cell[t] = set·ncell + cell
__global__ void __launch_bounds__(AN_T) k_an_cell_count(KParams P, Dev d, AnGrid G, int32_t* ccnt, int32_t* cell,
                                                        int32_t* rank) {
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  const int n0 = G.hi[0] - G.lo[0], n1 = G.nsets > 1 ? G.hi[1] - G.lo[1] : 0;
  if (t >= n0 + n1) return;
  const int set = t >= n0, p = set ? G.lo[1] + (t - n0) : G.lo[0] + t;
  const int c = set * G.ncx * G.ncy + an_cell(G, an_xy(P, d, p));
  cell[t] = c;
  rank[t] = atomicAdd(&ccnt[c], 1);
}

__global__ void __launch_bounds__(AN_T) k_an_cell_scatter(KParams P, Dev d, AnGrid G, const int32_t* __restrict__ cstart,
                                                          const int32_t* __restrict__ cell,
                                                          const int32_t* __restrict__ rank, double2* pts) {
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  const int n0 = G.hi[0] - G.lo[0], n1 = G.nsets > 1 ? G.hi[1] - G.lo[1] : 0;
  if (t >= n0 + n1) return;
  const int p = t >= n0 ? G.lo[1] + (t - n0) : G.lo[0] + t;
  pts[cstart[cell[t]] + rank[t]] = an_xy(P, d, p);
}

// Workgroups stride over the cells.  For cell c the i points are its set-0
// points; the j points are those of set 0 in c itself (pairs i < j) and its
// four forward neighbours (same species: the half shell), or of set 1 in all
// nine cells (AB).  Both sides are staged in LDS in chunks of `chunk` points,
// so any cell population is handled; each lane then takes pairs of the
// staged block.  The distance and the bin follow kmc.h to the letter.
__global__ void __launch_bounds__(AN_T) k_an_pairs(AnGrid G, const int32_t* __restrict__ cstart,
                                                   const double2* __restrict__ pts,
                                                   const double* __restrict__ edges2, int nbins, float inv_dr,
                                                   int chunk, unsigned long long* counts) {
  extern __shared__ __attribute__((aligned(16))) unsigned long long an_lds[];  // 2 × chunk staged points (16-byte elements first), then [nbins] bins
  double2* si = reinterpret_cast<double2*>(an_lds);
  double2* sj = si + chunk;
  unsigned long long* bins = an_lds + 4 * (size_t)chunk;
  const int ncell = G.ncx * G.ncy, same = G.nsets == 1;
  const double r2max = edges2[nbins];
  for (int b = threadIdx.x; b < nbins; b += AN_T) bins[b] = 0ull;
  for (int c = blockIdx.x; c < ncell; c += gridDim.x) {
    const int i0 = cstart[c], i1 = cstart[c + 1];
    if (i0 == i1) continue;
    const int cx = c % G.ncx, cy = c / G.ncx;
    const int nnb = same ? 5 : 9;
    for (int q = 0; q < nnb; ++q) {
      // same species: self, (+1,0), (−1,+1), (0,+1), (+1,+1); AB: the 3 × 3 block
      int ox, oy;
      if (same) {
        ox = q == 0 ? 0 : q == 1 ? 1 : q - 3;
        oy = q < 2 ? 0 : 1;
      } else {
        ox = q % 3 - 1;
        oy = q / 3 - 1;
      }
      const int jc = ((cy + oy + G.ncy) % G.ncy) * G.ncx + (cx + ox + G.ncx) % G.ncx;
      const int j0 = cstart[(same ? 0 : ncell) + jc], j1 = cstart[(same ? 0 : ncell) + jc + 1];
      if (j0 == j1) continue;
      const bool self = same && q == 0;
      for (int ib = i0; ib < i1; ib += chunk) {
        const int ni = min(chunk, i1 - ib);
        for (int jb = self ? ib : j0; jb < j1; jb += chunk) {  // self: chunks before ib hold only j < i
          const int nj = min(chunk, j1 - jb);
          __syncthreads();  // the previous block's reads are done
          for (int t = threadIdx.x; t < ni; t += AN_T) si[t] = pts[ib + t];
          for (int t = threadIdx.x; t < nj; t += AN_T) sj[t] = pts[jb + t];
          __syncthreads();
          for (int e = threadIdx.x; e < ni * nj; e += AN_T) {
            const int a = e / nj, bq = e - a * nj;
            if (self && ib + a >= jb + bq) continue;
            double dx = si[a].x - sj[bq].x;
            dx = dx - G.box_x * kmcm::round_(dx / G.box_x);
            double dy = si[a].y - sj[bq].y;
            dy = dy - G.box_y * kmcm::round_(dy / G.box_y);
            const double d2 = dx * dx + dy * dy;
            if (!(d2 < r2max)) continue;
            // k = #{m in 1..nbins : edges2[m] <= d2}: a float guess, corrected against the table
            int k = min(max((int)(__fsqrt_rn((float)d2) * inv_dr), 0), nbins - 1);
            while (k < nbins && edges2[k + 1] <= d2) ++k;
            while (k > 0 && edges2[k] > d2) --k;
            if (k < nbins) atomicAdd(&bins[k], 1ull);
          }
        }
      }
    }
  }
  __syncthreads();
  for (int b = threadIdx.x; b < nbins; b += AN_T)
    if (bins[b]) atomicAdd(&counts[b], bins[b]);
}

}  // namespace kmcd
