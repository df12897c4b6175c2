// kmc_proximity.hip — proximity clusters of the committed state (DESIGN.md
// §23): DBSCAN / friends-of-friends over the integer coordinates of §14, the
// neighbour-count and nearest-neighbour histograms, and the purity of the
// clusters against the bond graph's components.  Read-only over the state like
// kmc_bondorder.hip, whose grid (BoArgs, bo_run, the kmcb:: expressions) the
// walks here share; the union-find is kmc_analysis.hip's (an_find / an_unite),
// and the bond components come from its k_an_hook / k_an_flatten into this
// layer's own buffers.  Every result is an integer reached by atomicAdd /
// atomicMin / atomicMax or by a rule that is local to one point: any schedule
// gives the same bits.
//
// Included by kmc_engine.hip after kmc_encounter.hip; the host side of the call
// is kmc_observe.hip §proximity clusters.
#include "kmc_proximity.h"
#include "kmc_device.h"
#include "kmc_observe.h"

namespace kmcd {

#define PX_T BO_T            // threads per workgroup of every kernel here
#define PX_WAVES BO_WAVES
#define PX_WG_MAX BO_WG_MAX  // workgroups of the grid-stride kernels
#define PX_Q 128             // queued core pairs per wave: fewer than 64 left over plus at most 64 new
#define PX_SH_LDS 1024       // size bins privatised in LDS; larger sizes go to the global bins directly
#define PX_NSUM 16           // words of PxOut::sum

// PxOut::sum
enum {
  PX_N_SEL, PX_N_CORE, PX_N_BORDER, PX_N_NOISE, PX_N_ALONE, PX_N_CLUSTERS, PX_N_MULTI, PX_SUM_NN, PX_N_EDGES,
  PX_N_PURE, PX_N_WHOLE, PX_N_BMULTI, PX_N_BKEPT
};

// what the call adds to the grid's BoArgs (which: 0 A, 1 B, 2 both; base, n: the slots [base, base + n))
struct PxArgs {
  int min_pts, max_size, nbins, N;
  float inv_dr;  // 1 / (dr * 1024): guesses the nearest-neighbour bin, the integer edges decide
};

// device-side summary of one call
struct PxOut {
  unsigned long long sum[PX_NSUM];
  unsigned long long best;  // largest cluster: size << 32 | (0xffffffff - root): atomicMax, ties to the smallest label
  uint32_t n_clist, n_blist;  // the compacted cores / non-cores with a neighbour
  uint32_t err;               // 1: a reference index or a find loop left its range
  uint32_t pad;
};

// host side: scratch of the first call, its own.  s = by sorted position, r = by reference index, all [N]
struct PxState {
  int32_t *cell = nullptr, *rank = nullptr;            // by the set's thread: cell and rank of the binning
  CellBins bins;
  longlong2* pts = nullptr;                            // s: integer coordinates
  int32_t *ref = nullptr, *clist = nullptr, *blist = nullptr;  // s: reference index; sorted positions of the two lists
  uint8_t *core_s = nullptr, *kind = nullptr, *mask = nullptr; // s: 1 for a core; r: kind; r: the caller's mask
  int32_t *nn = nullptr, *parent = nullptr, *label = nullptr, *cnt = nullptr;  // r: N_i, union-find, label (root + 1), members
  int64_t* M = nullptr;                                // r: squared nearest-neighbour distance
  int32_t *cparent = nullptr, *clab = nullptr;         // r: the bond graph's union-find and component roots
  int32_t *cmin = nullptr, *cmax = nullptr;            // r (cluster root): range of c over the members
  int32_t *pmin = nullptr, *pmax = nullptr, *bsel = nullptr;  // r (component root): range of the label, selected members
  unsigned long long *size_hist = nullptr, *nn_hist = nullptr, *nnd_hist = nullptr;  // [65536], [64], [4096]
  int64_t* E2 = nullptr;                               // [PX_NND_BINS] squared edges
  PxOut* out = nullptr;
  AnOut* an_out = nullptr;                             // the component kernels' error word
  hipEvent_t ev[3] = {nullptr, nullptr, nullptr};      // after the binning, the count walk, the flatten
  double ms[4] = {0.0, 0.0, 0.0, 0.0};
  int q = PX_Q;  // KMC_DEBUG_PX_QUEUE: the union walk flushes its queue at fewer pairs (the flush path at test size)
};

// slot p of the set's thread t; selected by KMC_SK_BOUND's rule
__device__ __forceinline__ bool px_bound(const KParams& P, const Dev& d, int p) {
  const int NA = P.NA, NB = P.NB;
  if (p < NA) return (A_NEI2(d, p) != 0) | (A_NEI3(d, p) != 0);
  const int b = p - NA;
  return (B_NEI(d, b, 2) != 0) | (B_NEI(d, b, 3) != 0) | (B_NEI(d, b, 4) != 0);
}

// ------------------------------------------------------------ init
// by reference index: both union-finds at themselves, the ranges empty
__global__ void __launch_bounds__(PX_T) k_px_init(int N, int32_t* parent, int32_t* cparent, int32_t* nn, uint8_t* kind,
                                                  int32_t* label, int32_t* cnt, int32_t* cmin, int32_t* cmax,
                                                  int32_t* pmin, int32_t* pmax, int32_t* bsel) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= N) return;
  parent[i] = i;
  cparent[i] = i;
  nn[i] = 0;
  kind[i] = 0;
  label[i] = 0;
  cnt[i] = 0;
  cmin[i] = 0x7fffffff;
  cmax[i] = -1;
  pmin[i] = 0x7fffffff;
  pmax[i] = -1;
  bsel[i] = 0;
}

// ------------------------------------------------------------ select and bin
// cell[t] = the cell of the set's slot a.base + t, -1 when it is not selected; rank[t] within the cell
__global__ void __launch_bounds__(PX_T) k_px_cell_count(KParams P, Dev d, BoArgs a, const uint8_t* __restrict__ mask,
                                                        int32_t* ccnt, int32_t* cell, int32_t* rank, PxOut* out) {
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= a.n) return;
  const int p = a.base + t;  // slot < N
  const int ref = d.id_of[p];
  bool sel = a.select == 0 || px_bound(P, d, p);
  if ((unsigned)ref >= (unsigned)P.N) {
    atomicOr(&out->err, 1u);
    sel = false;
  }
  if (sel && mask) sel = mask[ref] != 0;  // ref < N
  if (!sel) {
    cell[t] = -1;
    return;
  }
  const int c = bo_cell(a, bo_XY(P, d, p));
  cell[t] = c;
  rank[t] = atomicAdd(&ccnt[c], 1);  // c < ncx * ncy
}

__global__ void __launch_bounds__(PX_T) k_px_cell_scatter(KParams P, Dev d, BoArgs a, const int32_t* __restrict__ cstart,
                                                          const int32_t* __restrict__ cell,
                                                          const int32_t* __restrict__ rank, longlong2* pts,
                                                          int32_t* refs) {
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= a.n) return;
  const int c = cell[t];
  if (c < 0) return;
  const int p = a.base + t;
  const int pos = cstart[c] + rank[t];  // < the number of binned points <= n
  pts[pos] = bo_XY(P, d, p);
  refs[pos] = d.id_of[p];  // checked by the count: < N
}

// ------------------------------------------------------------ the walk
// One lane per centre of 64 consecutive sorted points, k_bo_local_queue's walk:
// every pass moves each unfinished lane one candidate on through its six runs
// (bo_run), so the loop ends after at most 6 runs of at most nsel points.
// f(j, D2) sees every candidate j != i of the centre's 3 x 3 cells.
struct PxCentre {
  longlong2 me;
  int cx, cy, r, j, j1;
};

__device__ __forceinline__ PxCentre px_centre(const BoArgs& a, longlong2 me) {
  PxCentre c;
  c.me = me;
  c.cx = kmcb::cell_of(kmcb::wrap(me.x, a.BX), a.ncx, a.BX);
  c.cy = kmcb::cell_of(kmcb::wrap(me.y, a.BY), a.ncy, a.BY);
  c.r = -1;
  c.j = c.j1 = 0;
  return c;
}

// the lane's next candidate: false when the centre has none left; else *jj < nsel and its squared distance
__device__ __forceinline__ bool px_next(const BoArgs& a, const int32_t* __restrict__ cstart,
                                        const longlong2* __restrict__ pts, PxCentre& c, bool live, int* jj,
                                        long long* D2) {
  while (live && c.j == c.j1 && c.r < 5) {
    ++c.r;
    bo_run(a, cstart, c.cx, c.cy, c.r, &c.j, &c.j1);
  }
  if (!(live && c.j < c.j1)) return false;
  const longlong2 q = pts[c.j];  // j < nsel
  *jj = c.j++;
  const long long dx = kmcb::fold(q.x - c.me.x, a.BX), dy = kmcb::fold(q.y - c.me.y, a.BY);
  *D2 = dx * dx + dy * dy;
  return true;
}

// appends the sorted positions of the lanes with `put` to list (one atomic per wave): fewer than nsel entries in all
__device__ __forceinline__ void px_append(bool put, int i, int32_t* list, uint32_t* n) {
  const unsigned long long m = __ballot(put);
  if (m == 0ull) return;
  const int lane = threadIdx.x & 63;
  uint32_t base = 0;
  if (lane == __ffsll((long long)m) - 1) base = atomicAdd(n, (uint32_t)__popcll(m));
  base = __shfl(base, __ffsll((long long)m) - 1);
  if (put) list[base + __popcll(m & ((1ull << lane) - 1ull))] = i;
}

// count walk: N_i and M_i of every binned point; cores and the non-cores with a neighbour are listed
__global__ void __launch_bounds__(PX_T) k_px_count(BoArgs a, PxArgs x, const int32_t* __restrict__ cstart,
                                                   const longlong2* __restrict__ pts, const int32_t* __restrict__ refs,
                                                   int32_t* nn, int64_t* M, uint8_t* kind, uint8_t* core_s,
                                                   int32_t* clist, int32_t* blist, PxOut* out) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int nsel = cstart[a.ncx * a.ncy];  // the binned points (<= n)
  const int nchunk = (nsel + 63) / 64;
  for (int ch = blockIdx.x * PX_WAVES + w; ch < nchunk; ch += gridDim.x * PX_WAVES) {  // the same for the whole wave
    const int i = ch * 64 + lane;
    const bool live = i < nsel;
    PxCentre c = px_centre(a, live ? pts[i] : make_longlong2(0, 0));
    int N = 0;
    long long best = 0x7fffffffffffffffll;
    for (;;) {
      int j;
      long long D2;
      const bool has = px_next(a, cstart, pts, c, live, &j, &D2);
      if (__ballot(has) == 0ull) break;
      if (has && j != i && D2 <= a.RC2) {
        ++N;
        best = D2 < best ? D2 : best;
      }
    }
    bool core = false;
    if (live) {
      const int ref = refs[i];  // < N
      core = kmcx::is_core(N, x.min_pts);
      nn[ref] = N;
      M[ref] = N ? best : 0;
      kind[ref] = core ? 3 : 1;  // a non-core is noise until the border walk finds it a core
      core_s[i] = core ? 1 : 0;
    }
    px_append(live && core, i, clist, &out->n_clist);
    px_append(live && !core && N > 0, i, blist, &out->n_blist);
  }
}

// union walk: only the listed cores walk again.  A lane's hits (a core j within
// eps whose reference index is below the centre's) are compacted into the
// wave's LDS queue, and whenever qcap are queued the lanes unite one pair each:
// the divergent find loops run with every lane busy.  parent[x] <= x always, so
// a chain descends and a find ends within N links; a failed hook means another
// lane hooked that root, which happens fewer than N times (an_unite's bound).
__global__ void __launch_bounds__(PX_T) k_px_union(BoArgs a, PxArgs x, int qcap, const int32_t* __restrict__ cstart,
                                                   const longlong2* __restrict__ pts, const int32_t* __restrict__ refs,
                                                   const uint8_t* __restrict__ core_s,
                                                   const int32_t* __restrict__ clist, int32_t* parent, PxOut* out) {
  __shared__ int qa[PX_WAVES][PX_Q], qb[PX_WAVES][PX_Q];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;  // w < PX_WAVES
  const int ncore = (int)out->n_clist;  // written by the count walk's launch; <= nsel
  const int nchunk = (ncore + 63) / 64;
  unsigned long long edges = 0ull;
  for (int ch = blockIdx.x * PX_WAVES + w; ch < nchunk; ch += gridDim.x * PX_WAVES) {
    const int t = ch * 64 + lane;
    const bool live = t < ncore;
    const int i = live ? clist[t] : 0;  // sorted position < nsel
    const int myref = live ? refs[i] : 0;
    PxCentre c = px_centre(a, live ? pts[i] : make_longlong2(0, 0));
    int qn = 0;  // queued pairs: the same in every lane
    for (;;) {
      int j = 0;
      long long D2;
      const bool has = px_next(a, cstart, pts, c, live, &j, &D2);
      if (__ballot(has) == 0ull) break;
      int rj = 0;
      bool hit = has && j != i && D2 <= a.RC2 && core_s[j] != 0;
      if (hit) {
        rj = refs[j];  // < N
        hit = rj < myref;
      }
      const unsigned long long hm = __ballot(hit);
      if (hit) {
        const int pos = qn + __popcll(hm & ((1ull << lane) - 1ull));  // qn <= 63 and at most 63 lanes below: < PX_Q
        qa[w][pos] = myref;
        qb[w][pos] = rj;
        ++edges;
      }
      qn += __popcll(hm);
      if (qn >= qcap) {  // qcap <= 64
        bo_wave_sync();
        const int n = min(qn, 64);
        if (lane < n) an_unite(parent, qa[w][qn - n + lane], qb[w][qn - n + lane], x.N, &out->err);
        qn -= n;
        bo_wave_sync();  // read before the next hits overwrite the tail
      }
    }
    bo_wave_sync();
    if (lane < qn) an_unite(parent, qa[w][lane], qb[w][lane], x.N, &out->err);  // the rest: qn <= 63
    bo_wave_sync();
  }
  for (int o = 32; o > 0; o >>= 1) edges += __shfl_down(edges, o);
  if (lane == 0 && edges) atomicAdd(&out->sum[PX_N_EDGES], edges);
}

// after the unions every root is final: a core's label is its root + 1 (the smallest reference index of its cluster)
__global__ void __launch_bounds__(PX_T) k_px_flatten(int N, const uint8_t* __restrict__ kind,
                                                     const int32_t* __restrict__ parent, int32_t* label, PxOut* out) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= N || kind[i] != 3) return;
  int xx = i;
  for (int it = 0; it <= N; ++it) {
    const int p = parent[xx];
    if (p == xx) {
      label[i] = xx + 1;
      return;
    }
    xx = p;
  }
  atomicOr(&out->err, 1u);
}

// border walk: a listed non-core takes the label of its nearest core (smallest
// D2, then smallest reference index) — its own side's decision, no atomics
__global__ void __launch_bounds__(PX_T) k_px_border(BoArgs a, const int32_t* __restrict__ cstart,
                                                    const longlong2* __restrict__ pts, const int32_t* __restrict__ refs,
                                                    const uint8_t* __restrict__ core_s,
                                                    const int32_t* __restrict__ blist, uint8_t* kind, int32_t* label,
                                                    PxOut* out) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int nb = (int)out->n_blist;  // <= nsel
  const int nchunk = (nb + 63) / 64;
  for (int ch = blockIdx.x * PX_WAVES + w; ch < nchunk; ch += gridDim.x * PX_WAVES) {
    const int t = ch * 64 + lane;
    const bool live = t < nb;
    const int i = live ? blist[t] : 0;  // sorted position < nsel
    PxCentre c = px_centre(a, live ? pts[i] : make_longlong2(0, 0));
    long long bestD = 0;
    int bestR = -1;
    for (;;) {
      int j = 0;
      long long D2;
      const bool has = px_next(a, cstart, pts, c, live, &j, &D2);
      if (__ballot(has) == 0ull) break;
      if (has && j != i && D2 <= a.RC2 && core_s[j] != 0) {
        const int rj = refs[j];  // < N
        if (kmcx::nearer(D2, rj, bestD, bestR)) {
          bestD = D2;
          bestR = rj;
        }
      }
    }
    if (live && bestR >= 0) {
      const int ref = refs[i];
      kind[ref] = 2;
      label[ref] = label[bestR];  // a core's label: written by the flatten launch, not here
    }
  }
}

// ------------------------------------------------------------ reduce
// by reference index, every selected point: the counts, the two per-point
// histograms (privatised in LDS), the members of its cluster, and the ranges
// that purity is read from
__global__ void __launch_bounds__(PX_T) k_px_points(PxArgs x, const uint8_t* __restrict__ kind,
                                                    const int32_t* __restrict__ nn, const int64_t* __restrict__ M,
                                                    const int32_t* __restrict__ label, const int32_t* __restrict__ clab,
                                                    const int64_t* __restrict__ E2, int32_t* cnt, int32_t* cmin,
                                                    int32_t* cmax, int32_t* pmin, int32_t* pmax, int32_t* bsel,
                                                    unsigned long long* nn_hist, unsigned long long* nnd_hist,
                                                    PxOut* out) {
  extern __shared__ __attribute__((aligned(16))) unsigned long long px_lds[];  // [PX_NSUM] sums, [PX_NN_ROWS], [nbins]
  const int nl = PX_NSUM + PX_NN_ROWS + x.nbins;
  for (int b = threadIdx.x; b < nl; b += PX_T) px_lds[b] = 0ull;
  __syncthreads();
  for (int i = blockIdx.x * PX_T + threadIdx.x; i < x.N; i += gridDim.x * PX_T) {
    const int k = kind[i];
    if (k == 0) continue;
    const int N = nn[i], L = label[i], c = clab[i];  // c < N: a root of the bond graph
    atomicAdd(&px_lds[PX_N_SEL], 1ull);
    atomicAdd(&px_lds[k == 3 ? PX_N_CORE : k == 2 ? PX_N_BORDER : PX_N_NOISE], 1ull);
    atomicAdd(&px_lds[PX_SUM_NN], (unsigned long long)N);
    atomicAdd(&px_lds[PX_NSUM + min(N, PX_NN_ROWS - 1)], 1ull);
    if (N == 0) {
      atomicAdd(&px_lds[PX_N_ALONE], 1ull);
    } else {
      const int64_t m = M[i];
      // nnd_bin < nbins
      atomicAdd(&px_lds[PX_NSUM + PX_NN_ROWS + kmcx::nnd_bin(E2, x.nbins, m, (int)(__fsqrt_rn((float)m) * x.inv_dr))],
                1ull);
    }
    atomicAdd(&bsel[c], 1);
    atomicMin(&pmin[c], L);
    atomicMax(&pmax[c], L);
    if (L > 0) {  // L - 1 < N: a cluster's root
      atomicAdd(&cnt[L - 1], 1);
      atomicMin(&cmin[L - 1], c);
      atomicMax(&cmax[L - 1], c);
    }
  }
  __syncthreads();
  for (int b = threadIdx.x; b < nl; b += PX_T) {
    if (!px_lds[b]) continue;
    if (b < PX_NSUM) atomicAdd(&out->sum[b], px_lds[b]);
    else if (b < PX_NSUM + PX_NN_ROWS) atomicAdd(&nn_hist[b - PX_NSUM], px_lds[b]);
    else atomicAdd(&nnd_hist[b - PX_NSUM - PX_NN_ROWS], px_lds[b]);  // < nbins
  }
}

// by reference index, every root: a cluster's size bin, the largest cluster and
// its purity; a bond component's selected members and whether one cluster keeps them
__global__ void __launch_bounds__(PX_T) k_px_roots(PxArgs x, const uint8_t* __restrict__ kind,
                                                   const int32_t* __restrict__ label, const int32_t* __restrict__ cnt,
                                                   const int32_t* __restrict__ cmin, const int32_t* __restrict__ cmax,
                                                   const int32_t* __restrict__ pmin, const int32_t* __restrict__ pmax,
                                                   const int32_t* __restrict__ bsel, unsigned long long* size_hist,
                                                   PxOut* out) {
  __shared__ unsigned long long sums[PX_NSUM], bins[PX_SH_LDS], best;
  for (int b = threadIdx.x; b < PX_SH_LDS; b += PX_T) bins[b] = 0ull;
  if (threadIdx.x < PX_NSUM) sums[threadIdx.x] = 0ull;
  if (threadIdx.x == 0) best = 0ull;
  __syncthreads();
  for (int i = blockIdx.x * PX_T + threadIdx.x; i < x.N; i += gridDim.x * PX_T) {
    if (kind[i] == 3 && label[i] == i + 1) {
      const int size = cnt[i];  // >= 1: the root itself
      const int bin = min(size, x.max_size);
      if (bin < PX_SH_LDS) atomicAdd(&bins[bin], 1ull);
      else atomicAdd(&size_hist[bin], 1ull);  // bin <= max_size <= 65535
      atomicAdd(&sums[PX_N_CLUSTERS], 1ull);
      atomicMax(&best, ((unsigned long long)size << 32) | (0xffffffffu - (uint32_t)i));
      if (size >= 2) {
        atomicAdd(&sums[PX_N_MULTI], 1ull);
        const int c = cmin[i];
        if (c == cmax[i]) {  // c < N: every member named it
          atomicAdd(&sums[PX_N_PURE], 1ull);
          if (bsel[c] == size) atomicAdd(&sums[PX_N_WHOLE], 1ull);
        }
      }
    }
    if (bsel[i] >= 2) {
      atomicAdd(&sums[PX_N_BMULTI], 1ull);
      if (pmin[i] == pmax[i] && pmin[i] > 0) atomicAdd(&sums[PX_N_BKEPT], 1ull);
    }
  }
  __syncthreads();
  for (int b = threadIdx.x; b < PX_SH_LDS; b += PX_T)
    if (bins[b] && b <= x.max_size) atomicAdd(&size_hist[b], bins[b]);
  if (threadIdx.x < PX_NSUM && sums[threadIdx.x]) atomicAdd(&out->sum[threadIdx.x], sums[threadIdx.x]);
  if (threadIdx.x == 0 && best) atomicMax(&out->best, best);
}

}  // namespace kmcd
