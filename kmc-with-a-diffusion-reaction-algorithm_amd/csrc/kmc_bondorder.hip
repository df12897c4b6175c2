// kmc_bondorder.hip — bond-orientational order of the committed state
// (DESIGN.md §14): per selected protein of one species the exact int64 sums of
// its neighbours' fixed-point (cos, sin) of n theta, their histogram and global
// sums, and the pair correlation of the normalised values.  Like
// kmc_analysis.hip the kernels are read-only over the state (Dev::cur, a_int /
// b_int, whose links are slot + 1) and name proteins by their reference index
// through id_of.  Every sum is an integer: any schedule gives the same bits.
//
// Included by kmc_engine.hip after kmc_structure.hip (one translation unit, the
// library's flags: -ffp-contract=off, so a term is what include/kmc.h writes
// down and nothing else); the host side of the calls is kmc_observe.hip
// §bond-orientational order.
#include "kmc_bondorder.h"
#include "kmc_device.h"
#include "kmc_observe.h"

namespace kmcd {

#define BO_T 256        // threads per workgroup of every kernel here
#define BO_WAVES (BO_T / 64)
#define BO_WG_MAX 2048  // workgroups of the grid-stride kernels (8 per CU)
#define BO_Q 128        // queued hits per wave: fewer than 64 left over plus at most 64 new
#define BO_CHUNK 256    // points per staged chunk of the correlation (KMC_DEBUG_BO_CHUNK lowers it)

struct BoArgs {
  int which, mode, fold, select;
  int base, n;       // the species' slots [base, base + n); its reference indices are base + [0, n) too
  int ncx, ncy;      // cells of the grid in use (the cutoff's, then the correlation's)
  long long BX, BY;  // the box in integer coordinates, 1 <= BX, BY < 2^31
  long long RC2;     // squared cutoff (KMC_BO_WITHIN)
};

// device-side summary of one call
struct BoOut {
  unsigned long long sum[6];  // n_sel, n_with, sum_nn, sum_pc, sum_ps, sum_m
  uint32_t err;               // 1: a link or an index left its range; 2: more than BO_NN_MAX neighbours
  uint32_t pad;
};

// host side: scratch of the first bond order call, its own
struct BoState {
  int32_t *cell = nullptr, *rank = nullptr, *ref = nullptr, *nn = nullptr;  // [max(NA, NB)]
  CellBins bins;
  longlong2* pts = nullptr;                            // [max(NA, NB)] integer coordinates sorted by cell
  int2 *pcs = nullptr, *pcs_sorted = nullptr;          // (pc, ps) by reference index / sorted by cell
  unsigned long long *C = nullptr, *S = nullptr;       // [max(NA, NB)] sums by reference index
  unsigned long long *hist = nullptr, *corr = nullptr; // [BO_NN_ROWS][BO_HIST_BINS]; [2][BO_CORR_BINS]
  int64_t* E2 = nullptr;                               // [BO_CORR_BINS + 1] squared integer bin edges
  BoOut* out = nullptr;
  int chunk = BO_CHUNK;  // KMC_DEBUG_BO_CHUNK: smaller staged chunks of the correlation (the chunked path at test size)
};

// orders the wave's own LDS traffic (its lanes run in lockstep; nothing here is shared between waves)
__device__ __forceinline__ void bo_wave_sync() {
  __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");
  __builtin_amdgcn_wave_barrier();
}

// i = index within the species by slot (< a.n)
__device__ __forceinline__ bool bo_selected(const KParams& P, const Dev& d, const BoArgs& a, int i) {
  const int NA = P.NA, NB = P.NB;
  if (a.select == 0) return true;
  if (a.which == 0) return (A_NEI2(d, i) != 0) | (A_NEI3(d, i) != 0);
  return (B_NEI(d, i, 2) != 0) | (B_NEI(d, i, 3) != 0) | (B_NEI(d, i, 4) != 0);
}

__device__ __forceinline__ longlong2 bo_XY(const KParams& P, const Dev& d, int p) {
  const double2 xy = p < P.NA ? d.cur.Axy(p, 1, 1) : d.cur.Bxy(p - P.NA, 1, 1);  // slot p < N
  return make_longlong2((long long)kmcm::round_(xy.x * 1024.0), (long long)kmcm::round_(xy.y * 1024.0));
}

__device__ __forceinline__ int bo_cell(const BoArgs& a, longlong2 q) {
  // cell_of < nc on either axis: the index is below ncx * ncy
  return kmcb::cell_of(kmcb::wrap(q.y, a.BY), a.ncy, a.BY) * a.ncx + kmcb::cell_of(kmcb::wrap(q.x, a.BX), a.ncx, a.BX);
}

// ------------------------------------------------------------ the grid
// count: cell[t] = the cell of the species' slot t, -1 when it is not binned
// (not selected, or — for the correlation's grid — without neighbours);
// rank[t] = its position within the cell
__global__ void __launch_bounds__(BO_T) k_bo_cell_count(KParams P, Dev d, BoArgs a, const int32_t* __restrict__ nn_filter,
                                                        int32_t* ccnt, int32_t* cell, int32_t* rank, BoOut* out) {
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= a.n) return;
  const int p = a.base + t;           // slot < N
  const int ref = d.id_of[p] - a.base;  // the re-sort keeps a species' slots and reference indices in one range
  bool sel = bo_selected(P, d, a, t);
  if ((unsigned)ref >= (unsigned)a.n) {
    atomicOr(&out->err, 1u);
    sel = false;
  }
  if (sel && nn_filter) sel = nn_filter[ref] > 0;  // ref < n
  if (!sel) {
    cell[t] = -1;
    return;
  }
  const int c = bo_cell(a, bo_XY(P, d, p));
  cell[t] = c;
  rank[t] = atomicAdd(&ccnt[c], 1);  // c < ncx * ncy
}

// scatter: (X, Y) and the reference index by cell; the correlation's grid also carries (pc, ps)
__global__ void __launch_bounds__(BO_T) k_bo_cell_scatter(KParams P, Dev d, BoArgs a, const int32_t* __restrict__ cstart,
                                                          const int32_t* __restrict__ cell,
                                                          const int32_t* __restrict__ rank, longlong2* pts,
                                                          int32_t* refs, const int2* __restrict__ pcs_in, int2* pcs_out) {
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= a.n) return;
  const int c = cell[t];
  if (c < 0) return;
  const int p = a.base + t, ref = d.id_of[p] - a.base;  // checked by the count: ref < n
  const int pos = cstart[c] + rank[t];                  // < the number of binned points <= n
  pts[pos] = bo_XY(P, d, p);
  refs[pos] = ref;
  if (pcs_in) pcs_out[pos] = pcs_in[ref];
}

// ------------------------------------------------------------ the local pass, KMC_BO_WITHIN
// The candidates of a centre in cell (cx, cy) are the 3 x 3 cells around it.
// In the row-major grid a row's three cells are one contiguous run of the
// sorted points, or two where the row wraps: run r = 2 * row + part, row 0..2
// for cy - 1 .. cy + 1, part 0 the cells max(cx - 1, 0) .. min(cx + 1, ncx - 1),
// part 1 the wrapped cell (empty away from the edge).  ncx, ncy >= 3: no cell
// comes twice.
__device__ __forceinline__ void bo_run(const BoArgs& a, const int32_t* __restrict__ cstart, int cx, int cy, int r,
                                       int* j0, int* j1) {
  const int ry = (cy + (r >> 1) - 1 + a.ncy) % a.ncy;  // < ncy
  int c0, c1;
  if ((r & 1) == 0) {
    c0 = max(cx - 1, 0);
    c1 = min(cx + 1, a.ncx - 1);
  } else if (cx == 0) {
    c0 = c1 = a.ncx - 1;
  } else if (cx == a.ncx - 1) {
    c0 = c1 = 0;
  } else {
    *j0 = *j1 = 0;
    return;
  }
  *j0 = cstart[ry * a.ncx + c0];      // cell index < ncx * ncy
  *j1 = cstart[ry * a.ncx + c1 + 1];  // <= ncx * ncy: cstart has one entry more than cells
}

// A wave owns 64 consecutive centres of the sorted order (one lane per centre
// evaluating its own hits on the spot measured 1.25-1.4x slower: DESIGN.md §14).  Each
// lane walks its own centre's candidates through the integer filter; the hits
// are compacted into the wave's LDS queue (ballot + prefix count) and, whenever
// 64 are queued, all 64 lanes evaluate one term each and add it to the
// centre's LDS accumulators.  One flush per centre; nothing crosses waves.
__global__ void __launch_bounds__(BO_T) k_bo_local_queue(BoArgs a, const int32_t* __restrict__ cstart,
                                                         const longlong2* __restrict__ pts,
                                                         const int32_t* __restrict__ refs, unsigned long long* C,
                                                         unsigned long long* S, int32_t* nn) {
  __shared__ unsigned long long accC[BO_T], accS[BO_T];
  __shared__ int qdx[BO_WAVES][BO_Q], qdy[BO_WAVES][BO_Q];  // |DX|, |DY| < 2^30
  __shared__ unsigned char qwho[BO_WAVES][BO_Q];            // the centre's lane
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, wbase = w * 64;  // w < BO_WAVES
  const int nsel = cstart[a.ncx * a.ncy];  // the binned points (<= n)
  const int nchunk = (nsel + 63) / 64;
  // one queued term by this lane: entry e < BO_Q, its centre's accumulators at wbase + qwho < BO_T
  auto eval = [&](int e) {
    int64_t tc, ts;
    kmcb::term(a.fold, qdx[w][e], qdy[w][e], &tc, &ts);
    const int o = wbase + qwho[w][e];
    atomicAdd(&accC[o], (unsigned long long)tc);
    atomicAdd(&accS[o], (unsigned long long)ts);
  };
  for (int ch = blockIdx.x * BO_WAVES + w; ch < nchunk; ch += gridDim.x * BO_WAVES) {  // the same for the whole wave
    const int i = ch * 64 + lane;
    const bool live = i < nsel;
    accC[threadIdx.x] = 0ull;
    accS[threadIdx.x] = 0ull;
    const longlong2 me = live ? pts[i] : make_longlong2(0, 0);
    const int cx = kmcb::cell_of(kmcb::wrap(me.x, a.BX), a.ncx, a.BX), cy = kmcb::cell_of(kmcb::wrap(me.y, a.BY), a.ncy, a.BY);
    int r = -1, j = 0, j1 = 0, N = 0;
    int qn = 0;  // queued hits: the same in every lane
    bo_wave_sync();
    for (;;) {  // every pass moves each unfinished lane one candidate on: at most 6 runs of at most nsel points
      while (live && j == j1 && r < 5) {
        ++r;
        bo_run(a, cstart, cx, cy, r, &j, &j1);
      }
      const bool has = live && j < j1;
      if (__ballot(has) == 0ull) break;
      bool hit = false;
      int DX = 0, DY = 0;
      if (has) {
        const longlong2 q = pts[j];  // j < nsel
        ++j;
        const long long dx = kmcb::fold(q.x - me.x, a.BX), dy = kmcb::fold(q.y - me.y, a.BY);
        const long long D2 = dx * dx + dy * dy;
        hit = D2 > 0 && D2 <= a.RC2;
        DX = (int)dx;
        DY = (int)dy;
      }
      const unsigned long long hm = __ballot(hit);
      if (hit) {
        const int pos = qn + __popcll(hm & ((1ull << lane) - 1ull));  // qn <= 63 and at most 63 lanes below: < BO_Q
        qdx[w][pos] = DX;
        qdy[w][pos] = DY;
        qwho[w][pos] = (unsigned char)lane;
        ++N;
      }
      qn += __popcll(hm);
      if (qn >= 64) {
        bo_wave_sync();
        eval(qn - 64 + lane);  // the newest 64: 0 <= entry < qn <= 127
        qn -= 64;
        bo_wave_sync();  // read before the next hits overwrite the tail
      }
    }
    bo_wave_sync();
    if (lane < qn) eval(lane);  // the rest: qn <= 63
    bo_wave_sync();
    if (live) {
      const int ref = refs[i];  // < n
      C[ref] = accC[threadIdx.x];
      S[ref] = accS[threadIdx.x];
      nn[ref] = N;
    }
    bo_wave_sync();  // flushed before the next chunk clears the accumulators
  }
}

// ------------------------------------------------------------ the local pass, KMC_BO_LINKED
// One lane per ligand slot; the three link chains b -> r -> r' -> b' are loaded
// stage by stage, all three together.  Three terms at most: no loop to bound.
__global__ void __launch_bounds__(BO_T) k_bo_local_linked(KParams P, Dev d, BoArgs a, unsigned long long* C,
                                                          unsigned long long* S, int32_t* nn, BoOut* out) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  const int NA = P.NA, NB = P.NB, N = P.N;
  if (b >= NB) return;
  if (!bo_selected(P, d, a, b)) return;
  const int ref = d.id_of[NA + b] - NA;
  if ((unsigned)ref >= (unsigned)NB) {
    atomicOr(&out->err, 1u);
    return;
  }
  int r[3], r2[3], l[3];
  bool bad = false;
#pragma unroll
  for (int e = 0; e < 3; ++e) {
    r[e] = B_NEI(d, b, e + 2);
    if (r[e] < 0 || r[e] > NA) bad = true, r[e] = 0;  // a ligand links receptors: slot + 1 in [1, NA]
  }
#pragma unroll
  for (int e = 0; e < 3; ++e) {
    r2[e] = r[e] ? A_NEI3(d, r[e] - 1) : 0;  // index < NA
    if (r2[e] < 0 || r2[e] > NA) bad = true, r2[e] = 0;
  }
#pragma unroll
  for (int e = 0; e < 3; ++e) {
    l[e] = r2[e] ? A_NEI2(d, r2[e] - 1) : 0;  // index < NA
    if (l[e] != 0 && (l[e] <= NA || l[e] > N)) bad = true, l[e] = 0;  // a receptor's nei2 is a ligand: slot + 1 in (NA, N]
  }
  if (bad) {
    atomicOr(&out->err, 1u);
    return;
  }
  const longlong2 me = bo_XY(P, d, NA + b);
  long long sc = 0, ss = 0;
  int cnt = 0;
#pragma unroll
  for (int e = 0; e < 3; ++e) {
    if (l[e] == 0) continue;
    const int b2 = l[e] - 1 - NA;  // < NB
    if (b2 == b || !bo_selected(P, d, a, b2)) continue;
    const longlong2 q = bo_XY(P, d, NA + b2);
    const long long DX = kmcb::fold(q.x - me.x, a.BX), DY = kmcb::fold(q.y - me.y, a.BY);
    if (DX == 0 && DY == 0) continue;
    int64_t tc, ts;
    kmcb::term(a.fold, DX, DY, &tc, &ts);
    sc += tc;
    ss += ts;
    ++cnt;
  }
  C[ref] = (unsigned long long)sc;  // ref < NB
  S[ref] = (unsigned long long)ss;
  nn[ref] = cnt;
}

// ------------------------------------------------------------ reduce
// By reference index: nn < 0 marks a protein outside the set.  (pc, ps) are
// kept for the correlation; the histogram (when wanted) and the six sums are
// privatised in LDS and flushed with one 64-bit atomic per non-empty entry.
__global__ void __launch_bounds__(BO_T) k_bo_reduce(int n, int nbins, const unsigned long long* __restrict__ C,
                                                    const unsigned long long* __restrict__ S,
                                                    const int32_t* __restrict__ nn, int2* pcs,
                                                    unsigned long long* hist, BoOut* out) {
  extern __shared__ __attribute__((aligned(16))) unsigned long long bo_lds[];  // [6] sums, then [BO_NN_ROWS * nbins] bins
  const int nh = hist ? BO_NN_ROWS * nbins : 0;
  for (int b = threadIdx.x; b < 6 + nh; b += BO_T) bo_lds[b] = 0ull;
  __syncthreads();
  for (int i = blockIdx.x * BO_T + threadIdx.x; i < n; i += gridDim.x * BO_T) {
    const int N = nn[i];
    if (N < 0) {
      pcs[i] = make_int2(0, 0);
      continue;
    }
    if (N > BO_NN_MAX) {
      pcs[i] = make_int2(0, 0);
      atomicOr(&out->err, 2u);
      continue;
    }
    const long long pc = N ? kmcb::normalise((long long)C[i], N) : 0, ps = N ? kmcb::normalise((long long)S[i], N) : 0;
    const long long m = pc * pc + ps * ps;
    pcs[i] = make_int2((int)pc, (int)ps);  // |pc|, |ps| <= 2^15
    atomicAdd(&bo_lds[0], 1ull);
    if (N) {
      atomicAdd(&bo_lds[1], 1ull);
      atomicAdd(&bo_lds[2], (unsigned long long)N);
      atomicAdd(&bo_lds[3], (unsigned long long)pc);
      atomicAdd(&bo_lds[4], (unsigned long long)ps);
      atomicAdd(&bo_lds[5], (unsigned long long)m);
    }
    // row < BO_NN_ROWS, mag_bin < nbins: below nh
    if (hist) atomicAdd(&bo_lds[6 + min(N, BO_NN_ROWS - 1) * nbins + kmcb::mag_bin(m, nbins)], 1ull);
  }
  __syncthreads();
  for (int b = threadIdx.x; b < 6 + nh; b += BO_T) {
    if (!bo_lds[b]) continue;
    if (b < 6) atomicAdd(&out->sum[b], bo_lds[b]);
    else atomicAdd(&hist[b - 6], bo_lds[b]);  // < BO_NN_ROWS * nbins
  }
}

// ------------------------------------------------------------ correlation
// The half-stencil pair walk of k_an_pairs on the grid sized by r_max, over the
// binned points (N > 0 only): for cell c the i points are its own, the j points
// those of c itself (pairs i < j of the sorted order) and of its four forward
// neighbours.  Both sides are staged in LDS in chunks of `chunk` points, so any
// cell population is handled.  The float square root only guesses the bin; the
// integer edges decide.
__global__ void __launch_bounds__(BO_T) k_bo_corr(BoArgs a, const int32_t* __restrict__ cstart,
                                                  const longlong2* __restrict__ pts, const int2* __restrict__ pcs,
                                                  const int64_t* __restrict__ E2, int nbins, float inv_dr, int chunk,
                                                  unsigned long long* corr) {
  extern __shared__ __attribute__((aligned(16))) unsigned long long bo_lds[];  // 2 x chunk points (16 bytes each), 2 x chunk (pc, ps), [2 nbins] bins
  longlong2* si = reinterpret_cast<longlong2*>(bo_lds);
  longlong2* sj = si + chunk;
  int2* pi = reinterpret_cast<int2*>(sj + chunk);
  int2* pj = pi + chunk;
  unsigned long long* bins = reinterpret_cast<unsigned long long*>(pj + chunk);
  const int ncell = a.ncx * a.ncy;
  const long long d2max = E2[nbins];
  for (int b = threadIdx.x; b < 2 * nbins; b += BO_T) bins[b] = 0ull;
  for (int c = blockIdx.x; c < ncell; c += gridDim.x) {
    const int i0 = cstart[c], i1 = cstart[c + 1];  // c + 1 <= ncell
    if (i0 == i1) continue;
    const int cx = c % a.ncx, cy = c / a.ncx;
    for (int q = 0; q < 5; ++q) {
      // self, (+1, 0), (-1, +1), (0, +1), (+1, +1): every unordered pair of cells once (ncx, ncy >= 3)
      const int ox = q == 0 ? 0 : q == 1 ? 1 : q - 3, oy = q < 2 ? 0 : 1;
      const int jc = ((cy + oy) % a.ncy) * a.ncx + (cx + ox + a.ncx) % a.ncx;  // < ncell
      const int j0 = cstart[jc], j1 = cstart[jc + 1];
      if (j0 == j1) continue;
      const bool self = q == 0;
      for (int ib = i0; ib < i1; ib += chunk) {
        const int ni = min(chunk, i1 - ib);
        for (int jb = self ? ib : j0; jb < j1; jb += chunk) {  // self: chunks before ib hold only j < i
          const int nj = min(chunk, j1 - jb);
          __syncthreads();  // the previous block's reads are done
          for (int t = threadIdx.x; t < ni; t += BO_T) {  // t < chunk; ib + t < i1
            si[t] = pts[ib + t];
            pi[t] = pcs[ib + t];
          }
          for (int t = threadIdx.x; t < nj; t += BO_T) {  // t < chunk; jb + t < j1
            sj[t] = pts[jb + t];
            pj[t] = pcs[jb + t];
          }
          __syncthreads();
          for (int e = threadIdx.x; e < ni * nj; e += BO_T) {  // ni * nj <= chunk^2 <= 2^16
            const int ia = e / nj, jq = e - ia * nj;           // ia < ni, jq < nj
            if (self && ib + ia >= jb + jq) continue;
            const long long DX = kmcb::fold(sj[jq].x - si[ia].x, a.BX), DY = kmcb::fold(sj[jq].y - si[ia].y, a.BY);
            const long long D2 = DX * DX + DY * DY;
            if (D2 >= d2max) continue;
            const int k = kmcb::corr_bin(E2, nbins, D2, (int)(__fsqrt_rn((float)D2) * inv_dr));
            if (k >= nbins) continue;
            const long long v = (long long)pi[ia].x * pj[jq].x + (long long)pi[ia].y * pj[jq].y;
            atomicAdd(&bins[k], (unsigned long long)v);  // k < nbins
            atomicAdd(&bins[nbins + k], 1ull);
          }
        }
      }
    }
  }
  __syncthreads();
  for (int b = threadIdx.x; b < 2 * nbins; b += BO_T)
    if (bins[b]) atomicAdd(&corr[b], bins[b]);  // corr is [2][nbins]
}

}  // namespace kmcd
