// kmc_pairdyn.hip — pair dynamics over the committed state:
// the distinct and the (folded) self part of the van Hove function and the
// spatial correlation of displacements, against the one origin of
// kmc_pd_begin.  Like the lag correlator nothing here runs inside a step: the
// kernels are launched by kmc_pd_* between kmc_step calls, read what
// kmc_get_state would return and write only the recorder's own arrays.
//
// The per-protein state is indexed by REFERENCE index and advanced by
// k_pd_update as k_lag_update's first pass advances the lag correlator's.  The
// sample sorts points by the cell of a search grid (count / bins_scan /
// scatter) and walks pairs with a WAVE to a cell: the wave stages its cell's i
// points and a neighbour cell's j points in an LDS region of its own, with
// wave-level synchronisation only, its lanes take the staged pairs, and the
// workgroup's four waves share the LDS bins.  One walker serves both parts:
// the ordered 3 x 3 walk between the origin set and the current set (part A)
// and the half-shell walk within the origin set with the displacements as
// payload (part B).
//
// Included by kmc_engine.hip after kmc_orient.hip (one translation unit, the
// library's flags); the expressions are kmc_pairdyn.h's, shared with
// kmc_host_pd_* (kmc_host_observe.cpp); the host side of the calls is kmc_observe.hip
// §pair dynamics.
#include "kmc_device.h"
#include "kmc_observe.h"
#include "kmc_pairdyn.h"

namespace kmcd {

#define PD_T 256      // threads per workgroup
#define PD_WAVES 4    // waves, and so cells, a workgroup takes at once
#define PD_CHUNK 64   // points a wave stages per side (KMC_DEBUG_PD_CHUNK lowers it)
#define PD_A_BINS 6   // part A's tables: gd[4] then gs[2]
#define PD_B_KINDS 3  // part B's kinds

typedef unsigned long long pd_u64;

struct Pd {
  longlong2* prev;  // [N] integer position at the last update
  longlong2* U;     // [N] unwrapped integer position
  longlong2* X0;    // [N] position at the begin
  uint8_t* flags;   // [N] PD_JUMPED
  int32_t* opos;    // [N] the protein's place in the origin list
  int4* opt;        // [N] the origin list sorted by cell: (fold(X0).x, fold(X0).y, reference index, 0)
  int4* npt;        // [N] the current list sorted by cell: (fold(U).x, fold(U).y, reference index, 0)
  int4* upl;        // [N] part B's payload in origin-list order: (u.x, u.y, valid, 0)
  int32_t* cell;    // [N] cell and rank of the point being binned
  int32_t* rank;
  int32_t* ccnt;    // [ncell + 1] counts of the binning under way
  int32_t* ocstart; // [ncell + 1] the origin list's cell starts
  int32_t* ncstart; // [ncell + 1] the current list's
  int32_t* part;    // the scan's tile sums
  pd_u64* E2;       // [nbins + 1] squared edges
  pd_u64* out;      // gd [4][nbins], gs [2][nbins], cu [3][nbins][PD_CU_WORDS], then n_jumped
};

// host side: everything is allocated by kmc_pd_begin and freed by kmc_pd_end
struct PdState {
  Recorder rec;
  Scratch scratch;
  Pd dev = {};
  kmc_pd_config cfg = {};
  kmcp::Grid G = {};
  float inv_dr = 0.0f;   // bins per coordinate quantum: the float guess of a bin
  int chunk = PD_CHUNK;  // KMC_DEBUG_PD_CHUNK: smaller staged chunks (the chunked path at test size)
};

__device__ __forceinline__ int pd_cell(const kmcp::Grid& G, long long fx, long long fy) {
  return kmcp::cell(fy, G.ncy, G.BY) * G.ncx + kmcp::cell(fx, G.ncx, G.BX);
}

// update 0: the per-protein state, and the origin's cell and rank
__global__ void __launch_bounds__(PD_T) k_pd_begin(KParams P, Dev d, Pd D, kmcp::Grid G) {
  const int i = blockIdx.x * PD_T + threadIdx.x;
  if (i >= P.N) return;
  const longlong2 X = lag_xy(P, d, d.slot_of[i]);
  D.prev[i] = X;
  D.U[i] = X;
  D.X0[i] = X;
  D.flags[i] = 0;
  const int c = pd_cell(G, kmcp::fold(X.x, G.BX), kmcp::fold(X.y, G.BY));
  D.cell[i] = c;
  D.rank[i] = atomicAdd(&D.ccnt[c], 1);
}

__global__ void __launch_bounds__(PD_T) k_pd_origin_scatter(int N, Pd D, kmcp::Grid G) {
  const int i = blockIdx.x * PD_T + threadIdx.x;
  if (i >= N) return;
  const longlong2 X = D.X0[i];
  const int at = D.ocstart[D.cell[i]] + D.rank[i];
  D.opos[i] = at;
  D.opt[at] = make_int4((int)kmcp::fold(X.x, G.BX), (int)kmcp::fold(X.y, G.BY), i, 0);
}

// The per-protein step (include/kmc.h): workgroups stride over the blocks of
// 256 reference indices, the position gathered through slot_of.
__global__ void __launch_bounds__(PD_T) k_pd_update(KParams P, Dev d, Pd D, kmcp::Grid G, int nblk, pd_u64* n_jumped) {
  pd_u64 jumped = 0;  // lane 0 of each wave
  for (int blk = blockIdx.x; blk < nblk; blk += gridDim.x) {
    const int i = blk * PD_T + threadIdx.x;
    bool jp = false;
    if (i < P.N) {
      const longlong2 X = lag_xy(P, d, d.slot_of[i]);
      const longlong2 pv = D.prev[i];
      const long long dx = kmcl::min_image(X.x - pv.x, G.BX), dy = kmcl::min_image(X.y - pv.y, G.BY);
      longlong2 U = D.U[i];
      U.x += dx;
      U.y += dy;
      D.U[i] = U;
      D.prev[i] = X;
      uint8_t f = D.flags[i];
      if ((dx < 0 ? -dx : dx) >= G.J || (dy < 0 ? -dy : dy) >= G.J) D.flags[i] = f = (uint8_t)(f | PD_JUMPED);
      jp = f & PD_JUMPED;
    }
    const pd_u64 n = __popcll(__ballot(jp));
    if ((threadIdx.x & 63) == 0) jumped += n;
  }
  if ((threadIdx.x & 63) == 0 && jumped) atomicAdd(n_jumped, jumped);
}

// the sample's first pass: the current point's cell and rank, and part B's payload in origin-list order
__global__ void __launch_bounds__(PD_T) k_pd_now(int N, Pd D, kmcp::Grid G) {
  const int i = blockIdx.x * PD_T + threadIdx.x;
  if (i >= N) return;
  const longlong2 U = D.U[i], X0 = D.X0[i];
  const long long ux = U.x - X0.x, uy = U.y - X0.y;
  const bool ok = kmcp::valid(D.flags[i], ux, uy, G.F);
  D.upl[D.opos[i]] = ok ? make_int4((int)ux, (int)uy, 1, 0) : make_int4(0, 0, 0, 0);  // (valid: |u| < 2^24)
  const int c = pd_cell(G, kmcp::fold(U.x, G.BX), kmcp::fold(U.y, G.BY));
  D.cell[i] = c;
  D.rank[i] = atomicAdd(&D.ccnt[c], 1);
}

__global__ void __launch_bounds__(PD_T) k_pd_now_scatter(int N, Pd D, kmcp::Grid G) {
  const int i = blockIdx.x * PD_T + threadIdx.x;
  if (i >= N) return;
  const longlong2 U = D.U[i];
  D.npt[D.ncstart[D.cell[i]] + D.rank[i]] = make_int4((int)kmcp::fold(U.x, G.BX), (int)kmcp::fold(U.y, G.BY), i, 0);
}

// what one wave wrote to its LDS region is read by its other lanes: LDS
// operations of a wave complete in order, so compiler ordering is all it takes
__device__ __forceinline__ void pd_wave_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// the bin of d2: a float guess over the even spacing, corrected against the squared edges (kmcp::bin's k)
__device__ __forceinline__ int pd_bin(const pd_u64* E2, int nbins, float inv_dr, pd_u64 q) {
  int k = min(max((int)(__fsqrt_rn((float)q) * inv_dr), 0), nbins - 1);
  while (k < nbins && E2[k + 1] <= q) ++k;
  while (k > 0 && E2[k] > q) --k;
  return k;
}

// 128-bit add into an LDS partial (two words; the carry as geo_add128 takes it)
__device__ __forceinline__ void pd_lds_add128(pd_u64* w, long long v) {
  const pd_u64 lo = (pd_u64)v, hi = v < 0 ? ~0ull : 0ull;
  pd_u64 carry = 0;
  if (lo) {
    const pd_u64 old = atomicAdd(&w[0], lo);
    carry = (pd_u64)(old + lo < old);
  }
  if (hi + carry) atomicAdd(&w[1], hi + carry);
}

// The pair walker.  PART_B == false: part A, for every origin cell the ordered
// pairs of its origin points (i) with the current points (j) of the 3 x 3
// block; i == j is the self table's.  PART_B == true: part B, for every origin
// cell the unordered pairs within the origin list over the half shell, with
// the payload (u, valid) staged beside the points.  Wave w of workgroup b takes
// the cells (b * PD_WAVES + w) + n * gridDim.x * PD_WAVES.  Both sides are
// staged in chunks of `chunk` points, so any cell population is handled.  The
// LDS partials are 64-bit counts (one per pair: they cannot wrap) and 128-bit
// sums (two words each: they cannot wrap either), flushed once at the end with
// one 64-bit add per non-empty count and one geo_add128 per non-empty sum.
template <bool PART_B>
__global__ void __launch_bounds__(PD_T) k_pd_walk(Pd D, kmcp::Grid G, int NA, int chunk, float inv_dr) {
  extern __shared__ __attribute__((aligned(16))) pd_u64 pd_lds[];
  // [PD_WAVES] regions of (PART_B ? 4 : 2) * chunk int4, then [nbins + 1] squared edges, then the bins
  const int nb = G.nbins, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int per = (PART_B ? 4 : 2) * chunk;
  int4* si = reinterpret_cast<int4*>(pd_lds) + (size_t)wave * per;
  int4* sj = si + chunk;
  int4* ui = sj + chunk;  // (part B only)
  int4* uj = ui + chunk;
  pd_u64* E2 = pd_lds + 2 * (size_t)PD_WAVES * per;
  pd_u64* bins = E2 + nb + 1;
  const int nacc = PART_B ? PD_B_KINDS * nb * PD_CU_WORDS : PD_A_BINS * nb;
  for (int e = threadIdx.x; e <= nb; e += PD_T) E2[e] = D.E2[e];
  for (int e = threadIdx.x; e < nacc; e += PD_T) bins[e] = 0ull;
  __syncthreads();
  const int ncell = G.ncx * G.ncy;
  const int4* __restrict__ ipts = D.opt;
  const int4* __restrict__ jpts = PART_B ? D.opt : D.npt;
  const int32_t* __restrict__ icst = D.ocstart;
  const int32_t* __restrict__ jcst = PART_B ? D.ocstart : D.ncstart;
  for (int c = blockIdx.x * PD_WAVES + wave; c < ncell; c += gridDim.x * PD_WAVES) {
    const int i0 = icst[c], i1 = icst[c + 1];
    if (i0 == i1) continue;
    const int cx = c % G.ncx, cy = c / G.ncx;
    for (int q = 0; q < (PART_B ? 5 : 9); ++q) {
      int ox, oy;
      if (PART_B) {
        kmcp::half_shell(q, &ox, &oy);
      } else {
        ox = q % 3 - 1;
        oy = q / 3 - 1;
      }
      const int jc = ((cy + oy + G.ncy) % G.ncy) * G.ncx + (cx + ox + G.ncx) % G.ncx;
      const int j0 = jcst[jc], j1 = jcst[jc + 1];
      if (j0 == j1) continue;
      const bool self = PART_B && q == 0;
      for (int ib = i0; ib < i1; ib += chunk) {
        const int ni = min(chunk, i1 - ib);
        for (int jb = self ? ib : j0; jb < j1; jb += chunk) {  // self: chunks before ib hold only j < i
          const int nj = min(chunk, j1 - jb);
          pd_wave_sync();  // the previous block's reads are done
          for (int t = lane; t < ni; t += 64) {
            si[t] = ipts[ib + t];
            if (PART_B) ui[t] = D.upl[ib + t];
          }
          for (int t = lane; t < nj; t += 64) {
            sj[t] = jpts[jb + t];
            if (PART_B) uj[t] = D.upl[jb + t];
          }
          pd_wave_sync();
          for (int e = lane; e < ni * nj; e += 64) {
            const int a = e / nj, b = e - a * nj;
            if (self && ib + a >= jb + b) continue;
            const int4 pi = si[a], pj = sj[b];
            const pd_u64 q2 = kmcp::d2(kmcl::min_image((long long)pj.x - pi.x, G.BX),
                                       kmcl::min_image((long long)pj.y - pi.y, G.BY));
            if (q2 >= E2[nb]) continue;
            const int k = pd_bin(E2, nb, inv_dr, q2);
            const int s_i = pi.z >= NA, s_j = pj.z >= NA;
            if (PART_B) {
              pd_u64* cell = bins + ((size_t)kmcp::kind_b(s_i, s_j) * nb + k) * PD_CU_WORDS;
              atomicAdd(&cell[0], 1ull);
              const int4 va = ui[a], vb = uj[b];
              if (!(va.z & vb.z)) continue;
              atomicAdd(&cell[1], 1ull);
              pd_lds_add128(cell + 2, kmcp::dot(va.x, va.y, vb.x, vb.y));
              pd_lds_add128(cell + 4, kmcp::sq(va.x, va.y, vb.x, vb.y));
            } else {
              const int table = pi.z == pj.z ? 4 + s_i : kmcp::kind_a(s_i, s_j);
              atomicAdd(&bins[(size_t)table * nb + k], 1ull);
            }
          }
        }
      }
    }
  }
  __syncthreads();
  pd_u64* out = D.out + (PART_B ? (size_t)PD_A_BINS * nb : 0);
  if (PART_B) {
    for (int e = threadIdx.x; e < PD_B_KINDS * nb; e += PD_T) {
      const pd_u64* cell = bins + (size_t)e * PD_CU_WORDS;
      pd_u64* o = out + (size_t)e * PD_CU_WORDS;
      if (cell[0]) atomicAdd(&o[0], cell[0]);
      if (cell[1]) atomicAdd(&o[1], cell[1]);
      if (cell[2] | cell[3]) geo_add128(o + 2, geo_ld128(cell + 2));
      if (cell[4] | cell[5]) geo_add128(o + 4, geo_ld128(cell + 4));
    }
  } else {
    for (int e = threadIdx.x; e < nacc; e += PD_T)
      if (bins[e]) atomicAdd(&out[e], bins[e]);
  }
}

}  // namespace kmcd
