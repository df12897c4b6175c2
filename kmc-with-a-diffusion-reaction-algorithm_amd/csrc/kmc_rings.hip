// kmc_rings.hip — ring statistics and valency census of the ligand network
// of the committed state: the multigraph whose vertices are the
// ligands and whose edges are the ligand – receptor = receptor – ligand
// bridges, its adjacency and valency bins, and the rings of up to RG_MAX
// bridges with the chordless ones among them.  Like the other layers the
// kernels are read-only over the state (a_int / b_int, whose links are slot +
// 1) and name proteins by their reference index through id_of.  Everything is
// an integer count: any schedule and any slot order give the same numbers.
//
// Included by kmc_engine.hip after kmc_coag.hip (one translation unit, the
// library's flags); the host side of the calls is kmc_observe.hip §rings.
#include "kmc_device.h"
#include "kmc_observe.h"
#include "kmc_rings.h"

namespace kmcd {

#define RG_T 256        // threads per workgroup of both kernels
#define RG_WG_MAX 2048  // workgroups of the grid-stride ring kernel (8 per CU)

// the counters of kmc_net_out the adjacency kernel sums
enum : int { RG_BRIDGES = 0, RG_LOOPS, RG_HALF, RG_FREE_DIMERS, RG_VERTICES, RG_COMPONENTS, RG_NCNT };
#define RG_NBINS (16 + 4 + RG_NCNT)  // lig[4][4], rec[4], the counters: one LDS array, one flush

// device-side results of one call
struct RgOut {
  unsigned long long bins[RG_NBINS];
  unsigned long long counts[2][RG_MAX + 1];  // rings by length: all, chordless
  unsigned long long hops;                   // adjacency rows the ring kernel gathered along its paths (kmc_rings_hops)
  uint32_t nwork;                            // ligands on the worklist (<= NB)
  uint32_t err;                              // 1: a link of the wrong kind, an asymmetric bridge or an index out of range
};

// host side: scratch of the first call, its own (the component labels too: kmc_components' buffers are not touched)
struct RgState {
  int32_t *parent = nullptr, *label = nullptr;  // [N] union-find and its labels (k_an_init / k_an_hook / k_an_flatten)
  unsigned long long* cnt = nullptr;            // [N] k_an_init's member counts (unused here)
  int32_t* flag = nullptr;                      // [N] by label: the component holds a bridge
  AnOut* an_out = nullptr;
  int4* rows = nullptr;        // [NB] adjacency by ligand slot
  int32_t* work = nullptr;     // [NB] the ligand slots with >= 2 bridge ends
  uint32_t* member = nullptr;  // [2][NB] ring lengths by reference index: all, chordless
  RgOut* out = nullptr;
  int64_t hops = 0;  // of the last kmc_rings call
};

// An adjacency row, 16 bytes: x, y, z = the ligand (slot + 1 within the
// ligands, 0: none) bridged to site 2, 3, 4; w = the ligand's own reference
// index (within the ligands) << 8 | the far sites' numbers - 2, two bits each.
__device__ __forceinline__ int rg_nbr(const int4& r, int e) { return e == 0 ? r.x : e == 1 ? r.y : r.z; }  // e = site - 2
__device__ __forceinline__ int rg_site(const int4& r, int e) { return (int)(((uint32_t)r.w >> (2 * e)) & 3u) + 2; }
__device__ __forceinline__ int rg_ref(const int4& r) { return (int)((uint32_t)r.w >> 8); }  // < NB <= 2^24

// ------------------------------------------------------------ adjacency
// Lane t serves ligand slot t (t < NB) and receptor slot t (t < NA).  The
// ligand's three chains are loaded stage by stage (kmcr::hops); the row, the
// valency bins and the counters follow.  label / flag are by reference index:
// the first ligand with a bridge end to flag its component counts it.  The
// ligands with two or more bridge ends — the only ones a ring can pass — are
// compacted into the worklist wave by wave (ballot + prefix count, one atomic a
// wave), so the ring kernel's waves start full.  Bins and counters are
// privatised in LDS and flushed with one 64-bit atomic per non-empty entry.
__global__ void __launch_bounds__(RG_T) k_rg_adj(KParams P, Dev d, const int32_t* __restrict__ label, int32_t* flag,
                                                 int4* rows, int32_t* work, RgOut* out) {
  __shared__ unsigned long long bins[RG_NBINS];
  const int NA = P.NA, NB = P.NB, N = P.N;
  const int t = blockIdx.x * RG_T + threadIdx.x, lane = threadIdx.x & 63;
  for (int b = threadIdx.x; b < RG_NBINS; b += RG_T) bins[b] = 0ull;
  __syncthreads();
  bool cand = false;
  if (t < NB) {
    const int ref = d.id_of[NA + t] - NA;  // slot NA + t < N
    kmcr::Hops h;
    kmcr::hops(d.a_int, d.b_int, NA, NB, t, h);
    int4 row = make_int4(0, 0, 0, 0);
    if (h.bad || (unsigned)ref >= (unsigned)NB) {
      atomicOr(&out->err, 1u);
    } else {
      int occ = 0, ends = 0;
      uint32_t sites = 0;
#pragma unroll
      for (int e = 0; e < 3; ++e) {
        occ += h.r[e] != 0;
        if (h.r2[e] != 0 && h.l[e] == 0) atomicAdd(&bins[20 + RG_HALF], 1ull);
        if (h.l[e] == 0) continue;
        ++ends;
        sites |= (uint32_t)(h.s2[e] - 2) << (2 * e);
        if (kmcr::first_end(t + 1, e + 2, h.l[e], h.s2[e])) {
          atomicAdd(&bins[20 + RG_BRIDGES], 1ull);
          if (h.l[e] == t + 1) atomicAdd(&bins[20 + RG_LOOPS], 1ull);
        }
      }
      row = make_int4(h.l[0], h.l[1], h.l[2], (int)((uint32_t)ref << 8 | sites));  // each l in [0, NB]
      atomicAdd(&bins[occ * 4 + ends], 1ull);                                       // occ, ends <= 3: below 16
      if (ends >= 1) {
        atomicAdd(&bins[20 + RG_VERTICES], 1ull);
        const int lab = label[NA + ref];  // reference index NA + ref < N; a label is a reference index < N
        if ((unsigned)lab >= (unsigned)N) atomicOr(&out->err, 1u);
        else if (atomicExch(&flag[lab], 1) == 0) atomicAdd(&bins[20 + RG_COMPONENTS], 1ull);
      }
      cand = ends >= 2;
    }
    rows[t] = row;  // t < NB; an empty row where the chains failed: nothing is followed through them
  }
  if (t < NA) {
    const int32_t v2 = A_NEI2(d, t), v3 = A_NEI3(d, t);
    if (!kmcr::receptor_links_ok(v2, v3, t + 1, NA, NB)) {
      atomicOr(&out->err, 1u);
    } else {
      atomicAdd(&bins[16 + kmcr::rec_bin(v2, v3)], 1ull);
      if (v3 != 0) {
        const int32_t p2 = A_NEI2(d, v3 - 1), p3 = A_NEI3(d, v3 - 1);  // v3 - 1 < NA
        if (p3 != t + 1) atomicOr(&out->err, 1u);
        else if (v2 == 0 && p2 == 0 && t + 1 < v3) atomicAdd(&bins[20 + RG_FREE_DIMERS], 1ull);
      }
    }
  }
  // the worklist: every lane of the wave takes part in the ballot
  const unsigned long long m = __ballot(cand);
  if (m) {
    uint32_t base = 0;
    if (lane == 0) base = atomicAdd(&out->nwork, (uint32_t)__popcll(m));
    base = (uint32_t)__shfl((int)base, 0);
    if (cand) work[base + __popcll(m & ((1ull << lane) - 1ull))] = t;  // below the candidates' number <= NB
  }
  __syncthreads();
  for (int b = threadIdx.x; b < RG_NBINS; b += RG_T)
    if (bins[b]) atomicAdd(&out->bins[b], bins[b]);
}

// ------------------------------------------------------------ rings
// A ring is counted from its lowest ligand (by slot; any total order gives the
// same counts) and from there in one direction: task (root, s_first < s_last)
// walks the simple paths that leave the root by site s_first over ligands
// above the root and counts a ring when a path comes back into site s_last.
// Three tasks a worklist entry, one lane a task.
//
// Work: a visited ligand offers its two other sites, a path holds at most
// max_len ligands, so a task visits fewer than 2^(max_len - 1) ligands and a
// root costs at most 3 * 2^(max_len - 1) hops.  The loop below is bounded by
// that count whatever the rows hold.
//
// The depth-first walk keeps, per lane and in LDS laid out [depth][lane] (no
// bank conflict, no private array): path[k], the ligand at depth k, and
// pend[k], the one sibling at depth k still to visit (its bit in pmask).  The
// sites by which the path enters and leaves each depth are two bits a depth in
// the register words ins / outs.  On closing a ring of L ligands the chord rule
// (kmcr::chordless) reads the L rows again: closures are rare next to hops.
__global__ void __launch_bounds__(RG_T) k_rg_rings(int NB, int max_len, const int4* __restrict__ rows,
                                                   const int32_t* __restrict__ work, uint32_t* member, RgOut* out) {
  __shared__ int32_t path[RG_MAX][RG_T], pend[RG_MAX][RG_T];  // depth < max_len <= RG_MAX
  __shared__ unsigned long long cnt[2][RG_MAX + 1], hops;
  const int tid = threadIdx.x;
  for (int b = tid; b < 2 * (RG_MAX + 1); b += RG_T) (&cnt[0][0])[b] = 0ull;
  if (tid == 0) hops = 0ull;
  unsigned long long nh = 0;  // this lane's hops
  __syncthreads();
  const bool ok = out->err == 0;                    // the adjacency failed: its rows are not walked
  const uint32_t nwork = min(out->nwork, (uint32_t)NB);
  const uint32_t ntask = ok ? 3u * nwork : 0u;      // NB <= 2^24: no overflow
  for (uint32_t task = blockIdx.x * RG_T + tid; task < ntask; task += gridDim.x * RG_T) {
    const int root = work[task / 3] + 1;            // task / 3 < nwork; a ligand slot + 1 in [1, NB]
    const int pr = (int)(task % 3);                 // the site pairs (2, 3), (2, 4), (3, 4)
    const int sa = pr == 2 ? 3 : 2, sb = pr == 0 ? 3 : 4;
    const int4 r0 = rows[root - 1];
    ++nh;
    int v = rg_nbr(r0, sa - 2), in = rg_site(r0, sa - 2);
    if (v == 0) continue;
    if (v == root) {  // a loop: chordless always (its ligand's third site leads elsewhere)
      if (in != sb) continue;
      atomicAdd(&cnt[0][1], 1ull);
      atomicAdd(&cnt[1][1], 1ull);
      if (member) {
        atomicOr(&member[rg_ref(r0)], 2u);  // reference index < NB
        atomicOr(&member[NB + rg_ref(r0)], 2u);
      }
      continue;
    }
    if (v < root || max_len < 2) continue;
    int k = 1;
    uint32_t ins = (uint32_t)(sb - 2), outs = (uint32_t)(sa - 2), pmask = 0;  // depth 0: the root's two ring sites
    for (int it = 0; it < (1 << (RG_MAX - 1)); ++it) {
      // visit ligand v, entered by site in, at depth k in [1, max_len)
      path[k][tid] = v;
      ins = (ins & ~(3u << (2 * k))) | (uint32_t)(in - 2) << (2 * k);
      const int4 rw = rows[v - 1];  // v in [1, NB]
      ++nh;
      int go = 0, closed = 0;
#pragma unroll
      for (int q = 0; q < 2; ++q) {
        const int c = q == 0 ? (in == 2 ? 3 : 2) : (in == 4 ? 3 : 4);  // the two other sites, ascending
        const int w = rg_nbr(rw, c - 2), ws = rg_site(rw, c - 2);
        if (w == 0) continue;
        if (w == root) {
          if (ws == sb) closed = c;  // (at most once a visit: the root's site s_last holds one bridge)
          continue;
        }
        if (w < root || k + 1 >= max_len) continue;
        bool seen = false;
        for (int j = 1; j <= k; ++j) seen |= path[j][tid] == w;  // j < max_len
        if (seen) continue;
        const int packed = w << 4 | (ws - 2) << 2 | (c - 2);  // w <= 2^24
        if (!go) {
          go = packed;
        } else {
          pend[k + 1][tid] = packed;  // k + 1 < max_len
          pmask |= 1u << (k + 1);
        }
      }
      if (closed) {
        const int L = k + 1;  // <= max_len
        const uint32_t o = (outs & ~(3u << (2 * k))) | (uint32_t)(closed - 2) << (2 * k);
        auto vert = [&](int j) { return j == 0 ? root : path[j][tid]; };  // j < L
        auto off = [&](int i) {  // the ligand on the site vert(i) keeps off the ring
          return rg_nbr(rows[vert(i) - 1],
                        kmcr::off_site((int)((ins >> (2 * i)) & 3u) + 2, (int)((o >> (2 * i)) & 3u) + 2) - 2);
        };
        const bool chordless = kmcr::chordless(L, vert, off);
        atomicAdd(&cnt[0][L], 1ull);
        if (chordless) atomicAdd(&cnt[1][L], 1ull);
        if (member)
          for (int i = 0; i < L; ++i) {
            const int ref = rg_ref(rows[vert(i) - 1]);  // reference index < NB
            atomicOr(&member[ref], 1u << L);
            if (chordless) atomicOr(&member[NB + ref], 1u << L);
          }
      }
      if (go) {
        ++k;
      } else if (pmask) {
        k = 31 - __clz((int)pmask);  // the deepest sibling waiting: its ancestors path[1..k-1] are still in place
        go = pend[k][tid];
        pmask &= ~(1u << k);
      } else {
        break;
      }
      v = go >> 4;
      in = ((go >> 2) & 3) + 2;
      outs = (outs & ~(3u << (2 * (k - 1)))) | (uint32_t)(go & 3) << (2 * (k - 1));
    }
  }
  if (nh) atomicAdd(&hops, nh);
  __syncthreads();
  for (int b = tid; b < 2 * (RG_MAX + 1); b += RG_T)
    if ((&cnt[0][0])[b]) atomicAdd(&(&out->counts[0][0])[b], (&cnt[0][0])[b]);
  if (tid == 0 && hops) atomicAdd(&out->hops, hops);
}

}  // namespace kmcd
