// kmc_structure.hip — static structure factor of the committed state
// (DESIGN.md §13): per species the exact int64 sums of every protein's
// fixed-point (cos, sin) term at the wave vectors q(h, k) of the half plane.
// Like kmc_analysis.hip the kernel is read-only over the state (Dev::cur,
// a_int / b_int); the sums do not depend on the order of summation, so the
// slots are taken as they lie and no reference index is needed.
//
// Included by kmc_engine.hip after kmc_geometry.hip (one translation unit, the
// library's flags: -ffp-contract=off, so a term is the four products, the two
// sums and the two roundings include/kmc.h writes down and nothing else); the
// host side of the call is kmc_observe.hip §structure factor.
#include "kmc_device.h"
#include "kmc_structure.h"

namespace kmcd {

#define SK_T 256      // threads per workgroup
#define SK_TILE 32    // proteins whose axis tables one workgroup stages at a time
#define SK_QPL 8      // wave vectors a lane owns (two int64 accumulators each, in registers)
#define SK_QB (SK_T * SK_QPL)  // most contiguous q indices of one q-block (blockIdx.y)
#define SK_WG 1024    // workgroups of a launch over both grid axes (4 per CU)
// (cos, sin) pairs per staged protein: the h rows a q-block touches, then |k| = 0..kmax.  A block of
// qb <= SK_QB contiguous indices of rows 2 kmax + 1 wide lies in at most (qb - 1) / (2 kmax + 1) + 2
// rows and in no more than hmax + 1; the sum peaks at 82 (kmax = 64: 17 + 65), 41 KiB per tile
#define SK_E_MAX 82

struct SkArgs {
  int hmax, kmax, select;
  int nq, W;        // (hmax + 1) * W wave vectors, W = 2 kmax + 1
  int qb;           // q indices per q-block: nq spread evenly over the fewest blocks of at most SK_QB
  int nh_max, E;    // h rows reserved per protein; pairs per protein (nh_max + kmax + 1 <= SK_E_MAX)
  long long BX, BY;
};

// host side: [4][SK_NQ_MAX] sums, then the two selection counts; its own, whatever N
struct SkState {
  unsigned long long* sums = nullptr;
};

// rows spanned by the q-block whose first index is q0
__host__ __device__ __forceinline__ int sk_rows(int q0, int qb, int nq, int W, int* h_lo) {
  const int q1 = (q0 + qb < nq ? q0 + qb : nq) - 1;
  *h_lo = q0 / W;
  return q1 / W - q0 / W + 1;
}

// grid (workgroups striding over the tiles, q-blocks).  sums[4][nq]: C_A, S_A, C_B, S_B; nsel[2].
// Per species: stage a tile's integer coordinates and selection, fill its axis tables, add every
// selected protein's term to the owned accumulators; after the last tile one 64-bit atomic per
// owned q and component.  Every loop is bounded by N, SK_TILE * E or SK_QPL.
__global__ void __launch_bounds__(SK_T) k_sk_sums(KParams P, Dev d, SkArgs a, unsigned long long* sums,
                                                  unsigned long long* nsel) {
  extern __shared__ __attribute__((aligned(16))) double2 sk_lds[];  // [SK_TILE][E] tables, [SK_TILE] coordinates, flags
  double2* tab = sk_lds;
  longlong2* XY = reinterpret_cast<longlong2*>(sk_lds + (size_t)SK_TILE * a.E);
  int* sel = reinterpret_cast<int*>(XY + SK_TILE);  // [SK_TILE] selected, then [1] the workgroup's count
  const int tid = threadIdx.x, NA = P.NA, NB = P.NB;
  const int q0 = blockIdx.y * a.qb;
  const int q_end = q0 + a.qb < a.nq ? q0 + a.qb : a.nq;
  int h_lo;
  const int nh = sk_rows(q0, a.qb, a.nq, a.W, &h_lo);

  // the owned wave vectors: q0 + j * SK_T + tid, consecutive over the lanes (one h row broadcast, the k
  // entries side by side in LDS)
  int ih[SK_QPL], ik[SK_QPL];
  bool neg[SK_QPL], own[SK_QPL];
#pragma unroll
  for (int j = 0; j < SK_QPL; ++j) {
    const int q = q0 + j * SK_T + tid;
    own[j] = q < q_end;
    const int h = own[j] ? q / a.W : h_lo, k = own[j] ? q % a.W - a.kmax : 0;
    ih[j] = h - h_lo;                         // < nh <= nh_max
    ik[j] = a.nh_max + (k < 0 ? -k : k);      // < E
    neg[j] = k < 0;
  }

  for (int sp = 0; sp < 2; ++sp) {
    const int base = sp ? NA : 0, n = sp ? NB : NA;
    const int ntile = (n + SK_TILE - 1) / SK_TILE;
    long long accC[SK_QPL], accS[SK_QPL];
#pragma unroll
    for (int j = 0; j < SK_QPL; ++j) accC[j] = accS[j] = 0;
    if (tid == 0) sel[SK_TILE] = 0;
    for (int tile = blockIdx.x; tile < ntile; tile += gridDim.x) {
      const int first = tile * SK_TILE, cnt = n - first < SK_TILE ? n - first : SK_TILE;
      __syncthreads();  // the previous tile's tables are read no more
      if (tid < cnt) {
        const int i = first + tid, p = base + i;  // slot p < N
        const double2 xy = an_xy(P, d, p);
        XY[tid] = make_longlong2((long long)kmcm::round_(xy.x * 1024.0), (long long)kmcm::round_(xy.y * 1024.0));
        int s = 1;
        if (a.select == 1) {
          if (sp == 0) s = (A_NEI2(d, i) != 0) | (A_NEI3(d, i) != 0);
          else s = (B_NEI(d, i, 2) != 0) | (B_NEI(d, i, 3) != 0) | (B_NEI(d, i, 4) != 0);
        }
        sel[tid] = s;
        if (s && blockIdx.y == 0) atomicAdd(&sel[SK_TILE], 1);
      }
      __syncthreads();
      const int per = nh + a.kmax + 1;  // pairs this q-block needs per protein
      for (int e = tid; e < cnt * per; e += SK_T) {
        const int t = e / per, r = e - t * per;
        if (!sel[t]) continue;
        double c, s;
        if (r < nh) kmcs::axis_phase(h_lo + r, XY[t].x, a.BX, &c, &s);
        else kmcs::axis_phase(r - nh, XY[t].y, a.BY, &c, &s);
        tab[(size_t)t * a.E + (r < nh ? r : a.nh_max + (r - nh))] = make_double2(c, s);
      }
      __syncthreads();
      for (int t = 0; t < cnt; ++t) {
        if (!sel[t]) continue;  // the same for the whole workgroup
        const double2* row = tab + (size_t)t * a.E;
#pragma unroll
        for (int j = 0; j < SK_QPL; ++j) {
          if (!own[j]) continue;
          const double2 x = row[ih[j]], y = row[ik[j]];
          int64_t tc, ts;
          kmcs::term(x.x, x.y, y.x, y.y, neg[j], &tc, &ts);
          accC[j] += tc;
          accS[j] += ts;
        }
      }
    }
#pragma unroll
    for (int j = 0; j < SK_QPL; ++j) {
      if (!own[j]) continue;
      const size_t q = (size_t)q0 + j * SK_T + tid;  // < nq
      if (accC[j]) atomicAdd(&sums[(size_t)(2 * sp) * a.nq + q], (unsigned long long)accC[j]);
      if (accS[j]) atomicAdd(&sums[(size_t)(2 * sp + 1) * a.nq + q], (unsigned long long)accS[j]);
    }
    __syncthreads();  // every selected protein of the workgroup's tiles is counted
    if (tid == 0 && blockIdx.y == 0 && sel[SK_TILE]) atomicAdd(&nsel[sp], (unsigned long long)sel[SK_TILE]);
    __syncthreads();  // ... and read before the next species clears the count
  }
}

}  // namespace kmcd
