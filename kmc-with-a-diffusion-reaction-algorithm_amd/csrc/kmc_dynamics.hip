// kmc_dynamics.hip — displacement tracking over the committed state
// (DESIGN.md §11): unwrapped displacements since a time origin for the MSD and
// the self part of the van Hove function, and the survival of the origin's
// bonds.  Like kmc_analysis.hip nothing here runs inside a step: the kernels
// are launched by explicit calls between kmc_step calls, read what
// kmc_get_state would return and write only the tracker's own arrays.
//
// The tracker's arrays are indexed by REFERENCE index (slots are permuted by
// the re-sort); the kernels iterate by reference index, so the tracker's ~80
// bytes per protein stream in order and only the protein's current position
// (one 16-byte access) and links are gathered through slot_of.
//
// Included by kmc_engine.hip after kmc_bondorder.hip (one translation unit, the
// library's flags: -ffp-contract=off keeps every product and sum below its own
// rounding, as the numpy reference computes them); the host side of the calls
// is kmc_observe.hip §displacement tracking.
#include "kmc_device.h"
#include "kmc_observe.h"

namespace kmcd {

#define TRK_T 256         // threads per workgroup = the width of one reduction block
#define TRK_CLASSES 5     // KMC_TRACK_CLASSES
#define TRK_NSUM 10       // sum_u2[class], then sum_u2_clean[class]
#define TRK_BINS_MAX 512  // KMC_TRACK_MAX_BINS
#define TRK_NCNT 16       // n[5], n_clean[5], rl0 rl_now rl_kept cis0 cis_now cis_kept

// flag bits: 1 changed, 2 jumped (the public ones); 4 / 8: the receptor's
// R–L link (nei2, nei4) / cis link (nei3) differed from the origin at an update
enum : uint8_t { TRK_CHANGED = 1, TRK_JUMPED = 2, TRK_RL = 4, TRK_CIS = 8 };

struct Trk {
  double2* prev;   // [N] position at the last update
  double2* u;      // [N] unwrapped displacement since the origin
  uint8_t* flags;  // [N]
  uint8_t* cls;    // [N] class at the origin
  int32_t* link0;  // [3][N] origin links: receptor nei2 (ref + 1), nei4, nei3 (ref + 1); ligand nei2..4 (ref + 1)
};

struct TrkAcc {
  unsigned long long max_dx, max_dy;      // bit patterns of the largest |dx|, |dy| since begin
  unsigned long long n_jumped, n_changed; // of the last update
};

struct TrkOut {
  unsigned long long cnt[TRK_NCNT];
};

// host side: scratch of the first kmc_track_begin, none before it; rec.on: an
// origin is set (a new state drops it)
struct TrkState {
  Recorder rec;
  Scratch scratch;
  Trk dev = {nullptr, nullptr, nullptr, nullptr, nullptr};
  TrkAcc* acc = nullptr;
  TrkOut* out = nullptr;
  double* part[2] = {nullptr, nullptr};  // the reduction tree's levels, ping-pong
  double* edges = nullptr;               // [TRK_BINS_MAX + 1] squared bin edges
  unsigned long long* vh = nullptr;      // [TRK_CLASSES][TRK_BINS_MAX] van Hove bins
  double max_jump = 0.0;
};

// the links of the protein in slot `slot` as the tracker names them (a link out
// of range counts as none).  Its own reads: on top of prot_links it is a line
// longer (a receptor's entries go around nei4) and the tracker's kernels move
__device__ __forceinline__ void trk_links(const KParams& P, const Dev& d, int slot, int32_t l[3]) {
  const int NA = P.NA, NB = P.NB, N = P.N;
  auto ref = [&](int v) { return v >= 1 && v <= N ? d.id_of[v - 1] + 1 : 0; };
  if (slot < NA) {
    l[0] = ref(A_NEI2(d, slot));
    l[1] = A_NEI4(d, slot);
    l[2] = ref(A_NEI3(d, slot));
  } else {
    for (int j = 2; j <= 4; ++j) l[j - 2] = ref(B_NEI(d, slot - NA, j));
  }
}

__global__ void __launch_bounds__(TRK_T) k_trk_begin(KParams P, Dev d, Trk T) {
  const int i = blockIdx.x * TRK_T + threadIdx.x;
  const int N = P.N;
  if (i >= N) return;
  const int slot = d.slot_of[i];
  T.prev[i] = an_xy(P, d, slot);
  T.u[i] = make_double2(0.0, 0.0);
  T.flags[i] = 0;
  int32_t l[3];
  trk_links(P, d, slot, l);
  for (int k = 0; k < 3; ++k) T.link0[(size_t)k * N + i] = l[k];
  T.cls[i] = i < P.NA ? (l[0] != 0 ? 2 : l[2] != 0 ? 1 : 0) : ((l[0] | l[1] | l[2]) != 0 ? 4 : 3);
}

__device__ __forceinline__ unsigned long long trk_wave_max(unsigned long long v) {
  for (int o = 32; o; o >>= 1) {
    const unsigned long long w = __shfl_xor(v, o);
    v = w > v ? w : v;
  }
  return v;
}

// one protein per thread, in the order of include/kmc.h; the maxima and the
// flag counts go wave -> LDS -> one global atomic per workgroup
__global__ void __launch_bounds__(TRK_T) k_trk_update(KParams P, Dev d, Trk T, double max_jump, TrkAcc* acc) {
  __shared__ unsigned long long sm[4];
  if (threadIdx.x < 4) sm[threadIdx.x] = 0ull;
  __syncthreads();
  const int i = blockIdx.x * TRK_T + threadIdx.x;
  const int N = P.N;
  unsigned long long ax = 0ull, ay = 0ull;
  bool jumped = false, changed = false;
  if (i < N) {
    const int slot = d.slot_of[i];
    const double2 xy = an_xy(P, d, slot);
    const double2 pv = T.prev[i];
    double dx = xy.x - pv.x;
    dx = dx - P.box_x * kmcm::round_(dx / P.box_x);
    double dy = xy.y - pv.y;
    dy = dy - P.box_y * kmcm::round_(dy / P.box_y);
    double2 u = T.u[i];
    u.x = u.x + dx;
    u.y = u.y + dy;
    T.u[i] = u;
    T.prev[i] = xy;
    const double fx = kmcm::fabs_(dx), fy = kmcm::fabs_(dy);
    int32_t l[3];
    trk_links(P, d, slot, l);
    const bool c0 = l[0] != T.link0[i], c1 = l[1] != T.link0[(size_t)N + i], c2 = l[2] != T.link0[2 * (size_t)N + i];
    uint8_t f = T.flags[i];
    if (fx >= max_jump || fy >= max_jump) f |= TRK_JUMPED;
    if (i < P.NA) {
      if (c0 || c1) f |= TRK_CHANGED | TRK_RL;
      if (c2) f |= TRK_CHANGED | TRK_CIS;
    } else if (c0 || c1 || c2) {
      f |= TRK_CHANGED;
    }
    T.flags[i] = f;
    ax = (unsigned long long)__double_as_longlong(fx);
    ay = (unsigned long long)__double_as_longlong(fy);
    jumped = f & TRK_JUMPED;
    changed = f & TRK_CHANGED;
  }
  ax = trk_wave_max(ax);
  ay = trk_wave_max(ay);
  const unsigned long long nj = __popcll(__ballot(jumped)), nc = __popcll(__ballot(changed));
  if ((threadIdx.x & 63) == 0) {
    atomicMax(&sm[0], ax);
    atomicMax(&sm[1], ay);
    if (nj) atomicAdd(&sm[2], nj);
    if (nc) atomicAdd(&sm[3], nc);
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    if (sm[0]) atomicMax(&acc->max_dx, sm[0]);
    if (sm[1]) atomicMax(&acc->max_dy, sm[1]);
    if (sm[2]) atomicAdd(&acc->n_jumped, sm[2]);
    if (sm[3]) atomicAdd(&acc->n_changed, sm[3]);
  }
}

// The halving tree of include/kmc.h over one block of 256 terms per sum: the
// LDS holds t[s][256]; h = 128 and 64 through LDS, h <= 32 by __shfl_down in
// wave 0 (lane j < h reads lane j + h < 2h, which the step before left valid).
// dst[s * stride] receives the block's value.  All 256 threads call it.
__device__ __forceinline__ void trk_tree(double* t, int nsum, double* dst, size_t stride) {
  const int j = threadIdx.x;
  __syncthreads();
  if (j < 128)
    for (int s = 0; s < nsum; ++s) t[s * TRK_T + j] = t[s * TRK_T + j] + t[s * TRK_T + j + 128];
  __syncthreads();
  if (j < 64) {
    for (int s = 0; s < nsum; ++s) {
      double v = t[s * TRK_T + j] + t[s * TRK_T + j + 64];
      for (int h = 32; h; h >>= 1) v = v + __shfl_down(v, h);
      if (j == 0) dst[(size_t)s * stride] = v;
    }
  }
  __syncthreads();  // t is free again
}

// Workgroups stride over the blocks of 256 reference indices.  Per block the
// ten sums' terms are reduced by the tree into part[s][block]; the counts
// (summed per wave by ballots first) and the van Hove bins are privatised in
// LDS across the blocks a workgroup takes and flushed with one 64-bit atomic
// per non-empty entry.
__global__ void __launch_bounds__(TRK_T) k_trk_sample(KParams P, Dev d, Trk T, const double* __restrict__ edges2,
                                                      int nbins, float inv_dr, unsigned long long* vh, int nblk,
                                                      double* part, TrkOut* out) {
  extern __shared__ __attribute__((aligned(16))) unsigned long long trk_lds[];  // t[10][256], cnt[16], bins[5][nbins]
  double* t = reinterpret_cast<double*>(trk_lds);
  unsigned long long* cnt = trk_lds + TRK_NSUM * TRK_T;
  unsigned long long* bins = cnt + TRK_NCNT;
  const int nb = vh ? TRK_CLASSES * nbins : 0;
  const int N = P.N, NA = P.NA, j = threadIdx.x;
  for (int b = j; b < TRK_NCNT + nb; b += TRK_T) cnt[b] = 0ull;
  const double r2max = edges2[nbins];
  __syncthreads();
  for (int blk = blockIdx.x; blk < nblk; blk += gridDim.x) {
    const int i = blk * TRK_T + j;
    for (int s = 0; s < TRK_NSUM; ++s) t[s * TRK_T + j] = 0.0;
    uint32_t m = 0;  // bit b: this protein counts in cnt[b]
    if (i < N) {
      const double2 u = T.u[i];
      const double q = u.x * u.x + u.y * u.y;
      const uint8_t f = T.flags[i];
      const int c = T.cls[i];
      const bool clean = (f & (TRK_CHANGED | TRK_JUMPED)) == 0;
      t[c * TRK_T + j] = q;
      m |= 1u << c;
      if (clean) {
        t[(TRK_CLASSES + c) * TRK_T + j] = q;
        m |= 1u << (TRK_CLASSES + c);
        if (nb && q < r2max) {
          // k = #{m in 1..nbins : edges2[m] <= q}: a float guess, corrected against the table
          int k = min(max((int)(__fsqrt_rn((float)q) * inv_dr), 0), nbins - 1);
          while (k < nbins && edges2[k + 1] <= q) ++k;
          while (k > 0 && edges2[k] > q) --k;
          if (k < nbins) atomicAdd(&bins[c * nbins + k], 1ull);
        }
      }
      if (i < NA) {
        const int32_t o2 = T.link0[i], o4 = T.link0[(size_t)N + i], o3 = T.link0[2 * (size_t)N + i];
        const bool rl = o2 != 0, cis = o3 != 0 && i + 1 < o3;  // a cis bond counts at its lower-index receptor
        if (rl || cis) {
          int32_t l[3];
          trk_links(P, d, d.slot_of[i], l);
          if (rl) m |= 1u << 10 | (l[0] == o2 && l[1] == o4 ? 1u << 11 : 0u) | (!(f & TRK_RL) ? 1u << 12 : 0u);
          if (cis) m |= 1u << 13 | (l[2] == o3 ? 1u << 14 : 0u) | (!(f & TRK_CIS) ? 1u << 15 : 0u);
        }
      }
    }
    // the counts per wave: one ballot per counter, lane 0 adds the non-zero ones
    for (int b = 0; b < TRK_NCNT; ++b) {
      const unsigned long long k = __popcll(__ballot(m >> b & 1u));
      if ((j & 63) == 0 && k) atomicAdd(&cnt[b], k);
    }
    trk_tree(t, TRK_NSUM, part + blk, (size_t)nblk);
  }
  __syncthreads();
  for (int b = j; b < TRK_NCNT; b += TRK_T)
    if (cnt[b]) atomicAdd(&out->cnt[b], cnt[b]);
  for (int b = j; b < nb; b += TRK_T)
    if (bins[b]) atomicAdd(&vh[b], bins[b]);
}

// the next level of the tree: in[s][n] -> out[s][ceil(n / 256)], padded with 0.0;
// blockIdx.y = the sum
__global__ void __launch_bounds__(TRK_T) k_trk_tree(const double* __restrict__ in, int n, double* out, int nout) {
  __shared__ double t[TRK_T];
  const int s = blockIdx.y, idx = blockIdx.x * TRK_T + threadIdx.x;
  t[threadIdx.x] = idx < n ? in[(size_t)s * n + idx] : 0.0;
  trk_tree(t, 1, out + (size_t)s * nout + blockIdx.x, 0);
}

}  // namespace kmcd
