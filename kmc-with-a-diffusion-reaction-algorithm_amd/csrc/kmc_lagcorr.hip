// kmc_lagcorr.hip — the multi-origin lag correlator over the committed state
// (DESIGN.md §18): rings of unwrapped integer positions stored at log-spaced
// strides, correlated with the current positions at every update, for MSD(τ),
// α2(τ) and F_s(q, τ) averaged over every time origin of the run.  Like the
// tracker nothing here runs inside a step: the kernels are launched by
// kmc_lag_* between kmc_step calls, read what kmc_get_state would return and
// write only the recorder's own arrays.
//
// Everything is indexed by REFERENCE index, as the tracker's arrays are: a
// thread serves one reference index, gathers the protein's position and links
// through slot_of (trk_links) and streams the rest — its own element of the
// per-protein state and of every ring entry an update's tasks name.  A thread
// reads and writes only its own element of a ring entry, so the new origins
// are stored in the launch that correlated with the old ones.
//
// Included by kmc_engine.hip after kmc_rings.hip (one translation unit, the
// library's flags); the expressions are kmc_lagcorr.h's, shared with
// kmc_host_lag_* (kmc_host_observe.cpp); the host side of the calls is kmc_observe.hip
// §lag correlator.
#include "kmc_device.h"
#include "kmc_lagcorr.h"
#include "kmc_observe.h"

namespace kmcd {

#define LAG_T 256        // threads per workgroup = one block of reference indices
#define LAG_CHUNK 64     // tasks whose partials the LDS holds at a time
#define LAG_FLUSH 32     // blocks between two flushes: 2^13 terms below 2^50 stay below 2^63
#define LAG_CELL 17      // 64-bit words of a kmc_lag_cell
// the LDS partials of one (task, class): three counts, m2_all, m2_clean, the
// three parts of q², fs[4]
enum { LAG_W_ALL, LAG_W_CLEAN, LAG_W_FAR, LAG_W_M2A, LAG_W_M2C, LAG_W_A2, LAG_W_AB, LAG_W_B2, LAG_W_FS, LAG_W = 12 };

typedef unsigned long long lag_u64;

struct Lag {
  longlong2* prev;      // [N] integer position at the last update
  longlong2* U;         // [N] unwrapped integer position
  int32_t* links;       // [3][N] trk_links as of the last update
  int32_t* last_event;  // [N] the last update that saw a jump or a change of links
  uint8_t* cls;         // [N] class at the last update
  longlong2* ring;      // [L * P][N] the stored origins
};

struct LagArgs {
  long long BX, BY, J, F;
  int n, L, P, nq, ntasks;
  int h[LAG_MAX_Q];
};

// host side: everything is allocated by kmc_lag_begin and freed by kmc_lag_end
struct LagState {
  Recorder rec;
  Scratch scratch;
  Lag dev = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
  kmcl::Task* tasks = nullptr;  // [LAG_MAX_ROWS] the update's task list
  lag_u64* table = nullptr;     // [rows][5][LAG_CELL]
  lag_u64* n_events = nullptr;  // proteins with an event at the last update
  kmc_lag_config cfg = {};
  LagArgs a = {};
  int64_t n_pairs[LAG_MAX_ROWS] = {0};
};

__device__ __forceinline__ longlong2 lag_xy(const KParams& P, const Dev& d, int slot) {
  const double2 xy = an_xy(P, d, slot);
  return make_longlong2((long long)kmcm::round_(xy.x * 1024.0), (long long)kmcm::round_(xy.y * 1024.0));
}

__global__ void __launch_bounds__(LAG_T) k_lag_begin(KParams P, Dev d, Lag G, int L, int slots) {
  const int i = blockIdx.x * LAG_T + threadIdx.x;
  const int N = P.N;
  if (i >= N) return;
  const int slot = d.slot_of[i];
  const longlong2 X = lag_xy(P, d, slot);
  G.prev[i] = X;
  G.U[i] = X;
  int32_t l[3];
  trk_links(P, d, slot, l);
  for (int k = 0; k < 3; ++k) G.links[(size_t)k * N + i] = l[k];
  G.last_event[i] = 0;
  G.cls[i] = (uint8_t)kmcl::cls(i < P.NA, l);
  for (int lv = 0; lv < L; ++lv) G.ring[(size_t)(lv * slots) * N + i] = X;  // the origin of update 0: slot 0 of every level
}

__device__ __forceinline__ lag_u64 lag_wave_sum(lag_u64 v) {
  for (int o = 32; o; o >>= 1) v += __shfl_xor(v, o);
  return v;
}

// the workgroup's partials of nt tasks go to the table: one 64-bit or one
// carry-propagating 128-bit add per non-empty word, which is zeroed.  All 256
// threads call it; the barriers make the words whole before and free after.
__device__ __forceinline__ void lag_flush(lag_u64* acc, const kmcl::Task* __restrict__ tasks, int nt, lag_u64* table) {
  __syncthreads();
  for (int e = threadIdx.x; e < nt * LAG_CLASSES * LAG_W; e += LAG_T) {
    const lag_u64 v = acc[e];
    if (!v) continue;
    acc[e] = 0ull;
    const int w = e % LAG_W, c = e / LAG_W % LAG_CLASSES, t = e / (LAG_W * LAG_CLASSES);
    lag_u64* cell = table + ((size_t)tasks[t].row * LAG_CLASSES + c) * LAG_CELL;
    switch (w) {
      case LAG_W_ALL:
      case LAG_W_CLEAN:
      case LAG_W_FAR: atomicAdd(&cell[w], v); break;
      case LAG_W_M2A: geo_add128(cell + 3, (__int128)v); break;
      case LAG_W_M2C: geo_add128(cell + 5, (__int128)v); break;
      case LAG_W_A2: geo_add128(cell + 7, (__int128)((unsigned __int128)v << (2 * LAG_SPLIT))); break;
      case LAG_W_AB: geo_add128(cell + 7, (__int128)((unsigned __int128)v << (LAG_SPLIT + 1))); break;
      case LAG_W_B2: geo_add128(cell + 7, (__int128)v); break;
      default: geo_add128(cell + 9 + 2 * (w - LAG_W_FS), (__int128)(long long)v); break;  // fs: a signed partial
    }
  }
  __syncthreads();
}

// One update (include/kmc.h): the per-protein step, the tasks' pair terms, the
// new origins.  Workgroups stride over the blocks of 256 reference indices.
// The tasks are walked in chunks of LAG_CHUNK, whose partials the LDS holds;
// the first chunk's pass advances the per-protein state and the last one's
// stores the origins (program order within the one thread that owns element i
// keeps the reads of a ring entry before its overwrite).  Per task the counts
// go by ballot and popcount and the sums by a wave reduction per class present
// in the wave, then one LDS add per wave and non-zero word.
__global__ void __launch_bounds__(LAG_T) k_lag_update(KParams P, Dev d, Lag G, LagArgs A,
                                                      const kmcl::Task* __restrict__ tasks, int nblk, lag_u64* table,
                                                      lag_u64* n_events) {
  extern __shared__ __attribute__((aligned(16))) lag_u64 lag_lds[];  // [min(ntasks, LAG_CHUNK)][5][LAG_W]
  const int N = P.N, NA = P.NA, j = threadIdx.x;
  const bool lane0 = (j & 63) == 0;
  const int nacc = min(A.ntasks, LAG_CHUNK) * LAG_CLASSES * LAG_W;
  for (int e = j; e < nacc; e += LAG_T) lag_lds[e] = 0ull;
  __syncthreads();
  lag_u64 events = 0;  // lane 0 of each wave: the events its proteins saw
  for (int t0 = 0; t0 < A.ntasks; t0 += LAG_CHUNK) {
    const int nt = min(A.ntasks - t0, LAG_CHUNK);
    const bool first = t0 == 0, last = t0 + LAG_CHUNK >= A.ntasks;
    int since = 0;
    for (int blk = blockIdx.x; blk < nblk; blk += gridDim.x) {
      const int i = blk * LAG_T + j;
      const bool in = i < N;
      longlong2 U = make_longlong2(0, 0);
      int c = -1, le = 0;
      if (in && first) {
        const int slot = d.slot_of[i];
        const longlong2 X = lag_xy(P, d, slot);
        const longlong2 pv = G.prev[i];
        const long long dx = kmcl::min_image(X.x - pv.x, A.BX), dy = kmcl::min_image(X.y - pv.y, A.BY);
        U = G.U[i];
        U.x += dx;
        U.y += dy;
        G.U[i] = U;
        G.prev[i] = X;
        int32_t l[3];
        trk_links(P, d, slot, l);
        bool ev = (dx < 0 ? -dx : dx) >= A.J || (dy < 0 ? -dy : dy) >= A.J;
        for (int k = 0; k < 3; ++k) {
          int32_t* p = &G.links[(size_t)k * N + i];
          if (*p != l[k]) {
            ev = true;
            *p = l[k];
          }
        }
        le = G.last_event[i];
        if (ev) G.last_event[i] = le = A.n;
        c = kmcl::cls(i < NA, l);
        G.cls[i] = (uint8_t)c;
        const lag_u64 ne = __popcll(__ballot(ev));
        if (lane0) events += ne;
      } else if (in) {
        U = G.U[i];
        le = G.last_event[i];
        c = G.cls[i];
      }
      // the classes present in this wave (wave-uniform)
      uint32_t present = 0;
      for (int k = 0; k < LAG_CLASSES; ++k) present |= __ballot(c == k) ? 1u << k : 0u;
      for (int t = 0; t < nt; ++t) {
        const kmcl::Task tk = tasks[t0 + t];
        uint64_t q = 0, a2 = 0, ab = 0, b2 = 0;
        long long fs[LAG_MAX_Q] = {0, 0, 0, 0};
        bool isfar = false, clean = false;
        if (in) {
          const longlong2 O = G.ring[(size_t)tk.ring * N + i];
          const long long Dx = U.x - O.x, Dy = U.y - O.y;
          isfar = kmcl::far(Dx, Dy, A.F);
          if (!isfar) {
            q = kmcl::sq(Dx, Dy);
            clean = le <= tk.nk;
            if (clean) {
              kmcl::split(q, &a2, &ab, &b2);
              for (int k = 0; k < A.nq; ++k) fs[k] = kmcl::fs_term(A.h[k], Dx, Dy, A.BX, A.BY);
            }
          }
        }
        lag_u64* acc = lag_lds + (size_t)t * LAG_CLASSES * LAG_W;
        for (int k = 0; k < LAG_CLASSES; ++k) {
          if (!(present >> k & 1u)) continue;
          const bool mine = c == k;
          lag_u64* w = acc + k * LAG_W;
          const lag_u64 n_all = __popcll(__ballot(mine && !isfar)), n_clean = __popcll(__ballot(mine && clean)),
                        n_far = __popcll(__ballot(mine && isfar));
          const lag_u64 s_all = lag_wave_sum(mine ? q : 0ull);
          if (lane0) {
            if (n_all) atomicAdd(&w[LAG_W_ALL], n_all);
            if (n_far) atomicAdd(&w[LAG_W_FAR], n_far);
            if (s_all) atomicAdd(&w[LAG_W_M2A], s_all);
          }
          if (!n_clean) continue;  // (wave-uniform)
          const bool mc = mine && clean;
          const lag_u64 s_clean = lag_wave_sum(mc ? q : 0ull), s_a2 = lag_wave_sum(mc ? a2 : 0ull),
                        s_ab = lag_wave_sum(mc ? ab : 0ull), s_b2 = lag_wave_sum(mc ? b2 : 0ull);
          if (lane0) {
            atomicAdd(&w[LAG_W_CLEAN], n_clean);
            if (s_clean) atomicAdd(&w[LAG_W_M2C], s_clean);
            if (s_a2) atomicAdd(&w[LAG_W_A2], s_a2);
            if (s_ab) atomicAdd(&w[LAG_W_AB], s_ab);
            if (s_b2) atomicAdd(&w[LAG_W_B2], s_b2);
          }
          for (int m = 0; m < A.nq; ++m) {
            const lag_u64 s_fs = lag_wave_sum(mc ? (lag_u64)fs[m] : 0ull);
            if (lane0 && s_fs) atomicAdd(&w[LAG_W_FS + m], s_fs);
          }
        }
      }
      if (in && last)
        for (int lv = 0; lv < A.L && kmcl::fires(A.n, lv); ++lv) G.ring[(size_t)kmcl::store_ring(A.n, lv, A.P) * N + i] = U;
      if (++since == LAG_FLUSH) {
        lag_flush(lag_lds, tasks + t0, nt, table);
        since = 0;
      }
    }
    lag_flush(lag_lds, tasks + t0, nt, table);
  }
  if (lane0 && events) atomicAdd(n_events, events);
}

}  // namespace kmcd
