// kmc_orient.hip — the orientation layer over the committed state (DESIGN.md
// §19): a multiple-tau correlator of the rigid bodies' own vectors (a
// receptor's heading, a ligand's axis and arm) on the lag correlator's
// schedule, and a one-shot census of the ligands' poses.  Like the other
// layers nothing here runs inside a step: the kernels are launched by
// kmc_rot_* / kmc_ligand_pose between kmc_step calls, read what kmc_get_state
// would return and write only the layer's own arrays.
//
// Everything is indexed by REFERENCE index: a thread serves one reference
// index, gathers the protein's beads and links through slot_of and streams the
// rest — its own elements of the per-protein state and of every ring entry an
// update's tasks name.  A packed array (the current words, a ring entry) holds
// [NA] headings, [NB] axes, [NB] arms: a receptor owns one word and a ligand
// two, so a wave that straddles NA holds lanes of both kinds.  A thread reads
// and writes only its own words of a ring entry, so the new origins are stored
// in the launch that correlated with the old ones.
//
// Included by kmc_engine.hip after kmc_lagcorr.hip (one translation unit, the
// library's flags); the expressions are kmc_orient.h's, shared with
// kmc_host_rot_* (kmc_host_observe.cpp); the host side of the calls is kmc_observe.hip
// §orientation.
#include "kmc_device.h"
#include "kmc_observe.h"
#include "kmc_orient.h"

namespace kmcd {

#define ROT_T 256        // threads per workgroup = one block of reference indices
#define ROT_CHUNK 64     // tasks whose partials the LDS holds at a time
#define ROT_FLUSH 32     // blocks between two flushes: 2^13 terms below 2^34 stay below 2^47
#define ROT_CELL 8       // 64-bit words of a kmc_rot_cell
// the LDS partials of one (task, class, v): two counts, s1_all, s1_clean (two's
// complement), the three parts of d²
enum { ROT_W_ALL, ROT_W_CLEAN, ROT_W_S1A, ROT_W_S1C, ROT_W_A2, ROT_W_AB, ROT_W_B2, ROT_W };
#define ROT_TASK_W (LAG_CLASSES * ROT_VECS * ROT_W)  // LDS words of one task

struct Ori {
  lag_u64* vec;         // [NA + 2 NB] the packed current vectors
  int32_t* links;       // [3][N] trk_links as of the last update
  int32_t* last_event;  // [N] the last update that saw a change of links or a flip
  int8_t* chi;          // [N] a ligand's handedness at the last update (0: a receptor, a bad ligand)
  uint8_t* cls;         // [N] class at the last update
  lag_u64* ring;        // [L * P][NA + 2 NB] the stored origins
};

struct RotArgs {
  int n, L, P, ntasks;
};

// host side: everything is allocated by kmc_rot_begin and freed by kmc_rot_end
struct RotState {
  Recorder rec;
  Scratch scratch;
  Ori dev = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
  kmcl::Task* tasks = nullptr;  // [LAG_MAX_ROWS] the update's task list
  lag_u64* table = nullptr;     // [rows][5][2][ROT_CELL]
  lag_u64* counts = nullptr;    // [3] events, flips, bad proteins of the last update
  kmc_rot_config cfg = {};
  RotArgs a = {};
  int64_t n_pairs[LAG_MAX_ROWS] = {0};
};

// the pose census' buffers, kept between the calls
struct PoseState {
  lag_u64* hist = nullptr;  // [4 * 64 * 64] bins, then 9 counters: chi = +1 [4], chi = -1 [4], bad
};
#define POSE_HIST_MAX (POSE_CLASSES * POSE_MAX_BINS * POSE_MAX_BINS)
// workgroups of k_pose: each zeroes and flushes up to 64 KiB of bins, so the grid stays at two a CU and strides
// over the blocks of 256 ligands above POSE_WG_MAX * 256 = 131 072 ligands
#define POSE_WG_MAX 512

// The packed vectors and the handedness of the protein in slot `slot`: w[0] the
// heading or the axis, w[1] the arm (0 for a receptor); both ROT_BAD and chi 0
// for a bad protein.  A receptor reads rows 8 and 9, a ligand the xy rows 0, 1,
// 2, 4 and the z rows 8, 9, 10.  Nz: the axis' z component (the pose census).
__device__ __forceinline__ bool rot_vectors(const KParams& P, const Dev& d, int slot, lag_u64 w[2], int* chi,
                                            long long* Z, long long* Nz) {
  *chi = 0;
  *Z = *Nz = 0;
  if (slot < P.NA) {
    const double2 a = d.cur.Axy(slot, 3, 1), b = d.cur.Axy(slot, 3, 2);
    const double b31[2] = {a.x, a.y}, b32[2] = {b.x, b.y};
    const kmco::V3 h = kmco::heading(b31, b32);
    const bool ok = kmco::fits(h);
    w[0] = ok ? kmco::pack(h) : ROT_BAD;
    w[1] = 0ull;
    return ok;
  }
  const int b = slot - P.NA;
  const double2 x11 = d.cur.Bxy(b, 1, 1), x12 = d.cur.Bxy(b, 1, 2), x21 = d.cur.Bxy(b, 2, 1), x31 = d.cur.Bxy(b, 3, 1);
  const double2 z8 = d.cur.B2(b, 8), z9 = d.cur.B2(b, 9), z10 = d.cur.B2(b, 10);  // (z[1][1], z[2][1]), z[1][2], z[3][1]
  const double b11[3] = {x11.x, x11.y, z8.x}, b12[3] = {x12.x, x12.y, z9.x}, b21[3] = {x21.x, x21.y, z8.y},
               b31[3] = {x31.x, x31.y, z10.x};
  const kmco::Lig g = kmco::ligand(b11, b12, b21, b31);
  const bool ok = kmco::fits(g);
  w[0] = ok ? kmco::pack(g.n) : ROT_BAD;
  w[1] = ok ? kmco::pack(g.a) : ROT_BAD;
  if (ok) *chi = kmco::chi(g.n, g.a, g.c);
  *Z = kmco::q(z8.x);
  *Nz = g.n.z;
  return ok;
}

// where reference index i keeps word v of a packed array
__device__ __forceinline__ size_t rot_at(int i, int v, int NA, int NB) {
  return i < NA ? (size_t)i : (size_t)NA + (size_t)v * NB + (size_t)(i - NA);
}

__global__ void __launch_bounds__(ROT_T) k_rot_begin(KParams P, Dev d, Ori G, int L, int slots) {
  const int i = blockIdx.x * ROT_T + threadIdx.x;
  const int N = P.N, NA = P.NA, NB = P.NB;
  if (i >= N) return;
  const int slot = d.slot_of[i];
  lag_u64 w[2];
  int chi;
  long long Z, Nz;
  rot_vectors(P, d, slot, w, &chi, &Z, &Nz);
  const size_t W = (size_t)NA + 2 * (size_t)NB;
  const int nv = i < NA ? 1 : 2;
#pragma unroll
  for (int v = 0; v < ROT_VECS; ++v) {
    if (v >= nv) continue;
    const size_t at = rot_at(i, v, NA, NB);
    G.vec[at] = w[v];
    for (int lv = 0; lv < L; ++lv) G.ring[(size_t)(lv * slots) * W + at] = w[v];  // the origin of update 0: slot 0 of every level
  }
  int32_t l[3];
  trk_links(P, d, slot, l);
  for (int k = 0; k < 3; ++k) G.links[(size_t)k * N + i] = l[k];
  G.last_event[i] = 0;
  G.chi[i] = (int8_t)chi;
  G.cls[i] = (uint8_t)kmcl::cls(i < NA, l);
}

// the workgroup's partials of nt tasks go to the table: one 64-bit or one
// carry-propagating 128-bit add per non-empty word, which is zeroed.  All 256
// threads call it; the barriers make the words whole before and free after.
__device__ __forceinline__ void rot_flush(lag_u64* acc, const kmcl::Task* __restrict__ tasks, int nt, lag_u64* table) {
  __syncthreads();
  for (int e = threadIdx.x; e < nt * ROT_TASK_W; e += ROT_T) {
    const lag_u64 v = acc[e];
    if (!v) continue;
    acc[e] = 0ull;
    const int w = e % ROT_W, cv = e / ROT_W % (LAG_CLASSES * ROT_VECS), t = e / ROT_TASK_W;
    lag_u64* cell = table + ((size_t)tasks[t].row * (LAG_CLASSES * ROT_VECS) + cv) * ROT_CELL;
    switch (w) {
      case ROT_W_ALL:
      case ROT_W_CLEAN: atomicAdd(&cell[w], v); break;
      case ROT_W_S1A: geo_add128(cell + 2, (__int128)(long long)v); break;  // a signed partial
      case ROT_W_S1C: geo_add128(cell + 4, (__int128)(long long)v); break;
      case ROT_W_A2: geo_add128(cell + 6, (__int128)((unsigned __int128)v << (2 * ROT_SPLIT))); break;
      case ROT_W_AB: geo_add128(cell + 6, (__int128)((unsigned __int128)v << (ROT_SPLIT + 1))); break;
      default: geo_add128(cell + 6, (__int128)v); break;
    }
  }
  __syncthreads();
}

// One update (include/kmc.h): the per-protein step, the tasks' pair terms, the
// new origins.  Workgroups stride over the blocks of 256 reference indices.
// The tasks are walked in chunks of ROT_CHUNK, whose partials the LDS holds;
// the first chunk's pass advances the per-protein state and the last one's
// stores the origins (program order within the one thread that owns the words
// keeps the reads of a ring entry before its overwrite).  Per task and vector
// the counts go by ballot and popcount and the sums by a wave reduction per
// class present in the wave, then one LDS add per wave and non-zero word.  A
// lane takes part in vector v only when it owns one (nv: 1 for a receptor, 2
// for a ligand), so the receptor lanes of a wave that straddles NA add nothing
// to v = 1.
__global__ void __launch_bounds__(ROT_T) k_rot_update(KParams P, Dev d, Ori G, RotArgs A,
                                                      const kmcl::Task* __restrict__ tasks, int nblk, lag_u64* table,
                                                      lag_u64* counts) {
  extern __shared__ __attribute__((aligned(16))) lag_u64 rot_lds[];  // [min(ntasks, ROT_CHUNK)][5][2][ROT_W]
  const int N = P.N, NA = P.NA, NB = P.NB, j = threadIdx.x;
  const size_t W = (size_t)NA + 2 * (size_t)NB;
  const bool lane0 = (j & 63) == 0;
  const int nacc = min(A.ntasks, ROT_CHUNK) * ROT_TASK_W;
  for (int e = j; e < nacc; e += ROT_T) rot_lds[e] = 0ull;
  __syncthreads();
  lag_u64 events = 0, flips = 0, bads = 0;  // lane 0 of each wave: what its proteins saw
  const int npass = A.ntasks > 0 ? (A.ntasks + ROT_CHUNK - 1) / ROT_CHUNK : 1;  // (an update without a task still advances the state)
  for (int pass = 0; pass < npass; ++pass) {
    const int t0 = pass * ROT_CHUNK;
    const int nt = max(0, min(A.ntasks - t0, ROT_CHUNK));
    const bool first = pass == 0, last = pass == npass - 1;
    int since = 0;
    for (int blk = blockIdx.x; blk < nblk; blk += gridDim.x) {
      const int i = blk * ROT_T + j;
      const bool in = i < N;
      const int nv = !in ? 0 : i < NA ? 1 : 2;
      lag_u64 w[2] = {ROT_BAD, ROT_BAD};
      int c = -1, le = 0;
      if (in && first) {
        const int slot = d.slot_of[i];
        int chi;
        long long Z, Nz;
        const bool ok = rot_vectors(P, d, slot, w, &chi, &Z, &Nz);
#pragma unroll
        for (int v = 0; v < ROT_VECS; ++v)
          if (v < nv) G.vec[rot_at(i, v, NA, NB)] = w[v];
        int32_t l[3];
        trk_links(P, d, slot, l);
        const bool flip = G.chi[i] != (int8_t)chi;
        if (flip) G.chi[i] = (int8_t)chi;
        bool ev = flip;
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
        const lag_u64 ne = __popcll(__ballot(ev)), nf = __popcll(__ballot(flip)), nb = __popcll(__ballot(!ok));
        if (lane0) {
          events += ne;
          flips += nf;
          bads += nb;
        }
      } else if (in) {
#pragma unroll
        for (int v = 0; v < ROT_VECS; ++v)
          if (v < nv) w[v] = G.vec[rot_at(i, v, NA, NB)];
        le = G.last_event[i];
        c = G.cls[i];
      }
      const bool ok = in && !(w[0] & ROT_BAD);
      const kmco::V3 u0 = kmco::unpack(w[0]), u1 = kmco::unpack(w[1]);
      // the classes present in this wave (wave-uniform)
      uint32_t present = 0;
      for (int k = 0; k < LAG_CLASSES; ++k) present |= __ballot(c == k) ? 1u << k : 0u;
      for (int t = 0; t < nt; ++t) {
        const kmcl::Task tk = tasks[t0 + t];
        const bool clean = le <= tk.nk;
        long long dv[2] = {0, 0};
        bool filed[2] = {false, false};
#pragma unroll
        for (int v = 0; v < ROT_VECS; ++v) {
          if (v >= nv) continue;
          const lag_u64 o = G.ring[(size_t)tk.ring * W + rot_at(i, v, NA, NB)];
          filed[v] = ok && !(o & ROT_BAD);
          if (filed[v]) dv[v] = kmco::dot(v ? u1 : u0, kmco::unpack(o));
        }
        lag_u64* acc = rot_lds + (size_t)t * ROT_TASK_W;
        for (int k = 0; k < LAG_CLASSES; ++k) {
          if (!(present >> k & 1u)) continue;
#pragma unroll
          for (int v = 0; v < ROT_VECS; ++v) {
            if (v && k < 3) continue;  // (a receptor class has the heading alone)
            const bool mine = c == k && filed[v];
            lag_u64* wd = acc + (k * ROT_VECS + v) * ROT_W;
            const lag_u64 n_all = __popcll(__ballot(mine));
            if (!n_all) continue;  // (wave-uniform)
            const bool mc = mine && clean;
            const lag_u64 n_clean = __popcll(__ballot(mc));
            const lag_u64 s_all = lag_wave_sum(mine ? (lag_u64)dv[v] : 0ull);
            if (lane0) {
              atomicAdd(&wd[ROT_W_ALL], n_all);
              if (s_all) atomicAdd(&wd[ROT_W_S1A], s_all);
            }
            if (!n_clean) continue;  // (wave-uniform)
            uint64_t a2 = 0, ab = 0, b2 = 0;
            if (mc) kmco::split(dv[v], &a2, &ab, &b2);
            const lag_u64 s_clean = lag_wave_sum(mc ? (lag_u64)dv[v] : 0ull), s_a2 = lag_wave_sum(a2),
                          s_ab = lag_wave_sum(ab), s_b2 = lag_wave_sum(b2);
            if (lane0) {
              atomicAdd(&wd[ROT_W_CLEAN], n_clean);
              if (s_clean) atomicAdd(&wd[ROT_W_S1C], s_clean);
              if (s_a2) atomicAdd(&wd[ROT_W_A2], s_a2);
              if (s_ab) atomicAdd(&wd[ROT_W_AB], s_ab);
              if (s_b2) atomicAdd(&wd[ROT_W_B2], s_b2);
            }
          }
        }
      }
      if (last)
#pragma unroll
        for (int v = 0; v < ROT_VECS; ++v)
          for (int lv = 0; v < nv && lv < A.L && kmcl::fires(A.n, lv); ++lv)
            G.ring[(size_t)kmcl::store_ring(A.n, lv, A.P) * W + rot_at(i, v, NA, NB)] = w[v];
      if (++since == ROT_FLUSH) {
        rot_flush(rot_lds, tasks + t0, nt, table);
        since = 0;
      }
    }
    rot_flush(rot_lds, tasks + t0, nt, table);
  }
  if (lane0) {
    if (events) atomicAdd(&counts[0], events);
    if (flips) atomicAdd(&counts[1], flips);
    if (bads) atomicAdd(&counts[2], bads);
  }
}

// The pose census (include/kmc.h): one thread a ligand by reference index, the
// bins in 32-bit LDS words (a workgroup sees fewer than 2^31 ligands), the
// handedness and bad counts by ballot into lane 0's registers.  Workgroups
// stride over the blocks of 256 ligands.
__global__ void __launch_bounds__(ROT_T) k_pose(KParams P, Dev d, int nz, int nc, long long BZ, long long Lq, int nblk,
                                                lag_u64* hist, lag_u64* counts) {
  extern __shared__ __attribute__((aligned(16))) uint32_t pose_lds[];  // [4][nz][nc]
  const int NA = P.NA, NB = P.NB, j = threadIdx.x;
  const int nbin = POSE_CLASSES * nz * nc;
  const bool lane0 = (j & 63) == 0;
  for (int e = j; e < nbin; e += ROT_T) pose_lds[e] = 0u;
  __syncthreads();
  lag_u64 pos[POSE_CLASSES] = {0, 0, 0, 0}, neg[POSE_CLASSES] = {0, 0, 0, 0}, bads = 0;
  for (int blk = blockIdx.x; blk < nblk; blk += gridDim.x) {
    const int b = blk * ROT_T + j;
    const bool in = b < NB;
    int k = -1, chi = 0;
    bool ok = false;
    if (in) {
      const int slot = d.slot_of[NA + b];
      lag_u64 w[2];
      long long Z, Nz;
      ok = rot_vectors(P, d, slot, w, &chi, &Z, &Nz);
      int32_t l[3];
      trk_links(P, d, slot, l);
      k = (l[0] != 0) + (l[1] != 0) + (l[2] != 0);
      if (ok) atomicAdd(&pose_lds[(k * nz + kmco::pose_zbin(Z, BZ, nz)) * nc + kmco::pose_tbin(Nz, Lq, nc)], 1u);
    }
    const lag_u64 nb = __popcll(__ballot(in && !ok));
    if (lane0) bads += nb;
#pragma unroll
    for (int c = 0; c < POSE_CLASSES; ++c) {
      const lag_u64 np = __popcll(__ballot(k == c && chi > 0)), nn = __popcll(__ballot(k == c && chi < 0));
      if (lane0) {
        pos[c] += np;
        neg[c] += nn;
      }
    }
  }
  __syncthreads();
  for (int e = j; e < nbin; e += ROT_T)
    if (pose_lds[e]) atomicAdd(&hist[e], (lag_u64)pose_lds[e]);
  if (lane0) {
#pragma unroll
    for (int c = 0; c < POSE_CLASSES; ++c) {
      if (pos[c]) atomicAdd(&counts[c], pos[c]);
      if (neg[c]) atomicAdd(&counts[POSE_CLASSES + c], neg[c]);
    }
    if (bads) atomicAdd(&counts[2 * POSE_CLASSES], bads);
  }
}

}  // namespace kmcd
