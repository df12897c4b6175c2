// kmc_bodydyn.hip — body dynamics over the committed state:
// per cluster of the origin (a BODY: a connected component of the bond graph at
// kmc_bd_begin) the displacement of its centre, its rigid rotation and its
// fate, filed by (holds a ligand, size).  Like the pair dynamics nothing here
// runs inside a step: the kernels are launched by kmc_bd_* between kmc_step
// calls, read what kmc_get_state would return and write only the recorder's
// own arrays.
//
// Membership is static after the begin, so the sample does not add members to
// their root with atomics as k_geo_moments does.  The begin sorts the members
// by body into a list (count / bins_scan / scatter, the body's label as the
// key) and keeps ΣD0 and Σ|D0|² per body; the sample is a segmented reduction
// over that list:
//   k_bd_reduce  a wave takes a fixed span of 64 consecutive list entries,
//                whatever bodies they belong to — work is balanced by entries,
//                a huge body is split over many waves — gathers the members'
//                state through the list, finds the segment heads by ballot and
//                runs a wave-level segmented scan (shuffles) of Σu, ΣD0.u,
//                ΣD0×u, the OR of the flags and the extremes of the current
//                label.  A body that lies within the span is written with plain
//                stores; only the segments open at the span's ends go to the
//                body's (zero) accumulators with 64-bit atomics.
//   k_bd_finish  a thread per body: the root correction, the verdict, the
//                angle, and the table through bins privatised in LDS.
// Every sum is an integer sum modulo 2^64 or 2^128, so no result depends on an
// order: not on the order of a body's members in the list (their ranks come
// from an atomic counter) and not on the order of the atomics.
//
// Included by kmc_engine.hip after kmc_pairdyn.hip (one translation unit, the
// library's flags); the expressions are kmc_bodydyn.h's, shared with
// kmc_host_bd_* (kmc_host_observe.cpp); the host side of the calls is kmc_observe.hip
// §body dynamics.
#include "kmc_bodydyn.h"
#include "kmc_device.h"
#include "kmc_observe.h"

namespace kmcd {

#define BD_T 256   // threads per workgroup
#define BD_SPAN 64 // list entries a wave takes at a time (KMC_DEBUG_BD_SPAN lowers it)
#define BD_ACC 7   // 64-bit words per body: Σu.x, Σu.y, ΣD0.u, ΣD0×u, OR, max(L + 1), max(N − L)
#define BD_OUT 4   // words of Bd::out: newly jumped, newly changed, rows (the list's cursor), bodies

typedef unsigned long long bd_u64;

struct Bd {
  longlong2* prev;  // [N] integer position at the last update
  longlong2* U;     // [N] unwrapped integer position
  longlong2* X0;    // [N] position at the begin
  longlong2* D0;    // [N] unwrapped position against the root at the begin
  int32_t* links;   // [3][N] trk_links as of the last update
  uint8_t* flags;   // [N] BD_JUMPED | BD_CHANGED
  int32_t* label;   // [N] the body: its root, 0-based
  int32_t* list;    // [N] the members sorted by body
  int32_t* rank;    // [N] a member's place within its body
  int32_t* ccnt;    // [N + 1] members by root
  int32_t* start;   // [N + 1] their scan: a body's first list entry, by root
  int32_t* part;    // the scan's tile sums
  bd_u64* sd0;      // [N][2] ΣD0 by root
  bd_u64* sd2;      // [N] Σ|D0|² by root
  bd_u64* cnt;      // [N] receptors | ligands << 32 by root
  uint32_t* bits;   // [N] spanning bits | BD_WIDE by root
  bd_u64* acc;      // [N][BD_ACC] the sample's sums by root; zero between two calls
  bd_u64* table;    // [2][BD_MAX_SIZE + 1][BD_CELL_WORDS]
  bd_u64* out;      // [BD_OUT]
};

// host side: everything is allocated by kmc_bd_begin and freed by kmc_bd_end
struct BdState {
  Recorder rec;
  Scratch scratch;
  Bd dev = {};
  kmc_bd_body* rows = nullptr;  // [rows_cap] kmc_bd_bodies' rows (in the scratch group)
  size_t rows_cap = 0;
  kmc_bd_config cfg = {};
  long long J = 0, F = 0, BX = 0, BY = 0;
  int64_t n_bodies = 0;
  int span = BD_SPAN;  // KMC_DEBUG_BD_SPAN: shorter spans (the open-segment path at test size)
};

// update 0: the per-protein state, D0 and the body's static sums, the member's rank
__global__ void __launch_bounds__(BD_T) k_bd_begin(KParams P, Dev d, Bd D, const int32_t* __restrict__ glabel,
                                                   const int2* __restrict__ goff, const uint32_t* __restrict__ gspan,
                                                   const geo_u64* __restrict__ gcnt, long long BX, long long BY) {
  const int i = blockIdx.x * BD_T + threadIdx.x;
  const int N = P.N;
  bool root = false;
  if (i < N) {
    const int slot = d.slot_of[i];
    const longlong2 X = lag_xy(P, d, slot);
    D.prev[i] = X;
    D.U[i] = X;
    D.X0[i] = X;
    D.flags[i] = 0;
    int32_t l[3];
    trk_links(P, d, slot, l);
    for (int k = 0; k < 3; ++k) D.links[(size_t)k * N + i] = l[k];
    const int r = glabel[i];
    root = r == i;
    const uint32_t sp = gspan[r];
    const int2 o = sp ? make_int2(0, 0) : goff[i];  // (a spanning body's shifts depend on the tree: zero, as kmc_unwrap)
    const longlong2 Xr = lag_xy(P, d, d.slot_of[r]);
    const long long dx = X.x + (long long)o.x * BX - Xr.x, dy = X.y + (long long)o.y * BY - Xr.y;
    D.label[i] = r;
    D.D0[i] = make_longlong2(dx, dy);
    if (dx) atomicAdd(&D.sd0[2 * (size_t)r], (bd_u64)dx);
    if (dy) atomicAdd(&D.sd0[2 * (size_t)r + 1], (bd_u64)dy);
    if (dx | dy) atomicAdd(&D.sd2[r], kmcb::dot(dx, dy, dx, dy));
    if (kmcb::wide(dx, dy)) atomicOr(&D.bits[r], (uint32_t)BD_WIDE);
    if (root) {
      if (sp) atomicOr(&D.bits[r], sp);
      D.cnt[r] = gcnt[r];
    }
    D.rank[i] = atomicAdd(&D.ccnt[r], 1);
  }
  const bd_u64 nroot = __popcll(__ballot(root));
  if ((threadIdx.x & 63) == 0 && nroot) atomicAdd(&D.out[3], nroot);
}

__global__ void __launch_bounds__(BD_T) k_bd_scatter(int N, Bd D) {
  const int i = blockIdx.x * BD_T + threadIdx.x;
  if (i >= N) return;
  D.list[D.start[D.label[i]] + D.rank[i]] = i;
}

// The per-protein step (include/kmc.h): workgroups stride over the blocks of
// 256 reference indices, position and links gathered through slot_of.
__global__ void __launch_bounds__(BD_T) k_bd_update(KParams P, Dev d, Bd D, long long BX, long long BY, long long J,
                                                    int nblk) {
  const int N = P.N;
  bd_u64 jumped = 0, changed = 0;  // lane 0 of each wave: the proteins newly flagged
  for (int blk = blockIdx.x; blk < nblk; blk += gridDim.x) {
    const int i = blk * BD_T + threadIdx.x;
    bool nj = false, nc = false;
    if (i < N) {
      const int slot = d.slot_of[i];
      const longlong2 X = lag_xy(P, d, slot);
      const longlong2 pv = D.prev[i];
      const long long dx = kmcl::min_image(X.x - pv.x, BX), dy = kmcl::min_image(X.y - pv.y, BY);
      longlong2 U = D.U[i];
      U.x += dx;
      U.y += dy;
      D.U[i] = U;
      D.prev[i] = X;
      int32_t l[3];
      trk_links(P, d, slot, l);
      int f = 0;
      if ((dx < 0 ? -dx : dx) >= J || (dy < 0 ? -dy : dy) >= J) f |= BD_JUMPED;
      for (int k = 0; k < 3; ++k) {
        int32_t* p = &D.links[(size_t)k * N + i];
        if (*p != l[k]) {
          f |= BD_CHANGED;
          *p = l[k];
        }
      }
      const int old = D.flags[i];
      if (f & ~old) D.flags[i] = (uint8_t)(old | f);
      nj = f & ~old & BD_JUMPED;
      nc = f & ~old & BD_CHANGED;
    }
    const bd_u64 a = __popcll(__ballot(nj)), b = __popcll(__ballot(nc));
    if ((threadIdx.x & 63) == 0) {
      jumped += a;
      changed += b;
    }
  }
  if ((threadIdx.x & 63) == 0) {
    if (jumped) atomicAdd(&D.out[0], jumped);
    if (changed) atomicAdd(&D.out[1], changed);
  }
}

// v of the lane o below, added when that lane still belongs to this lane's segment
__device__ __forceinline__ bd_u64 bd_seg_add(bd_u64 v, int o, bool in) {
  const bd_u64 t = __shfl_up(v, o);
  return in ? v + t : v;
}

// The segmented reduction (see the head of the file).  cur is the current
// component label by reference index (0-based).  A wave strides over the spans;
// lanes at and above `span`, and past the list's end, hold no entry: each is a
// segment of its own that is never written.
__global__ void __launch_bounds__(BD_T) k_bd_reduce(Bd D, const int32_t* __restrict__ cur, int N, int span, long long F,
                                                    int nspans) {
  const int lane = threadIdx.x & 63;
  const int nwaves = gridDim.x * (BD_T / 64);
  for (int sp = blockIdx.x * (BD_T / 64) + (threadIdx.x >> 6); sp < nspans; sp += nwaves) {
    const long long e = (long long)sp * span + lane;
    const bool act = lane < span && e < N;
    int lab = -1 - lane;
    bd_u64 sux = 0, suy = 0, sdu = 0, scu = 0;
    uint32_t ob = 0, l1 = 0, nl = 0;
    if (act) {
      const int i = D.list[e];
      lab = D.label[i];
      const longlong2 U = D.U[i], X0 = D.X0[i], D0 = D.D0[i];
      const long long ux = U.x - X0.x, uy = U.y - X0.y;
      const int L = cur[i];
      sux = (bd_u64)ux;
      suy = (bd_u64)uy;
      sdu = kmcb::dot(D0.x, D0.y, ux, uy);
      scu = kmcb::cross(D0.x, D0.y, ux, uy);
      ob = (uint32_t)kmcb::member_bits(D.flags[i], ux, uy, F);
      l1 = (uint32_t)L + 1u;
      nl = (uint32_t)(N - L);
    }
    const int below = __shfl_up(lab, 1);
    const bool head = lane == 0 || below != lab;
    const bd_u64 hm = __ballot(head);
    const int h = 63 - __clzll(hm & (~0ull >> (63 - lane)));  // the head lane of this lane's segment
    for (int o = 1; o < 64; o <<= 1) {
      const bool in = lane - o >= h;
      sux = bd_seg_add(sux, o, in);
      suy = bd_seg_add(suy, o, in);
      sdu = bd_seg_add(sdu, o, in);
      scu = bd_seg_add(scu, o, in);
      const uint32_t tb = __shfl_up(ob, o), t1 = __shfl_up(l1, o), tn = __shfl_up(nl, o);
      if (in) {
        ob |= tb;
        l1 = max(l1, t1);
        nl = max(nl, tn);
      }
    }
    const bool tail = lane == 63 || (hm >> (lane + 1) & 1ull);  // the segment's last lane holds its totals
    if (!act || !tail) continue;
    const long long st = D.start[lab], end = D.start[lab + 1];  // (a non-root counts no member: the next root's start)
    bd_u64* a = D.acc + (size_t)lab * BD_ACC;
    if (e - (lane - h) == st && e + 1 == end) {  // the whole body lies in this span
      a[0] = sux;
      a[1] = suy;
      a[2] = sdu;
      a[3] = scu;
      a[4] = ob;
      a[5] = l1;
      a[6] = nl;
    } else {
      if (sux) atomicAdd(&a[0], sux);
      if (suy) atomicAdd(&a[1], suy);
      if (sdu) atomicAdd(&a[2], sdu);
      if (scu) atomicAdd(&a[3], scu);
      if (ob) atomicOr(&a[4], (bd_u64)ob);
      atomicMax(&a[5], (bd_u64)l1);
      atomicMax(&a[6], (bd_u64)nl);
    }
  }
}

// The sums of root r after k_bd_reduce, and the accumulators of a body that
// the atomics served back to zero (a body within one span is overwritten whole
// by the next reduce).  curcnt: the current components' packed member counts.
__device__ __forceinline__ kmcb::Sums bd_sums(const Bd& D, const bd_u64* __restrict__ curcnt, int r, int N, int span) {
  kmcb::Sums b;
  const bd_u64 c = D.cnt[r];
  b.n = (int)(uint32_t)c + (int)(c >> 32);
  b.bits = (int)D.bits[r];
  bd_u64* a = D.acc + (size_t)r * BD_ACC;
  b.sux = a[0];
  b.suy = a[1];
  b.sdu = a[2];
  b.scu = a[3];
  b.orbits = (int)a[4];
  b.lmax = min(max((int)a[5] - 1, 0), N - 1);  // (every body has a member, so both were written: the clamps
  b.lmin = min(max(N - (int)a[6], 0), N - 1);  // only keep the read below in bounds whatever the words hold)
  const int st = D.start[r];
  if (st / span != (st + b.n - 1) / span)
    for (int k = 0; k < BD_ACC; ++k) a[k] = 0ull;
  const bd_u64 cc = curcnt[b.lmin];
  b.cur_size = (int)(uint32_t)cc + (int)(cc >> 32);
  b.sd0x = D.sd0[2 * (size_t)r];
  b.sd0y = D.sd0[2 * (size_t)r + 1];
  b.sd2 = D.sd2[r];
  const longlong2 U = D.U[r], X0 = D.X0[r];
  b.urx = U.x - X0.x;
  b.ury = U.y - X0.y;
  return b;
}

// A thread per body (the roots among the reference indices, grid-stride): the
// verdict, the rotation terms, and the table through LDS bins — all 2 x
// (max_size + 1) cells of 16 words, up to 64 KiB — flushed once per workgroup:
// one add per non-empty count, geo_add128 per 128-bit sum.
__global__ void __launch_bounds__(BD_T) k_bd_finish(Bd D, const bd_u64* __restrict__ curcnt, int N, int max_size,
                                                    int span) {
  extern __shared__ __attribute__((aligned(16))) bd_u64 bd_lds[];  // [2][max_size + 1][BD_CELL_WORDS]
  const int nword = 2 * (max_size + 1) * BD_CELL_WORDS;
  for (int e = threadIdx.x; e < nword; e += BD_T) bd_lds[e] = 0ull;
  __syncthreads();
  for (int r = blockIdx.x * BD_T + threadIdx.x; r < N; r += gridDim.x * BD_T) {
    if (D.label[r] != r) continue;
    const kmcb::Sums b = bd_sums(D, curcnt, r, N, span);
    const kmcb::Verdict v = kmcb::verdict(b);
    const int hl = (D.cnt[r] >> 32) != 0;
    bd_u64* w = bd_lds + ((size_t)hl * (max_size + 1) + min(b.n, max_size)) * BD_CELL_WORDS;
    atomicAdd(&w[BD_W_BODIES], 1ull);
    atomicAdd(&w[BD_W_SIZE], (bd_u64)b.n);
    atomicAdd(&w[BD_W_INTACT + v.status], 1ull);
    if (v.is & BD_IS_PRISTINE) atomicAdd(&w[BD_W_PRISTINE], 1ull);
    if (!(v.is & BD_IS_VALID)) continue;
    atomicAdd(&w[BD_W_VALID], 1ull);
    geo_add128(w + BD_W_M2, (__int128)kmcb::trans_term(v.sux, v.suy));
    if (!(v.is & BD_IS_ROT)) {
      if (b.n >= 2) atomicAdd(&w[BD_W_SKIPPED], 1ull);
      continue;
    }
    if (v.C == 0 && v.S == 0) {
      atomicAdd(&w[BD_W_NULL], 1ull);
      continue;
    }
    int64_t c1, c2, p;
    kmcb::rot_terms(v.C, v.S, &c1, &c2, &p);
    atomicAdd(&w[BD_W_ROT], 1ull);
    if (c1) atomicAdd(&w[BD_W_C1], (bd_u64)c1);
    if (c2) atomicAdd(&w[BD_W_C2], (bd_u64)c2);
    geo_add128(w + BD_W_PHI2, (__int128)(p * p));
  }
  __syncthreads();
  for (int e = threadIdx.x; e < nword; e += BD_T) {
    const int k = e % BD_CELL_WORDS;
    if (k == BD_W_M2 + 1 || k == BD_W_PHI2 + 1) continue;  // the high word goes with the low one
    if (k == BD_W_M2 || k == BD_W_PHI2) {
      const __int128 v = geo_ld128(bd_lds + e);
      if (v) geo_add128(D.table + e, v);
    } else if (bd_lds[e]) {
      atomicAdd(&D.table[e], bd_lds[e]);
    }
  }
}

// the bodies of at least min_size members, appended through one cursor (its
// final value is the true count; rows past cap are not written)
__global__ void __launch_bounds__(BD_T) k_bd_rows(Bd D, const bd_u64* __restrict__ curcnt, int N, int span,
                                                  int min_size, long long cap, kmc_bd_body* rows) {
  const int r = blockIdx.x * BD_T + threadIdx.x;
  if (r >= N || D.label[r] != r) return;
  const kmcb::Sums b = bd_sums(D, curcnt, r, N, span);  // (every body: the open accumulators go back to zero)
  if (b.n < min_size) return;
  const bd_u64 at = atomicAdd(&D.out[2], 1ull);
  if (at >= (bd_u64)cap) return;
  const kmcb::Verdict v = kmcb::verdict(b);
  const bd_u64 c = D.cnt[r];
  kmc_bd_body o;
  o.label = r + 1;
  o.n_r = (int32_t)(uint32_t)c;
  o.n_l = (int32_t)(c >> 32);
  o.bits = b.bits;
  o.status = v.status;
  o.is = v.is;
  o.cur_label = b.lmin + 1;
  o.cur_size = b.cur_size;
  o.su[0] = v.sux;
  o.su[1] = v.suy;
  o.C = v.C;
  o.S = v.S;
  rows[at] = o;
}

}  // namespace kmcd
