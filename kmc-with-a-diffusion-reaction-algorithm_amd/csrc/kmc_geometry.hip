// kmc_geometry.hip — cluster geometry of the committed state:
// a periodic image shift for every protein, the spanning bits of every
// component and the exact integer moments of the unwrapped components.  Like
// kmc_analysis.hip the kernels are read-only over the state (Dev::cur, a_int /
// b_int, id_of), name proteins by their reference index and run in a fixed
// number of launches whatever the shape of the clusters.
//
// Included by kmc_engine.hip after kmc_analysis.hip, whose prot_links and an_xy
// it uses (one translation unit, the library's flags: -ffp-contract=off, so the
// edge shift below is the quotient and the rounding include/kmc.h writes down
// and nothing else); the host side of the calls is kmc_observe.hip §cluster
// geometry.
#include "kmc_device.h"

namespace kmcd {

// device-side results of one geometry call
struct GeoOut {
  unsigned long long n_measured, n_spanning, n_span_x, n_span_y, proteins_in_spanning;
  unsigned long long best;    // as AnOut::best: size << 32 | (0xffffffff − root)
  unsigned long long n_rows;  // list kernel: the roots that qualify (the cursor; may exceed the capacity)
  uint32_t err;               // 1: a loop ran out of its bound or a link left [1, N]; 2: an offset left int16
  uint32_t pad;
};

#define GEO_ACC 8            // 64-bit words per root: S1x, S1y, then (lo, hi) of S2xx, S2yy, S2xy
#define GEO_BIN 4            // 64-bit words per table bin: count, sum of sizes, (lo, hi) of the sum of m
#define GEO_MAX_SIZE 1023    // KMC_GEOM_MAX_SIZE: 1024 bins of 32 B = 32 KiB of LDS per workgroup
#define GEO_OFF_MAX 32767    // image shifts are int16
#define GEO_TABLE_WG 256     // workgroups of the table kernel: each ends with a handful of atomics on the same few
                             // words of GeoOut, which one device-scope line takes at ≈90 per µs only

typedef unsigned long long geo_u64;

// host side: scratch of the first geometry call, its own (an interleaved
// kmc_components / census / track_* call touches none of it)
struct GeoState {
  geo_u64 *word = nullptr, *cnt = nullptr;   // [N] (parent, rel) words; packed member counts by root
  geo_u64 *acc = nullptr, *table = nullptr;  // [N][GEO_ACC] moments by root; [GEO_MAX_SIZE + 1][GEO_BIN] bins
  longlong2* X = nullptr;                    // [N] integer coordinates
  int32_t* label = nullptr;
  int2* off = nullptr;       // [N] image shift against the root
  uint32_t* span = nullptr;  // [N] spanning bits by root
  GeoOut* out = nullptr;
  kmc_cluster* rows = nullptr;  // [rows_cap] kmc_cluster_list's rows
  size_t rows_cap = 0;
};

// one vertex word: parent << 32 | (uint16) rel_x << 16 | (uint16) rel_y, rel = off(vertex) − off(parent)
__device__ __forceinline__ geo_u64 geo_pack(int parent, int rx, int ry) {
  return (geo_u64)(uint32_t)parent << 32 | (geo_u64)(uint16_t)(int16_t)rx << 16 | (geo_u64)(uint16_t)(int16_t)ry;
}
__device__ __forceinline__ int geo_parent(geo_u64 w) { return (int)(uint32_t)(w >> 32); }
__device__ __forceinline__ int geo_rx(geo_u64 w) { return (int)(int16_t)(uint16_t)(w >> 16); }
__device__ __forceinline__ int geo_ry(geo_u64 w) { return (int)(int16_t)(uint16_t)w; }
__device__ __forceinline__ bool geo_fits(int v) { return v >= -GEO_OFF_MAX && v <= GEO_OFF_MAX; }

// relaxed 64-bit accesses: a (parent, rel) pair is always read and written whole
__device__ __forceinline__ geo_u64 geo_ld(const geo_u64* p) {
  return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ void geo_st(geo_u64* p, geo_u64 v) {
  __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// w[0..1] += v as one 128-bit two's-complement number, without a lock: the low
// word's add returns what it replaced, so exactly the adds that wrap it carry
// one into the high word.  Additions commute modulo 2^128: the total does not
// depend on their order.  Works on global and on LDS words.
__device__ __forceinline__ void geo_add128(geo_u64* w, __int128 v) {
  const geo_u64 lo = (geo_u64)(unsigned __int128)v, hi = (geo_u64)((unsigned __int128)v >> 64);
  geo_u64 carry = 0;
  if (lo) {
    const geo_u64 old = atomicAdd(&w[0], lo);
    carry = (geo_u64)(old + lo < old);
  }
  if (hi + carry) atomicAdd(&w[1], hi + carry);
}
__device__ __forceinline__ __int128 geo_ld128(const geo_u64* w) {
  return (__int128)((unsigned __int128)w[1] << 64 | (unsigned __int128)w[0]);
}

// n(i→j) = −(int) round_((x_j − x_i) / box), per axis (include/kmc.h)
__device__ __forceinline__ int geo_edge(double xi, double xj, double box, uint32_t* err) {
  const double r = kmcm::round_((xj - xi) / box);
  if (!(r >= -(double)GEO_OFF_MAX && r <= (double)GEO_OFF_MAX)) {
    atomicOr(err, 2u);
    return 0;
  }
  return -(int)r;
}

// ------------------------------------------------------------ weighted union-find
// As the components of kmc_analysis.hip — parent[x] <= x, a root is hooked under
// a smaller root only, every chain descends and ends at the smallest member —
// with one addition: the word of a non-root also holds off(x) − off(parent).
// A root's word is (self, 0, 0); the one CAS that hooks it defines its offset
// against the other tree for good, so from then on off(x) − off(y) of any two
// vertices of one tree is a fixed number, whichever path is summed.

// one slot per thread: the integer coordinates, and every per-vertex word of a call
__global__ void __launch_bounds__(AN_T) k_geo_init(KParams P, Dev d, geo_u64* word, longlong2* X, geo_u64* cnt,
                                                   uint32_t* span, geo_u64* acc) {
  const int p = blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= P.N) return;
  const int i = d.id_of[p];
  const double2 xy = an_xy(P, d, p);
  word[i] = geo_pack(i, 0, 0);
  X[i] = make_longlong2((long long)kmcm::round_(xy.x * 1024.0), (long long)kmcm::round_(xy.y * 1024.0));
  cnt[i] = 0ull;
  span[i] = 0u;
  for (int k = 0; k < GEO_ACC; ++k) acc[(size_t)i * GEO_ACC + k] = 0ull;
}

// Walks x to its root, adding off(x) − off(root) to (ox, oy), and halves the
// path: x is re-pointed at its grandparent with the sum of the two rels.  x is
// not a root then, a non-root never becomes one again and its offset against
// any ancestor is fixed, so whichever of two racing stores lands last, the
// word holds an ancestor and the true offset against it.
__device__ __forceinline__ bool geo_find(geo_u64* word, int& x, int& ox, int& oy, int N, uint32_t* err) {
  for (int it = 0; it <= N; ++it) {
    const geo_u64 w = geo_ld(&word[x]);
    const int p = geo_parent(w);
    if (p == x) return true;
    const geo_u64 wp = geo_ld(&word[p]);
    const int g = geo_parent(wp);
    const int rx = geo_rx(w) + geo_rx(wp), ry = geo_ry(w) + geo_ry(wp);  // a root's rel is (0, 0)
    if (g != p) {
      if (geo_fits(rx) && geo_fits(ry)) geo_st(&word[x], geo_pack(g, rx, ry));
      else atomicOr(err, 2u);
    }
    ox += rx;
    oy += ry;
    x = g;
  }
  atomicOr(err, 1u);
  return false;
}

// joins the trees of a and b so that off(b) − off(a) = (nx, ny); when they are
// one tree already nothing is written (k_geo_check compares the edge later)
__device__ __forceinline__ void geo_unite(geo_u64* word, int a, int b, int nx, int ny, int N, uint32_t* err) {
  int ax = 0, ay = 0, bx = 0, by = 0;  // off(first a) − off(a), off(first b) − off(b)
  for (int it = 0; it <= N; ++it) {
    if (!geo_find(word, a, ax, ay, N, err) || !geo_find(word, b, bx, by, N, err)) return;
    if (a == b) return;
    int hi, lo, rx, ry;  // rel = off(hi) − off(lo)
    if (a > b) {
      hi = a, lo = b, rx = bx - ax - nx, ry = by - ay - ny;
    } else {
      hi = b, lo = a, rx = ax - bx + nx, ry = ay - by + ny;
    }
    if (!geo_fits(rx) || !geo_fits(ry)) {
      atomicOr(err, 2u);
      return;
    }
    const geo_u64 self = geo_pack(hi, 0, 0);
    if (atomicCAS(&word[hi], self, geo_pack(lo, rx, ry)) == self) return;  // else: hi was hooked meanwhile, find on
  }
  atomicOr(err, 1u);
}

// the <= 3 neighbour slots of slot p (0-based; −1 none), false when a link leaves [1, N]
__device__ __forceinline__ bool geo_links(const KParams& P, const Dev& d, int p, int* nb) {
  prot_links(P, d, p, nb);
  bool ok = true;
  for (int e = 0; e < 3; ++e) {
    if (nb[e] < 0 || nb[e] > P.N) {
      ok = false;
      nb[e] = 0;
    }
    nb[e] -= 1;
  }
  return ok;
}

// one vertex (slot p) per thread: unite with its neighbours, carrying the edge shift
__global__ void __launch_bounds__(AN_T) k_geo_hook(KParams P, Dev d, geo_u64* word, GeoOut* out) {
  const int p = blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= P.N) return;
  int nb[3];
  if (!geo_links(P, d, p, nb)) atomicOr(&out->err, 1u);
  const int me = d.id_of[p];
  const double2 xi = an_xy(P, d, p);
  for (int e = 0; e < 3; ++e) {
    if (nb[e] < 0) continue;
    const double2 xj = an_xy(P, d, nb[e]);
    const int nx = geo_edge(xi.x, xj.x, P.box_x, &out->err), ny = geo_edge(xi.y, xj.y, P.box_y, &out->err);
    geo_unite(word, me, d.id_of[nb[e]], nx, ny, P.N, &out->err);
  }
}

// after the hooks every root is final: label[i], off(i) against the root (the
// component's smallest index, whose offset is (0, 0)) and the roots' packed
// member counts (receptors low word, ligands high word)
__global__ void __launch_bounds__(AN_T) k_geo_flatten(const geo_u64* __restrict__ word, int32_t* label, int2* off,
                                                      geo_u64* cnt, int NA, int N, GeoOut* out) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= N) return;
  int x = i, ox = 0, oy = 0;
  for (int it = 0; it <= N; ++it) {
    const geo_u64 w = word[x];
    const int p = geo_parent(w);
    if (p == x) {
      if (!geo_fits(ox) || !geo_fits(oy)) {
        atomicOr(&out->err, 2u);
        ox = oy = 0;
      }
      label[i] = x;
      off[i] = make_int2(ox, oy);
      atomicAdd(&cnt[x], i < NA ? 1ull : 1ull << 32);
      return;
    }
    ox += geo_rx(w);
    oy += geo_ry(w);
    x = p;
  }
  label[i] = i;
  off[i] = make_int2(0, 0);
  atomicOr(&out->err, 1u);
}

// every vertex's edges against the offsets: an edge the tree did not use closes
// a cycle, and a cycle whose shifts do not cancel wraps the box along that axis
__global__ void __launch_bounds__(AN_T) k_geo_check(KParams P, Dev d, const int32_t* __restrict__ label,
                                                    const int2* __restrict__ off, uint32_t* span, GeoOut* out) {
  const int p = blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= P.N) return;
  int nb[3];
  (void)geo_links(P, d, p, nb);
  const int me = d.id_of[p];
  const double2 xi = an_xy(P, d, p);
  const int2 oi = off[me];
  uint32_t bits = 0;
  for (int e = 0; e < 3; ++e) {
    if (nb[e] < 0) continue;
    const double2 xj = an_xy(P, d, nb[e]);
    const int2 oj = off[d.id_of[nb[e]]];
    if (oj.x - oi.x != geo_edge(xi.x, xj.x, P.box_x, &out->err)) bits |= 1u;
    if (oj.y - oi.y != geo_edge(xi.y, xj.y, P.box_y, &out->err)) bits |= 2u;
  }
  if (bits) atomicOr(&span[label[me]], bits);
}

// members of the unwrapped components add D = U_i − U_r and its products to the
// root's accumulators (the root itself adds zeros: it is skipped)
__global__ void __launch_bounds__(AN_T) k_geo_moments(const int32_t* __restrict__ label, const int2* __restrict__ off,
                                                      const longlong2* __restrict__ X,
                                                      const uint32_t* __restrict__ span, long long BX, long long BY,
                                                      int N, geo_u64* acc) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= N) return;
  const int r = label[i];
  if (r == i || span[r]) return;
  const int2 o = off[i];
  const longlong2 xi = X[i], xr = X[r];
  const long long dx = xi.x + (long long)o.x * BX - xr.x, dy = xi.y + (long long)o.y * BY - xr.y;
  geo_u64* a = acc + (size_t)r * GEO_ACC;
  if (dx) atomicAdd(&a[0], (geo_u64)dx);
  if (dy) atomicAdd(&a[1], (geo_u64)dy);
  geo_add128(a + 2, (__int128)dx * dx);
  geo_add128(a + 4, (__int128)dy * dy);
  geo_add128(a + 6, (__int128)dx * dy);
}

// m = n (S2xx + S2yy) − (S1x² + S1y²) of a root, exact
__device__ __forceinline__ __int128 geo_m(const geo_u64* a, int n) {
  const __int128 s1x = (long long)a[0], s1y = (long long)a[1];
  return (__int128)n * (geo_ld128(a + 2) + geo_ld128(a + 4)) - (s1x * s1x + s1y * s1y);
}

// the roots' table by size and the summary; bins and sums are privatised in
// LDS as in k_an_census, a workgroup flushes each non-empty bin once
__global__ void __launch_bounds__(AN_T) k_geo_table(const int32_t* __restrict__ label, const geo_u64* __restrict__ cnt,
                                                    const uint32_t* __restrict__ span, const geo_u64* __restrict__ acc,
                                                    int N, int max_size, geo_u64* table, GeoOut* out) {
  extern __shared__ __attribute__((aligned(16))) unsigned long long an_lds[];  // [nbin][GEO_BIN] bins, then 5 sums and the maximum
  const int nbin = table ? max_size + 1 : 0;
  geo_u64* sum = an_lds + (size_t)nbin * GEO_BIN;
  for (int b = threadIdx.x; b < nbin * GEO_BIN + 6; b += AN_T) an_lds[b] = 0ull;
  __syncthreads();
  geo_u64 best = 0;  // this thread's largest root: one LDS atomic per thread, not per root
  for (int i = blockIdx.x * AN_T + threadIdx.x; i < N; i += gridDim.x * AN_T) {
    if (label[i] != i) continue;
    const geo_u64 c = cnt[i];
    const int size = (int)(uint32_t)c + (int)(c >> 32);
    const uint32_t sp = span[i];
    best = max(best, (geo_u64)size << 32 | (0xffffffffu - (uint32_t)i));
    if (sp) {
      atomicAdd(&sum[1], 1ull);
      if (sp & 1u) atomicAdd(&sum[2], 1ull);
      if (sp & 2u) atomicAdd(&sum[3], 1ull);
      atomicAdd(&sum[4], (geo_u64)size);
      continue;
    }
    if (size < 2) continue;
    atomicAdd(&sum[0], 1ull);
    if (!nbin) continue;
    geo_u64* bin = an_lds + (size_t)min(size, max_size) * GEO_BIN;
    atomicAdd(&bin[0], 1ull);
    atomicAdd(&bin[1], (geo_u64)size);
    geo_add128(bin + 2, geo_m(acc + (size_t)i * GEO_ACC, size));
  }
  if (best) atomicMax(&sum[5], best);
  __syncthreads();
  for (int b = threadIdx.x; b < nbin; b += AN_T) {
    const geo_u64* bin = an_lds + (size_t)b * GEO_BIN;
    if (!bin[0]) continue;
    geo_u64* t = table + (size_t)b * GEO_BIN;
    atomicAdd(&t[0], bin[0]);
    atomicAdd(&t[1], bin[1]);
    geo_add128(t + 2, geo_ld128(bin + 2));
  }
  if (threadIdx.x == 0) {
    if (sum[0]) atomicAdd(&out->n_measured, sum[0]);
    if (sum[1]) atomicAdd(&out->n_spanning, sum[1]);
    if (sum[2]) atomicAdd(&out->n_span_x, sum[2]);
    if (sum[3]) atomicAdd(&out->n_span_y, sum[3]);
    if (sum[4]) atomicAdd(&out->proteins_in_spanning, sum[4]);
    if (sum[5]) atomicMax(&out->best, sum[5]);
  }
}

// the roots of at least min_size members, appended through one cursor (its
// final value is the true count; rows past cap are not written)
__global__ void __launch_bounds__(AN_T) k_geo_list(const int32_t* __restrict__ label, const geo_u64* __restrict__ cnt,
                                                   const uint32_t* __restrict__ span, const geo_u64* __restrict__ acc,
                                                   int N, int min_size, long long cap, kmc_cluster* rows, GeoOut* out) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= N || label[i] != i) return;
  const geo_u64 c = cnt[i];
  const int nr = (int)(uint32_t)c, nl = (int)(c >> 32);
  if (nr + nl < min_size) return;
  const geo_u64 at = atomicAdd(&out->n_rows, 1ull);
  if (at >= (geo_u64)cap) return;
  const geo_u64* a = acc + (size_t)i * GEO_ACC;  // all zero for a spanning root: its members added nothing
  kmc_cluster r;
  r.label = i + 1;
  r.n_r = nr;
  r.n_l = nl;
  r.span = (int32_t)span[i];
  r.s1x = (long long)a[0];
  r.s1y = (long long)a[1];
  r.s2xx.lo = a[2], r.s2xx.hi = (long long)a[3];
  r.s2yy.lo = a[4], r.s2yy.hi = (long long)a[5];
  r.s2xy.lo = a[6], r.s2xy.hi = (long long)a[7];
  rows[at] = r;
}

}  // namespace kmcd
