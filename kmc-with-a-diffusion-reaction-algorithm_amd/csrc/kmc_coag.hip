// kmc_coag.hip — cluster growth kinetics over the committed state (DESIGN.md
// §16): which clusters merged and which fell apart between two looks, by
// size.  Like kmc_kinetics.hip nothing here runs inside a step: the kernels
// are launched by explicit calls between kmc_step calls, read what
// kmc_get_state would return and write only the recorder's own arrays.
//
// Three partitions of the N proteins, all by REFERENCE index: the previous
// clusters (the labels and packed counts an_components left at the last
// look), the current clusters (the ones it leaves now) and the cores, the
// components of the bonds both looks hold.  The cores come from a second run
// of kmc_analysis.hip's lock-free union-find, hooked over the kept bonds only;
// a core's root then files what kmc_coag.h's rule says about its previous and
// its current cluster.  Integers only; every loop is bounded and an exhausted
// bound or a link out of range raises CfAcc::err.
//
// Included by kmc_engine.hip after kmc_kinetics.hip (and kmc_analysis.hip,
// whose receptor_bonds and an_unite it calls); the host side of the calls is
// kmc_observe.hip §cluster growth kinetics.
#include "kmc_coag.h"
#include "kmc_device.h"
#include "kmc_observe.h"

namespace kmcd {

#define CF_T 256  // threads per workgroup

// the recorder's device arrays
struct Cf {
  int32_t *rl_lig, *cis_with;     // [NA] the bonds of the last look, as reference indices (0: none)
  int32_t* label[2];              // [N] cluster labels (0-based roots) of the last two looks
  unsigned long long* cnt[2];     // [N] packed member counts at the roots
  int32_t *parent, *core;         // [N] union-find over the kept bonds; the core's label
  unsigned long long* core_cnt;   // [N] packed member counts at the core roots
  int32_t *pieces_prev, *pieces_cur;  // [N] cores per previous / current cluster, at the cluster's root
};

// the tables since begin, (S + 1)-strided, in one allocation
struct CfTab {
  unsigned long long merge[(CF_MAX_SIZE + 1) * (CF_MAX_SIZE + 1)], frag[(CF_MAX_SIZE + 1) * (CF_MAX_SIZE + 1)];
  unsigned long long merge_kind[CF_KINDS * CF_KINDS], frag_kind[CF_KINDS * CF_KINDS];
  unsigned long long merge_pieces[CF_PIECES], frag_pieces[CF_PIECES];
  unsigned long long merge_product[CF_MAX_SIZE + 1], frag_parent[CF_MAX_SIZE + 1];
};

enum : int { CF_EV_FORMED_RL = 0, CF_EV_FORMED_CIS, CF_EV_BROKEN_RL, CF_EV_BROKEN_CIS, CF_NEV };

struct CfAcc {
  unsigned long long ev[CF_NEV];              // since begin
  unsigned long long n_cores;                 // of the last update
  unsigned long long n_clusters, max_cluster; // of the last look
  unsigned long long n_s[CF_MAX_SIZE + 1];    // of the last look
  unsigned int err;                           // a link or a label left its range, or a find loop its bound
  unsigned int pad;
};

// host side: scratch of the first kmc_cf_begin, its own; rec.on: a recorder is
// running (a new state drops it)
struct CfState {
  Recorder rec;
  Scratch scratch;
  Cf dev = {nullptr, nullptr, {nullptr, nullptr}, {nullptr, nullptr}, nullptr, nullptr, nullptr, nullptr, nullptr};
  CfTab* tab = nullptr;
  CfAcc* acc = nullptr;
  int cur = 0;                       // which of the two label / count sets is the last look's
  int S = 0;                         // max_size of the begin
  int64_t ev[CF_NEV] = {0, 0, 0, 0}; // bonds formed / broken since begin, as of the last update
  int64_t cores = 0, clusters = 0, max = 0, closed = 0, opened = 0;
  int64_t ns[CF_MAX_SIZE + 1] = {0}; // n_s of the last look
  int64_t expo[CF_MAX_SIZE + 1] = {0};
  std::vector<__int128> expo2;       // [(S + 1)^2] since begin
};

// begin: the current bonds become the stored ones
__global__ void __launch_bounds__(CF_T) k_cf_begin(KParams P, Dev d, Cf F, CfAcc* acc) {
  const int i = blockIdx.x * CF_T + threadIdx.x;
  if (i >= P.NA) return;
  int32_t lig, cis;  // the current bonds as reference indices
  if (!receptor_bonds(P, d, i, lig, cis)) {
    atomicOr(&acc->err, 1u);
    lig = cis = 0;
  }
  F.rl_lig[i] = lig;
  F.cis_with[i] = cis;
}

__global__ void __launch_bounds__(CF_T) k_cf_init(Cf F, int N) {
  const int i = blockIdx.x * CF_T + threadIdx.x;
  if (i >= N) return;
  F.parent[i] = i;
  F.core_cnt[i] = 0ull;
  F.pieces_prev[i] = 0;
  F.pieces_cur[i] = 0;
}

// one receptor per thread by reference index: the ends of every bond that both
// looks hold are united, the bonds that were formed or broken counted (a cis
// bond at its lower index; per wave a ballot per counter, lane 0 adds into
// LDS, one global atomic per non-zero counter and workgroup), and a stored
// link is replaced only where it changed.
__global__ void __launch_bounds__(CF_T) k_cf_hook(KParams P, Dev d, Cf F, CfAcc* acc) {
  __shared__ unsigned long long sm[CF_NEV];
  if (threadIdx.x < CF_NEV) sm[threadIdx.x] = 0ull;
  __syncthreads();
  const int i = blockIdx.x * CF_T + threadIdx.x;
  uint32_t m = 0;
  bool bad = false;
  if (i < P.NA) {
    int32_t lig, cis;  // the current bonds as reference indices
    bad = !receptor_bonds(P, d, i, lig, cis);
    if (!bad) {  // (a call that met a bad link fails and drops the recorder)
      const int32_t old_lig = F.rl_lig[i], old_cis = F.cis_with[i], me = i + 1;
      if (lig != old_lig) {
        if (lig != 0) m |= 1u << CF_EV_FORMED_RL;
        if (old_lig != 0) m |= 1u << CF_EV_BROKEN_RL;
        F.rl_lig[i] = lig;
      } else if (lig != 0) {
        an_unite(F.parent, i, lig - 1, P.N, &acc->err);
      }
      if (cis != old_cis) {
        if (cis != 0 && me < cis) m |= 1u << CF_EV_FORMED_CIS;
        if (old_cis != 0 && me < old_cis) m |= 1u << CF_EV_BROKEN_CIS;
        F.cis_with[i] = cis;
      } else if (cis != 0 && me < cis) {
        an_unite(F.parent, i, cis - 1, P.N, &acc->err);
      }
    }
  }
  for (int b = 0; b < CF_NEV; ++b) {
    const unsigned long long k = __popcll(__ballot(m >> b & 1u));
    if ((threadIdx.x & 63) == 0 && k) atomicAdd(&sm[b], k);
  }
  const bool any_bad = __ballot(bad) != 0ull;
  if ((threadIdx.x & 63) == 0 && any_bad) atomicOr(&acc->err, 1u);
  __syncthreads();
  if (threadIdx.x < CF_NEV && sm[threadIdx.x]) atomicAdd(&acc->ev[threadIdx.x], sm[threadIdx.x]);
}

// after the hooks every root is final: one protein per thread writes its
// core's label and adds its packed count into the core's root; a core root
// counts itself into its previous and its current cluster
__global__ void __launch_bounds__(CF_T) k_cf_flatten(Cf F, const int32_t* __restrict__ prev,
                                                     const int32_t* __restrict__ cur, int NA, int N, CfAcc* acc) {
  __shared__ unsigned int roots;
  if (threadIdx.x == 0) roots = 0u;
  __syncthreads();
  const int i = blockIdx.x * CF_T + threadIdx.x;
  bool is_root = false;
  if (i < N) {
    int x = i, r = -1;
    for (int it = 0; it <= N; ++it) {
      const int p = F.parent[x];
      if (p == x) {
        r = x;
        break;
      }
      if ((unsigned)p >= (unsigned)N) break;
      x = p;
    }
    if (r < 0) {
      atomicOr(&acc->err, 1u);
      r = i;
    }
    F.core[i] = r;
    atomicAdd(&F.core_cnt[r], i < NA ? 1ull : 1ull << 32);
    if (r == i) {
      const int pl = prev[i], cl = cur[i];
      if ((unsigned)pl >= (unsigned)N || (unsigned)cl >= (unsigned)N) {
        atomicOr(&acc->err, 1u);
      } else {
        is_root = true;
        atomicAdd(&F.pieces_prev[pl], 1);
        atomicAdd(&F.pieces_cur[cl], 1);
      }
    }
  }
  const unsigned int k = (unsigned int)__popcll(__ballot(is_root));
  if ((threadIdx.x & 63) == 0 && k) atomicAdd(&roots, k);
  __syncthreads();
  if (threadIdx.x == 0 && roots) atomicAdd(&acc->n_cores, (unsigned long long)roots);
}

// The dense part of a look: every cluster root adds to the size histogram, the
// cluster count and the largest size.  Privatised in LDS (S + 1 <= 64 bins of
// 32 bits: a workgroup holds 256 proteins), each non-empty bin flushed once.
// Every thread of the workgroup calls it.
__device__ __forceinline__ void cf_sizes(bool root, int size, int S, unsigned int* bins, unsigned int* top,
                                         CfAcc* acc) {
  const int j = threadIdx.x;
  if (j <= CF_MAX_SIZE) bins[j] = 0u;
  if (j == 0) *top = 0u;
  __syncthreads();
  if (root) {
    atomicAdd(&bins[kmcc::clamp_size(size, S)], 1u);
    atomicMax(top, (unsigned int)size);
  }
  __syncthreads();
  if (j <= S && bins[j]) atomicAdd(&acc->n_s[j], (unsigned long long)bins[j]);
  if (j == 64) {
    unsigned int n = 0;
    for (int b = 0; b <= S; ++b) n += bins[b];
    if (n) atomicAdd(&acc->n_clusters, (unsigned long long)n);
    if (*top) atomicMax(&acc->max_cluster, (unsigned long long)*top);
  }
}

// begin / put: the size histogram of one label set
__global__ void __launch_bounds__(CF_T) k_cf_sizes(const int32_t* __restrict__ label,
                                                   const unsigned long long* __restrict__ cnt, int N, int S,
                                                   CfAcc* acc) {
  __shared__ unsigned int bins[CF_MAX_SIZE + 1], top;
  const int i = blockIdx.x * CF_T + threadIdx.x;
  const bool root = i < N && label[i] == i;
  cf_sizes(root, root ? kmcc::size_of(cnt[i]) : 0, S, bins, &top, acc);
}

// one protein per thread.  A core root files what kmc_coag.h's rule says about
// its previous cluster (fragmentation) and its current one (merger): events
// are rare per update, so they go straight to 64-bit global atomics.  A
// current-cluster root joins the dense size histogram.
__global__ void __launch_bounds__(CF_T) k_cf_events(Cf F, const int32_t* __restrict__ prev,
                                                    const unsigned long long* __restrict__ prev_cnt,
                                                    const int32_t* __restrict__ cur,
                                                    const unsigned long long* __restrict__ cur_cnt, int N, int S,
                                                    CfTab* T, CfAcc* acc) {
  __shared__ unsigned int bins[CF_MAX_SIZE + 1], top;
  const int i = blockIdx.x * CF_T + threadIdx.x;
  bool root = false;
  int size = 0;
  if (i < N) {
    const int cl = cur[i];
    if (F.parent[i] == i) {
      const int pl = prev[i];
      if ((unsigned)pl < (unsigned)N && (unsigned)cl < (unsigned)N) {  // (else k_cf_flatten raised err)
        const unsigned long long c = F.core_cnt[i];
        const int k0 = F.pieces_prev[pl], k1 = F.pieces_cur[cl];
        if (k0 >= 2) {
          const kmcc::Filing f = kmcc::file(i, c, pl, prev_cnt[pl], k0, S);
          if (f.pieces >= 0) atomicAdd(&T->frag_pieces[f.pieces], 1ull);
          if (f.whole >= 0) atomicAdd(&T->frag_parent[f.whole], 1ull);
          if (f.pair >= 0) atomicAdd(&T->frag[f.pair], 1ull);
          if (f.kinds >= 0) atomicAdd(&T->frag_kind[f.kinds], 1ull);
        }
        if (k1 >= 2) {
          const kmcc::Filing f = kmcc::file(i, c, cl, cur_cnt[cl], k1, S);
          if (f.pieces >= 0) atomicAdd(&T->merge_pieces[f.pieces], 1ull);
          if (f.whole >= 0) atomicAdd(&T->merge_product[f.whole], 1ull);
          if (f.pair >= 0) atomicAdd(&T->merge[f.pair], 1ull);
          if (f.kinds >= 0) atomicAdd(&T->merge_kind[f.kinds], 1ull);
        }
      }
    }
    if (cl == i) {
      root = true;
      size = kmcc::size_of(cur_cnt[i]);
    }
  }
  cf_sizes(root, size, S, bins, &top, acc);
}

}  // namespace kmcd
