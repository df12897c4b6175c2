// kmc_kinetics.hip — bond kinetics over the committed state:
// the lifetime of every R–L and cis bond, born before or after the recorder
// began, the waiting time until a receptor binds again (to the ligand it lost
// or to another one), the event counts and the occupancy behind the effective
// on- and off-rates.  Like kmc_dynamics.hip nothing here runs inside a step:
// the kernels are launched by explicit calls between kmc_step calls, read what
// kmc_get_state would return and write only the recorder's own arrays.
//
// The recorder's arrays are indexed by the receptor's REFERENCE index; the
// kernels iterate by reference index, so its 41 bytes per receptor stream in
// order (and are written back only where a field changed), and only slot_of,
// the three links at the slot, up to two id_of and the partner's nei2 are
// gathered.  The per-receptor transition and the bin rule are kmc_kinetics.h's,
// shared with the host counterpart.  Integers only.
//
// Included by kmc_engine.hip after kmc_dynamics.hip (and kmc_analysis.hip,
// whose receptor_bonds kin_cur calls); the host side of the calls is
// kmc_observe.hip §bond kinetics.
#include "kmc_device.h"
#include "kmc_observe.h"
#include "kmc_kinetics.h"

namespace kmcd {

#define KIN_T 256  // threads per workgroup

struct Kin {
  int32_t *rl_lig, *rl_site, *cis_with, *last_lig;  // [NA]
  long long *rl_since, *cis_since, *free_since;     // [NA]
  uint8_t* bits;                                    // [NA]
};

struct KinAcc {
  unsigned long long ev[KIN_NEV];  // since begin
  unsigned long long occ[3];       // of the last begin / update: rl, mono, complex
  unsigned long long alive[2];     // of the last sample: left-censored R–L / cis bonds still alive
  unsigned int err;                // a link left its range in the last call
  unsigned int pad;
};

// host side: scratch of the first kmc_kin_begin, its own; rec.on: a recorder is
// running (a new state drops it)
struct KinState {
  Recorder rec;
  Scratch scratch;
  Kin dev = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
  KinAcc* acc = nullptr;
  unsigned long long* hist = nullptr;  // [KIN_HISTS][KIN_BINS]: rows 0-6 since begin, 7 and 8 of the last sample
  int64_t occ[3] = {0, 0, 0};          // rl, mono, complex at the last update
  int64_t exp[5] = {0, 0, 0, 0, 0};    // exposures since begin
};

// the current links of receptor i (0-based reference index) as the recorder
// names them; false when a slot or a link leaves its range (nothing is read
// through it then)
__device__ __forceinline__ bool kin_cur(const KParams& P, const Dev& d, int i, kmck::Cur& c) {
  c.site = 0;
  c.cx = false;
  return receptor_bonds(P, d, i, c.lig, c.cis, &c.site, &c.cx);
}

// the counters: per wave one ballot per counter, lane 0 adds the non-zero
// ones into LDS, thread b then sends counter b with one atomic per workgroup
__device__ __forceinline__ void kin_count(uint32_t m, bool bad, unsigned long long* sm, KinAcc* acc) {
  for (int b = 0; b < kmck::KIN_NCNT; ++b) {
    const unsigned long long k = __popcll(__ballot(m >> b & 1u));
    if ((threadIdx.x & 63) == 0 && k) atomicAdd(&sm[b], k);
  }
  const bool any_bad = __ballot(bad) != 0ull;
  if ((threadIdx.x & 63) == 0 && any_bad) atomicOr(&acc->err, 1u);
  __syncthreads();
  const int b = threadIdx.x;
  if (b < kmck::KIN_NCNT && sm[b]) atomicAdd(b < KIN_NEV ? &acc->ev[b] : &acc->occ[b - KIN_NEV], sm[b]);
}

__global__ void __launch_bounds__(KIN_T) k_kin_begin(KParams P, Dev d, Kin K, long long t, KinAcc* acc) {
  __shared__ unsigned long long sm[kmck::KIN_NCNT];
  if (threadIdx.x < kmck::KIN_NCNT) sm[threadIdx.x] = 0ull;
  __syncthreads();
  const int i = blockIdx.x * KIN_T + threadIdx.x;
  uint32_t m = 0;
  bool bad = false;
  if (i < P.NA) {
    kmck::Cur c;
    bad = !kin_cur(P, d, i, c);
    kmck::Rec r;
    m = kmck::begin(i + 1, t, c, r);
    K.rl_lig[i] = r.rl_lig;
    K.rl_site[i] = r.rl_site;
    K.cis_with[i] = r.cis_with;
    K.last_lig[i] = r.last_lig;
    K.rl_since[i] = r.rl_since;
    K.cis_since[i] = r.cis_since;
    K.free_since[i] = r.free_since;
    K.bits[i] = r.bits;
  }
  kin_count(m, bad, sm, acc);
}

// one receptor per thread, in the order of include/kmc.h.  Events are rare per
// update (bonds × per-step probability), so their histogram entries go
// straight to 64-bit global atomics, and a record is written back only in the
// fields that changed.
__global__ void __launch_bounds__(KIN_T) k_kin_update(KParams P, Dev d, Kin K, long long t, unsigned long long* hist,
                                                      KinAcc* acc) {
  __shared__ unsigned long long sm[kmck::KIN_NCNT];
  if (threadIdx.x < kmck::KIN_NCNT) sm[threadIdx.x] = 0ull;
  __syncthreads();
  const int i = blockIdx.x * KIN_T + threadIdx.x;
  uint32_t m = 0;
  bool bad = false;
  if (i < P.NA) {
    kmck::Cur c;
    bad = !kin_cur(P, d, i, c);
    kmck::Rec r, o;
    o.rl_lig = K.rl_lig[i];
    o.rl_site = K.rl_site[i];
    o.cis_with = K.cis_with[i];
    o.last_lig = K.last_lig[i];
    o.rl_since = K.rl_since[i];
    o.cis_since = K.cis_since[i];
    o.free_since = K.free_since[i];
    o.bits = K.bits[i];
    r = o;
    if (!bad) {  // (a call that met a bad link fails and drops the recorder)
      int row[3], nh;
      int64_t val[3];
      m = kmck::transition(i + 1, t, c, r, row, val, &nh);
      for (int k = 0; k < 3; ++k)
        if (k < nh) atomicAdd(&hist[row[k] * KIN_BINS + kmck::bin(val[k])], 1ull);
      if (r.rl_lig != o.rl_lig) K.rl_lig[i] = r.rl_lig;
      if (r.rl_site != o.rl_site) K.rl_site[i] = r.rl_site;
      if (r.cis_with != o.cis_with) K.cis_with[i] = r.cis_with;
      if (r.last_lig != o.last_lig) K.last_lig[i] = r.last_lig;
      if (r.rl_since != o.rl_since) K.rl_since[i] = r.rl_since;
      if (r.cis_since != o.cis_since) K.cis_since[i] = r.cis_since;
      if (r.free_since != o.free_since) K.free_since[i] = r.free_since;
      if (r.bits != o.bits) K.bits[i] = r.bits;
    }
  }
  kin_count(m, bad, sm, acc);
}

// rows 7 and 8: the ages of the living, non-censored bonds as of the last
// update.  The pass is dense (every living bond), so the two rows are
// privatised in LDS (4 KiB) across the blocks a workgroup takes and the
// non-empty bins flushed with one 64-bit atomic each.  Reads the recorder only.
__global__ void __launch_bounds__(KIN_T) k_kin_sample(int NA, Kin K, long long t_last, int nblk,
                                                      unsigned long long* rows, KinAcc* acc) {
  __shared__ unsigned long long bins[2 * KIN_BINS];
  __shared__ unsigned long long cens[2];
  const int j = threadIdx.x;
  for (int b = j; b < 2 * KIN_BINS; b += KIN_T) bins[b] = 0ull;
  if (j < 2) cens[j] = 0ull;
  __syncthreads();
  for (int blk = blockIdx.x; blk < nblk; blk += gridDim.x) {
    const int i = blk * KIN_T + j;
    uint32_t m = 0;
    if (i < NA) {
      kmck::Rec r;
      r.rl_lig = K.rl_lig[i];
      r.cis_with = K.cis_with[i];
      r.bits = K.bits[i];
      m = kmck::alive(i + 1, r);
      if (m & 1u) atomicAdd(&bins[kmck::bin(t_last - K.rl_since[i])], 1ull);
      if (m & 2u) atomicAdd(&bins[KIN_BINS + kmck::bin(t_last - K.cis_since[i])], 1ull);
    }
    for (int b = 0; b < 2; ++b) {
      const unsigned long long k = __popcll(__ballot(m >> (2 + b) & 1u));
      if ((j & 63) == 0 && k) atomicAdd(&cens[b], k);
    }
  }
  __syncthreads();
  for (int b = j; b < 2 * KIN_BINS; b += KIN_T)
    if (bins[b]) atomicAdd(&rows[b], bins[b]);
  if (j < 2 && cens[j]) atomicAdd(&acc->alive[j], cens[j]);
}

}  // namespace kmcd
