// kmc_proximity.h — the expressions of the proximity clustering that the device
// kernels (kmc_proximity.hip) and the sequential host counterpart
// (kmc_host_prox_clusters, kmc_host_observe.cpp) must evaluate bit for bit alike
// (include/kmc.h).  The integer coordinates, the periodic
// displacement, the cell of the grid and the distance bins' edges are §14's
// (kmc_bondorder.h); what is new here is decided by integers alone.
#pragma once
#include <stdint.h>

#include "kmc_bondorder.h"

namespace kmcx {

#define PX_NN_ROWS 64        // KMC_PX_NN_ROWS
#define PX_MAX_SIZE 65535    // most bins of the size histogram beyond bin 0
#define PX_NND_BINS 4096     // most bins of the nearest-neighbour histogram
#define PX_MIN_PTS_MAX (1 << 30)

// a point with N neighbours is a core: itself and its neighbours make min_pts
KMC_HD bool is_core(int32_t N, int32_t min_pts) { return (int64_t)N + 1 >= (int64_t)min_pts; }

// the border rule: core (D2, ref) is nearer than the best so far (best_ref < 0: none yet)
KMC_HD bool nearer(int64_t D2, int32_t ref, int64_t best_D2, int32_t best_ref) {
  return best_ref < 0 || D2 < best_D2 || (D2 == best_D2 && ref < best_ref);
}

// bin of the squared nearest-neighbour distance M: #{m in 1..nbins-1 : E2[m] <= M}
// over the squared edges E2[0..nbins-1] (E2[0] = 0), walked from the guess k
KMC_HD int nnd_bin(const int64_t* E2, int nbins, int64_t M, int k) { return kmcb::corr_bin(E2, nbins - 1, M, k); }

}  // namespace kmcx
