// kmc_observe.h — the host-side pieces every analysis layer's state is built
// from (the state structs next to the layers' kernels, kmc_sim's members); the
// functions over them are at the top of kmc_observe.hip.
#pragma once
#include <stdint.h>

#include <vector>

namespace kmcd {

// counting sort of points by cell: grown when a grid outgrows cap (bins_reserve), scanned by bins_scan
struct CellBins {
  int32_t *ccnt = nullptr, *cstart = nullptr, *part = nullptr;  // [cap] cell counts, their scan, tile sums
  size_t cap = 0;
};

// the device buffers a layer allocated (salloc) and frees together (scratch_free)
struct Scratch {
  std::vector<void*> ptrs;
};

// a recorder over the trajectory: on between its begin and its end, a failed call or a new state
struct Recorder {
  bool on = false;
  int64_t origin = 0, last = 0, updates = 0;  // steps of the begin and of the last update; updates since begin
};

}  // namespace kmcd
