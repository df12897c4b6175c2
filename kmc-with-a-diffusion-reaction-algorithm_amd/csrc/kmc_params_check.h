// kmc_params_check.h — the parameter envelope kmc_create accepts (host only).
//
// One rule, shared by kmc_create, kmc_host_check_params / kmc_host_validate and
// the CPU oracle's oracle_create, so that "accepted" means the same thing at
// every link of reference -> oracle -> engine:
//
//   sizes      n_a >= 0, n_b >= 0, 1 <= n_a + n_b <= 2^24
//   finite     every double field is finite (no NaN, no +-inf)
//   positive   box_x, box_y, box_z, time_step, pai, ra_radius, rb_radius,
//              bond_dist_cutoff, cis_dist_cutoff and the three angle cutoffs > 0
//   bounded    ra_radius <= 20, rb_radius <= 30, bond_dist_cutoff <= 18,
//              cis_dist_cutoff <= 15 (the reference's values: the cell size and
//              every float prefilter reach are derived for them; smaller values
//              only shrink every reach)
//   >= 0       every D, rot_D and rate (0 switches the move or reaction off)
//
// Every comparison is written so that a NaN fails it.
#pragma once
#include <cmath>
#include <cstdint>

#include "../../include/kmc.h"

namespace kmcp {

// nullptr when p is inside the envelope, else the name of the first offending field
inline const char* check_params(const kmc_params* p) {
  if (!p) return "params";
  if (p->n_a < 0) return "n_a";
  if (p->n_b < 0) return "n_b";
  if ((int64_t)p->n_a + p->n_b < 1 || (int64_t)p->n_a + p->n_b > (1 << 24)) return "n_a + n_b";
  struct F {
    const char* name;
    double v, lo, hi;  // lo < v (strict when lo_open) and v <= hi
    bool lo_open;
  };
  const double big = HUGE_VAL;
  const F f[] = {
      {"time_step", p->time_step, 0, big, true},
      {"box_x", p->box_x, 0, big, true},
      {"box_y", p->box_y, 0, big, true},
      {"box_z", p->box_z, 0, big, true},
      {"pai", p->pai, 0, big, true},
      {"ra_radius", p->ra_radius, 0, 20.0, true},
      {"rb_radius", p->rb_radius, 0, 30.0, true},
      {"bond_dist_cutoff", p->bond_dist_cutoff, 0, 18.0, true},
      {"cis_dist_cutoff", p->cis_dist_cutoff, 0, 15.0, true},
      {"bond_thetapd_cutoff", p->bond_thetapd_cutoff, 0, big, true},
      {"bond_thetaot_cutoff", p->bond_thetaot_cutoff, 0, big, true},
      {"cis_thetaot_cutoff", p->cis_thetaot_cutoff, 0, big, true},
      {"ra_D", p->ra_D, 0, big, false},
      {"ra_rot_D", p->ra_rot_D, 0, big, false},
      {"rb_D", p->rb_D, 0, big, false},
      {"rb_rot_D", p->rb_rot_D, 0, big, false},
      {"cis_D", p->cis_D, 0, big, false},
      {"cis_rot_D", p->cis_rot_D, 0, big, false},
      {"bond_D", p->bond_D, 0, big, false},
      {"bond_rot_D", p->bond_rot_D, 0, big, false},
      {"mono_cis_ass_rate", p->mono_cis_ass_rate, 0, big, false},
      {"mono_cis_diss_rate", p->mono_cis_diss_rate, 0, big, false},
      {"cis_ass_rate", p->cis_ass_rate, 0, big, false},
      {"cis_diss_rate", p->cis_diss_rate, 0, big, false},
      {"ass_rate", p->ass_rate, 0, big, false},
      {"diss_rate", p->diss_rate, 0, big, false},
  };
  for (const F& e : f) {
    if (!std::isfinite(e.v)) return e.name;
    if (!(e.lo_open ? e.v > e.lo : e.v >= e.lo) || !(e.v <= e.hi)) return e.name;
  }
  return nullptr;
}

}  // namespace kmcp
