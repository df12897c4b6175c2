// kmc_orient.h — the expressions of the orientation layer that the device
// kernels (kmc_orient.hip) and the sequential host counterparts
// (kmc_host_rot_*, kmc_host_ligand_pose, kmc_host_observe.cpp) must evaluate alike
// (include/kmc.h): the quantised body vectors, their packing,
// the handedness, the pair term and the pose bins.  Integers throughout.  The
// firing schedule, the ring index and the five classes are kmc_lagcorr.h's.
#pragma once
#include <stdint.h>

#include "kmc_lagcorr.h"  // rows, fires, tasks, store_ring, row_of, cls

namespace kmco {

#define ROT_LIMIT 65536            // 2^16 quanta: a component at or above it makes the protein "bad"
#define ROT_SPLIT 17               // |d| = a 2^17 + b
#define ROT_VECS 2                 // KMC_ROT_VECS: vector indices of a table cell (receptors use v = 0 alone)
#define ROT_BAD (1ull << 63)       // KMC_ROT_BAD: the packed word of a bad protein's vector
#define POSE_MAX_BINS 64           // KMC_POSE_MAX_BINS
#define POSE_CLASSES 4             // KMC_POSE_CLASSES: 0..3 occupied sites

struct V3 {
  int64_t x, y, z;
};

// §12's coordinate quantum, per bead; a vector is the difference of two quantised beads
KMC_HD int64_t q(double x) { return (int64_t)kmcm::round_(x * 1024.0); }

KMC_HD V3 sub(V3 a, V3 b) { return V3{a.x - b.x, a.y - b.y, a.z - b.z}; }

KMC_HD bool fits(V3 v) {
  return v.x > -ROT_LIMIT && v.x < ROT_LIMIT && v.y > -ROT_LIMIT && v.y < ROT_LIMIT && v.z > -ROT_LIMIT && v.z < ROT_LIMIT;
}

// three signed 21-bit fields (a vector that fits needs 17); bit 63 stays clear
KMC_HD uint64_t pack(V3 v) {
  const uint64_t M = (1ull << 21) - 1;
  return ((uint64_t)v.x & M) | ((uint64_t)v.y & M) << 21 | ((uint64_t)v.z & M) << 42;
}
KMC_HD V3 unpack(uint64_t w) {
  return V3{(int64_t)(w << 43) >> 43, (int64_t)(w << 22) >> 43, (int64_t)(w << 1) >> 43};
}

// |d| < 3 2^32 for two vectors that fit
KMC_HD int64_t dot(V3 a, V3 b) { return a.x * b.x + a.y * b.y + a.z * b.z; }

// the sign of n . (a x c): cross components below 2^33, the product below 3 2^49 < 2^51
KMC_HD int chi(V3 n, V3 a, V3 c) {
  const int64_t t = n.x * (a.y * c.z - a.z * c.y) + n.y * (a.z * c.x - a.x * c.z) + n.z * (a.x * c.y - a.y * c.x);
  return t > 0 ? 1 : t < 0 ? -1 : 0;
}

// |d| = a 2^17 + b with a, b < 2^17 (|d| < 2^34): a², ab and b² are below 2^34
// each and are summed apart in 64-bit words; d² = a² 2^34 + ab 2^18 + b² (sq)
KMC_HD void split(int64_t d, uint64_t* a2, uint64_t* ab, uint64_t* b2) {
  const uint64_t m = (uint64_t)(d < 0 ? -d : d);
  const uint64_t a = m >> ROT_SPLIT, b = m & ((1ull << ROT_SPLIT) - 1);
  *a2 = a * a;
  *ab = a * b;
  *b2 = b * b;
}
KMC_HD unsigned __int128 sq(uint64_t a2, uint64_t ab, uint64_t b2) {
  return ((unsigned __int128)a2 << (2 * ROT_SPLIT)) + ((unsigned __int128)ab << (ROT_SPLIT + 1)) + b2;
}

// A receptor's heading: the xy projection of bead [3][2] - bead [3][1]; z is 0
// by definition (receptors stay vertical, so the heading is the orientation).
KMC_HD V3 heading(const double b31[2], const double b32[2]) {
  return V3{q(b32[0]) - q(b31[0]), q(b32[1]) - q(b31[1]), 0};
}

// A ligand's axis N = [1][2] - [1][1], arm A = [2][1] - [1][1] and third
// vector C = [3][1] - [1][1], which only the handedness reads.
struct Lig {
  V3 n, a, c;
};
KMC_HD Lig ligand(const double b11[3], const double b12[3], const double b21[3], const double b31[3]) {
  const V3 o{q(b11[0]), q(b11[1]), q(b11[2])};
  Lig g;
  g.n = sub(V3{q(b12[0]), q(b12[1]), q(b12[2])}, o);
  g.a = sub(V3{q(b21[0]), q(b21[1]), q(b21[2])}, o);
  g.c = sub(V3{q(b31[0]), q(b31[1]), q(b31[2])}, o);
  return g;
}
KMC_HD bool fits(const Lig& g) { return fits(g.n) && fits(g.a) && fits(g.c); }

// the pose bins of a ligand that fits: z of bead [1][1] over [0, BZ] and the
// axis' z component over [-Lq, Lq]; both clamp
KMC_HD int pose_zbin(int64_t qz, int64_t BZ, int nz) {
  if (qz <= 0) return 0;
  if (qz >= BZ) return nz - 1;
  const int64_t b = qz * nz / BZ;
  return b > nz - 1 ? nz - 1 : (int)b;
}
KMC_HD int pose_tbin(int64_t Nz, int64_t Lq, int nc) {
  const int64_t b = (Nz + Lq) * nc / (2 * Lq + 1);  // (|Nz| < 2^16: the product stays far below 2^63)
  return Nz + Lq < 0 ? 0 : b > nc - 1 ? nc - 1 : (int)b;
}

// the configuration's bounds (include/kmc.h): what is wrong with it, or nullptr
inline const char* check(int every, int levels, int slots) {
  if (every < 1) return "rot: every >= 1";
  if (levels < 1 || levels > LAG_MAX_LEVELS) return "rot: 1 <= levels <= 20";
  if (slots < 2 || slots > LAG_MAX_SLOTS || slots % 2) return "rot: slots even, 2 <= slots <= 16";
  return nullptr;
}
inline const char* pose_check(int nz, int nc, double box_z, double rb_radius, int64_t* BZ, int64_t* Lq) {
  if (nz < 1 || nz > POSE_MAX_BINS || nc < 1 || nc > POSE_MAX_BINS) return "pose: 1 <= nz, nc <= 64";
  *BZ = q(box_z);
  *Lq = q(rb_radius);
  if (!(*BZ >= 1)) return "pose: box_z below the coordinate quantum";
  if (!(*Lq >= 1 && *Lq < ROT_LIMIT)) return "pose: rb_radius out of range";
  return nullptr;
}

}  // namespace kmco
