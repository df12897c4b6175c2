// kmc_coag.h — the expressions of the cluster growth recorder that the device
// kernels (kmc_coag.hip) and the sequential host counterparts (kmc_host_cf_*,
// kmc_host_observe.cpp) must evaluate alike (include/kmc.h): the size
// clamp, the ordered index of a size pair, the kind of a piece from its packed
// (receptors, ligands) counts, the pieces clamp, and the two filing rules of a
// core.  Integers only.
#pragma once
#include <stdint.h>

#include "kmc_math.h"  // KMC_HD

namespace kmcc {

#define CF_MAX_SIZE 63  // KMC_CF_MAX_SIZE: the largest size clamp S
#define CF_MIN_SIZE 2
#define CF_PIECES 9     // KMC_CF_PIECES: rows of merge_pieces / frag_pieces, index min(k, 8)
#define CF_KINDS 4      // KMC_CF_KINDS: kinds of a piece

// kinds of a piece
enum : int { CF_KIND_R = 0, CF_KIND_L = 1, CF_KIND_RR = 2, CF_KIND_OTHER = 3 };

// size of a packed count word: receptors in the low word, ligands in the high one
KMC_HD int size_of(uint64_t c) { return (int)(uint32_t)c + (int)(c >> 32); }

// index of size n >= 1 in a table clamped at S: n below S, else S ("S or more")
KMC_HD int clamp_size(int n, int S) { return n < S ? n : S; }

// bin of the unordered pair of (clamped) indices a, b in an (S + 1)^2 table: the upper triangle
KMC_HD int pair_index(int a, int b, int S) { return a <= b ? a * (S + 1) + b : b * (S + 1) + a; }

// kind of a piece from its packed counts
KMC_HD int kind_of(uint64_t c) {
  const uint32_t nr = (uint32_t)c, nl = (uint32_t)(c >> 32);
  if (nr == 1 && nl == 0) return CF_KIND_R;
  if (nr == 0 && nl == 1) return CF_KIND_L;
  if (nr == 2 && nl == 0) return CF_KIND_RR;
  return CF_KIND_OTHER;
}

KMC_HD int clamp_pieces(int k) { return k < CF_PIECES - 1 ? k : CF_PIECES - 1; }

// What one core files on one side of an update.  The core has root `root` and
// packed counts `core`; on this side (previous: fragmentation, current:
// merger) it lies in the cluster with label `label`, packed counts `whole`
// and `k` cores.  Nothing is filed when k < 2.  The core whose root is the
// label files the event itself (pieces[min(k, 8)], sizes[|whole|]); when k ==
// 2 the other core files the binary event: the sizes (|core|, |whole| −
// |core|) and the kinds of the two pieces, the other piece's counts being the
// field-wise difference of the two words.
struct Filing {
  int pieces;  // index into pieces[], −1: none
  int whole;   // index into the product / parent sizes, −1: none
  int pair;    // index into the (S + 1)^2 table, −1: none
  int kinds;   // index into the CF_KINDS^2 kind table, −1: none
};

KMC_HD Filing file(int32_t root, uint64_t core, int32_t label, uint64_t whole, int k, int S) {
  Filing f = {-1, -1, -1, -1};
  if (k < 2) return f;
  if (root == label) {
    f.pieces = clamp_pieces(k);
    f.whole = clamp_size(size_of(whole), S);
  } else if (k == 2) {
    const uint64_t other = whole - core;  // no field borrows: the core is a part of the whole
    f.pair = pair_index(clamp_size(size_of(core), S), clamp_size(size_of(other), S), S);
    f.kinds = pair_index(kind_of(core), kind_of(other), CF_KINDS - 1);
  }
  return f;
}

}  // namespace kmcc
