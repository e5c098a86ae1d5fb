// Records of the weight-copy kernels (elementwise.hip: cast, refresh of many copies, AdamW + refresh), the search for the record that
// owns a block, and the condition under which a tile is moved four elements at a time.  Plain C++ shared by the kernels and by
// tests/host/test_weight_tile.cpp.
#pragma once
#include <stdint.h>

#include "tile_index.h"

// One matrix with compute copies: rows x cols fp32 master w (dense, row stride cols), the row-major 16-bit copy w16 (row stride ld) and
// the transposed one w16t (row stride ldt), either of which may be NULL.  The matrix owns tiles [tile0, tile0 of the next record) of
// a 1-D grid of 64 x 64 tiles, tiles_x of them per tile row.
struct CastDesc {
  const float* w;
  uint16_t* w16;
  uint16_t* w16t;
  int rows, cols, ld, ldt, tile0, tiles_x;
};
static_assert(sizeof(CastDesc) == 48, "vmc_cast_weights_multi descriptor layout (include/vmc.h)");

// A parameter without compute copies: n elements at offset off of the arenas, blocks [block0, block0 of the next record), 1024
// elements per block.
struct AdamRange {
  unsigned long long off;
  int n, block0;
};
static_assert(sizeof(AdamRange) == 16, "vmc_adam_cast_multi range layout (include/vmc.h)");

VMC_HD int first_block(const CastDesc& d) { return d.tile0; }
VMC_HD int first_block(const AdamRange& r) { return r.block0; }

// Index of the last of the n records (first blocks ascending, rec[0] starts at block 0) whose first block is <= b.
template <typename R>
VMC_HD int owner_of_block(const R* __restrict__ rec, int n, int b) {
  int lo = 0, hi = n - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (first_block(rec[mid]) <= b) lo = mid; else hi = mid - 1;
  }
  return lo;
}

// The vector path of a tile: 16-byte accesses to the master (and to whatever lies at the same offset of 16-byte aligned parallel
// arrays: gradient and moments), 8-byte stores to both copies.  Every row of the matrix must allow it, so shape and strides are
// multiples of 4; a record that fails is moved element by element instead.
VMC_HD bool tile_vec_ok(const CastDesc& d) {
  return ((uintptr_t)d.w & 15) == 0 && (d.cols & 3) == 0 && (d.rows & 3) == 0 &&
         (!d.w16 || ((d.ld & 3) == 0 && ((uintptr_t)d.w16 & 7) == 0)) && (!d.w16t || ((d.ldt & 3) == 0 && ((uintptr_t)d.w16t & 7) == 0));
}
