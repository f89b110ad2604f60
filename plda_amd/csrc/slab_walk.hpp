// plda_amd/csrc/slab_walk.hpp -- the walk of the operand forms of the clustering family (score_ahc, score_spectral,
// score_dense_pca_ahc) over one slab of fp32 score blocks.  Host only: no handle, no HIP (tests/test_slab_walk.py compiles it
// on its own).
//
// The N x N block of a recording takes slab_padded(N) floats, so every block starts at a 256-byte boundary.  Consecutive
// recordings share a slab for as long as their blocks fit the budget; a recording larger than the budget still gets a slab of
// its own.  A run [r0, r1) is what one slab holds; block r of it starts at boff[r - r0], and the closing entry boff[r1 - r0] is
// the number of floats the run takes.
#pragma once

#include <algorithm>
#include <cstdint>
#include <vector>

namespace plda {

inline int64_t slab_padded(int64_t n) { return (n * n + 63) / 64 * 64; }

struct SlabWalk {
  const int64_t *offsets;
  int64_t R, budget;           // recordings; floats of one slab
  int64_t largest = 0;         // floats of the largest run
  int64_t slabs = 0;           // runs of the whole walk
  int64_t r0 = 0, r1 = 0;      // the current run (none before the first next())
  std::vector<int64_t> boff;   // r1 - r0 + 1 entries

  SlabWalk(const int64_t *offsets_, int64_t R_, int64_t budget_floats) : offsets(offsets_), R(R_), budget(budget_floats) {
    while (next()) { largest = std::max(largest, boff.back()); ++slabs; }
    rewind();
  }
  void rewind() { r0 = r1 = 0; }
  // moves to the next run; false behind the last one
  bool next() {
    r0 = r1;
    boff.assign(1, 0);
    while (r1 < R) {
      const int64_t f = slab_padded(offsets[r1 + 1] - offsets[r1]);
      if (boff.back() && boff.back() + f > budget) break;
      boff.push_back(boff.back() + f);
      ++r1;
    }
    return r1 > r0;
  }
};

}  // namespace plda
