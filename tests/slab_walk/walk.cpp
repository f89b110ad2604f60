// tests/slab_walk/walk.cpp -- plda_amd/csrc/slab_walk.hpp on its own (tests/test_slab_walk.py): the walk over the recordings
// whose sizes are given on the command line.
//   walk BUDGET_FLOATS N_0 N_1 ...
// prints "largest slabs", then one line per run: "r0 r1 boff[0] ... boff[r1 - r0]".
#include <cstdio>
#include <cstdlib>

#include "slab_walk.hpp"

int main(int argc, char **argv) {
  if (argc < 3) return 2;
  const int64_t budget = std::strtoll(argv[1], nullptr, 10);
  std::vector<int64_t> offsets(1, 0);
  for (int i = 2; i < argc; ++i) offsets.push_back(offsets.back() + std::strtoll(argv[i], nullptr, 10));
  plda::SlabWalk walk(offsets.data(), (int64_t)offsets.size() - 1, budget);
  std::printf("%lld %lld\n", (long long)walk.largest, (long long)walk.slabs);
  for (int pass = 0; pass < 2; ++pass) {      // twice: a rewound walk gives the same runs
    walk.rewind();
    while (walk.next()) {
      std::printf("%lld %lld", (long long)walk.r0, (long long)walk.r1);
      for (int64_t b : walk.boff) std::printf(" %lld", (long long)b);
      std::printf("\n");
    }
  }
  return 0;
}
