// Prints the host plan of the ragged evidence grid (csrc/blr_grid_ragged_plan.hpp) as one JSON object.  Plain C++17: the host
// compiler builds it, no HIP header and no device.
//   c++ -std=c++17 -o grid_ragged_plan_dump tools/grid_ragged_plan_dump.cpp
//   ./grid_ragged_plan_dump OFFSET0 OFFSET1 ...
// (also the program to run under -fsanitize=address,undefined: nothing to preload)
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../bayesianlinearregressors.jl_amd/csrc/blr_grid_ragged_plan.hpp"

using namespace blr;

int main(int argc, char** argv) {
  if (argc < 2) { fprintf(stderr, "usage: %s OFFSETS...\n", argv[0]); return 2; }
  std::vector<int64_t> offsets;
  for (int i = 1; i < argc; ++i) offsets.push_back(atoll(argv[i]));
  const int64_t B = (int64_t)offsets.size() - 1;
  for (int64_t b = 0; b < B; ++b)
    if (offsets[b + 1] < offsets[b] || offsets[0] < 0 || offsets[b + 1] - offsets[b] > (1 << 30)) {
      fprintf(stderr, "offsets must be non-negative and non-decreasing, every count <= 2^30\n");
      return 2;
    }
  if (B >= (1 << 24) || grid_ragged_slots(offsets.data(), B) >= (1 << 24)) { fprintf(stderr, "too many column blocks\n"); return 2; }
  GridRaggedPlan p;
  plan_grid_ragged(offsets.data(), B, p);
  printf("{\"slots\": %lld, \"reduce\": %s, \"slot0\": [", (long long)p.slots, p.reduce ? "true" : "false");
  for (size_t k = 0; k < p.slot0.size(); ++k) printf("%s%d", k ? ", " : "", p.slot0[k]);
  printf("], \"items\": [");
  for (size_t k = 0; k < p.items.size(); ++k)
    printf("%s{\"reg\": %d, \"n0\": %d, \"n\": %d, \"slot\": %d}", k ? ", " : "", p.items[k].reg, p.items[k].n0, p.items[k].n, p.items[k].slot);
  printf("]}\n");
  return 0;
}
