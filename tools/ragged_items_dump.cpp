// Prints the work-item plan of the ragged marginals / leave-one-out (csrc/blr_ragged_items.hpp) as one JSON object.  Needs no device.
//   hipcc -std=c++17 --offload-arch=gfx950 -o ragged_items_dump tools/ragged_items_dump.cpp
//   ./ragged_items_dump CUS ELEM [KEY=VALUE ...] -- OFFSET0 OFFSET1 ...
// (also the program to run under -Xarch_host -fsanitize=address,undefined: plain host code, nothing to preload)
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../bayesianlinearregressors.jl_amd/csrc/blr_ragged_items.hpp"

using namespace blr;

int main(int argc, char** argv) {
  if (argc < 4) { fprintf(stderr, "usage: %s CUS ELEM [KEY=VALUE ...] -- OFFSETS...\n", argv[0]); return 2; }
  const int cus = atoi(argv[1]), elem = atoi(argv[2]);
  if (cus < 1 || (elem != 4 && elem != 8)) { fprintf(stderr, "bad CUS or ELEM\n"); return 2; }
  BlrOptions opt;
  int i = 3;
  for (; i < argc && strcmp(argv[i], "--"); ++i) {
    const std::string kv(argv[i]);
    const size_t eq = kv.find('=');
    if (eq == std::string::npos || opt.set(kv.substr(0, eq).c_str(), kv.substr(eq + 1).c_str())) { fprintf(stderr, "bad option %s\n", argv[i]); return 2; }
  }
  std::vector<int64_t> offsets;
  for (++i; i < argc; ++i) offsets.push_back(atoll(argv[i]));
  if (offsets.empty()) { fprintf(stderr, "no offsets\n"); return 2; }
  const int64_t B = (int64_t)offsets.size() - 1;
  for (int64_t b = 0; b < B; ++b)
    if (offsets[b + 1] < offsets[b] || offsets[0] < 0) { fprintf(stderr, "offsets must be non-negative and non-decreasing\n"); return 2; }
  RaggedPlan p;
  plan_ragged(offsets.data(), B, cus, elem, opt, p);
  printf("{\"W\": %lld, \"last_chunks\": %lld, \"image_bytes\": %lld, \"chunks\": [", (long long)p.W, (long long)p.last_chunks,
         (long long)(kRaggedImageElems * elem));
  for (size_t c = 0; c < p.chunks.size(); ++c)
    printf("%s{\"b0\": %lld, \"nb\": %lld, \"item0\": %lld, \"nitems\": %lld}", c ? ", " : "", (long long)p.chunks[c].b0, (long long)p.chunks[c].nb,
           (long long)p.chunks[c].item0, (long long)p.chunks[c].nitems);
  printf("], \"items\": [");
  for (size_t k = 0; k < p.items.size(); ++k)
    printf("%s[%d, %d, %d]", k ? ", " : "", p.items[k].reg, p.items[k].first_tile, p.items[k].ntiles);
  printf("]}\n");
  return 0;
}
