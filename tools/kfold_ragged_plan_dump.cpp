// Prints the host plan of the ragged leave-fold-out predictives (csrc/blr_kfold_ragged_plan.hpp) as one JSON object.  Needs no device.
//   hipcc -std=c++17 --offload-arch=gfx950 -o kfold_ragged_plan_dump tools/kfold_ragged_plan_dump.cpp
//   ./kfold_ragged_plan_dump CUS ELEM D F [KEY=VALUE ...] -- OFFSET0 OFFSET1 ...
// (also the program to run under -Xarch_host -fsanitize=address,undefined: plain host code, nothing to preload)
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../bayesianlinearregressors.jl_amd/csrc/blr_kfold_ragged_plan.hpp"

using namespace blr;

static void print_list(const char* key, const std::vector<int64_t>& v) {
  printf("\"%s\": [", key);
  for (size_t k = 0; k < v.size(); ++k) printf("%s%lld", k ? ", " : "", (long long)v[k]);
  printf("]");
}

int main(int argc, char** argv) {
  if (argc < 6) { fprintf(stderr, "usage: %s CUS ELEM D F [KEY=VALUE ...] -- OFFSETS...\n", argv[0]); return 2; }
  const int cus = atoi(argv[1]), elem = atoi(argv[2]), D = atoi(argv[3]), F = atoi(argv[4]);
  if (cus < 1 || (elem != 4 && elem != 8) || D < 1 || D > 128 || F < 1 || F > kFoldRaggedMaxF) { fprintf(stderr, "bad CUS, ELEM, D or F\n"); return 2; }
  BlrOptions opt;
  int i = 5;
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
  KfoldRaggedPlan p;
  plan_kfold_ragged(offsets.data(), B, F, D, cus, elem, opt, p);
  printf("{\"W\": %lld, \"last_chunks\": %lld, \"image_bytes\": %lld, \"row_bytes\": %lld, \"max_rows\": %lld, \"max_nb\": %lld, \"chunks\": [",
         (long long)p.W, (long long)p.last_chunks, (long long)(kRaggedImageElems * elem), (long long)(16 * ((D + 15) / 16) * elem),
         (long long)p.max_rows, (long long)p.max_nb);
  for (size_t c = 0; c < p.chunks.size(); ++c)
    printf("%s{\"b0\": %lld, \"nb\": %lld, \"item0\": %lld, \"nitems\": %lld}", c ? ", " : "", (long long)p.chunks[c].b0, (long long)p.chunks[c].nb,
           (long long)p.chunks[c].item0, (long long)p.chunks[c].nitems);
  printf("], \"items\": [");
  for (size_t k = 0; k < p.items.size(); ++k)
    printf("%s[%d, %d, %d]", k ? ", " : "", p.items[k].reg, p.items[k].first_tile, p.items[k].ntiles);
  printf("], ");
  print_list("pack_offsets", p.pack_offsets);
  printf(", ");
  print_list("fold_offsets", p.fold_offsets);
  printf("}\n");
  return 0;
}
