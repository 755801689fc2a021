// Prints the host plan of the ragged large-fold leave-fold-out predictives (csrc/blr_kfold_large_ragged_plan.hpp) as one JSON object.
// Needs no device.
//   hipcc -std=c++17 --offload-arch=gfx950 -o kfold_large_ragged_plan_dump tools/kfold_large_ragged_plan_dump.cpp
//   ./kfold_large_ragged_plan_dump CUS ELEM D [KEY=VALUE ...] -- OFFSET0 OFFSET1 ... -- F0 F1 ...
// (also the program to run under -Xarch_host -fsanitize=address,undefined: plain host code, nothing to preload)
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../bayesianlinearregressors.jl_amd/csrc/blr_kfold_large_ragged_plan.hpp"

using namespace blr;

static void print_items(const char* key, const std::vector<KflrItem>& v) {
  printf("\"%s\": [", key);
  for (size_t k = 0; k < v.size(); ++k) printf("%s[%d, %d, %d, %d]", k ? ", " : "", v[k].reg, v[k].fold, v[k].part, v[k].nparts);
  printf("]");
}

int main(int argc, char** argv) {
  if (argc < 6) { fprintf(stderr, "usage: %s CUS ELEM D [KEY=VALUE ...] -- OFFSETS... -- FOLD_SIZES...\n", argv[0]); return 2; }
  const int cus = atoi(argv[1]), elem = atoi(argv[2]), D = atoi(argv[3]);
  if (cus < 1 || (elem != 4 && elem != 8) || D < 1 || D > 128) { fprintf(stderr, "bad CUS, ELEM or D\n"); return 2; }
  BlrOptions opt;
  int i = 4;
  for (; i < argc && strcmp(argv[i], "--"); ++i) {
    const std::string kv(argv[i]);
    const size_t eq = kv.find('=');
    if (eq == std::string::npos || opt.set(kv.substr(0, eq).c_str(), kv.substr(eq + 1).c_str())) { fprintf(stderr, "bad option %s\n", argv[i]); return 2; }
  }
  std::vector<int64_t> offsets, sizes;
  for (++i; i < argc && strcmp(argv[i], "--"); ++i) offsets.push_back(atoll(argv[i]));
  for (++i; i < argc; ++i) sizes.push_back(atoll(argv[i]));
  if (offsets.empty() || sizes.size() + 1 != offsets.size()) { fprintf(stderr, "B + 1 offsets and B fold sizes\n"); return 2; }
  const int64_t B = (int64_t)sizes.size();
  for (int64_t b = 0; b < B; ++b) {
    if (offsets[b + 1] < offsets[b] || offsets[0] < 0) { fprintf(stderr, "offsets must be non-negative and non-decreasing\n"); return 2; }
    if (sizes[b] < 1 || kflr_folds(offsets[b + 1] - offsets[b], sizes[b]) > kKflrMaxFolds) { fprintf(stderr, "bad fold size\n"); return 2; }
  }
  KflrPlan p;
  plan_kfold_large_ragged(offsets.data(), sizes.data(), B, D, cus, elem, opt, p);
  const long long DP = 16 * ((D + 15) / 16);
  printf("{\"tiles_per_group\": %lld, \"last_chunks\": %lld, \"stat_bytes\": %lld, \"u_bytes\": %lld, \"image_bytes\": %lld, \"max_grid\": %lld, "
         "\"max_nb\": %lld, \"max_folds\": %lld, \"max_slots\": %lld, \"regs\": [",
         (long long)p.tiles_per_group, (long long)p.last_chunks, (DP * (DP + 1) / 2 + DP) * 8, (long long)D * D * elem, (long long)(kKflrImageElems * elem),
         (long long)kKflrMaxGrid, (long long)p.max_nb, (long long)p.max_folds, (long long)p.max_slots);
  for (size_t b = 0; b < p.regs.size(); ++b) {
    const KflrReg& r = p.regs[b];
    printf("%s{\"row0\": %lld, \"n\": %d, \"F\": %d, \"nfolds\": %d, \"fold0\": %lld, \"slot0\": %lld, \"S\": %d}", b ? ", " : "", (long long)r.row0, r.n, r.F,
           r.nfolds, (long long)r.fold0, (long long)r.slot0, r.S);
  }
  printf("], \"fold_offsets\": [");
  for (size_t k = 0; k < p.fold_offsets.size(); ++k) printf("%s%lld", k ? ", " : "", (long long)p.fold_offsets[k]);
  printf("], \"chunks\": [");
  for (size_t c = 0; c < p.chunks.size(); ++c) {
    const KflrChunk& k = p.chunks[c];
    printf("%s{\"b0\": %lld, \"nb\": %lld, \"fold0\": %lld, \"nfolds\": %lld, \"slot0\": %lld, \"nslots\": %lld, \"stat0\": %lld, \"nstat\": %lld, "
           "\"red0\": %lld, \"nred\": %lld, \"pred0\": %lld, \"npred\": %lld}",
           c ? ", " : "", (long long)k.b0, (long long)k.nb, (long long)k.fold0, (long long)k.nfolds, (long long)k.slot0, (long long)k.nslots,
           (long long)k.stat0, (long long)k.nstat, (long long)k.red0, (long long)k.nred, (long long)k.pred0, (long long)k.npred);
  }
  printf("], ");
  print_items("stat", p.stat);
  printf(", ");
  print_items("red", p.red);
  printf(", ");
  print_items("pred", p.pred);
  printf("}\n");
  return 0;
}
