// Prints the host plan of the ragged condition / forget pair (csrc/blr_revise_ragged_plan.hpp) as one JSON object.  Plain C++17: the
// host compiler builds it, no HIP header and no device.
//   c++ -std=c++17 -o revise_ragged_plan_dump tools/revise_ragged_plan_dump.cpp
//   ./revise_ragged_plan_dump update|downdate D [SWEEP=always|never|auto] [MAX_CHUNK=n] [NO_DOWNDATE_LDS=1] -- OFFSET0 OFFSET1 ...
// (also the program to run under -fsanitize=address,undefined: nothing to preload)
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../bayesianlinearregressors.jl_amd/csrc/blr_revise_ragged_plan.hpp"

using namespace blr;

// the three handle options the planner reads, with blr_set_option's keys and values
struct Options {
  int sweep = 0, max_chunk = 0;
  bool no_downdate_lds = false;
  bool set(const std::string& key, const std::string& value) {
    if (key == "SWEEP") {
      if (value == "auto") sweep = 0;
      else if (value == "always") sweep = 1;
      else if (value == "never") sweep = 2;
      else return false;
      return true;
    }
    if (key == "MAX_CHUNK") {
      max_chunk = atoi(value.c_str());
      return max_chunk >= 1 && max_chunk <= 65535;
    }
    if (key == "NO_DOWNDATE_LDS") {
      no_downdate_lds = !value.empty();
      return true;
    }
    return false;
  }
};

static void print_list(const char* key, const std::vector<int32_t>& v) {
  printf("\"%s\": [", key);
  for (size_t k = 0; k < v.size(); ++k) printf("%s%d", k ? ", " : "", v[k]);
  printf("]");
}

int main(int argc, char** argv) {
  if (argc < 4) { fprintf(stderr, "usage: %s update|downdate D [KEY=VALUE ...] -- OFFSETS...\n", argv[0]); return 2; }
  const bool down = !strcmp(argv[1], "downdate");
  const long D = atol(argv[2]);
  if ((!down && strcmp(argv[1], "update")) || D < 1 || D > 8192) { fprintf(stderr, "bad direction or D\n"); return 2; }
  Options opt;
  int i = 3;
  for (; i < argc && strcmp(argv[i], "--"); ++i) {
    const std::string kv(argv[i]);
    const size_t eq = kv.find('=');
    if (eq == std::string::npos || !opt.set(kv.substr(0, eq), kv.substr(eq + 1))) { fprintf(stderr, "bad option %s\n", argv[i]); return 2; }
  }
  std::vector<int64_t> offsets;
  for (++i; i < argc; ++i) offsets.push_back(atoll(argv[i]));
  if (offsets.empty()) { fprintf(stderr, "no offsets\n"); return 2; }
  const int64_t B = (int64_t)offsets.size() - 1;
  for (int64_t b = 0; b < B; ++b)
    if (offsets[b + 1] < offsets[b] || offsets[0] < 0) { fprintf(stderr, "offsets must be non-negative and non-decreasing\n"); return 2; }
  ReviseRaggedPlan p;
  plan_revise_ragged(offsets.data(), B, D, down, opt, p);
  printf("{\"serial\": %s, \"chunk\": %lld, \"last_chunks\": %lld, ", p.serial ? "true" : "false", (long long)p.chunk, (long long)p.last_chunks);
  print_list("idle", p.idle);
  printf(", ");
  print_list("sweep", p.sweep);
  printf(", ");
  print_list("refit", p.refit);
  printf("}\n");
  return 0;
}
