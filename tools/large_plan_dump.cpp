// Prints the plan of the large-D update (csrc/blr_large_plan.hpp) for a fixed table of shapes on a 256-CU part, one JSON line per
// case with every field of LargePlan.  Needs no device: tests/test_large_plan_cpu.py compares the lines with tests/golden/large_plan.json.
//   hipcc -std=c++17 --offload-arch=gfx950 -o large_plan_dump tools/large_plan_dump.cpp && ./large_plan_dump
// (also the program to run under -Xarch_host -fsanitize=address,undefined: plain host code, nothing to preload)
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <initializer_list>
#include <string>
#include <utility>
#include <vector>

#include "../bayesianlinearregressors.jl_amd/csrc/blr_large_plan.hpp"

using namespace blr;

struct Case {
  const char* name;
  LargeShape s;
  std::vector<std::pair<const char*, const char*>> options;  // blr_set_option keys and values
};

// -> the plan, or the planner's error message
static const char* plan_case(const Case& c, const BlrOptions& opt, GramPlanCache& cache, LargePlan& p) {
  return plan_large(c.s, opt, 256, large_ws_cap(opt), cache, p);
}

static void emit(const Case& c, const BlrOptions& opt, const char* err, const LargePlan& p) {
  printf("{\"case\": \"%s\", \"cap\": %zu, ", c.name, large_ws_cap(opt));
  if (err) {
    printf("\"error\": \"%s\", \"route\": \"%s\"}\n", err, p.route ? p.route : "");
    return;
  }
  printf("\"bf3\": %d, \"planes\": %d, \"planes4\": %d, \"rff\": %d, \"x_ring\": %d, \"NP\": %d, \"route\": \"%s\", ", p.bf3, p.planes, p.planes4, p.rff, p.x_ring, p.NP,
         p.route);
  printf("\"DP\": %d, \"NC\": %d, \"NCA\": %d, \"DPA\": %d, \"lda\": %lld, \"ntiles\": %d, \"ntiles_g\": %d, \"NKB\": %d, \"nbchunks\": %d, "
         "\"bslots\": %d, ", p.DP, p.NC, p.NCA, p.DPA, (long long)p.lda, p.ntiles, p.ntiles_g, p.NKB, p.nbchunks, p.bslots);
  printf("\"nsplit\": %d, \"nsplit_diag\": %d, \"nlong\": %d, ", p.nsplit, p.nsplit_diag, p.nlong);
  const LargeLayout& o = p.o;
  printf("\"offsets\": {\"abar\": %zu, \"w\": %zu, \"xp\": %zu, \"gp\": %zu, \"bp\": %zu, \"mu\": %zu, \"qs\": %zu, \"r\": %zu, \"wv\": %zu, "
         "\"q\": %zu, \"l\": %zu, \"m\": %zu, \"sc\": %zu}, \"per\": %zu, ", o.abar, o.w, o.xp, o.gp, o.bp, o.mu, o.qs, o.r, o.wv, o.q, o.l,
         o.m, o.sc, o.per);
  printf("\"G\": %d}\n", p.G);
}

// `large_plan_dump --stdin`: one case per line of standard input,
//   name elem D N col|row iso|diag diag|dense|factor aligned(0|1) G [KEY=VALUE ...]
// printed as the same JSON lines (one plan cache for the run, fresh options per line).  tests/test_large_d_lattice_cpu.py holds the
// route rule of tests/_large_d_problems.py against it.
static int plan_stdin() {
  GramPlanCache cache;
  char line[1024];
  while (fgets(line, sizeof line, stdin)) {
    std::vector<std::string> tok;
    for (char* t = strtok(line, " \t\r\n"); t; t = strtok(nullptr, " \t\r\n")) tok.emplace_back(t);
    if (tok.empty()) continue;
    if (tok.size() < 9) { fprintf(stderr, "%s: 9 fields expected\n", tok[0].c_str()); return 1; }
    auto pick = [&](const std::string& v, std::initializer_list<std::pair<const char*, int>> names, int* out) {
      for (const auto& kv : names)
        if (v == kv.first) { *out = kv.second; return true; }
      fprintf(stderr, "%s: unknown value %s\n", tok[0].c_str(), v.c_str());
      return false;
    };
    LargeShape s{};
    s.elem = atoi(tok[1].c_str()); s.D = atoi(tok[2].c_str()); s.N = atoi(tok[3].c_str());
    if (!pick(tok[4], {{"col", LAYOUT_COLVECS}, {"row", LAYOUT_ROWVECS}}, &s.layout)) return 1;
    if (!pick(tok[5], {{"iso", NOISE_ISOTROPIC}, {"diag", NOISE_DIAGONAL}}, &s.noise_kind)) return 1;
    if (!pick(tok[6], {{"diag", PRIOR_DIAGONAL}, {"dense", PRIOR_DENSE}, {"factor", PRIOR_UPPER_FACTOR}}, &s.prior_kind)) return 1;
    s.x_aligned = atoi(tok[7].c_str()) != 0; s.G = atoi(tok[8].c_str());
    if ((s.elem != 4 && s.elem != 8) || s.D < 1 || s.N < 0 || s.G < 1) { fprintf(stderr, "%s: bad shape\n", tok[0].c_str()); return 1; }
    BlrOptions opt;
    for (size_t i = 9; i < tok.size(); ++i) {
      const size_t eq = tok[i].find('=');
      if (eq == std::string::npos || opt.set(tok[i].substr(0, eq).c_str(), tok[i].substr(eq + 1).c_str())) {
        fprintf(stderr, "%s: bad option %s\n", tok[0].c_str(), tok[i].c_str());
        return 1;
      }
    }
    const Case c{tok[0].c_str(), s, {}};
    LargePlan p{};
    const char* err = plan_case(c, opt, cache, p);
    emit(c, opt, err, p);
  }
  return 0;
}

int main(int argc, char** argv) {
  if (argc == 2 && std::string(argv[1]) == "--stdin") return plan_stdin();
  if (argc != 1) { fprintf(stderr, "usage: %s [--stdin]\n", argv[0]); return 2; }
  const int CV = LAYOUT_COLVECS, RV = LAYOUT_ROWVECS, ISO = NOISE_ISOTROPIC, DIAG = NOISE_DIAGONAL;
  const int PD = PRIOR_DIAGONAL, PF = PRIOR_UPPER_FACTOR, PDENSE = PRIOR_DENSE;
  //                                              elem  D     N      layout noise prior aligned rff    Din S  G
  const std::vector<Case> cases = {
      {"f64_D256_N1000",                         {8, 256,  1000,  CV, ISO,  PD, true,  false, 0,  0, 1},   {}},
      {"f64_D256_N1000_rowvecs",                 {8, 256,  1000,  RV, ISO,  PD, true,  false, 0,  0, 1},   {}},
      {"f32_noplanes_D1024_N16384",              {4, 1024, 16384, CV, ISO,  PD, true,  false, 0,  0, 1},   {{"NO_PLANES", "1"}}},
      {"f32_noplanes_D2048_N16384",              {4, 2048, 16384, CV, ISO,  PD, true,  false, 0,  0, 1},   {{"NO_PLANES", "1"}}},
      {"f32_noplanes_D2048_N16384_again",        {4, 2048, 16384, CV, ISO,  PD, true,  false, 0,  0, 1},   {{"NO_PLANES", "1"}}},
      {"f32_noplanes_D1024_N16384_unaligned",    {4, 1024, 16384, CV, ISO,  PD, false, false, 0,  0, 1},   {{"NO_PLANES", "1"}}},
      {"f32_noplanes_D1024_N16384_rowvecs",      {4, 1024, 16384, RV, ISO,  PD, true,  false, 0,  0, 1},   {{"NO_PLANES", "1"}}},
      {"f32_noplanes_noring_D1024_N16384",       {4, 1024, 16384, CV, ISO,  PD, true,  false, 0,  0, 1},   {{"NO_PLANES", "1"}, {"NO_GRAM_RING", "1"}}},
      {"f32_noplanes_nodiagsplit_D1024_N16384",  {4, 1024, 16384, CV, ISO,  PD, true,  false, 0,  0, 1},   {{"NO_PLANES", "1"}, {"NO_DIAG_SPLIT", "1"}}},
      {"f32_nobf16x3_D1024_N16384",              {4, 1024, 16384, CV, ISO,  PD, true,  false, 0,  0, 1},   {{"NO_BF16X3", "1"}}},
      {"f32_nobf16x3_D2048_N16384",              {4, 2048, 16384, CV, ISO,  PD, true,  false, 0,  0, 1},   {{"NO_BF16X3", "1"}}},
      {"f32_default_D1024_N16384",               {4, 1024, 16384, CV, ISO,  PD, true,  false, 0,  0, 1},   {}},
      {"f32_default_D2048_N16384",               {4, 2048, 16384, CV, ISO,  PD, true,  false, 0,  0, 1},   {}},
      {"f32_default_D1024_N16384_unaligned",     {4, 1024, 16384, CV, ISO,  PD, false, false, 0,  0, 1},   {}},
      {"f32_default_D1024_N16384_rowvecs",       {4, 1024, 16384, RV, ISO,  PD, true,  false, 0,  0, 1},   {}},
      {"f32_planes8_D1024_N16384",               {4, 1024, 16384, CV, ISO,  PD, true,  false, 0,  0, 1},   {{"PLANES8", "1"}}},
      {"f32_nofp16planes_D1024_N16385",          {4, 1024, 16385, CV, ISO,  PD, true,  false, 0,  0, 1},   {{"NO_FP16_PLANES", "1"}}},
      {"f32_rff_Din4_D512_N4096",                {4, 512,  4096,  CV, ISO,  PD, true,  true,  4,  0, 1},   {}},
      {"f32_rff_Din16_D512_N4096",               {4, 512,  4096,  CV, ISO,  PD, true,  true,  16, 0, 1},   {}},
      {"f32_rff_Din16_nofp16planes",             {4, 512,  4096,  CV, ISO,  PD, true,  true,  16, 0, 1},   {{"NO_FP16_PLANES", "1"}}},
      {"f32_rff_Din16_planes8",                  {4, 512,  4096,  CV, ISO,  PD, true,  true,  16, 0, 1},   {{"PLANES8", "1"}}},
      {"f32_rff_noplanes_error",                 {4, 512,  4096,  CV, ISO,  PD, true,  true,  16, 0, 1},   {{"NO_PLANES", "1"}}},
      {"f32_rff_Din833_error",                   {4, 512,  4096,  CV, ISO,  PD, true,  true,  833, 0, 1},  {}},
      {"f32_multi_S3_D1024_N16384",              {4, 1024, 16384, CV, ISO,  PD, true,  false, 0,  3, 1},   {}},
      {"f32_multi_S100_D200_N777_diag",          {4, 200,  777,   CV, DIAG, PDENSE, true, false, 0, 100, 1}, {}},
      {"f32_multi_S3_factor_error",              {4, 1024, 16384, CV, ISO,  PF, true,  false, 0,  3, 1},   {}},
      {"f32_multi_S3_nofp16planes_error",        {4, 1024, 16384, CV, ISO,  PD, true,  false, 0,  3, 1},   {{"NO_FP16_PLANES", "1"}}},
      {"f32_noplanes_splits_15_11",              {4, 1024, 16384, CV, ISO,  PD, true,  false, 0,  0, 1},   {{"NO_PLANES", "1"}, {"GRAM_SPLITS", "15,11"}}},
      {"f32_noplanes_splits_14_14",              {4, 1024, 16384, CV, ISO,  PD, true,  false, 0,  0, 1},   {{"NO_PLANES", "1"}, {"GRAM_SPLITS", "14,14"}}},
      {"f32_noplanes_splits_8_4_64",             {4, 2048, 16384, CV, ISO,  PD, true,  false, 0,  0, 1},   {{"NO_PLANES", "1"}, {"GRAM_SPLITS", "8,4,64"}}},
      {"f32_noplanes_splits_8_8_500",            {4, 2048, 16384, CV, ISO,  PD, true,  false, 0,  0, 1},   {{"NO_PLANES", "1"}, {"GRAM_SPLITS", "8,8,500"}}},
      {"f32_noplanes_splits_15_11_unaligned",    {4, 1024, 16384, CV, ISO,  PD, false, false, 0,  0, 1},   {{"NO_PLANES", "1"}, {"GRAM_SPLITS", "15,11"}}},
      {"f32_noplanes_splits_99_1_ignored",       {4, 1024, 16384, CV, ISO,  PD, true,  false, 0,  0, 1},   {{"NO_PLANES", "1"}, {"GRAM_SPLITS", "99,1"}}},
      {"f32_default_splits_5_5",                 {4, 1024, 16384, CV, ISO,  PD, true,  false, 0,  0, 1},   {{"GRAM_SPLITS", "5,5"}}},
      {"f64_splits_6_3",                         {8, 512,  8192,  CV, ISO,  PD, true,  false, 0,  0, 1},   {{"GRAM_SPLITS", "6,3"}}},
      {"f32_factor_prior_D384_N200",             {4, 384,  200,   CV, ISO,  PF, true,  false, 0,  0, 1},   {}},
      {"f32_factor_prior_noplanes_D384_N200",    {4, 384,  200,   CV, ISO,  PF, true,  false, 0,  0, 1},   {{"NO_PLANES", "1"}}},
      {"f64_factor_prior_D384_N200",             {8, 384,  200,   CV, ISO,  PF, true,  false, 0,  0, 1},   {}},
      {"f32_dense_prior_D384_N200",              {4, 384,  200,   CV, ISO,  PDENSE, true, false, 0, 0, 1}, {}},
      {"f64_dense_prior_D384_N200",              {8, 384,  200,   RV, ISO,  PDENSE, true, false, 0, 0, 1}, {}},
      {"f32_diag_noise_D384_N200",               {4, 384,  200,   CV, DIAG, PD, true,  false, 0,  0, 1},   {}},
      {"f64_diag_noise_factor_D384_N201",        {8, 384,  201,   CV, DIAG, PF, true,  false, 0,  0, 1},   {}},
      {"f32_D200_N300",                          {4, 200,  300,   CV, ISO,  PD, true,  false, 0,  0, 1},   {}},
      {"f32_noplanes_D200_N300",                 {4, 200,  300,   CV, ISO,  PD, true,  false, 0,  0, 1},   {{"NO_PLANES", "1"}}},
      {"f64_D200_N300",                          {8, 200,  300,   CV, ISO,  PD, true,  false, 0,  0, 1},   {}},
      {"f32_D256_N0",                            {4, 256,  0,     CV, ISO,  PD, true,  false, 0,  0, 1},   {}},
      {"f64_D256_N0_G4",                         {8, 256,  0,     CV, ISO,  PD, true,  false, 0,  0, 4},   {}},
      {"f32_D256_N1",                            {4, 256,  1,     CV, ISO,  PD, true,  false, 0,  0, 1},   {}},
      {"f32_D8192_N100000",                      {4, 8192, 100000, CV, ISO, PD, true,  false, 0,  0, 1},   {}},
      {"f32_G128_D256_N512",                     {4, 256,  512,   CV, ISO,  PD, true,  false, 0,  0, 128}, {}},
      {"f32_G128_D256_N512_ws12",                {4, 256,  512,   CV, ISO,  PD, true,  false, 0,  0, 128}, {{"CHAIN_WS_MB", "12"}}},
      {"f32_G128_D256_N512_ws1",                 {4, 256,  512,   CV, ISO,  PD, true,  false, 0,  0, 128}, {{"CHAIN_WS_MB", "1"}}},
      {"f32_noplanes_G128_D256_N512",            {4, 256,  512,   CV, ISO,  PD, true,  false, 0,  0, 128}, {{"NO_PLANES", "1"}}},
      {"f32_noplanes_G128_D256_N512_ws12",       {4, 256,  512,   CV, ISO,  PD, true,  false, 0,  0, 128}, {{"NO_PLANES", "1"}, {"CHAIN_WS_MB", "12"}}},
      {"f32_noplanes_G8_D512_N4096_ws40",        {4, 512,  4096,  CV, ISO,  PD, true,  false, 0,  0, 8},   {{"NO_PLANES", "1"}, {"CHAIN_WS_MB", "40"}}},
      {"f64_G128_D256_N512",                     {8, 256,  512,   CV, ISO,  PD, true,  false, 0,  0, 128}, {}},
      {"f64_G128_D256_N512_ws12",                {8, 256,  512,   CV, ISO,  PD, true,  false, 0,  0, 128}, {{"CHAIN_WS_MB", "12"}}},
      {"f64_G16_D1024_N2048_ws100",              {8, 1024, 2048,  CV, DIAG, PDENSE, true, false, 0, 0, 16}, {{"CHAIN_WS_MB", "100"}}},
      {"f32_G3_D384_N200_factor_diag",           {4, 384,  200,   CV, DIAG, PF, true,  false, 0,  0, 3},   {}},
  };
  GramPlanCache cache;  // one for the process, as a handle keeps one: the second D = 2048 case finds the first one's plan
  for (const Case& c : cases) {
    BlrOptions opt;
    for (const auto& kv : c.options)
      if (opt.set(kv.first, kv.second)) { fprintf(stderr, "%s: bad option %s\n", c.name, kv.first); return 1; }
    LargePlan p{};
    const char* err = plan_case(c, opt, cache, p);
    emit(c, opt, err, p);
  }
  return 0;
}
