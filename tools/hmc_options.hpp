// hmc_options.hpp — hmc_resolve's command line: the reference's option names
// and defaults (HMC.cpp:17-47).  Header-only and free of the C-ABI so that the
// host sanitizer test (tests/test_sanitize.py) can drive it.
#pragma once
#include <cstdlib>
#include <string>
#include <vector>

namespace hmc_cli {

struct Options {
  double min_freq_abs = 1.5, min_freq = -1.0;
  int max_iteration = 1, sample_size = 10, min_len = 1, max_len = 30, device = 0;
  std::vector<std::string> files;
  std::string model = "MV", format = "PHASE";
  int mc_order = 1, num_patterns = -1;
  bool exact = false, output_patterns = false, output_posteriors = false, output_switch_posteriors = false;
  std::string output_pair_posteriors;  // --output-pair-posteriors FILE
  int pair_span = 0;                   // --pair-span K (required with it, >= 1)
  bool have_pair_span = false;
  std::string output_draws;            // --output-draws FILE
  int draws = 100;                     // --draws D (>= 1)
  unsigned long long seed = 0;         // --seed S
  bool have_draws = false, have_seed = false;
  std::string output_dosages;          // --output-dosages FILE
  std::string haplotypes;              // --haplotypes HAPFILE (required with it)
  std::string output_map;              // --output-map FILE
  std::string output_map_given;        // --output-map-given FILE
  std::string evidence;                // --evidence EVFILE (required with it)
  std::string output_ranked;           // --output-ranked FILE
  int ranked = 4;                      // --ranked K (1 .. 16)
  bool have_ranked = false;
  std::string output_windows;          // --output-windows FILE
  std::string windows;                 // --windows WINFILE (required with it)
  int window_k = 8;                    // --window-k K (1 .. 1024)
  bool have_window_k = false;
  bool extended_range = false;         // --extended-range (needs one of the --output-*posteriors / --output-draws / --output-dosages / --output-map / --output-ranked / --output-windows options)
};

// --output-posteriors (no reference counterpart): <first file>.posteriors, the
// posterior of every unordered genotype at the loci where an input allele is
// missing.  The numbers belong to the model of the run's last E-step — the
// final model, since the EM always ends on an E-step — which is not the model
// of the written resolutions when that last E-step's likelihood dropped.
constexpr const char *USAGE =
    "Usage: hmc_resolve [option ...] datafiles\n"
    "  -f, --input-format F  PHASE (default), HPM, HPM2, BENCH2 or BENCH3\n"
    "  -a, --min-freq-abs X  minimum pattern frequency in haplotypes (default 1.5)\n"
    "  -r, --min-freq-rel X  minimum pattern frequency as a fraction (replaces -a)\n"
    "  -n, --num-patterns N  mine by pattern count instead of frequency\n"
    "  -m, --model M         MV (default), MC or MA;  -o, --mc-order K (default 1)\n"
    "  -i, --max-iteration N EM iterations (default 1)\n"
    "  --sample-size S       candidates kept per individual (default 10)\n"
    "  --min-pattern-len N   (default 1)   --max-pattern-len N   (default 30)\n"
    "  --exact-estimate      M-steps by expected counts instead of sampling\n"
    "  --output-patterns X   also write <datafile>.patterns\n"
    "  --device D            GPU index (default 0)\n"
    "  -d, --debug LEVEL     accepted and ignored\n"
    "  --output-posteriors   write <datafile>.posteriors: genotype posteriors at missing loci under the\n"
    "                        final model (the model of the last E-step of the run)\n"
    "  --output-switch-posteriors  write <datafile>.switches: for every pair of consecutive heterozygous\n"
    "                        loci of an individual, the probability that their lower alleles share a\n"
    "                        haplotype (cis) and that they do not (trans), under the final model\n"
    "  --output-pair-posteriors FILE --pair-span K  write FILE: cis and trans for every pair of an\n"
    "                        individual's heterozygous loci at most K heterozygous loci apart (K >= 1)\n"
    "  --output-draws FILE [--draws D] [--seed S]  write FILE: D haplotype pairs per individual drawn\n"
    "                        from the exact posterior under the final model, each with its posterior\n"
    "                        (default D = 100, S = 0; a draw depends on S, the individual and its index)\n"
    "  --output-dosages FILE --haplotypes HAPFILE  write FILE: for every individual the exact expected\n"
    "                        copies of each haplotype of HAPFILE (lines: name start a a a ... [| b b b ...],\n"
    "                        start the 0-based first locus, alleles as the genotype files spell them, ? = any)\n"
    "  --output-map FILE     write FILE: for every individual the most probable haplotype pair under the\n"
    "                        final model, found exactly (no k-best cut), with its status and posterior\n"
    "  --output-map-given FILE --evidence EVFILE  write FILE: as --output-map, over the haplotype pairs\n"
    "                        consistent with the phase sets of EVFILE (tab-separated lines: Id Marker Set\n"
    "                        Allele — the allele on the set's first haplotype, as the genotype files spell\n"
    "                        it; # starts a comment line), with the probability of that evidence\n"
    "  --output-ranked FILE [--ranked K]  write FILE: for every individual the K most probable haplotype\n"
    "                        pairs under the final model, each once, in order, with their posteriors\n"
    "                        (default K = 4, at most 16; an exact ranking, no k-best cut)\n"
    "  --output-windows FILE --windows WINFILE [--window-k K]  write FILE: for every individual and every\n"
    "                        window of WINFILE (lines: name start len, start the 0-based first locus) the K\n"
    "                        most probable haplotype pairs over the window's loci, each with its posterior\n"
    "                        summed over everything outside the window (default K = 8, at most 1024)\n"
    "  --extended-range      the nine options above in extended range: individuals whose likelihood\n"
    "                        underflows a double (panels of more than about 1 200 loci) get lines too";

// 0 on success; otherwise `err` says what is wrong (a missing value, an
// unknown option, no data file).
inline int parse_options(int argc, const char *const *argv, Options &o, std::string &err) {
  for (int i = 1; i < argc; ++i) {
    const std::string a = argv[i];
    const char *v = nullptr;
    auto next = [&]() -> bool {
      if (i + 1 >= argc) {
        err = "missing value for " + a;
        return false;
      }
      v = argv[++i];
      return true;
    };
    if (a == "-a" || a == "--min-freq-abs") { if (!next()) return 1; o.min_freq_abs = atof(v); }
    else if (a == "-r" || a == "--min-freq-rel") { if (!next()) return 1; o.min_freq = atof(v); o.min_freq_abs = 0; }
    else if (a == "-i" || a == "--max-iteration") { if (!next()) return 1; o.max_iteration = atoi(v); }
    else if (a == "--sample-size") { if (!next()) return 1; o.sample_size = atoi(v); }
    else if (a == "--min-pattern-len") { if (!next()) return 1; o.min_len = atoi(v); }
    else if (a == "--max-pattern-len") { if (!next()) return 1; o.max_len = atoi(v); }
    else if (a == "--device") { if (!next()) return 1; o.device = atoi(v); }
    else if (a == "-d" || a == "--debug") { if (!next()) return 1; }                      // Logger level (HMC.cpp:28)
    else if (a == "-f" || a == "--input-format") { if (!next()) return 1; o.format = v; }  // HMC.cpp:29
    else if (a == "--exact-estimate") o.exact = true;                                      // HMC.cpp:42
    else if (a == "--output-patterns") { if (!next()) return 1; o.output_patterns = true; }  // HMC.cpp:30, 229-232
    else if (a == "--output-posteriors") o.output_posteriors = true;
    else if (a == "--output-switch-posteriors") o.output_switch_posteriors = true;
    else if (a == "--output-pair-posteriors") { if (!next()) return 1; o.output_pair_posteriors = v; }
    else if (a == "--pair-span") { if (!next()) return 1; o.pair_span = atoi(v); o.have_pair_span = true; }
    else if (a == "--output-draws") { if (!next()) return 1; o.output_draws = v; }
    else if (a == "--draws") { if (!next()) return 1; o.draws = atoi(v); o.have_draws = true; }
    else if (a == "--output-dosages") { if (!next()) return 1; o.output_dosages = v; }
    else if (a == "--output-map") { if (!next()) return 1; o.output_map = v; }
    else if (a == "--output-map-given") { if (!next()) return 1; o.output_map_given = v; }
    else if (a == "--evidence") { if (!next()) return 1; o.evidence = v; }
    else if (a == "--output-ranked") { if (!next()) return 1; o.output_ranked = v; }
    else if (a == "--ranked") { if (!next()) return 1; o.ranked = atoi(v); o.have_ranked = true; }
    else if (a == "--output-windows") { if (!next()) return 1; o.output_windows = v; }
    else if (a == "--windows") { if (!next()) return 1; o.windows = v; }
    else if (a == "--window-k") { if (!next()) return 1; o.window_k = atoi(v); o.have_window_k = true; }
    else if (a == "--haplotypes") { if (!next()) return 1; o.haplotypes = v; }
    else if (a == "--extended-range") o.extended_range = true;
    else if (a == "--seed") { if (!next()) return 1; o.seed = strtoull(v, nullptr, 10); o.have_seed = true; }
    else if (a == "-m" || a == "--model") { if (!next()) return 1; o.model = v; }          // HMC.cpp:35
    else if (a == "-o" || a == "--mc-order") { if (!next()) return 1; o.mc_order = atoi(v); }      // HMC.cpp:41
    else if (a == "-n" || a == "--num-patterns") { if (!next()) return 1; o.num_patterns = atoi(v); }  // HMC.cpp:38
    else if (!a.empty() && a[0] == '-') { err = "unknown option " + a; return 1; }
    else o.files.push_back(a);
  }
  if (o.files.empty()) {
    err = USAGE;
    return 1;
  }
  if (!o.output_pair_posteriors.empty() && (!o.have_pair_span || o.pair_span < 1)) {
    err = "--output-pair-posteriors needs --pair-span K with K >= 1\n" + std::string(USAGE);
    return 1;
  }
  if (o.have_pair_span && o.output_pair_posteriors.empty()) {
    err = "--pair-span needs --output-pair-posteriors FILE\n" + std::string(USAGE);
    return 1;
  }
  if (!o.output_draws.empty() && o.draws < 1) {
    err = "--output-draws needs --draws D with D >= 1\n" + std::string(USAGE);
    return 1;
  }
  if ((o.have_draws || o.have_seed) && o.output_draws.empty()) {
    err = "--draws and --seed need --output-draws FILE\n" + std::string(USAGE);
    return 1;
  }
  if (o.output_dosages.empty() != o.haplotypes.empty()) {
    err = "--output-dosages FILE and --haplotypes HAPFILE need each other\n" + std::string(USAGE);
    return 1;
  }
  if (o.output_map_given.empty() != o.evidence.empty()) {
    err = "--output-map-given FILE and --evidence EVFILE need each other\n" + std::string(USAGE);
    return 1;
  }
  if (!o.output_ranked.empty() && (o.ranked < 1 || o.ranked > 16)) {
    err = "--output-ranked needs --ranked K with 1 <= K <= 16\n" + std::string(USAGE);
    return 1;
  }
  if (o.have_ranked && o.output_ranked.empty()) {
    err = "--ranked needs --output-ranked FILE\n" + std::string(USAGE);
    return 1;
  }
  if (o.output_windows.empty() != o.windows.empty()) {
    err = "--output-windows FILE and --windows WINFILE need each other\n" + std::string(USAGE);
    return 1;
  }
  if (!o.output_windows.empty() && (o.window_k < 1 || o.window_k > 1024)) {
    err = "--output-windows needs --window-k K with 1 <= K <= 1024\n" + std::string(USAGE);
    return 1;
  }
  if (o.have_window_k && o.output_windows.empty()) {
    err = "--window-k needs --output-windows FILE\n" + std::string(USAGE);
    return 1;
  }
  if (o.extended_range && !o.output_posteriors && !o.output_switch_posteriors && o.output_pair_posteriors.empty() &&
      o.output_draws.empty() && o.output_dosages.empty() && o.output_map.empty() && o.output_map_given.empty() &&
      o.output_ranked.empty() && o.output_windows.empty()) {
    err = "--extended-range needs --output-posteriors, --output-switch-posteriors, --output-pair-posteriors, --output-draws, --output-dosages, --output-map, --output-map-given, --output-ranked or --output-windows\n" +
          std::string(USAGE);
    return 1;
  }
  return 0;
}

}  // namespace hmc_cli
