// hmc_resolve — C++ drop-in for HMC's resolve mode (HMC.cpp:179-233) built on
// the C-ABI of libhmc_amd.so.  Reads the input files in the given format
// (HaploFile::getHaploFile + readGenoData), runs HaploModel::run on the GPU
// and writes <first file>.reconstructed in the same format
// (HaploFile::writeGenoData; BENCH2/3 also rewrite the position file, as
// HaploFileBench::writeGenoData does), and with --output-patterns the
// .patterns dump (HMC.cpp:229-232).  Options use the reference's names and
// defaults (HMC.cpp:17-47).
//
//   hmc_resolve [-f PHASE|HPM|HPM2|BENCH2|BENCH3] [-a 1.5] [-r min_freq] [-n num]
//               [-m MV|MC|MA] [-o mc_order] [--exact-estimate] [-i 1]
//               [--sample-size 10] [--min-pattern-len 1] [--max-pattern-len 30]
//               [--output-patterns x] [--output-posteriors] [--output-switch-posteriors]
//               [--output-pair-posteriors FILE --pair-span K]
//               [--output-draws FILE [--draws 100] [--seed 0]]
//               [--output-dosages FILE --haplotypes HAPFILE] [--output-map FILE]
//               [--output-map-given FILE --evidence EVFILE]
//               [--output-ranked FILE [--ranked 4]]
//               [--output-windows FILE --windows WINFILE [--window-k 8]] [--extended-range] [--device 0] datafile ...
// --output-posteriors (no reference counterpart) writes <first file>.posteriors:
// genotype posteriors at the loci with a missing input allele, under the final
// model (hmc_write_posteriors).  --output-switch-posteriors (none either)
// writes <first file>.switches: cis and trans posteriors between consecutive
// heterozygous loci under the same model (hmc_write_switch_posteriors).
// --output-pair-posteriors FILE --pair-span K (none either) writes FILE: cis
// and trans for every pair of an individual's heterozygous loci at most K
// heterozygous loci apart (hmc_write_pair_posteriors).
// --output-draws FILE [--draws D] [--seed S] (none either) writes FILE: D
// haplotype pairs per individual drawn from the exact posterior under the
// final model, each with its posterior (hmc_write_posterior_draws).
// --output-dosages FILE --haplotypes HAPFILE (none either) writes FILE: for
// every individual the exact expected copies of each haplotype listed in
// HAPFILE (hmc_hapfile.hpp; hmc_write_haplotype_dosages).
// --output-map FILE (none either) writes FILE: every individual's most
// probable haplotype pair under the final model, found exactly, with its
// status and posterior (hmc_write_map_phase).
// --output-map-given FILE --evidence EVFILE (none either) writes FILE: as
// --output-map over the haplotype pairs consistent with the phase sets listed
// in EVFILE (hmc_read_evidence), with the probability of that evidence
// (hmc_write_map_phase_given).
// --output-ranked FILE [--ranked K] (none either) writes FILE: every
// individual's K most probable haplotype pairs under the final model, each
// once, in order, with their posteriors (hmc_write_ranked_phasings).
// --output-windows FILE --windows WINFILE [--window-k K] (none either) writes
// FILE: for every individual and every window listed in WINFILE
// (hmc_winfile.hpp) the K most probable haplotype pairs over the window's loci,
// each with its posterior summed over everything outside the window
// (hmc_write_window_phasings); the Window column is the window's place in WINFILE, from 0.
// --extended-range (none either) runs those nine in extended range
// (hmc_set_posterior_range): individuals whose likelihood underflows a double
// get lines too.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <string>
#include <vector>

#include "../include/hmc_amd.h"
#include "hmc_hapfile.hpp"
#include "hmc_options.hpp"
#include "hmc_winfile.hpp"

int main(int argc, char **argv) {
  hmc_cli::Options o;
  std::string perr;
  if (hmc_cli::parse_options(argc, argv, o, perr)) {
    fprintf(stderr, "%s\n", perr.c_str());
    return 1;
  }
  const double min_freq_abs = o.min_freq_abs, min_freq = o.min_freq;
  const int max_iteration = o.max_iteration, sample_size = o.sample_size, min_len = o.min_len, max_len = o.max_len,
            device = o.device, mc_order = o.mc_order, num_patterns = o.num_patterns;
  const std::vector<std::string> &files = o.files;
  const std::string &model = o.model, &format = o.format;
  const bool exact = o.exact, output_patterns = o.output_patterns;
  hmc_ctx *ctx = nullptr;
  int rc = hmc_ctx_create(device, &ctx);
  auto die = [&](const char *what) {
    fprintf(stderr, "%s failed (%d): %s\n", what, rc, hmc_ctx_error(ctx));
    hmc_ctx_destroy(ctx);
    exit(1);
  };
  if (rc) die("hmc_ctx_create");
  if ((rc = hmc_set_params(ctx, min_freq_abs, min_freq, min_len, max_len, sample_size))) die("hmc_set_params");
  if ((rc = hmc_set_model(ctx, model.c_str(), mc_order))) die("hmc_set_model");
  if ((rc = hmc_set_num_patterns(ctx, num_patterns))) die("hmc_set_num_patterns");
  if ((rc = hmc_set_exact_estimate(ctx, exact ? 1 : 0))) die("hmc_set_exact_estimate");
  printf("Reading genotype file ...\n");
  std::vector<const char *> names;
  for (auto &f : files) names.push_back(f.c_str());
  if ((rc = hmc_load_files(ctx, format.c_str(), names.data(), (int)names.size()))) die("hmc_load_files");
  int N = 0, L = 0, A = 0;
  hmc_panel_info(ctx, &N, &L, &A);
  printf("Succesfully read Haplotype file with %d markers and %d genotypes.\n", L, N);
  hmc_cli::HapList haps;
  if (!o.haplotypes.empty()) {  // read before the run: a malformed list fails at once
    std::string types((size_t)L + 1, '\0'), herr;
    if ((rc = hmc_parse_files(format.c_str(), names.data(), (int)names.size(), nullptr, nullptr, nullptr, &types[0], nullptr)))
      die("hmc_parse_files");
    types.resize((size_t)L);
    std::ifstream hf(o.haplotypes);
    if (!hf) {
      fprintf(stderr, "Can not open file %s!\n", o.haplotypes.c_str());
      hmc_ctx_destroy(ctx);
      return 1;
    }
    if (hmc_cli::parse_hapfile(hf, types, haps, herr)) {
      fprintf(stderr, "%s\n", herr.c_str());
      hmc_ctx_destroy(ctx);
      return 1;
    }
  }
  hmc_cli::WinList wins;
  if (!o.windows.empty()) {  // read before the run: a malformed list fails at once
    std::string werr;
    std::ifstream wf(o.windows);
    if (!wf) {
      fprintf(stderr, "Can not open file %s!\n", o.windows.c_str());
      hmc_ctx_destroy(ctx);
      return 1;
    }
    if (hmc_cli::parse_winfile(wf, L, wins, werr)) {
      fprintf(stderr, "%s\n", werr.c_str());
      hmc_ctx_destroy(ctx);
      return 1;
    }
  }
  std::vector<int32_t> ev_i, ev_l, ev_s, ev_f;
  if (!o.evidence.empty()) {  // read before the run: a malformed file fails at once
    int64_t n_ev = 0;
    if ((rc = hmc_read_evidence(ctx, o.evidence.c_str(), &n_ev, nullptr, nullptr, nullptr, nullptr, 0))) die("hmc_read_evidence");
    ev_i.resize((size_t)n_ev + 1);
    ev_l.resize((size_t)n_ev + 1);
    ev_s.resize((size_t)n_ev + 1);
    ev_f.resize((size_t)n_ev + 1);
    if ((rc = hmc_read_evidence(ctx, o.evidence.c_str(), &n_ev, ev_i.data(), ev_l.data(), ev_s.data(), ev_f.data(), n_ev)))
      die("hmc_read_evidence");
    ev_i.resize((size_t)n_ev);
  }
  hmc_iter_log log[256];
  int iters = 0, np0 = 0;
  double t_m0 = 0;
  uint64_t rm0 = 0;
  if ((rc = hmc_run(ctx, max_iteration, log, 256, &iters, &t_m0, &rm0, &np0))) die("hmc_run");
  printf("Found haplotype patterns: %d (%.3f s)\n", np0, t_m0);
  double solve = t_m0;
  for (int k = 0; k < iters && k < 256; ++k) {
    printf("  Switch Error = %f, IHP = %f, IGP = %f, LL = %f\n", log[k].switch_error, log[k].ihp, log[k].igp,
           log[k].log_likelihood);  // HaploModel.cpp:135-136
    printf("  iteration %d: LL = %f, patterns = %d, E %.3f s, M %.3f s\n", k + 1, log[k].log_likelihood,
           log[k].n_patterns, log[k].t_estep_s, log[k].t_mstep_s);
    solve += log[k].t_estep_s + log[k].t_mstep_s;
  }
  printf("Solving Time = %f\n", solve);
  // HaploFile::writeGenoData(resolutions, ".reconstructed") on the first file
  std::vector<std::string> outs{files[0] + ".reconstructed"};
  if (format == "BENCH2" || format == "BENCH3") outs.push_back(files.size() > 1 ? files[1] : "");
  std::vector<const char *> onames;
  for (auto &f : outs) onames.push_back(f.c_str());
  if ((rc = hmc_write_files(ctx, format.c_str(), onames.data(), (int)onames.size()))) die("hmc_write_files");
  if (output_patterns) {
    const std::string pf = files[0] + ".patterns";
    if ((rc = hmc_write_patterns(ctx, pf.c_str()))) die("hmc_write_patterns");
  }
  if ((rc = hmc_set_posterior_range(ctx, o.extended_range ? 1 : 0))) die("hmc_set_posterior_range");
  if (o.output_posteriors) {  // of the run's last E-step: hmc_run ends on an E-step of the final model
    const std::string qf = files[0] + ".posteriors";
    if ((rc = hmc_write_posteriors(ctx, qf.c_str()))) die("hmc_write_posteriors");
  }
  if (o.output_switch_posteriors) {  // of the same E-step
    const std::string sf = files[0] + ".switches";
    if ((rc = hmc_write_switch_posteriors(ctx, sf.c_str()))) die("hmc_write_switch_posteriors");
  }
  if (!o.output_pair_posteriors.empty()) {  // of the same E-step
    if ((rc = hmc_write_pair_posteriors(ctx, o.output_pair_posteriors.c_str(), o.pair_span))) die("hmc_write_pair_posteriors");
  }
  if (!o.output_draws.empty()) {  // of the same E-step
    if ((rc = hmc_write_posterior_draws(ctx, o.output_draws.c_str(), o.draws, o.seed))) die("hmc_write_posterior_draws");
  }
  if (!o.output_dosages.empty()) {  // of the same E-step
    std::vector<const char *> hn;
    for (auto &x : haps.names) hn.push_back(x.c_str());
    const std::vector<int32_t> ha = haps.padded(false), hb = haps.padded(true);
    if ((rc = hmc_write_haplotype_dosages(ctx, o.output_dosages.c_str(), (int)hn.size(), hn.data(), haps.start.data(),
                                          haps.len.data(), haps.maxlen, ha.data(), haps.two_sided ? hb.data() : nullptr)))
      die("hmc_write_haplotype_dosages");
  }
  if (!o.output_map.empty()) {  // of the same E-step
    if ((rc = hmc_write_map_phase(ctx, o.output_map.c_str()))) die("hmc_write_map_phase");
  }
  if (!o.output_map_given.empty()) {  // of the same E-step
    if ((rc = hmc_write_map_phase_given(ctx, o.output_map_given.c_str(), (int64_t)ev_i.size(), ev_i.data(), ev_l.data(),
                                        ev_s.data(), ev_f.data())))
      die("hmc_write_map_phase_given");
  }
  if (!o.output_ranked.empty()) {  // of the same E-step
    if ((rc = hmc_write_ranked_phasings(ctx, o.output_ranked.c_str(), o.ranked))) die("hmc_write_ranked_phasings");
  }
  if (!o.output_windows.empty()) {  // of the same E-step
    if ((rc = hmc_write_window_phasings(ctx, o.output_windows.c_str(), (int)wins.names.size(), wins.start.data(), wins.len.data(),
                                        o.window_k)))
      die("hmc_write_window_phasings");
  }
  hmc_ctx_destroy(ctx);
  return 0;
}
