/* hmc_amd.h — C-ABI of libhmc_amd.so, the MI355X-native HaploModel EM.
 *
 * The reference (Wu-Lab/HMC v0.9.1) has no plugin or FFI surface: its hot path
 * is the C++ class seam HaploModel::run -> HaploBuilder::resolve /
 * PatternManager::findPatternByFreq inside one binary.  Each entry point below
 * replaces one of those seams; the citation names the reference interface it
 * stands in for.  Conventions:
 *   - plain pointers and sizes, no C++ or torch types;
 *   - host buffers are caller-owned, device buffers are owned by the context;
 *   - every function returns 0 (HMC_OK) or a negative HMC_E* code; the text of
 *     the last failure is available from hmc_ctx_error().  The reference's
 *     fatal errors (Logger::error + exit(1)) become return codes here;
 *   - allele symbols are the reference's Allele values (the ASCII code for SNP
 *     'S' loci, the integer for microsatellite 'M' loci), -1 = missing;
 *   - one host thread per context.
 */
#ifndef HMC_AMD_H
#define HMC_AMD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define HMC_OK 0
#define HMC_EARG -1         /* invalid argument / call order */
#define HMC_EHIP -2         /* HIP runtime failure */
#define HMC_EIO -3          /* file could not be read or written */
#define HMC_EUNSUPPORTED -4 /* parameter outside what the GPU path implements */
#define HMC_ENOPATTERN -5   /* "Can not find matching pattern!" (HaploBuilder.cpp:215-217) */
#define HMC_ERCCL -6        /* RCCL failure */
#define HMC_ENOMEM -7       /* device memory exhausted */

typedef struct hmc_ctx hmc_ctx;

/* ---- context ---------------------------------------------------------- */
/* One context per GPU.  Replaces constructing HaploModel (HaploModel.h:29). */
int hmc_ctx_create(int device, hmc_ctx **out);
/* Multi-GPU: one process per GPU; `unique_id` = 128 bytes from
 * hmc_rccl_unique_id() on rank 0, broadcast by the caller.  Individuals are
 * sharded in contiguous blocks; the M-step all-reduces per-level sums. */
int hmc_rccl_unique_id(void *out128);
int hmc_ctx_create_dist(int device, int rank, int world, const void *unique_id, hmc_ctx **out);
/* Multi-GPU on a communicator the caller already owns (an ncclComm_t, RCCL):
 * rank and world are taken from it; hmc_ctx_destroy leaves it alive.  The
 * seam of SURVEY.md §8(b) (hmc_ctx_create(device, rccl_comm_or_null, ...)),
 * replacing HaploModel's construction (HaploModel.h:29) inside a host that
 * runs its own RCCL. */
int hmc_ctx_create_comm(int device, void *rccl_comm, hmc_ctx **out);
/* An RCCL communicator made by the RCCL this library is linked with (for
 * hosts without their own RCCL binding, and tests: a communicator from a
 * second copy of librccl in the process would not be usable here). */
int hmc_rccl_comm_init(int device, int world, int rank, const void *unique_id, void **comm);
int hmc_rccl_comm_destroy(void *comm);
/* Same sharding with a caller-supplied collective instead of RCCL: fn must
 * sum `n` doubles element-wise across ranks in place and return 0.  Lets
 * several ranks share one GPU (tests) or run over any host transport. */
typedef int (*hmc_allreduce_fn)(double *buf, size_t n, void *user);
int hmc_ctx_create_hostcoll(int device, int rank, int world, hmc_allreduce_fn fn, void *user, hmc_ctx **out);
/* Test hook: a one-rank context made with a unique id or a communicator runs
 * every collective of the sharded path anyway (results unchanged), so the
 * RCCL calls are exercised on a one-GPU machine.  HMC_EARG on a context
 * without a communicator. */
int hmc_set_force_collectives(hmc_ctx *ctx, int on);
void hmc_ctx_destroy(hmc_ctx *ctx);
const char *hmc_ctx_error(const hmc_ctx *ctx);

/* Cross-rank sums of a sharded run (M-step candidate sums per mining level,
 * log-likelihood, total sample weight).  0 (default) = ordered: rank r
 * continues each running sum of ranks 0..r-1 over its contiguous block of
 * items, which reproduces the reference's sequential sums
 * (PatternManager.cpp:254-262, HaploModel.cpp:110, HaploData.cpp:120-126) bit
 * for bit — a point-to-point chain per mining level (ncclRecv from r-1,
 * the rank's adds, ncclSend to r+1; one ncclBroadcast from W-1); 1 = all-reduce of per-rank
 * partial sums (one collective, sums reassociated: last-bit drift, which can
 * flip a pattern at the min_freq threshold). */
int hmc_set_reduction(hmc_ctx *ctx, int mode);

/* HaploModel public parameters (HaploModel.h:15-26; CLI defaults HMC.cpp:35-47).
 * min_freq_abs > 0 overrides min_freq exactly as HaploModel::findPatterns does
 * (HaploModel.cpp:54-56).  sample_size 1..64 (HaploPair's k-best lists,
 * HaploBuilder.cpp:44, HaploPair.cpp:85-88; above 32 the split E-step only);
 * larger values fail the E-step with HMC_EUNSUPPORTED. */
int hmc_set_params(hmc_ctx *ctx, double min_freq_abs, double min_freq, int min_pattern_len, int max_pattern_len,
                   int sample_size);

/* HaploModel::setModel + mc_order (HaploModel.cpp:26-36, 65-76; HMC.cpp:35,41):
 * "MV" (default; patterns by frequency), "MC" (Markov chain of order mc_order:
 * PatternManager::findPatternBlock(mc_order+1), every candidate of that length,
 * head length mc_order+1), "MA" (MV; its adjustFrequency only range-checks). */
int hmc_set_model(hmc_ctx *ctx, const char *model, int mc_order);
/* HaploModel::exact_estimate (--exact-estimate, HMC.cpp:42; HaploModel.cpp:
 * 140-141): after an E-step, hmc_find_patterns (and hmc_run) re-estimate the
 * table with PatternManager::estimatePatterns (PatternManager.cpp:364-438):
 * expected pattern counts under the current model, from a forward-backward
 * pass and a ForwardPatternTree walk per individual and start locus
 * (HaploBuilder.cpp:263-450), candidates grown by extendPatterns; M0 still
 * mines the genotypes.  Model MC re-estimates the table in place.
 * Frequencies agree with the reference to rounding (its sums run in pointer
 * order); they are deterministic and independent of the sharding. */
int hmc_set_exact_estimate(hmc_ctx *ctx, int on);
/* Last exact M-step: rounds of estimateFrequency, candidates estimated, and
 * device ms of the trie walks. */
int hmc_last_exact_stats(const hmc_ctx *ctx, int *rounds, uint64_t *candidates, double *walk_ms);
/* The last exact M-step's breadth-first walk: work units (trie nodes of an
 * individual and start locus), kernel launches, units deferred for room, and
 * the individuals walked over pruned records (forward likelihoods that
 * underflow: extend()'s test, HaploBuilder.cpp:237, 291-314). */
int hmc_last_exact_walk(const hmc_ctx *ctx, int64_t *units, int64_t *launches, int64_t *deferred, int *pruned);
/* HaploModel::num_patterns (HMC.cpp:38): > 0 mines with
 * PatternManager::findPatternByNum (PatternManager.cpp:44-70, models MV/MA);
 * <= 0 (default) with findPatternByFreq. */
int hmc_set_num_patterns(hmc_ctx *ctx, int num_patterns);

/* ---- panel (GenoData / HaploFile) --------------------------------------- */
/* HaploFile::readGenoData for the PHASE format (HaploFile.cpp:54-118). */
int hmc_load_phase(hmc_ctx *ctx, const char *path);
/* Same panel from memory: alleles[N][2][L] symbols, types[L] ('S' or 'M').
 * Runs GenoData::checkAlleleSymbol (GenoData.cpp:78-118) and uploads. */
int hmc_load_genotypes(hmc_ctx *ctx, int N, int L, const int32_t *alleles, const char *types);
int hmc_panel_info(const hmc_ctx *ctx, int *N, int *L, int *max_alleles);
/* This rank's individuals [i0, i1): contiguous blocks balanced by E-step cost
 * (L/8 + heterozygous-or-missing loci per individual); [0, N) on one rank. */
int hmc_shard_range(const hmc_ctx *ctx, int *i0, int *i1);
/* Measurement hook of a one-rank context: from here on the E-step and the
 * M-step's scans cover individuals [i0, i1) of the loaded panel only, with
 * the current model (e.g. the M0 mined over the whole panel) — rank r's own
 * E-step work of an N-rank run, on one GPU (tools/cfg4_rank.py).  Drops the
 * samples and every per-individual estimate.  Replaces no reference
 * interface. */
int hmc_set_shard(hmc_ctx *ctx, int i0, int i1);
/* Per-locus allele tables: num[L], sym[L][max_alleles], freq[L][max_alleles]
 * (GenoData::allele_num / allele_symbol / allele_frequency, GenoData.h:43-49). */
int hmc_allele_table(const hmc_ctx *ctx, int32_t *num, int32_t *sym, double *freq);

/* ---- M-step: PatternManager::findPatternByFreq (PatternManager.cpp:27-42) --
 * Mines from the genotypes while no E-step samples exist (M0), from the
 * weighted samples afterwards, then runs initialize() (ids, head list,
 * successors).  *n_patterns = patterns found; *r_m = candidate x item scan
 * steps (SURVEY.md §8d R_M, local to this rank). */
int hmc_find_patterns(hmc_ctx *ctx, int *n_patterns, uint64_t *r_m);
/* Per-level seam of the same search: PatternManager::checkFrequency
 * (PatternManager.cpp:146-193, called for each candidate by searchPattern
 * :100-144) for n caller-given candidates of length `level` — start[n],
 * alleles[n][level] as symbols.  freq[c] = the pattern frequency the reference
 * assigns: genotype branch (no samples yet) sum over individuals of
 * getMatchingFrequency (:267-291) / N, sample branch sum of matching sample
 * weights / total weight; sums in item order and, across ranks, in rank order
 * (hmc_set_reduction).  *scanned = n x items of this rank. */
int hmc_mine_level(hmc_ctx *ctx, int level, int n, const int32_t *start, const int32_t *alleles, double *freq,
                   uint64_t *scanned);
int hmc_model_info(const hmc_ctx *ctx, int *n_patterns, int *head_len);
/* Blocks of start loci for the search (0 = automatic: one block up to about
 * 2.5e7 individual-loci of panel, else blocks of about that size; always one
 * block for findPatternByNum and heads longer than 1 locus).  The roots of
 * searchPattern's DFS are independent (PatternManager.cpp:90-108): blocks
 * from locus L-1 down give the same table, ids and successors, with the
 * candidate-node memory of two blocks and the matching lists of one, for any
 * pattern length.  A block whose nodes or lists do not fit in device memory
 * (or in hmc_set_mine_memory's cap) is re-run with half the width, and the
 * blocks below it keep that width. */
int hmc_set_mine_block(hmc_ctx *ctx, int start_loci);
/* Last E-step: the largest frontier (states at one locus of one individual)
 * and the state capacity it ran with (grows by doubling on overflow, up to
 * 2 097 151 states: 21-bit state ids in the records and list links). */
int hmc_last_estep_frontier(hmc_ctx *ctx, int *max_states, int *frontier_cap);
/* Cap on one search level's matching lists, in bytes (0 = device memory
 * only; 12 B per entry of the genotype branch, 4 B of the sample branch):
 * a level over the cap splits its block as if memory had run out. */
int hmc_set_mine_memory(hmc_ctx *ctx, uint64_t list_bytes);
/* Last search: blocks, candidate nodes created (all blocks) and the size of
 * the node arrays kept (GB, ~70 B per node). */
int hmc_last_mine_stats(const hmc_ctx *ctx, int *blocks, int64_t *nodes, double *node_window_gb);
/* Cross-rank reduction of the last pattern search (multi-rank contexts):
 * device ms from the first to the last collective of each mining level,
 * summed (the ordered chain's mine_sum launches included), and the number of
 * levels reduced.  0 / 0 on one rank.  Replaces no reference interface
 * (the reference is single-process). */
int hmc_last_mine_reduction(const hmc_ctx *ctx, double *ms, int *levels);
/* Point-to-point hops of the ordered chain issued by this context since its
 * creation: ncclSend calls, ncclRecv calls and bytes received (a forced
 * one-rank context sends each hop to itself, grouped).  Replaces no reference
 * interface. */
int hmc_comm_stats(const hmc_ctx *ctx, int64_t *sends, int64_t *recvs, uint64_t *bytes_received);
/* Structure pass (tuning, results unchanged): LDS probes of the key table
 * (m_best_pair) before a key goes to its HBM tier; default 16. */
int hmc_set_key_probes(hmc_ctx *ctx, int probes);
/* Structure pass (tuning, results unchanged): the block's LDS split — key
 * slots and contributions per frontier state, in tenths (0 = defaults: 40 and
 * 20 at 4 waves per individual, 20 and 20 otherwise). */
int hmc_set_structure_tier(hmc_ctx *ctx, int key_mult10, int contrib_mult10);
/* Bounded waits of an RCCL context (default 1800 s): every stream sync polls
 * ncclCommGetAsyncError; on an asynchronous error or after `seconds` without
 * the stream draining, the communicator is aborted (ncclCommAbort — a
 * caller-owned communicator too: do not destroy it afterwards) and the call
 * returns HMC_ERCCL, as does every later collective of the context.  A rank
 * whose neighbour died therefore ends instead of hanging in ncclRecv. */
int hmc_set_comm_timeout(hmc_ctx *ctx, double seconds);
/* Test hook of the bounded wait: keeps the context stream busy for `ms`
 * (one wavefront, bounded) and syncs it through the same wait. */
int hmc_debug_stall(hmc_ctx *ctx, double ms);
/* Pattern table in id order (HaploPattern.h:16-98).  succ[P][max_alleles]
 * holds pattern ids (-1 = none); alleles[P][maxlen] symbols (-1 padding).
 * Any output pointer may be NULL. */
int hmc_get_patterns(hmc_ctx *ctx, int32_t *start, int32_t *len, double *freq, double *prefix, double *tp,
                     int32_t *succ, int32_t *alleles, int maxlen);
/* Install an externally built pattern table (test seam: lets the E-step be
 * checked against another implementation's M-step output).  last_symbol[P] is
 * the pattern's last allele; succ as above. */
int hmc_set_patterns(hmc_ctx *ctx, int P, const int32_t *start, const int32_t *len, const double *freq,
                     const double *tp, const int32_t *succ, const int32_t *last_symbol);
/* The same with every pattern's whole string, alleles[P][maxlen] as
 * hmc_get_patterns returns them, and its prefix frequency.  The strings are
 * kept, so unlike hmc_set_patterns the table may have head_len > 1 and may be
 * followed by an exact M-step. */
int hmc_set_patterns_spelled(hmc_ctx *ctx, int P, const int32_t *start, const int32_t *len, const int32_t *alleles,
                             int maxlen, const double *freq, const double *prefix, const double *tp,
                             const int32_t *succ);

/* ---- E-step: HaploModel::resolveAll (HaploModel.cpp:79-115) ------------
 * Resolves every individual of this rank's shard with HaploBuilder::resolve
 * (HaploBuilder.cpp:35-126), keeps the weighted samples on the device for the
 * next M-step, and returns the log-likelihood (all ranks), the number of
 * samples (this rank) and R_E (retained k-best links, this rank). */
int hmc_resolve_all(hmc_ctx *ctx, double *log_likelihood, int *n_samples, uint64_t *r_e);
/* Per individual of the shard: genotype probability (total forward
 * likelihood), number of candidates, status (0 ok, 1 unresolved), and per
 * candidate [n][sample_size] prior / posterior / sample weight. */
int hmc_get_estep(hmc_ctx *ctx, double *total, int32_t *ncand, int32_t *status, double *prior, double *posterior,
                  double *weight);
/* Largest number of HaploPair states any locus of each individual held in the
 * last E-step (diagnostic). */
int hmc_get_estep_stats(hmc_ctx *ctx, int32_t *fmax);
/* Per individual of the shard: E-step time of the last E-step in units of
 * 1024 shader clocks (value pass; the scheduling key of the next E-step). */
int hmc_get_estep_cost(hmc_ctx *ctx, int32_t *cost);
/* Diagnostic build (libhmc_amd_diag.so) only: shader-cycle / event counters
 * of the last E-step summed over waves, out40[0, 20) the value pass (or fused
 * kernel), out40[20, 36) the structure pass; zeros in the product build. */
int hmc_get_stamps(hmc_ctx *ctx, uint64_t *out40);
/* HaploData samples of this rank: alleles[H][L] symbols, weights[H]. */
int hmc_get_samples(hmc_ctx *ctx, int32_t *alleles, double *weights, double *total_weight);
/* Drop the samples so the next hmc_find_patterns mines the genotypes again
 * (HaploBuilder::setGenoData clears m_samples, HaploBuilder.cpp:19-23). */
int hmc_clear_samples(hmc_ctx *ctx);
/* Selected pair per individual of the last E-step ([n][2][L] symbols;
 * unresolved individuals keep the input genotype, HaploBuilder.cpp:117-124). */
int hmc_get_resolutions(hmc_ctx *ctx, int32_t *out);
/* Posterior of the unordered genotype at every (individual, locus) of this
 * rank's shard where an input allele is missing, under the current model:
 * P({x, y} at the locus | genotype) = the sum of forward x backward likelihood
 * over the lattice states that carry {x, y}, over P(genotype) — exact, with no
 * k-best cut and no sampling (hmc_get_resolutions gives the alleles of the
 * best pair of the E-step's k-best list only; hmc_map_phase gives the most
 * probable pair).  Needs a preceding hmc_resolve_all (any
 * E-step mode); runs its own forward-backward pass and changes no later
 * result.  With indiv, locus, status and post all NULL the call only counts:
 * *n_sites from the panel, *n_pairs = A (A + 1) / 2 for A = max_alleles
 * (hmc_panel_info), and no device work.  Otherwise (any of the four may be
 * NULL) sites come individual-major with loci ascending: indiv[n_sites]
 * (panel index), locus[n_sites], status[n_sites], post[n_sites][n_pairs].
 * status: 0 ok; 1 the individual is unresolved; 2 the individual's
 * P(genotype) (hmc_get_estep's total) is subnormal, below DBL_MIN — panels of
 * thousands of loci: the likelihoods are raw doubles and have lost their bits
 * there, a row could miss 1 by any amount.  Rows of status 1 and 2 are zeros.
 * Bin hi (hi + 1) / 2 + lo holds the pair of allele indices lo <= hi, which
 * index the locus's allele table (hmc_allele_table: sym[locus][lo],
 * sym[locus][hi]); bins no state carries are 0.  A row of status 0 sums to 1
 * up to rounding.  A site at a
 * locus below head_len (an individual with a missing allele at a head locus)
 * comes from the reference's head pairing (initHeadList, HaploBuilder.cpp:
 * 153-224), which is not a phasing model: only its normalisation holds there.
 * HMC_EARG when no E-step has run or the model has changed since the last one
 * (an M-step, hmc_set_patterns): P(genotype) of that E-step is the divisor.
 * The bits do not depend on launch shapes, store budgets or sharding.
 * HMC_EUNSUPPORTED as for the exact M-step (more than 44 alleles at a locus,
 * too many contributions at a locus, an injected table with head_len > 1).
 * Replaces no reference interface. */
int hmc_genotype_posteriors(hmc_ctx *ctx, int64_t *n_sites, int *n_pairs, int32_t *indiv, int32_t *locus, int32_t *status,
                            double *post);
/* Last hmc_genotype_posteriors: device ms of its structure passes, of the
 * forward-backward kernel and of the site kernel; groups the individuals ran
 * in; individuals on pruned records (underflowing forward likelihoods). */
int hmc_last_posterior_stats(const hmc_ctx *ctx, double *structure_ms, double *fb_ms, double *sites_ms, int *groups,
                             int *n_pruned);

/* Switch posteriors: how sure the phase is between consecutive heterozygous
 * loci.  For an individual let h1 < h2 < ... be the loci where both input
 * alleles are present and differ; its sites are the pairs (locus_a, locus_b) =
 * (h_q, h_q+1) (the loci between are homozygous or have a missing allele).
 * post[site][0] (cis) = P(the allele of lower allele-table index at locus_a
 * and the one of lower index at locus_b lie on the same haplotype | genotype)
 * under the current model, post[site][1] (trans) the same for different
 * haplotypes (indices as in hmc_allele_table).  Both are exact sums of forward
 * x backward likelihood over the lattice states, with no k-best cut and no
 * sampling, and each is a sum of its own: a row of status 0 sums to 1 up to
 * rounding.  Needs a preceding hmc_resolve_all (any E-step mode); runs its own
 * forward-backward pass and changes no later result.  With indiv, locus_a,
 * locus_b, status and post all NULL the call only counts: *n_sites from the
 * panel, no device work and no model needed.  Otherwise (any of the five may
 * be NULL) sites of this rank's shard come individual-major with locus_a
 * ascending: indiv[n_sites] (panel index), locus_a[n_sites], locus_b[n_sites],
 * status[n_sites], post[n_sites][2].  status as for hmc_genotype_posteriors:
 * 0 ok; 1 the individual is unresolved; 2 its P(genotype) is below DBL_MIN;
 * rows of status 1 and 2 are zeros.  A site with locus_a below head_len of an
 * individual with a missing allele at a head locus comes from the reference's
 * head pairing, which is not a phasing model: only the normalisation holds.
 * HMC_EARG when no E-step has run or the model has changed since the last one;
 * HMC_EUNSUPPORTED as for hmc_genotype_posteriors.  The bits do not depend on
 * launch shapes, store budgets, sharding or hmc_set_switch_tier.
 * Replaces no reference interface. */
int hmc_switch_posteriors(hmc_ctx *ctx, int64_t *n_sites, int32_t *indiv, int32_t *locus_a, int32_t *locus_b, int32_t *status,
                          double *post);
/* Last hmc_switch_posteriors: device ms of its structure passes, of the
 * forward-backward kernel and of the labelled forward sweep; groups the
 * individuals ran in; individuals on pruned records; individuals whose largest
 * frontier exceeded the sweep's LDS tier and went through device memory.
 * Replaces no reference interface. */
int hmc_last_switch_stats(const hmc_ctx *ctx, double *structure_ms, double *fb_ms, double *sweep_ms, int *groups,
                          int *n_pruned, int *n_spilled);
/* Pair posteriors: cis / trans for any two heterozygous loci of an individual,
 * any distance apart (compound heterozygotes, phase-confidence matrices).  A
 * query q is (indiv[q], locus_a[q], locus_b[q]) with locus_a < locus_b, both
 * heterozygous in the input (both alleles present and different); queries need
 * not be consecutive, sorted or distinct.  post[q][0] (cis) and post[q][1]
 * (trans) are defined as for hmc_switch_posteriors, by lower allele-table
 * index, and are exact sums over the lattice states: the consecutive switch
 * posteriors cannot be multiplied along the way, because the switches are not
 * independent under a variable-order chain.  One labelled forward sweep per
 * individual carries several anchors at once; anchors that overlap more than
 * the sweep holds take further rounds, so any set of queries works.  Rows come
 * in the caller's order: status[n], post[n][2] (either may be NULL); status
 * 0 / 1 / 2 as for hmc_switch_posteriors, rows of status 1 and 2 are zeros.
 * For a query whose locus_b is the next heterozygous locus after locus_a the
 * row has the bits hmc_switch_posteriors returns for that site.  n = 0 is
 * HMC_OK with no device work.  HMC_EARG, with a message naming the first
 * offending query, when an individual is outside this rank's shard, when
 * locus_a >= locus_b, when a locus is out of range or when a locus is not
 * heterozygous in the input for that individual; HMC_EARG when no E-step has
 * run or the model has changed since the last one; HMC_EUNSUPPORTED as for
 * hmc_genotype_posteriors.  Runs its own forward-backward pass and changes no
 * later result.  The bits of a row depend on the model and on (indiv,
 * locus_a, locus_b) alone: not on the other queries of the call, launch
 * shapes, store budgets, sharding or hmc_set_pair_tuning.
 * Replaces no reference interface. */
int hmc_pair_posteriors(hmc_ctx *ctx, int64_t n, const int32_t *indiv, const int32_t *locus_a, const int32_t *locus_b,
                        int32_t *status, double *post);
/* The queries (h_q, h_q+d), 1 <= d <= span, of every individual of this
 * rank's shard, h1 < h2 < ... its heterozygous loci: individual-major, then
 * locus_a ascending, then locus_b ascending; *n of them.  With indiv, locus_a
 * and locus_b NULL the call only counts; it needs no model and no device.
 * span = 1 is the site list of hmc_switch_posteriors.  HMC_EARG for span < 1.
 * Replaces no reference interface. */
int hmc_pair_span_list(hmc_ctx *ctx, int span, int64_t *n, int32_t *indiv, int32_t *locus_a, int32_t *locus_b);
/* Last hmc_pair_posteriors: device ms of its structure passes, of the
 * forward-backward kernel and of the labelled forward sweep; groups the
 * individuals ran in; individuals on pruned records; individuals whose largest
 * frontier exceeded the sweep's LDS tier and went through device memory; the
 * slots per state (NS) the sweep used; the largest number of rounds any
 * individual took.  Replaces no reference interface. */
int hmc_last_pair_stats(const hmc_ctx *ctx, double *structure_ms, double *fb_ms, double *sweep_ms, int *groups, int *n_pruned,
                        int *n_spilled, int *slots, int *max_rounds);
/* Haplotype dosages: the exact expected number of copies of caller-given
 * haplotypes an individual carries, under the model of the last E-step — what
 * haplotype association and haplotype-frequency estimates need (the column
 * mean over individuals, halved, is the population haplotype frequency).
 * A pattern p is the window start[p] .. start[p] + len[p] - 1 with two rows of
 * allele symbols, alleles_a[p][k] and alleles_b[p][k] (k < len[p]; arrays of
 * [n_patterns][maxlen], entries past len[p] ignored); -1 in a row means "any
 * allele"; alleles_b = NULL means all -1.  For haplotypes x, y let M_p(x, y)
 * be true when at every locus k of the window A[k] is -1 or equals x[k] and
 * B[k] is -1 or equals y[k].  With post({h0, h1}) the exact posterior over
 * unordered pairs (the one hmc_posterior_draws samples):
 *     d[i][p] = sum over pairs {h0, h1} of post({h0, h1}) ([M_p(h0, h1)] + [M_p(h1, h0)])
 * — always two terms, also when h0 = h1.  Consequences:
 *   B all -1 (one-sided): d is the expected number of the individual's two
 *     haplotypes that carry A on the window, the haplotype dosage, in [0, 2];
 *     a homozygous carrier has 2.
 *   Some locus where A and B are both given and differ: no pair matches in
 *     both orientations, so d is the posterior probability of the
 *     configuration, in [0, 1].  Two heterozygous loci with -1 between them
 *     give cis or trans; every locus given is the posterior of that whole pair
 *     (a read-backed phase set, another tool's phasing, the truth set).
 *   A and B both all -1: d = 2 up to rounding (allowed: a normalisation check).
 *   A symbol the locus's allele table does not hold matches nothing: d is
 *     exactly 0.0, no error (scans include absent haplotypes).
 * The sum runs over the lattice states exactly, by a labelled forward sweep
 * that filters by the pattern at every locus of its window: a path adds its
 * posterior once for each orientation in which its two haplotypes match, and
 * by the path-to-pair bookkeeping stated under hmc_posterior_draws (a
 * heterozygous head state carries its factor 2, a heterozygous pair behind a
 * homozygous prefix is two paths of half each, a homozygous pair is one path)
 * the paths of a pair add exactly the two-term sum above.
 * indiv[n] are panel indices inside this rank's shard, in any order, repeats
 * allowed; indiv = NULL means the whole shard (n is ignored).  Outputs, either
 * of which may be NULL: dosage[n][n_patterns], status[n]; status 0 / 1 / 2 as
 * for hmc_switch_posteriors, rows of status 1 and 2 are zeros.  For an
 * individual with a missing allele at a head locus, loci below head_len come
 * from the reference's head pairing, which is not a phasing model: for a
 * window that touches them only the normalisation holds.
 * n = 0 or n_patterns = 0 is HMC_OK with no device work.  HMC_EARG, with a
 * message naming the first offender, for an individual outside this rank's
 * shard and for a pattern with start < 0, len < 1, len > maxlen or start + len
 * > L; HMC_EARG when no E-step has run or the model has changed since the last
 * one; HMC_EUNSUPPORTED as for hmc_genotype_posteriors.  Runs its own
 * forward-backward pass, over the individuals asked for only, and changes no
 * later result; the rows go through the device in batches of at most 512 MiB.
 * The bits of d[i][p] depend on the model, the range setting
 * (hmc_set_posterior_range), i and p's own (start, len, A, B) alone: not on
 * the other patterns or their order, the other individuals, the slots, rounds
 * and tier of hmc_set_dosage_tuning, launch shapes, store budgets, groups or
 * sharding.  Replaces no reference interface. */
int hmc_haplotype_dosages(hmc_ctx *ctx, int64_t n, const int32_t *indiv, int n_patterns, const int32_t *start,
                          const int32_t *len, int maxlen, const int32_t *alleles_a, const int32_t *alleles_b, double *dosage,
                          int32_t *status);
/* Last hmc_haplotype_dosages: as hmc_last_pair_stats; rounds: the sweeps over
 * the records the call's plan took (more than one when more windows overlap
 * than the sweep has slots).  All zero after a call with n = 0 or
 * n_patterns = 0.  Replaces no reference interface. */
int hmc_last_dosage_stats(const hmc_ctx *ctx, double *structure_ms, double *fb_ms, double *sweep_ms, int *groups, int *n_pruned,
                          int *n_spilled, int *slots, int *rounds);
/* Posterior draws: whole haplotype pairs sampled from the exact posterior
 * P(pair | genotype) under the model of the last E-step — what multiple
 * imputation and the posterior of any statistic that is no one- or two-locus
 * marginal need.  (hmc_get_samples is the E-step's truncated, deterministic
 * k-best list, not a sample; "samples" keeps meaning those.)
 * indiv[n] are panel indices inside this rank's shard, in any order, repeats
 * allowed; indiv = NULL means the whole shard (n is ignored).  Outputs, any of
 * which may be NULL: hap[n][draws][2][L] symbols, prob[n][draws], status[n].
 * status 0 ok; 1 the individual is unresolved; 2 its P(genotype) is below
 * DBL_MIN (as hmc_genotype_posteriors).  Rows of status 1 and 2 carry the
 * input genotype in every draw (as hmc_get_resolutions does for unresolved
 * individuals) and prob 0.
 *
 * One draw is one path through the forward lattice.  Record j (head_len <= j
 * <= L) holds the states after j loci; a state t has a transition product
 * tpv[t] and, above the head record, a list of contributions in record order,
 * each naming a predecessor state of record j - 1 and a rev flag; fwd_j[t] is
 * the forward likelihood exact_fb computes (tpv[t] times the sum of the
 * predecessors' fwd in list order; at the head record tpv[t], doubled for a
 * heterozygous head pair).
 *   Selection rule, used for every choice: given terms x_0, x_1, ... >= 0 in a
 *   fixed order, a full sum T and a uniform u, take the first index whose
 *   running sum exceeds u * T (one rounded product); if none does, the last
 *   index with a positive term.  A term of 0 is never chosen.
 *   Final record (step 0): terms fwd_L[t] in state order, F states in chunks
 *   of 64.  Chunk c's sum is the butterfly sum of its 64 values (zeros past
 *   F): v[i] += v[i ^ 32], then ^ 16, 8, 4, 2, 1.  The chunk prefix is S_c =
 *   S_c-1 + (chunk c's sum), in chunk order from S_-1 = 0, and T = S_last.
 *   The chunk is the first with S_c > u * T; inside it the running sum starts
 *   at S_c-1 and adds fwd_L[t] state by state, and the rule above picks t
 *   among the chunk's states.
 *   Record j = L, L - 1, ..., head_len + 1 (step 1 + (L - j)), current state
 *   t: terms fwd_(j-1)[pred(r)] over t's contributions r in record order, T
 *   their sum accumulated from 0 in that order (the common factor tpv[t]
 *   cancels), the running sum likewise.  The chosen contribution's
 *   predecessor is the state at record j - 1.
 *   Uniforms: Philox4x32-10 with key (seed & 0xFFFFFFFF, seed >> 32) and
 *   counter (step, draw index, panel index of the individual, 0) gives words
 *   w0..w3; u = ((w0 >> 5) * 2^26 + (w1 >> 6)) * 2^-53, in [0, 1).
 *   Haplotypes, as the E-step's traceback spells a candidate: a side parity
 *   starts at 0; at record j the state's two alleles (a, b) of locus j - 1 go
 *   to haplotypes (parity, 1 - parity), then the parity flips if the chosen
 *   contribution has rev set.  The head state supplies loci below head_len
 *   from its two head patterns.  Which of a draw's two haplotypes comes first
 *   carries no information.
 *   prob = the exact posterior of the unordered pair drawn: p = tpv of the
 *   final state, times tpv of each chosen state from record L - 1 down to the
 *   head record, one multiplication each in that order; doubled if the two
 *   haplotypes differ at any locus; divided by the last E-step's P(genotype)
 *   (hmc_get_estep's total).  A heterozygous pair with a homozygous prefix is
 *   reached by two paths (rev or not out of the homozygous state), each with
 *   half of it; a heterozygous head carries the factor 2 itself; a homozygous
 *   pair has one path: the factor belongs to the pair, not the path.
 * So a draw's bits depend on the model and on (seed, individual, draw index)
 * alone: not on `draws` (draw d of 8 is draw d of 8 192), the other
 * individuals of the call, sharding, launch shapes, store budgets or groups.
 * An individual with a missing allele at a head locus draws its loci below
 * head_len from the reference's head pairing (initHeadList, HaploBuilder.cpp:
 * 153-224), which is not a phasing model.
 * Needs a preceding hmc_resolve_all (any E-step mode); runs its own exact-mode
 * structure pass and forward pass, over the individuals asked for only, and
 * changes no later result.  The kernel stores allele indices draw-minor and a
 * second kernel transposes them into hap's layout as symbols; the individuals
 * go through the device in batches whose outputs take at most 512 MiB (one
 * individual at least: 8 draws + 10 draws L bytes each), so the host memory a
 * call needs is the caller's three outputs plus one batch of prob.  n = 0 is
 * HMC_OK with no device work.  HMC_EARG when no E-step has run or the model
 * has changed since the last one, with a message naming the first individual
 * outside the shard, or for draws < 1; HMC_EUNSUPPORTED as for
 * hmc_genotype_posteriors.
 * Replaces no reference interface. */
int hmc_posterior_draws(hmc_ctx *ctx, int64_t n, const int32_t *indiv, int draws, uint64_t seed, int32_t *hap, double *prob,
                        int32_t *status);
/* Last hmc_posterior_draws: device ms of its structure passes, of the forward
 * kernel and of the draw kernel with its transposition; groups the individuals ran in;
 * individuals on pruned records.  Replaces no reference interface. */
int hmc_last_draw_stats(const hmc_ctx *ctx, double *structure_ms, double *fb_ms, double *draw_ms, int *groups, int *n_pruned);
/* MAP phasing: the haplotype pair of largest exact posterior P(pair |
 * genotype) under the model of the last E-step, and that posterior — the
 * phasing to report, with its confidence.  (hmc_get_resolutions gives the best
 * pair of the E-step's k-best list, which is the most probable pair only when
 * the maximiser survived the beam; a posterior draw finds the mode by luck.)
 * indiv[n] are panel indices inside this rank's shard, in any order, repeats
 * allowed; indiv = NULL means the whole shard (n is ignored).  Outputs, any of
 * which may be NULL: hap[n][2][L] symbols, prob[n], status[n]; status 0 / 1 / 2
 * as for hmc_posterior_draws, rows of status 1 and 2 carry the input genotype
 * and prob 0.
 *
 * The lattice is the one stated under hmc_posterior_draws.  A pair's value is
 * the draws' prob numerator: the product of its path's tpv, doubled if the two
 * haplotypes differ anywhere.  A heterozygous pair behind a homozygous prefix
 * is two mirror paths of half each, and one state is reached by homozygous and
 * by heterozygous prefixes (variable-order contexts forget history), so the
 * max-product sweep carries two values per state t of a record:
 *   Vh[t]  the best product over paths to t whose two haplotypes are equal so far,
 *   Vd[t]  the best pair value, the factor 2 inside, over paths that differ already.
 *   Head record: a homozygous head state has (Vh, Vd) = (tpv, 0), a
 *   heterozygous one (0, tpv * 2.0).
 *   Record j above it, state t with alleles (xa, xb) and contributions r in
 *   record order, primes for record j - 1:
 *     xa == xb:  Vh[t] = tpv[t] * max_r Vh'[pred r],  Vd[t] = tpv[t] * max_r Vd'[pred r]
 *     else:      Vh[t] = 0,  Vd[t] = tpv[t] * max_r max(Vd'[pred r], 2.0 * Vh'[pred r])
 *   — one multiplication per state and label, after the maximum.
 *   Tie rules.  Final record: candidates (t, label) in order of t, Vh before
 *   Vd within a state; the largest value, among equals the first.  Going down
 *   from state t with label l at record j: the first contribution in record
 *   order that attains the maximum above; l = h reads Vh', l = d with xa == xb
 *   reads Vd', l = d with xa != xb reads per contribution Vd' and then
 *   2.0 * Vh' (choosing the latter continues with label h).
 *   Haplotypes are spelled as a draw's: side parity, flipped by the chosen
 *   contribution's rev flag after the state's alleles are written; the head
 *   state supplies loci below head_len.  Which haplotype comes first carries
 *   no information.
 *   prob by the draws' rule, so that the two calls mean the same number: tpv
 *   of the final state times tpv of each chosen state down to the head record,
 *   one multiplication each in that order; doubled if the haplotypes differ at
 *   any locus; divided by P(genotype).
 * Range (hmc_set_posterior_range).  Regular: raw doubles, the divisor is the
 * last E-step's P(genotype); an individual whose forward likelihood underflows
 * goes through the pruned records as in the other posterior calls, and one
 * whose max-product values fall below DBL_MIN (the best pair is far less
 * probable than the genotype, so on long panels its product underflows where
 * P(genotype) does not) is swept again with rescaled records as in extended
 * range — the same choices wherever the raw values kept their bits — so
 * status 0 / 1 / 2 fall exactly where hmc_posterior_draws puts them; the traced
 * product is kept as mantissa and exponent in both ranges.  Extended:
 * every record's values (both labels) are multiplied by the power of two that
 * brings the record's largest into [0.5, 1) — exact, so no choice changes,
 * except that an entry more than 2^1021 below its record's maximum loses bits,
 * which could only matter for a path that far behind — the traced product is
 * kept as mantissa and exponent, the divisor is the scaled forward pass's own
 * total, and status 2 never occurs.
 * The result's bits depend on the model, the range setting and the individual
 * alone: not on the other individuals of the call, sharding, launch shapes,
 * store budgets or groups.  An individual with a missing allele at a head
 * locus gets its loci below head_len from the reference's head pairing, which
 * is not a phasing model.
 * Needs a preceding hmc_resolve_all (any E-step mode); runs its own exact-mode
 * structure pass, forward pass (which lays out the value store, finds the
 * underflowing individuals and, in extended range, gives the divisor) and
 * max-product sweep with traceback, over the individuals asked for only, and
 * changes no later result.  n = 0 is HMC_OK with no device work.  HMC_EARG and
 * HMC_EUNSUPPORTED as for hmc_posterior_draws.
 * Replaces no reference interface. */
int hmc_map_phase(hmc_ctx *ctx, int64_t n, const int32_t *indiv, int32_t *hap, double *prob, int32_t *status);
/* Last hmc_map_phase: device ms of its structure passes, of the forward
 * kernel and of the max-product sweep with its traceback and transposition;
 * groups the individuals ran in; individuals on pruned records.  Replaces no
 * reference interface. */
int hmc_last_map_stats(const hmc_ctx *ctx, double *structure_ms, double *fb_ms, double *sweep_ms, int *groups, int *n_pruned);
/* MAP phasing given phase sets: hmc_map_phase over the haplotype pairs that
 * are consistent with caller-given phase evidence (what a read pair, a trio or
 * an assembly fixes, as VCF's 0|1 with a PS tag writes it), and the
 * probability of that evidence.  A variable-order chain couples the switches,
 * so the answer is not hmc_map_phase's with a few loci flipped.
 * indiv[n], hap[n][2][L], prob[n], status[n] as for hmc_map_phase (indiv = NULL:
 * the whole shard); evidence[n]; any output may be NULL.
 *   Entries.  Entry e of n_ev says: for individual ev_indiv[e] (a panel
 *   index), in phase set ev_set[e] (any int32, a name only), the allele with
 *   symbol ev_first[e] at locus ev_locus[e] lies on that set's first haplotype;
 *   the individual's other input allele there lies on the set's second.
 *   Entries come in any order; entries of individuals not asked for in this
 *   call (or outside this rank's shard) are ignored, so one table serves many
 *   calls; a set of a single locus constrains nothing and is allowed.
 *   Meaning.  A pair {h0, h1} is consistent with a set when one of its two
 *   haplotypes carries the first-haplotype allele at every locus of the set —
 *   which of the two may differ from set to set — and with the evidence when it
 *   is consistent with every set of the individual.
 *   hap is the consistent pair of largest exact posterior P(pair | genotype),
 *   prob that posterior by hmc_map_phase's rule (same order, same mantissa and
 *   exponent bookkeeping: a pair keeps the one number it has in hmc_map_phase,
 *   hmc_ranked_phasings and the draws), evidence = P(evidence | genotype), the
 *   sum of the posteriors of all consistent pairs.  The posterior given the
 *   evidence is prob / evidence; the caller divides.
 *   Status 0 / 1 / 2 exactly where hmc_map_phase puts them; 3: the lattice has a
 *   path but none consistent with the evidence (the computed evidence is
 *   exactly 0; this includes an individual swept over pruned records).  Rows
 *   of status 1, 2 and 3 carry the input genotype, prob 0 and evidence 0.
 *   An individual with no entries, or with single-locus sets only, gets
 *   hmc_map_phase's bytes and evidence exactly 1.0.
 *
 * The sweep.  A set needs an orientation label c per state: its first
 * haplotype lies on the state's a side (c = 0) or b side (c = 1); a
 * predecessor's label c arrives as c ^ rev(r).  Every path through a set's
 * first locus is heterozygous from there on, so between a set's first and last
 * locus the two values of a state are (V[0], V[1]) by label (a span record),
 * and elsewhere hmc_map_phase's (Vh, Vd).  The record of locus k is k + 1 (the
 * head record for k < head_len).  State t with alleles (xa, xb):
 *   first locus of a set:  m = max_r max(Vd'[pred r], 2.0 * Vh'[pred r]), or
 *     max_r max(V'[0][pred r], V'[1][pred r]) when the record below ends the
 *     previous set; V[0][t] = tpv[t] * m if xa is the first-haplotype allele,
 *     V[1][t] = tpv[t] * m if xb is, the other label 0;
 *   further up to the set's last locus:  V[c][t] = tpv[t] * max_r V'[c ^ rev(r)][pred r];
 *     at a locus of the set the label whose side does not carry the
 *     first-haplotype allele is stored as 0, at other loci both labels pass;
 *   the record above a set's last:  hmc_map_phase's recurrence with
 *     Vd' = max(V'[0], V'[1]) and Vh' = 0.
 *   Loci below head_len are matched at the head record from the states' head
 *   patterns; for an individual with a missing allele at a head locus those
 *   loci come from the reference's head pairing, so for evidence that touches
 *   them only consistency holds.
 *   Tie rules.  Final record: candidates (t, label) in order of t, label 0
 *   (Vh or V[0]) before label 1; the largest value, among equals the first.
 *   Going down, the first contribution in record order that attains the
 *   maximum; where a contribution offers two values — Vd' then 2.0 * Vh', or
 *   V'[0] then V'[1] — the first of equals.  A label stored as 0 is never
 *   chosen.  Spelling and prob as hmc_map_phase.
 *   evidence is the same sweep with ordered sums in place of maxima
 *   (contributions in record order; the final record in state order), every
 *   record rescaled by a power of two in both ranges, divided by the range's
 *   P(genotype).  Mirror paths need no care: both pass or both fail every set.
 * The bits of a row depend on the model, the range, the individual and its own
 * set of entries: not on entry order, the integers used as set names, other
 * individuals or their evidence, batches, launch shapes, store budgets or
 * sharding; flipping a set wholesale (ev_first replaced by the other input
 * allele at every locus of the set) changes no byte.
 * HMC_EARG, with a message naming the first offending entry: ev_indiv outside
 * the panel; a locus out of range; a locus where the individual's input is not
 * heterozygous with both alleles present; ev_first neither of the two input
 * alleles; the same (individual, locus) in two entries.  HMC_EUNSUPPORTED,
 * naming the individual: two of its sets interleave ([first locus, last locus]
 * overlap).  Otherwise HMC_EARG and HMC_EUNSUPPORTED as for hmc_map_phase.
 * Needs a preceding hmc_resolve_all; runs its own exact-mode structure pass and
 * forward pass over the individuals asked for only and changes no later
 * result.  n = 0 is HMC_OK with no device work and zeroed stats.  Replaces no
 * reference interface. */
int hmc_map_phase_given(hmc_ctx *ctx, int64_t n, const int32_t *indiv, int64_t n_ev, const int32_t *ev_indiv,
                        const int32_t *ev_locus, const int32_t *ev_set, const int32_t *ev_first, int32_t *hap, double *prob,
                        double *evidence, int32_t *status);
/* Last hmc_map_phase_given: as hmc_last_map_stats, and the individuals that
 * ran the constrained sweep (the others took hmc_map_phase's).  Replaces no
 * reference interface. */
int hmc_last_given_stats(const hmc_ctx *ctx, double *structure_ms, double *fb_ms, double *sweep_ms, int *groups, int *n_pruned,
                         int *n_constrained);
/* Ranked phasings: the k haplotype pairs of largest exact posterior P(pair |
 * genotype) under the model of the last E-step, each once, with its posterior
 * — what "MAP pair, posterior 0.41" leaves open: the top diplotypes with their
 * probabilities, whether the second-best phasing flips a call, how many
 * phasings cover 95 %.  (The E-step's k-best list, hmc_get_estep /
 * hmc_get_samples, is a beam cut at every locus and no exact ranking; a
 * posterior draw finds the runners-up by luck and with repeats.)
 * indiv[n] are panel indices inside this rank's shard, in any order, repeats
 * allowed; indiv = NULL means the whole shard (n is ignored).  1 <= k <= 16.
 * Outputs, any of which may be NULL: hap[n][k][2][L] symbols, prob[n][k],
 * count[n], status[n].
 *   Rows.  Row r of individual i is the pair of (r + 1)-th largest exact
 *   posterior among *unordered* haplotype pairs; each pair is listed at most
 *   once.
 *   Count.  count[i] = min(k, the pairs whose computed value is positive);
 *   rows r >= count[i] carry the input genotype (as hmc_get_resolutions gives
 *   it for unresolved individuals) and prob 0.0.
 *   Status 0 / 1 / 2 exactly where hmc_map_phase puts them; for status 1 and
 *   2 count is 0 and every row is the input genotype at prob 0.
 *   prob by the rule of hmc_map_phase and hmc_posterior_draws: tpv of the
 *   final state times tpv of each chosen state down to the head record, one
 *   multiplication each in that order, kept as mantissa and exponent, doubled
 *   if the two haplotypes differ anywhere, divided by P(genotype) — a pair has
 *   one number in this call, in hmc_map_phase and wherever a draw hits it.
 *   Row 0 is hmc_map_phase's answer byte for byte (hap, prob, status), in both
 *   ranges.
 *   k does not enter: row r has the same bytes for every k > r.  Nor do the
 *   other individuals of the call, sharding, launch shapes, store budgets,
 *   groups, or the list width the kernel was built with.
 *
 * The sweep is hmc_map_phase's with lists in place of maxima.  Every state t
 * of a record keeps two descending lists of at most K values (K the list
 * width, at least k; empty slots are 0): Lh[t] over paths whose two haplotypes
 * are equal so far, Ld[t] over paths that differ already, the pair factor 2
 * inside.
 *   Head record: a homozygous head state has Lh = (tpv), Ld = (); a
 *   heterozygous one Lh = (), Ld = (tpv * 2.0).
 *   Record j above it, state t with alleles (xa, xb), contributions r in
 *   record order, p = pred(r), primes for record j - 1.  Candidates:
 *     xa == xb, for Lh[t]:  (Lh'[p][q], key (r, q));
 *     xa == xb, for Ld[t]:  (Ld'[p][q], key (r, q));
 *     xa != xb:  Lh[t] is empty; for Ld[t] every r gives (Ld'[p][q], key
 *       (r, 0, q)) and (2.0 * Lh'[p][q], key (r, 1, q)) — the latter unless an
 *       earlier contribution of t names the same predecessor p.
 *   The mirror.  A heterozygous pair behind a homozygous prefix is two mirror
 *   paths of half each: out of the state that both haplotypes share, rev or
 *   not.  For one value they tie and the first wins; in a list both would
 *   appear, the same pair twice.  Paths whose haplotypes are equal so far share
 *   their contexts, so the two mirrors are the two contributions of t that come
 *   from one predecessor, and the 2 h candidates are taken from the first of
 *   them only.  (Ld' is taken from both: once the haplotypes differ, the two
 *   orientations are two different pairs.)
 *   Order.  Candidates by value descending, then key ascending
 *   lexicographically; the first K with a value > 0 are kept and then
 *   multiplied by tpv[t], one multiplication per kept entry — after the
 *   selection, so a power of two on a whole record changes no choice.
 *   Final record: candidates (t, label, q) with key (2 t + label, q), h = 0
 *   and d = 1, in the same order; the first k are the rows.
 *   Traceback: every row goes down by the choice that produced its entry;
 *   spelling (side parity, the rev flip after writing, the head state's loci)
 *   and prob are hmc_map_phase's.
 *   Scaling: every record's 2 F K values are multiplied by the power of two
 *   that brings the record's largest into [0.5, 1), in both ranges.  That
 *   largest value is a rank-0 entry, hmc_map_phase's maximum, so row 0 makes
 *   hmc_map_phase's choices; an entry more than 2^1021 below its record's
 *   maximum loses bits.
 * At K = 1 these are hmc_map_phase's rules.  Two pairs whose computed values
 * differ by less than the rounding of at most 2L + 2 operations may be listed
 * in either order; no pair is listed twice and none of a larger computed
 * value is skipped.
 * Range (hmc_set_posterior_range) as for hmc_map_phase: regular divides by the
 * last E-step's P(genotype) and gives status 2 where that is below DBL_MIN;
 * extended divides by the scaled forward pass's own total and never gives
 * status 2; individuals whose forward likelihood underflows are swept over the
 * pruned records.
 * Needs a preceding hmc_resolve_all (any E-step mode); runs its own exact-mode
 * structure pass, forward pass and list sweep with the tracebacks, over the
 * individuals asked for only, and changes no later result.  The lists live in
 * a device store of this call's own, 24 K bytes per state and record, and the
 * individuals go through in batches that fit the value store's budget
 * (hmc_set_store_budgets); an individual alone may take 1.5 K times that
 * budget (its lists against its values, which fit the value store), and
 * HMC_ENOMEM names one whose lists exceed even that.  n = 0 is HMC_OK with no device work and zeroed stats.  HMC_EARG
 * and HMC_EUNSUPPORTED as for hmc_map_phase; HMC_EARG also for k < 1 or
 * k > 16.  Replaces no reference interface. */
int hmc_ranked_phasings(hmc_ctx *ctx, int64_t n, const int32_t *indiv, int k, int32_t *hap, double *prob, int32_t *count,
                        int32_t *status);
/* Last hmc_ranked_phasings: device ms of its structure passes, of the forward
 * kernel and of the list sweep with its tracebacks and transposition; groups
 * the individuals ran in; individuals on pruned records; the list width of
 * the kernel that ran (the smallest of 2, 4, 8, 16 that holds k).  Replaces no
 * reference interface. */
int hmc_last_ranked_stats(const hmc_ctx *ctx, double *structure_ms, double *fb_ms, double *sweep_ms, int *groups,
                          int *n_pruned, int *k_built);
/* Window phasings: for every individual asked for and every window of loci,
 * the distinct haplotype pairs the individual can carry over the window, each
 * with its exact posterior summed over everything outside the window, the k
 * most probable in order — the diplotype call of a gene-sized window.  The
 * sum-product sibling of hmc_ranked_phasings (whose whole-panel pairs all have
 * vanishing posteriors on long panels) and the discovering sibling of
 * hmc_haplotype_dosages (which prices patterns the caller already knows).
 * indiv[n] as for hmc_map_phase: panel indices inside this rank's shard, any
 * order, repeats allowed, NULL = the whole shard.  Windows start[w], len[w]
 * (1 <= len[w] <= maxlen, inside [0, L)) may overlap, repeat and come in any
 * order; one call runs one structure pass and one forward-backward pass over
 * the individuals asked for and serves every window from them.  1 <= k <= 1024.
 * Outputs, any of which may be NULL: hap[n][n_windows][k][2][maxlen] allele
 * symbols (-1 past len[w]), prob[n][n_windows][k], count[n][n_windows] rows
 * that are real, n_config[n][n_windows] pairs of positive computed posterior,
 * status[n][n_windows].
 * Configurations.  A locus of the window is fixed for an individual when both
 * input alleles are present and equal, else branching.  An ordered
 * configuration is the pair of allele strings (a side, b side) over the
 * branching loci; there are C = the product over them of 2 (heterozygous),
 * 2 A - 1 (one allele missing) or A^2 (both missing), A the locus's alleles
 * (hmc_allele_table).  C above the cap (1 024; hmc_set_window_tuning lowers
 * it) is status 4 — whatever the individual's own status — with the input
 * genotype over the window at prob 0, count 0 and n_config 0.  Status 0, 1, 2
 * as for hmc_map_phase; rows of status 1 and 2 likewise.
 * Rows.  A row spells an unordered window pair {x, y} once, hap[..][0] the
 * lexicographically smaller string by allele-table index; prob = the sum of
 * post({h0, h1}) over the whole-panel unordered pairs whose restriction to
 * the window is {x, y}, post the posterior hmc_posterior_draws samples.  Rows
 * by prob descending, then by (hap[0] indices, hap[1] indices) ascending; the
 * first k of prob > 0 are the rows, count = min(k, n_config); rows past count
 * carry the input genotype over the window at prob 0.  Row r has the same
 * bytes for every k > r.
 * Arithmetic.  prob is the very double hmc_haplotype_dosages returns for that
 * individual and the two-sided pattern (start[w], len[w], A = hap[0], B =
 * hap[1]), in both ranges — exactly half of it when hap[0] = hap[1], where
 * the dosage counts both orientations.  In full: at the window's first record
 * every state's forward value goes to the one ordered configuration the state
 * spells there (a head record of head_len > 1 spells all of the window's head
 * loci at once) and every other configuration gets 0; per record above it each
 * (state t, configuration) takes the running sum over t's contributions in
 * stored order of (previous value x tpv[t]), a reversed link taking the
 * side-swapped configuration, the first term assigning and later ones adding,
 * extended range multiplying by the record's exponent step; at the window's
 * last record S_c is the ordered sum against the backward values (lane l adds
 * states l, l + 64, ..., then the fixed butterfly) and prob = (S_c +
 * S_swap(c)) / P(genotype) with one addition and one division, S_c /
 * P(genotype) when c = swap(c).  A row's bits depend on the model, the range,
 * the individual and its own (start, len): not on the other windows or
 * individuals, k, the cap, the configuration width the kernel was built with,
 * the tier, launch shapes, batches, groups or sharding.
 * For an individual with a missing allele at a head locus, window loci below
 * head_len come from the reference's head pairing, which is not a phasing
 * model: for a window that touches them only the normalisation holds.
 * Needs a preceding hmc_resolve_all (any E-step mode) and changes no later
 * result.  n = 0 or n_windows = 0 is HMC_OK with no device work and zeroed
 * stats.  HMC_EARG, with a message naming the first offender, for a window
 * with start < 0, len < 1, len > maxlen or start + len > L, k outside
 * [1, 1024], an individual outside this rank's shard, no E-step or a model
 * changed since the last one; HMC_EUNSUPPORTED as for
 * hmc_genotype_posteriors; HMC_ENOMEM, naming the individual, when one
 * individual's two frontiers at the configuration width it needs exceed the
 * 4 GiB scratch budget.  Replaces no reference interface. */
int hmc_window_phasings(hmc_ctx *ctx, int64_t n, const int32_t *indiv, int n_windows, const int32_t *start,
                        const int32_t *len, int maxlen, int k, int32_t *hap, double *prob, int32_t *count,
                        int32_t *n_config, int32_t *status);
/* Last hmc_window_phasings: device ms of its structure passes, of the
 * forward-backward kernel and of the window sweeps; groups; individuals on
 * pruned records; individuals whose frontiers went through the device-memory
 * scratch; the widest configuration width NC that ran (4, 16, 64, 256 or
 * 1 024: a group's individuals run sorted by the width their largest C needs,
 * one width per launch); (individual, window) pairs over the cap.  Replaces no
 * reference interface. */
int hmc_last_window_stats(const hmc_ctx *ctx, double *structure_ms, double *fb_ms, double *sweep_ms, int *groups,
                          int *n_pruned, int *n_spilled, int *configs_built, int *n_over_cap);
/* Range of the posterior family (hmc_genotype_posteriors, hmc_switch_posteriors,
 * hmc_pair_posteriors, hmc_posterior_draws, hmc_map_phase,
 * hmc_ranked_phasings and their hmc_write_* forms).
 * extended = 0 (default): the forward-backward pass keeps raw doubles and
 * divides by the last E-step's P(genotype); an individual whose P(genotype) is
 * below DBL_MIN gets status 2, one whose forward likelihood underflowed to 0
 * in the E-step status 1 — from about 1 200 loci on.
 * extended = 1: the pass multiplies every record (the states after one locus)
 * by the power of two that brings the record's largest value into [0.5, 1),
 * forward and backward, and keeps the cumulative exponents; the divisor is
 * the pass's own total, the final record's scaled forward values summed in
 * state order, with its exponent, and the consumers cancel the exponents with
 * ldexp.  Status 2 never occurs; status 1 only for a lattice with no path (the
 * structure pass finds the individual unresolved, or the total is exactly 0);
 * an individual the E-step gave up on for underflow gets status 0 and real
 * rows, draws and prob (prob may be subnormal or 0 when the pair's posterior is
 * that small); hmc_last_*_stats report n_pruned = 0.  The same HMC_EARG and
 * HMC_EUNSUPPORTED conditions apply.
 * Between the modes: scaling by powers of two is exact, so an extended result
 * depends on the real-valued posterior and the summation order alone, not on
 * where the rescalings fall; multiplying every freq and tp of the table by one
 * power of two changes no bit of any extended result.  Where the regular mode
 * gives status 0 and none of its intermediates is subnormal, the two modes
 * differ only through the divisor — the E-step's P(genotype) against the sum
 * of this pass's own final forward values — and agree within the sum of their
 * rounding bounds; they are byte-identical exactly where those two totals are.
 * The setting changes no E-step, M-step or later result.  HMC_EARG for any
 * other value.  Replaces no reference interface. */
int hmc_set_posterior_range(hmc_ctx *ctx, int extended);
/* P(genotype) of individuals under the model of the last E-step in extended
 * range: mantissa[q] x 2^exponent[q] with mantissa in [0.5, 1) — the
 * likelihood the E-step reports as 0 or subnormal on long panels.  Always the
 * scaled forward pass, whatever hmc_set_posterior_range says; forward only, as
 * the draws.  indiv[n] are panel indices inside this rank's shard, any order,
 * repeats allowed; indiv = NULL means the whole shard (n is ignored).  Any
 * output may be NULL.  status 0 ok; 1 the lattice has no path: (0.0, 0).  The
 * value is the sum of the final record's forward values in state order (each
 * the ordered sum exact_fb computes), which need not be the E-step's total to
 * the last bit.  n = 0 is HMC_OK with no device work.  HMC_EARG and
 * HMC_EUNSUPPORTED as for hmc_posterior_draws.  Replaces no reference interface. */
int hmc_genotype_likelihoods(hmc_ctx *ctx, int64_t n, const int32_t *indiv, double *mantissa, int32_t *exponent,
                             int32_t *status);
/* Last hmc_genotype_likelihoods: device ms of its structure passes and of the
 * forward kernel; groups.  Replaces no reference interface. */
int hmc_last_likelihood_stats(const hmc_ctx *ctx, double *structure_ms, double *fb_ms, int *groups);
/* ---- whole EM: HaploModel::run (HaploModel.cpp:117-155) ------------------ */
typedef struct hmc_iter_log {
  double log_likelihood;
  double t_estep_s, t_mstep_s; /* wall time of E_k and of M_k (0 if no M-step) */
  uint64_t r_e, r_m;
  int n_patterns;              /* patterns after M_k */
  int n_samples;
  /* HaploComp of the input panel (phase as given) against the accepted
   * resolutions after E_k (HaploModel.cpp:134-136) */
  double switch_error, ihp, igp;
} hmc_iter_log;
/* Runs M0 + up to max_iteration EM iterations with the reference's
 * convergence rule.  log[] receives up to log_cap iterations; *iterations the
 * number run; *t_m0_s, *r_m0, *n_patterns0 describe M0. */
int hmc_run(hmc_ctx *ctx, int max_iteration, hmc_iter_log *log, int log_cap, int *iterations, double *t_m0_s,
            uint64_t *r_m0, int *n_patterns0);
/* One iteration of that loop (HaploModel.cpp:130-144) for a host that drives
 * the EM itself, after a first hmc_find_patterns: E-step, accept the
 * resolutions if the LL did not drop below *old_ll, HaploComp, the continue
 * rule (*go), and the M-step when continuing — or always, with always_mstep
 * (a fixed number of steps, as bench.py times).  *old_ll (start: -DBL_MAX)
 * becomes the LL when the M-step ran. */
int hmc_em_iteration(hmc_ctx *ctx, int iteration, int max_iteration, int always_mstep, double *old_ll,
                     hmc_iter_log *log, int *go);
/* Model snapshot for hosts that repeat the EM from one M-step (bench.py runs
 * the reference's converged chain from M0 again and again).  hmc_model_save
 * keeps a device copy of the current pattern table; hmc_em_rewind restores it
 * and returns the EM to the state HaploModel::run has right after build()
 * (HaploModel.cpp:121-129): no samples, resolutions = the input genotypes,
 * nothing carried over from earlier E-steps (their scheduling costs and store
 * sizes); the next hmc_em_iteration(1, ..., *old_ll = -DBL_MAX) starts a fresh
 * chain.  Results equal a fresh context's.  After a rewind, hmc_get_patterns
 * spells whole allele strings only if no table was mined since the save (the
 * candidate tree that spells them is not kept); otherwise the last allele. */
int hmc_model_save(hmc_ctx *ctx);
int hmc_em_rewind(hmc_ctx *ctx);
/* HaploComp (HaploComp.cpp:29-155) of the input panel, phase as given,
 * against the accepted resolutions: switch error, incorrect-haplotype and
 * incorrect-genotype percentages over all ranks' individuals.  Replaces the
 * HaploComp compare(&genos, &resolutions) of HaploModel.cpp:134. */
int hmc_haplocomp(hmc_ctx *ctx, double *switch_error, double *ihp, double *igp);
/* Accepted resolutions of the last hmc_run ([n][2][L] symbols). */
int hmc_get_best_resolutions(hmc_ctx *ctx, int32_t *out);
/* HaploFile::writeGenoData (HaploFile.cpp:120-153) of the accepted
 * resolutions (single-rank contexts): the loaded file's positions ("P" line)
 * and ids ('#' prepended only to an id starting with a digit), or the
 * defaults k*1000 and 1..N for a panel loaded from memory. */
int hmc_write_phase(hmc_ctx *ctx, const char *path);
/* HaploFile::getHaploFile(format, file names) + readGenoData / writeGenoData
 * (HaploFile.cpp:13-52, 54-153, 205-640).  format / file names:
 *   "PHASE", "HPM", "HPM2"  one file;
 *   "BENCH2"                genotype file, position file;
 *   "BENCH3"                genotype file, position file, children file — the
 *                           children are appended as ordinary unphased
 *                           genotypes, unphased_num = the parents, and HaploComp
 *                           covers the parents only (HaploFile.cpp:446-484,
 *                           HaploComp.cpp:40).
 * hmc_parse_files needs no context or device: it returns the panel (alleles
 * [N][2][L] symbols, -1 missing; types [L+1] 'S'/'M'; unphased_num); pass NULL
 * buffers first to learn N and L.  hmc_load_files = parse + hmc_load_genotypes
 * (keeps ids, marker names, positions for the writers).  hmc_write_files
 * writes the accepted resolutions in that format (BENCH2/3: genotype file +
 * position file). */
int hmc_parse_files(const char *format, const char *const *paths, int n_paths, int *N, int *L, int32_t *alleles,
                    char *types, int *unphased_num);
int hmc_load_files(hmc_ctx *ctx, const char *format, const char *const *paths, int n_paths);
int hmc_write_files(hmc_ctx *ctx, const char *format, const char *const *paths, int n_paths);
/* GenoData::unphased_num (GenoData.h:37) of the loaded panel. */
int hmc_unphased_num(const hmc_ctx *ctx, int *unphased_num);
/* One- and two-file shorthands of the three calls above (path2 may be NULL). */
int hmc_parse_file(const char *format, const char *path, const char *path2, int *N, int *L, int32_t *alleles,
                   char *types);
int hmc_load_file(hmc_ctx *ctx, const char *format, const char *path, const char *path2);
int hmc_write_file(hmc_ctx *ctx, const char *format, const char *path, const char *path2);
/* HaploFile::writePattern (HaploFile.cpp:155-171; HMC.cpp:229-232, the
 * --output-patterns ".patterns" file) of the current pattern table: header
 * "Frequency\tLength\t<marker names>", one line per pattern in id order with
 * frequency / N, length and the long-format alleles (-1 outside the pattern).
 * The reference divides by genotype_num() of a GenoData that no longer exists
 * when it writes, so the N used here is the panel's: unpinned. */
int hmc_write_patterns(hmc_ctx *ctx, const char *path);
/* hmc_genotype_posteriors as text (hmc_resolve --output-posteriors): the
 * header "Id\tMarker\tAlleleLo\tAlleleHi\tPosterior", then one line per site
 * and pair of non-zero probability, in the call's site order and then bin
 * order: individual id, marker name, the two allele symbols as the genotype
 * files spell them, the posterior as %.17g (reads back to the same double).
 * Needs a preceding hmc_resolve_all or hmc_run; the numbers belong to the
 * model of that last E-step.  Replaces no reference interface. */
int hmc_write_posteriors(hmc_ctx *ctx, const char *path);

/* hmc_switch_posteriors as text (hmc_resolve --output-switch-posteriors): the
 * header "Id\tMarkerA\tMarkerB\tAlleleA\tAlleleB\tCis\tTrans", then one line
 * per site of status 0 in the call's site order: individual id, the two marker
 * names, the lower-index allele's symbol at each of the two loci as the
 * genotype files spell them, cis and trans as %.17g (they read back to the
 * same doubles).  Needs a preceding hmc_resolve_all or hmc_run.
 * Replaces no reference interface. */
int hmc_write_switch_posteriors(hmc_ctx *ctx, const char *path);
/* hmc_pair_posteriors of hmc_pair_span_list(span) as text (hmc_resolve
 * --output-pair-posteriors FILE --pair-span K): the header
 * "Id\tMarkerA\tMarkerB\tAlleleA\tAlleleB\tCis\tTrans", then one line per query
 * of status 0 in the list's order, spelled as hmc_write_switch_posteriors
 * spells a site (%.17g: the numbers read back to the same doubles).  Needs a
 * preceding hmc_resolve_all or hmc_run; HMC_EARG for span < 1.
 * Replaces no reference interface. */
int hmc_write_pair_posteriors(hmc_ctx *ctx, const char *path, int span);
/* hmc_posterior_draws of the whole shard as text (hmc_resolve --output-draws
 * FILE --draws D --seed S): the header
 * "Id\tDraw\tPosterior\tHaplotype0\tHaplotype1", then one line per individual
 * of status 0 and per draw, individual-major: the individual's id, the draw
 * index, the pair's posterior as %.17g (reads back to the same double), and
 * each haplotype as its alleles, spelled as the genotype files spell them and
 * separated by single spaces.  Needs a preceding hmc_resolve_all or hmc_run;
 * HMC_EARG for draws < 1.  Replaces no reference interface. */
int hmc_write_posterior_draws(hmc_ctx *ctx, const char *path, int draws, uint64_t seed);
/* hmc_map_phase of the whole shard as text (hmc_resolve --output-map FILE):
 * the header "Id\tStatus\tPosterior", then per individual of the shard, in
 * order, three lines: the individual's id, its status and the pair's posterior
 * as %.17g (reads back to the same double), tab-separated; then each of the
 * two haplotypes on a line of its own, its alleles spelled as
 * hmc_write_posterior_draws spells them and separated by single spaces ('?'
 * for a missing input allele in a row of status 1 or 2).  Needs a preceding
 * hmc_resolve_all or hmc_run.  Replaces no reference interface. */
int hmc_write_map_phase(hmc_ctx *ctx, const char *path);
/* hmc_map_phase_given of the whole shard as text (hmc_resolve
 * --output-map-given FILE --evidence EVFILE): hmc_write_map_phase's three-line
 * form with the header "Id\tStatus\tPosterior\tEvidence", both numbers as
 * %.17g.  Replaces no reference interface. */
int hmc_write_map_phase_given(hmc_ctx *ctx, const char *path, int64_t n_ev, const int32_t *ev_indiv, const int32_t *ev_locus,
                              const int32_t *ev_set, const int32_t *ev_first);
/* The evidence file of hmc_resolve --evidence into the four entry arrays:
 * tab-separated lines "Id  Marker  Set  Allele" with ids and marker names as
 * the loaded genotype files give them, Set an integer, the allele spelled as
 * the genotype files spell alleles; empty lines are skipped, and so are lines
 * starting with '#' unless they have four fields of which the first is an
 * individual's id (PHASE files give ids that start with '#').  *n_ev gets the number of entries; at most cap are written (call
 * with cap = 0 first).  HMC_EARG with a message naming the line.  Replaces no
 * reference interface. */
int hmc_read_evidence(hmc_ctx *ctx, const char *path, int64_t *n_ev, int32_t *ev_indiv, int32_t *ev_locus, int32_t *ev_set,
                      int32_t *ev_first, int64_t cap);
/* hmc_ranked_phasings of the whole shard as text (hmc_resolve --output-ranked
 * FILE --ranked K): the header "Id\tRank\tPosterior\tHaplotype0\tHaplotype1",
 * then one line per individual of status 0 and per rank < count,
 * individual-major: the id, the rank (from 0), the pair's posterior as %.17g
 * (reads back to the same double) and the two haplotypes, tab-separated, each
 * haplotype spelled as hmc_write_posterior_draws spells it.  Needs a preceding
 * hmc_resolve_all or hmc_run; HMC_EARG for k < 1 or k > 16.  Replaces no
 * reference interface. */
int hmc_write_ranked_phasings(hmc_ctx *ctx, const char *path, int k);
/* hmc_haplotype_dosages of the whole shard as text (hmc_resolve
 * --output-dosages FILE --haplotypes HAPFILE): the header
 * "Id\tHaplotype\tDosage", then one line per individual of status 0 and per
 * pattern, individual-major: the individual's id, names[p], the dosage as
 * %.17g (reads back to the same double).  Patterns as for
 * hmc_haplotype_dosages, with the same errors.  Needs a preceding
 * hmc_resolve_all or hmc_run.  Replaces no reference interface. */
int hmc_write_haplotype_dosages(hmc_ctx *ctx, const char *path, int n_patterns, const char *const *names,
                                const int32_t *start, const int32_t *len, int maxlen, const int32_t *alleles_a,
                                const int32_t *alleles_b);
/* hmc_window_phasings of the whole shard as text (hmc_resolve --output-windows
 * FILE --windows WINFILE --window-k K): the header
 * "Id\tWindow\tStart\tLength\tRank\tPosterior\tHaplotype0\tHaplotype1", then one
 * line per individual, window (its index in the call) and rank < count of
 * status 0, individual-major: the posterior as %.17g (reads back to the same
 * double) and the two haplotypes over the window's loci, spelled as
 * hmc_write_posterior_draws spells them.  Windows and errors as for
 * hmc_window_phasings.  Needs a preceding hmc_resolve_all or hmc_run.
 * Replaces no reference interface. */
int hmc_write_window_phasings(hmc_ctx *ctx, const char *path, int n_windows, const int32_t *start, const int32_t *len,
                              int k);
/* ---- tuning -------------------------------------------------------------- */
/* hmc_window_phasings, 0 = default for each.  max_configs: the cap on a
 * window's ordered configurations C (at most 1 024), above which an
 * (individual, window) pair is status 4.  tier_states: states per locus whose
 * frontiers the sweep keeps in LDS (16 (NC + 1) bytes per state; default and
 * most: 512, 150, 39, 9, 2 at NC = 4 .. 1 024); an individual with a larger
 * frontier keeps the windows that do not fit the LDS in a device-memory scratch.  HMC_EARG outside [0, 1024]
 * and [0, 512].  Results do not depend on it, status 4 aside.  Replaces no
 * reference interface. */
int hmc_set_window_tuning(hmc_ctx *ctx, int max_configs, int tier_states);
/* frontier_cap: initial states per locus and individual (doubles on
 * overflow, at most 2 097 151); trace_bytes: trace-store budget (0 =
 * automatic); waves: resident E-step waves (0 = automatic). */
int hmc_set_tuning(hmc_ctx *ctx, int frontier_cap, uint64_t trace_bytes, int waves);
/* E-step launch shape: wavefronts cooperating on one individual (1..4,
 * default 2) and individuals sharing one CU's LDS (default 8); 0 keeps the
 * current value.  A shape set here applies to every kernel; (0, 0) returns the
 * split E-step's value pass to its automatic shape: 1 wave x 20 individuals per
 * CU for groups of at least 32 individuals per CU, 2 x 8 from 8 per CU, else
 * 3 x 8; a value-pass shape given by one number only takes the other from the
 * same rule.  Results do not depend on the shape. */
int hmc_set_estep_shape(hmc_ctx *ctx, int waves_per_individual, int individuals_per_cu);
/* Launch shapes of the split E-step's two passes, 0 = automatic for each:
 * structure pass waves per individual (1, 4, 8 or 16; automatic: 4 on a model
 * with more patterns than the panel has individual-loci, the genotype-mined
 * M0, 16 when such a group has at most one individual per CU)
 * and individuals per CU (automatic: 1 at 16 waves, 2 at 4; else 12 above 8 per CU in
 * the group, 8 above 4, else 4), value pass waves per individual (1..4) and
 * individuals per CU (rule of hmc_set_estep_shape; groups averaging more than
 * 1 500 record words per locus take 8 x 2, or 16 / c waves x c per CU when
 * they have c < 4 individuals per CU).  Value-pass waves per individual 1..16.
 * Results do not depend on them. */
int hmc_set_pass_shapes(hmc_ctx *ctx, int structure_waves, int structure_ipc, int value_waves, int value_ipc);
/* Budgets of the split E-step's two stores in bytes, 0 = automatic: the
 * k-best trace store (min(42 % of free HBM, 120 GiB)) and the structure-record
 * store (min(28 %, 80 GiB); 0 with a trace budget given = the same number).
 * Individuals pass in groups whose records and traces fit them. */
int hmc_set_store_budgets(hmc_ctx *ctx, uint64_t trace_bytes, uint64_t record_bytes);
/* States per locus whose two label frontiers hmc_switch_posteriors keeps in
 * LDS (32 bytes per state); an individual with a larger frontier at any locus
 * goes through a device-memory scratch instead.  0 = the default (1 024);
 * HMC_EARG above 2 032, the most a workgroup's 64 KiB holds.  Results do not
 * depend on it (it lets small panels take the device-memory path).
 * Replaces no reference interface. */
int hmc_set_switch_tier(hmc_ctx *ctx, int states);
/* Schedule of hmc_pair_posteriors, 0 = automatic for each.  slots: anchors a
 * state carries at once (NS: 1, 2, 4 or 8; automatic: the smallest that holds
 * every individual's overlapping anchors in one round, 8 at most).  tier_states:
 * states per locus whose frontiers the sweep keeps in LDS (32 NS bytes per
 * state; automatic: 254 at every NS, measured faster than the whole 64 KiB at
 * the smaller NS); an individual with a larger frontier goes through a
 * device-memory scratch.  HMC_EARG for a slot count that is not instantiated
 * or a tier above 254, what the LDS holds at the largest NS.  Results do not
 * depend on it.
 * Replaces no reference interface. */
int hmc_set_pair_tuning(hmc_ctx *ctx, int slots, int tier_states);
/* Schedule of hmc_haplotype_dosages, 0 = automatic for each, as
 * hmc_set_pair_tuning.  slots: patterns a state carries at once (NS: 1, 2, 4 or
 * 8; automatic: the smallest of 1, 2, 4 that runs the call in one round, else
 * 4, which measured faster in twice the rounds than 8 does in half of them).
 * tier_states: states per locus whose frontiers the sweep keeps in LDS (32 NS
 * bytes per state; automatic: 254).  HMC_EARG for a slot count that is not
 * instantiated or a tier above 254.  Results do not depend on it.
 * Replaces no reference interface. */
int hmc_set_dosage_tuning(hmc_ctx *ctx, int slots, int tier_states);
/* E-step implementation: 0 (default) = two passes, a structure pass that
 * replays extendAll/addHaploPair (HaploBuilder.cpp:226-261) on pattern ids
 * and a value pass with the k-best lists; individuals whose forward
 * likelihood underflows are re-run through a structure pass that applies
 * extend()'s forward test (HaploBuilder.cpp:237); 1 = the fused single-pass
 * kernel (sample_size <= 32).  Both produce identical results. */
int hmc_set_estep_mode(hmc_ctx *ctx, int mode);
/* Split E-step of the last hmc_resolve_all: device ms of the structure pass,
 * the value pass and the underflow re-runs, and the number of individuals
 * re-run. */
int hmc_last_estep_split(const hmc_ctx *ctx, double *structure_ms, double *values_ms, double *fallback_ms,
                         int *n_fallback);
/* Launches of the last hmc_resolve_all: structure passes and value passes
 * (individuals pass in groups when their records / traces exceed the stores). */
int hmc_last_estep_passes(const hmc_ctx *ctx, int *structure_passes, int *value_passes);
/* Value pass of the split E-step.  Mode 0: k-best lists are kept by
 * likelihood value only; an individual for which that could change a result
 * (a non-zero likelihood tied across some list's S-cut — the set
 * std::nth_element keeps then depends on the list order, HaploPair.cpp:85-88 —
 * or final candidates with equal or zero priors, HaploBuilder.cpp:101-105) is
 * re-run with the libstdc++ permutations.  Mode 1: every individual with the
 * libstdc++ permutations.  Mode 2 (default): automatic — mode 0 on panels with
 * more than two alleles per locus once the model is smaller than the panel,
 * mode 1 otherwise and for the rest of the context once a mode-0 E-step
 * re-ran more than 35 % of its individuals.  Results are identical in every
 * mode; mode 0 pays off only where few individuals have such ties (at
 * BASELINE config 3 about half of them have final candidates with equal
 * priors, and mode 1 is faster; at config 5's later E-steps a quarter). */
int hmc_set_value_mode(hmc_ctx *ctx, int mode);
/* Phase-B layout of the value pass (results identical): the overflowing adds'
 * selections with two links per lane (S lanes and 64 / S lists per
 * wavefront, sample_size <= 16) instead of one (2S lanes, 64 / 2S lists).
 * Mode 0: never; 1: groups of heavy individuals (the first E-step on a
 * genotype-mined model: many chains of adds per locus); 2 (default): every
 * group. */
int hmc_set_value_layout(hmc_ctx *ctx, int mode);
/* Schedule of the value pass (results identical): 1 = locus by locus (every
 * state's constructor and appends, a block barrier, the chains of adds, a
 * barrier); 2 = dataflow (one wavefront builds the lists in locus order as
 * soon as a state's predecessors are final, the others run the chains of
 * adds of any open locus; `ring` = frontiers kept, 3 or 4, 0 = 3); 0
 * (default) = automatic.  The same HaploPair::add sequence per state
 * (HaploPair.cpp:35-89) either way. */
int hmc_set_value_pass(hmc_ctx *ctx, int mode, int ring);
/* Structure pass of the split E-step (results identical): 1 = per chunk of
 * contributions a ranking hand-off (lane masks, four block barriers per
 * chunk); 2 = three block scans per locus (creation order from each key's
 * first contribution, add order from each state's member segment); 0 =
 * automatic. */
int hmc_set_structure_pass(hmc_ctx *ctx, int version);
/* Dataflow value pass: wavefronts per individual that build the lists which
 * need no selection (the "A" waves, each a fixed share of every locus's
 * states), 1..8 and fewer than the waves per individual; 0 = by the launch
 * shape.  Results are identical. */
int hmc_set_dataflow_waves(hmc_ctx *ctx, int a_waves);
/* Structure pass over the pattern table in end-locus order (1, default) or
 * in the table's id order (0): the successor lookups of one locus fall in one
 * block of the table instead of lines spread over all of it.  Results are
 * identical. */
int hmc_set_end_order(hmc_ctx *ctx, int on);
/* Exact M-step trie walk (HaploBuilder.cpp:334-449 estimateFrequency): 0 or
 * 1 = the depth-first walk, one (individual, start locus) item per wavefront
 * (default); 4 = four items per wavefront (16 lanes each) and 2 = the
 * breadth-first walk, one trie node per lane (both measured slower: the
 * variants library only, HMC_EUNSUPPORTED in the product).  The frequency
 * sums are fixed-point integer adds, identical for any order. */
int hmc_set_exact_walk(hmc_ctx *ctx, int items_per_wave);
/* 1 when the last value-pass launch ran the dataflow schedule. */
int hmc_last_value_pass(const hmc_ctx *ctx, int *dataflow);
/* Windowed E-step (SURVEY §7 hard part 4): the loci in windows, each
 * window's last frontier saved as the next one's checkpoint; records are kept
 * for one window and full traces for two, the older one collected into
 * survivor nodes (the entries the traceback can still reach).  Results are
 * identical to the classic passes.  mode 0 (default): automatic — when the
 * first loci of a sample show that the classic passes could hold fewer than
 * two individuals per CU in a group (cfg 4's per-rank E1) or would need three
 * or more groups (cfg 3's E1); 1 never; 2 always (tests).  window_loci: loci
 * per window (0: from the store budgets).
 * Replaces no reference interface (HaploBuilder::resolve keeps every locus's
 * pairs alive, HaploBuilder.cpp:35-126). */
int hmc_set_estep_windows(hmc_ctx *ctx, int mode, int window_loci);
/* The last E-step's windows (0 = classic passes), loci per window, groups of
 * individuals, and device ms of the trace collections (part of the value
 * passes' time). */
int hmc_last_estep_windows(const hmc_ctx *ctx, int *windows, int *window_loci, int *groups, double *recompute_ms);
/* The last E-step's trace collections, summed over individuals and windows:
 * out[0] loci stepped over with the reached entries as a bitmap, out[1] as a
 * list of at most 64 entries, out[2] loci of the collected windows written
 * from bitmaps, out[3] individuals-and-windows that went from bitmap to list
 * inside the collected window.  All 0 for the classic passes. */
int hmc_last_collection_stats(const hmc_ctx *ctx, unsigned long long out[4]);
/* Restarts of the last E-step (a frontier or contribution capacity grown, or
 * a window's traces past the store: windows 0.6x as long, or for a fixed
 * window length smaller groups) and the window scale now in force (1.0 until
 * a trace-store overflow; reset by a panel load or hmc_set_shard). */
int hmc_last_estep_restarts(const hmc_ctx *ctx, int *restarts, double *window_scale);
/* Host wall time (ms) of the last hmc_em_iteration's phases, in this order:
 * [0] the E-step call, [1] its store (re)allocations and releases, [2] the
 * end-order table build, [3] the sample gather after the passes, [4] accepting
 * the resolutions, [5] HaploComp, [6] the M-step call, [7] the E-step's setup
 * before the passes (buffers, budgets, cost order).  [1]-[3] and [7] are parts
 * of [0].  Writes min(n, 8) values and returns 8.  Replaces no reference
 * interface (measurement of the per-rank host gap). */
int hmc_last_host_phases(const hmc_ctx *ctx, double *ms, int n);
/* Individuals the last E-step re-ran with the libstdc++ permutations (mode 0)
 * and the device time of those re-runs (ms, part of values_ms). */
int hmc_last_estep_order(const hmc_ctx *ctx, int *n_rerun, double *rerun_ms);
/* Device time (ms, HIP events on the context stream) of the last E-step
 * forward kernel, traceback and whole M-step. */
int hmc_last_timings(const hmc_ctx *ctx, double *estep_forward_ms, double *estep_traceback_ms, double *mstep_ms);

/* ---- CPU-side test hooks (no GPU needed) --------------------------------- */
/* The libstdc++-exact selection used by the E-step kernel (select.hpp), run on
 * host arrays: nth_element(v, v+nth, v+n, greater) and sort(v, v+n, greater)
 * of (lik, tag) records ordered by lik. */
void hmc_test_nth_element(double *lik, uint32_t *tag, int n, int nth);
void hmc_test_sort_small(double *lik, uint32_t *tag, int n);
/* std::sort(v, v+n, greater) for any n (introsort, heap sort at depth 0,
 * final insertion sort): the final candidate order for sample_size > 16. */
void hmc_test_sort(double *lik, uint32_t *tag, int n);
/* The E-step's mask-partition formulation of the same nth_element (n <= 32). */
void hmc_test_nth_element_masks(double *lik, uint32_t *tag, int n, int nth);
/* GPU check of the segmented wave selection the E-step kernel uses
 * (coop_select.hpp), 64/seg_width lists per wavefront: list b =
 * lik/tag[off[b] .. off[b]+n[b]) (n[b] <= seg_width <= 32) gets
 * nth_element(.., nth[b], greater) in place on `device`. */
int hmc_test_coop_nth_element(int device, double *lik, uint32_t *tag, const int32_t *off, const int32_t *n,
                              const int32_t *nth, int count, int total, int seg_width);
/* GPU check of the other selection layouts of the E-step's value pass, each
 * with the scratch and segmentation the pass gives it.  List b occupies
 * lik/tag[b*stride .. (b+1)*stride), its first n[b] entries the list; the rest
 * must come back unchanged.
 *   HMC_SELECT_PAIR    two links per lane, `width` = W lanes per list (1..16),
 *                      stride 2W, n[b] <= 2W: nth_element(.., nth[b], greater)
 *   HMC_SELECT_PAIR10  the same with W = 10 fixed at compile time (width 10)
 *   HMC_SELECT_WIDE    one list of n[b] <= 128 per wavefront (width 64),
 *                      stride 128: nth_element(.., nth[b], greater)
 *   HMC_SELECT_RANK    value-only lists, `width` = S (1..16), stride 2S,
 *                      n[b] <= 2S: the S largest to [0, S) in rank order when
 *                      n[b] > S; tie[b] = the non-zero value tied across the
 *                      S-cut, else 0 (values >= 0, no NaN; nth is not read)
 * Shapes the value pass does not instantiate are refused (HMC_EARG). */
enum { HMC_SELECT_PAIR = 0, HMC_SELECT_PAIR10 = 1, HMC_SELECT_WIDE = 2, HMC_SELECT_RANK = 3 };
int hmc_test_coop_select(int device, int mode, int width, double *lik, uint32_t *tag, const int32_t *n,
                         const int32_t *nth, double *tie, int count);
/* The uniform hmc_posterior_draws uses for decision `step` of draw `draw` of
 * the individual with panel index `indiv` (philox.hpp: Philox4x32-10, key =
 * the two halves of seed, counter = (step, draw, indiv, 0)), on the host. */
double hmc_test_draw_uniform(uint64_t seed, int32_t indiv, int32_t draw, int32_t step);
/* Library version string. */
const char *hmc_version(void);
/* Version, target, flags and build time of this libhmc_amd.so (bench.py
 * prints it with the path of the library it loaded). */
const char *hmc_build_info(void);
/* Environment read by the library (diagnostics only; none changes a result
 * or what runs): HMC_DEBUG_MEM, HMC_DIAG_MINE print E-step group / mining
 * statistics to stderr; HMC_FORCE_COLLECTIVES makes a one-rank context run
 * its RCCL collectives anyway (test hook). */

#ifdef __cplusplus
}
#endif
#endif /* HMC_AMD_H */
