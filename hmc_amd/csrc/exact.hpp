// exact.hpp — device arguments of the exact M-step kernels (exact.hip) and of
// the posterior queries over the same records (exact_query.hip).
#pragma once
#include "dosage_plan.hpp"
#include "evidence_plan.hpp"
#include "window_plan.hpp"
#include "hmc_internal.hpp"

namespace hmc {

// Fixed-point scale of the frequency accumulators: 2^-44 resolution, totals
// up to 2^19 individuals fit in 63 bits.
constexpr double EXACT_FIXED_SCALE = 17592186044416.0;  // 2^44

struct ExactArgs {
  int L, head_len, width;          // loci, head length, alleles per trie node (max alleles per locus)
  const int32_t *order;            // individuals of this group (batch indices)
  int n_order;
  const uint32_t *rec;             // structure records (exact mode)
  const unsigned long long *rec_off;  // [batch][L+1]
  int32_t *status;                 // [batch]: EST_OK, or EST_NEEDS_EXACT when a forward likelihood underflows
  const double *gprob;             // [batch] P(genotype) of the last E-step
  // fwd/bwd store: per individual a region at x_base, per locus fwd[F] bwd[F]
  uint32_t *x;
  const unsigned long long *x_base;   // [batch]
  unsigned long long *x_off;          // [batch][L+1] (written by exact_fb)
  // ForwardPatternTree of the round's candidates (host-built)
  const int32_t *tr_child;         // [nodes][width], -1 = none
  const int32_t *tr_data;          // [nodes] candidate index or -1
  const int32_t *tr_root;          // [L] root node of each start locus, -1 = empty
  int max_depth;                   // longest candidate
  const uint8_t *head_al;          // [P][head_len] head patterns' alleles (head_len > 1)
  // per-wave scratch (exact_walk_scratch_doubles): lists [max_depth+1][width][3][fmax],
  // children's frequencies [max_depth+2][width] (doubles), touched states
  // [max_depth+1][fmax] (u32); zero before the launch
  double *scratch;
  size_t scratch_stride;           // doubles
  int fmax;                        // most states of any locus of the group
  long long span = 0;              // the walk's per-item list span: most states over max_depth + 2 consecutive depths
  unsigned *span_max = nullptr;    // exact_span: atomicMax of each individual's largest span (zeroed by the host)
  unsigned long long *acc_freq, *acc_prefix;  // [candidates] fixed point
  long long item0 = 0, item1 = -1;  // walk items [item0, item1) of n_order x L (individual-major); -1 = all
  bool forward_only = false;        // exact_fb leaves the backward values unwritten (the posterior draws never read them)
  // Extended range (hmc_set_posterior_range, hmc_genotype_likelihoods; never the
  // exact M-step): exact_fb keeps every record in range by exact powers of two.
  // The x-store then holds fs_j[t] = fwd_j[t] 2^E_j and bs_j[t] = bwd_j[t] 2^G_j
  // with every record's maximum in [0.5, 1), and the record's two spare words
  // (after bwd[F]) hold E_j and G_j as int32.  Per individual, xtot = the sum of
  // fs_L in state order from 0.0 and xtot_exp = E_L: P(genotype) = xtot 2^-E_L.
  bool extended = false;
  double *xtot = nullptr;           // [batch]
  int32_t *xtot_exp = nullptr;      // [batch]
};

// Breadth-first trie walk (exact_walk_units): one lane per work unit — a trie
// node of one item (individual q of the group, start locus) at depth `depth`
// with the non-zero entries of its three lists (state ascending; weights w0
// both haplotypes match the node's pattern, w1 only the a side, w2 only the b
// side).  A lane scatters the entries along the forward links into its
// private accumulators, adds every child's frequency and prefix term, and
// emits the children that have non-zero lists and children of their own as the
// next level's units.  Roots (depth 0) carry no entries: every state after
// max(start, head_len) loci with its forward likelihood.
struct XUnits {
  int32_t *q = nullptr, *start = nullptr, *node = nullptr;  // node < 0: a hole (skipped)
  double *freq = nullptr;                                   // the node's frequency: its children's prefix term
  unsigned long long *e0 = nullptr;                         // first entry in the pool
  uint32_t *ne = nullptr;                                   // entries
};
struct XWalkArgs {
  XUnits u;                       // the unit pool
  uint32_t *e_t = nullptr;        // entry pool: state
  double *e_w = nullptr;          // [3][e_cap] weights
  unsigned long long e_cap = 0, u_cap = 0;
  unsigned long long in_base = 0; // this level's units: [in_base, in_base + n_in), or idx[0, n_in) when idx
  const int32_t *idx = nullptr;
  int n_in = 0, depth = 0;
  bool roots = false;
  unsigned long long *cursor = nullptr;  // [2] next free unit, next free entry (outputs)
  int32_t *defer = nullptr;       // input units whose outputs did not fit (re-run later)
  int *n_defer = nullptr;
  double *lacc = nullptr;         // per thread [2][3][fmax]: the a-allele and b-allele child of each state
  uint32_t *lbits = nullptr;      // per thread reached-state bitmap [fmax / 32 + 1]
  size_t lacc_stride = 0, lbits_stride = 0;  // doubles, words
};
hipError_t launch_exact_walk_units(const ExactArgs &a, const XWalkArgs &x, int grid, hipStream_t st);

hipError_t launch_exact_fb(const ExactArgs &a, int grid, hipStream_t st);
// ExactArgs::span_max (atomicMax, zeroed by the caller) over the group
hipError_t launch_exact_span(const ExactArgs &a, int grid, hipStream_t st);
// items_per_wave 1 (64 lanes per item) or 4 (16 lanes each); scratch: grid x items x stride
hipError_t launch_exact_walk(const ExactArgs &a, int grid, hipStream_t st, int items_per_wave = 1);
size_t exact_walk_scratch_doubles(int max_depth, long long span, int width);
// Tries of at most this many alleles per node keep, per depth and slot, the
// child ids and the non-zero masks of the walk in LDS (wider ones read them)
constexpr int XWALK_CACHE_W = 8;
__host__ __device__ inline int exact_walk_cache_w(int width) { return width <= XWALK_CACHE_W ? width : 0; }
// LDS of one walked item: per depth two masks, two record offsets, eleven ints
// and 64 cached touched states (u16), per depth and cached slot a non-zero mask
// and a child id, the reached-state bitmap (8-byte multiple)
__host__ __device__ inline size_t exact_walk_lds_bytes(int max_depth, int fmax, int width) {
  const size_t D = (size_t)max_depth + 2, wc = (size_t)exact_walk_cache_w(width);
  return (D * 32 + D * wc * 8 + D * 44 + D * wc * 4 + D * 128 + (size_t)((fmax + 31) / 32 + 1) * 4 + 7) & ~(size_t)7;
}
constexpr size_t EXACT_WALK_LDS_MAX = 160 * 1024;  // gfx950 LDS per workgroup

// Genotype posteriors at missing loci (exact_site_posteriors): the sites of
// the shard's individuals as a CSR over batch indices, loci ascending; one
// output row of n_pairs bins per site (bin of {x, y} = xpair_index(x, y)).
struct SiteArgs {
  const unsigned long long *site_off = nullptr;  // [batch + 1]
  const int32_t *site_locus = nullptr;           // [sites]
  double *post = nullptr;                        // [sites][n_pairs]
  int32_t *site_status = nullptr;                // [sites] 0 ok; rows of zeros: 1 individual unresolved, 2 P(genotype) subnormal
  int n_pairs = 0;                               // width (width + 1) / 2
};
constexpr double SITE_PG_MIN = 2.2250738585072014e-308;  // DBL_MIN: below it the likelihoods have lost their bits
// after exact_fb over the same group; any block size that is a multiple of 64 gives the same bits
hipError_t launch_exact_site_posteriors(const ExactArgs &a, const SiteArgs &s, int grid, hipStream_t st, int block = 256);

// Switch posteriors (exact_switch_posteriors): an individual's sites are the
// pairs of consecutive heterozygous loci (both input alleles present and
// different), as a CSR over batch indices with locus_a ascending, so that
// locus_b of a site is locus_a of the individual's next one; one output row
// (cis, trans) per site.
struct SwitchArgs {
  const unsigned long long *site_off = nullptr;  // [batch + 1]
  const int32_t *locus_a = nullptr, *locus_b = nullptr;  // [sites]
  double *post = nullptr;                        // [sites][2]
  int32_t *site_status = nullptr;                // [sites] as SiteArgs::site_status
  int tier = 0;                                  // states per record whose two label frontiers the LDS holds (32 B per state)
  double *scratch = nullptr;                     // [grid][4 scratch_states]: the frontiers of individuals past the tier
  int scratch_states = 0;                        // the group's fmax when scratch is given
};
constexpr int SWITCH_TIER_DEFAULT = 1024;  // 32 KiB of LDS: four blocks to a compute unit
constexpr int SWITCH_TIER_MAX = 2032;      // with the kernel's static LDS within the 64 KiB a launch gets unasked
// after exact_fb over the same group; block sizes 64, 128, 192 and 256 give the same bits
hipError_t launch_exact_switch_posteriors(const ExactArgs &a, const SwitchArgs &s, int grid, hipStream_t st, int block = 256);

// Pair posteriors (exact_pair_posteriors): cis / trans for pairs (a, b) of
// heterozygous loci any distance apart.  An individual's distinct queries are
// rows of a CSR over batch indices; its sweep is a host-built event list in
// the order the kernel executes it: per round (one sweep over the records)
// ascending record, and at a record the evaluations and frees of the anchors
// carried in before the anchors that start there (an anchor inside the head is
// followed at once by its own head evaluations).
enum : int32_t { PAIR_EV_EVAL = 0, PAIR_EV_FREE = 1, PAIR_EV_ANCHOR = 2 };
struct PairEvent {
  int32_t rec;    // the record the event happens at (head_len for loci inside the head)
  int32_t op;     // kind | slot << 2
  int32_t locus;  // anchor: locus a; evaluate: locus b
  int32_t row;    // evaluate: the output row; else -1
};
struct PairArgs {
  const unsigned long long *row_off = nullptr;  // [batch + 1]
  const unsigned long long *ev_off = nullptr;   // [batch + 1]
  const PairEvent *ev = nullptr;
  double *post = nullptr;                        // [rows][2]
  int32_t *row_status = nullptr;                 // [rows] as SiteArgs::site_status
  int tier = 0;                                  // an individual whose largest record has at most this many states sweeps in LDS
  int lds_states = 0;                            // states the launch's LDS holds: min(tier, the group's fmax), 32 NS B each
  double *scratch = nullptr;                     // [grid][4 NS scratch_states]: the frontiers of individuals past the tier
  int scratch_states = 0;                        // the group's fmax when scratch is given
};
// Slots per state (NS): 1, 2, 4 and 8 are instantiated.  pair_tier_max: the
// states whose frontiers the 64 KiB a launch gets unasked hold beside the
// kernel's static LDS.  The default tier is that of the largest NS at every
// NS (8 / 16 / 32 / 64 KiB of LDS): on cfg 2 the sweep measured faster with it
// than with the whole 64 KiB at NS = 2 and 4 (6.5 against 7.7 ms, 12.6 against
// 14.7 ms) — more blocks to a compute unit outweigh the frontiers
// that move to device memory.
constexpr int PAIR_SLOTS_MAX = 8;
constexpr bool pair_slots_ok(int ns) { return ns == 1 || ns == 2 || ns == 4 || ns == 8; }
constexpr int pair_tier_max(int ns) { return 65024 / (32 * ns); }  // 2032, 1016, 508, 254
constexpr int PAIR_TIER_DEFAULT = pair_tier_max(PAIR_SLOTS_MAX);
// after exact_fb over the same group; NS, block sizes 64 .. 256 and the grid do not change the bits
hipError_t launch_exact_pair_posteriors(const ExactArgs &a, const PairArgs &s, int ns, int grid, hipStream_t st, int block = 256);

// Haplotype dosages (exact_haplotype_dosages): expected copies of caller-given
// patterns.  The pattern set, and so the plan (dosage_plan.hpp), is the same
// for every individual of a call: codes[pattern][row A, row B][maxlen] bytes
// (an allele-table index of the locus, DOSE_ANY or DOSE_ABSENT: both above 43,
// the largest index the exact path supports) and one event list in execution
// order (DoseEvent).  Individual q of the group (ExactArgs::order) owns output
// row q.
struct DoseArgs {
  const DoseEvent *ev = nullptr;
  int n_events = 0;
  const uint8_t *codes = nullptr;                // [n_patterns][2][maxlen]
  int n_patterns = 0, maxlen = 0;
  double *dosage = nullptr;                      // [n_order][n_patterns]
  int32_t *status = nullptr;                     // [n_order] 0 ok; rows of zeros: 1 unresolved, 2 P(genotype) subnormal
  int tier = 0;                                  // as PairArgs
  int lds_states = 0;
  double *scratch = nullptr;                     // [grid][4 NS scratch_states]
  int scratch_states = 0;
};
constexpr int DOSE_SLOTS_AUTO_MAX = 4;  // the most slots the automatic schedule takes (8 only when asked for: measured slower)
// after exact_fb over the same group; NS (1, 2, 4, 8; tiers as pair_tier_max), block sizes 64 .. 256 and the grid do
// not change the bits
hipError_t launch_exact_haplotype_dosages(const ExactArgs &a, const DoseArgs &s, int ns, int grid, hipStream_t st, int block = 256);

// Posterior draws (exact_posterior_draws): `draws` lattice paths per
// individual of the group, sampled backwards through the forward values
// exact_fb left in the x-store.  Individual q of the group (ExactArgs::order)
// owns output slot q.  The lanes store allele indices draw-minor,
// al[slot][side][locus][draw] bytes, so the 64 lanes of a wavefront (64
// consecutive draws) store adjacent bytes; draws_to_symbols or the host copy
// turns them into the caller's [slot][draw][side][locus] symbols.  al may be
// NULL (no haplotypes asked for).  status is zeroed by the caller: the kernel
// writes the non-zero ones only.
struct DrawArgs {
  int draws = 0;
  unsigned long long seed = 0;
  int indiv0 = 0;                  // panel index of batch index 0 (the shard's first individual)
  uint8_t *al = nullptr;           // [slots][2][L][draws] allele indices
  double *prob = nullptr;          // [slots][draws]
  int32_t *status = nullptr;       // [slots] 0 ok, 1 unresolved, 2 P(genotype) subnormal
  double *csum = nullptr;          // [grid][csum_stride]: the final record's chunk prefix sums past the LDS tier
  int csum_stride = 0;             // chunks of 64 states of the group's largest record
  int lds_chunks = 0;              // final records of at most this many chunks keep their prefix sums in LDS (0: none do)
};
constexpr int DRAW_BLOCK = 256;        // draws per block: four wavefronts of 64
constexpr int DRAW_LDS_CHUNKS = 1024;  // final records of up to 65 536 states keep their prefix sums in LDS (8 KiB)
// after exact_fb over the same group; the grid does not change the bits
hipError_t launch_exact_posterior_draws(const ExactArgs &a, const DrawArgs &s, int grid, hipStream_t st);
// al[slots][2][L][D] allele indices -> hap[slots][D][2][L] symbols of sym[L][W] (64 x 64 tiles through LDS)
hipError_t launch_draws_to_symbols(const uint8_t *al, const int32_t *sym, int32_t *hap, int slots, int L, int D, int W,
                                   hipStream_t st);

// MAP phasing (exact_map_phase): the most probable haplotype pair of every
// individual of the group and its exact posterior, by a max-product sweep
// over the records and a traceback in the same launch.  The sweep keeps two
// doubles per state and record, in the x-store slots exact_fb's forward-only
// pass over the same group has laid out (x_off) and filled: Vh over fwd[F], Vd
// over bwd[F] — after this launch the store holds no forward values.
// Individual q of the group (ExactArgs::order) owns output slot q; al in
// DrawArgs' layout with one draw, al[slot][side][locus] bytes (may be NULL);
// status is zeroed by the caller: the kernel writes the non-zero ones only.
struct MapArgs {
  uint8_t *al = nullptr;           // [slots][2][L] allele indices
  double *prob = nullptr;          // [slots]
  int32_t *status = nullptr;       // [slots] 0 ok, 1 unresolved, 2 P(genotype) subnormal
};
// after exact_fb (forward only will do) over the same group; block sizes 64 .. 256 and the grid do not change the bits
hipError_t launch_exact_map_phase(const ExactArgs &a, const MapArgs &s, int grid, hipStream_t st, int block = 256);

// MAP phasing given phase sets (exact_map_phase_given): exact_map_phase over
// the pairs consistent with caller-given evidence, and P(evidence | genotype).
// Per individual of the shard (batch index) the host plan's events
// (evidence_plan.hpp: constrained loci ascending, a set's first and last
// marked) as a CSR; the kernel never searches the caller's entries.  Two
// sweeps over the x-store slots exact_fb's forward-only pass has laid out —
// sums, then maxima — and exact_map_phase's traceback; outputs as MapArgs,
// plus evidence[slot].  Status 3: no consistent path (the sums come to 0).
struct GivenArgs {
  const unsigned long long *ev_off = nullptr;  // [batch + 1]
  const GivenEvent *ev = nullptr;
  uint8_t *al = nullptr;           // [slots][2][L] allele indices
  double *prob = nullptr;          // [slots]
  double *evidence = nullptr;      // [slots]
  int32_t *status = nullptr;       // [slots] 0 ok, 1 unresolved, 2 P(genotype) subnormal, 3 no consistent path
};
// after exact_fb (forward only will do) over the same group; block sizes 64 .. 256 and the grid do not change the bits
hipError_t launch_exact_map_phase_given(const ExactArgs &a, const GivenArgs &s, int grid, hipStream_t st, int block = 256);

// Ranked phasings (exact_ranked_phasings): the k haplotype pairs of largest
// exact posterior of every individual of the group, each once, by a list
// max-product sweep (two descending lists of KL values per state, KL >= k the
// list width the kernel was built with) and k tracebacks in the same launch.
// The lists do not fit the x-store, which exact_fb's forward-only pass over the
// same group has laid out (x_off; read for the states per record) and which
// keeps its forward values: the sweep has a store of its own, per individual
// rank_store_bytes(kl, states, records) from store_base[slot], record j of
// F states as values [F][2][KL] doubles, back-pointers [F][2][KL] words, the
// record's cumulative exponent and a pad word.
// Individual q of the group (ExactArgs::order) owns output slot q; al in
// DrawArgs' layout with draws = k, al[slot][side][locus][row] bytes (may be
// NULL); rows at and past count[slot] are left unwritten; status is zeroed by
// the caller: the kernel writes the non-zero ones only.
struct RankArgs {
  int k = 0;                       // rows per individual, 1 .. KL
  uint8_t *al = nullptr;           // [slots][2][L][k] allele indices
  double *prob = nullptr;          // [slots][k]
  int32_t *count = nullptr;        // [slots] rows written
  int32_t *status = nullptr;       // [slots] 0 ok, 1 unresolved, 2 P(genotype) subnormal
  uint8_t *store = nullptr;        // the list store
  const unsigned long long *store_base = nullptr;  // [slots] byte offsets into it (multiples of 8)
};
constexpr int RANK_K_MAX = 16;
// the smallest list width that is built and holds k rows (2, 4, 8, 16)
constexpr int rank_width(int k) { return k <= 2 ? 2 : k <= 4 ? 4 : k <= 8 ? 8 : 16; }
// list store of one individual with `states` states over `records` records
constexpr unsigned long long rank_store_bytes(int kl, unsigned long long states, int records) {
  return 24ull * (unsigned)kl * states + 8ull * (unsigned)records;
}
// total[q] = the states of all records of individual q of the group (0 for one exact_fb skipped); after exact_fb
hipError_t launch_exact_state_totals(const ExactArgs &a, unsigned long long *total, hipStream_t st);
// after exact_fb (forward only will do) over the same group; kl, block sizes 64 .. 256 and the grid do not change the bits
hipError_t launch_exact_ranked_phasings(const ExactArgs &a, const RankArgs &s, int kl, int grid, hipStream_t st, int block = 256);

// Window phasings (exact_window_phasings): the distinct haplotype pairs an
// individual can carry over a window of loci, each with its exact posterior
// summed over everything outside the window, ranked.  A state t carries one
// double per ordered configuration of the window's branching loci seen so far
// (window_plan.hpp: the code grows by a digit at each branching locus), an odd
// number of doubles apart (the window's C rounded up) so that a wavefront's
// reads of one code across states spread over the LDS banks.  item[q][w]: the digits and the count C of individual q of
// the group (ExactArgs::order) and window w; C = 0 (over the cap) is skipped.
// Rows: code[q][w][rank] (the row's a side is the smaller string), prob, and
// per (q, w) the rows written and the configurations of positive posterior.
// code is set to -1, prob, count, n_config and status to zero by the caller:
// the kernel writes the rows it finds and the non-zero statuses only.
struct WindowArgs {
  int n_windows = 0, k = 0;
  const int32_t *start = nullptr, *len = nullptr;  // [n_windows]
  const WinItem *item = nullptr;                   // [n_order][n_windows]
  const WinDigit *dig = nullptr;
  int32_t *code = nullptr;                         // [n_order][n_windows][k]
  double *prob = nullptr;                          // [n_order][n_windows][k]
  int32_t *count = nullptr, *n_config = nullptr;   // [n_order][n_windows]
  int32_t *status = nullptr;                       // [n_order] 0 ok, 1 unresolved, 2 P(genotype) subnormal
  int tier = 0;                                    // an individual whose largest record has at most this many states sweeps in LDS
  int lds_states = 0;                              // states the launch's LDS holds, 16 (NC + 1) B each
  double *scratch = nullptr;                       // the frontiers of individuals past the tier: individual q's slice is
  const unsigned long long *scratch_off = nullptr; // [scratch_off[q], scratch_off[q + 1]) doubles ([n_order + 1]; empty: none)
};
// Widths NC that are instantiated: the smallest that holds a batch's largest C runs it.
constexpr int win_width(int c) { return c <= 4 ? 4 : c <= 16 ? 16 : c <= 64 ? 64 : c <= 256 ? 256 : 1024; }
constexpr bool win_width_ok(int nc) { return nc == 4 || nc == 16 || nc == 64 || nc == 256 || nc == 1024; }
// the states whose two frontiers 40 KiB of LDS hold beside the kernel's tables (about 21 KiB at NC = 1024)
constexpr int win_tier_max(int nc) { return 40960 / (16 * (nc + 1)); }  // 512, 150, 39, 9, 2
// after exact_fb over the same group; nc, block sizes 64 .. 256, the tier and the grid do not change the bits
hipError_t launch_exact_window_phasings(const ExactArgs &a, const WindowArgs &s, int nc, int grid, hipStream_t st, int block = 256);

}  // namespace hmc
