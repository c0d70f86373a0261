// exact_query.hip — the posterior queries over the exact lattice: kernels that
// read the records of the structure pass (estep_split.hip) and the forward and
// backward values exact_fb (exact.hip) leaves in the x-store.  Their host side
// is ctx_query.cpp; the device code they share is in exact_dev.hpp.
#include "hmc_internal.hpp"
#include "estep_common.hpp"
#include "exact.hpp"
#include "exact_dev.hpp"
#include "philox.hpp"

namespace hmc {

// Posterior of the unordered allele pair at every site (individual, locus with
// a missing input allele) of the group, from the forward and backward
// likelihoods exact_fb left in the x-store: the states after locus k + 1
// (record k + 1) carry the pair of alleles at locus k in their header word,
// sum over a locus's states of fwd * bwd is P(genotype), so the bin of {x, y}
// is the sum over the states that carry {x, y}, over P(genotype).  Loci before
// the last head locus read the head record and take their alleles from the
// states' two head patterns, as exact_walk does.
// One block per individual; a wavefront owns a whole bin: lane l adds the
// products of the bin's states l, l + 64, ... in ascending order, then the 64
// lanes are summed by the fixed butterfly (group_sum_fixed).  The order of a
// bin's sum depends on the record's state order alone, so every block size,
// grid, grouping and shard gives the same bits; no floating-point atomics.
// States of other bins (and bins no state carries) add +0.0.  With more bins
// than waves (three or more alleles) one scan of the record first marks the
// bins that some state carries in an LDS bitmap (integer or: order-free), and
// only those are summed — at most the pairs the genotype allows, a handful at
// a site with one known allele, instead of all A (A + 1) / 2; the others are
// the 0.0 their sum of zeros would give.
// An individual whose P(genotype) is subnormal (below DBL_MIN: thousands of
// loci) has lost the bits of its likelihoods — exact_fb and the value pass
// keep raw doubles — so its rows would not sum to 1: they are zeros with
// site status 2.
// EXT (ExactArgs::extended): the x-store holds exact_fb's scaled values; the
// divisor is the scaled total xtot and the split scaling sc = -ilogb(pg)
// becomes, per site, the exponent difference E_L - E_j - G_j: the sum over a
// record of fs bs 2^(E_L - E_j - G_j) is xtot, so nothing overflows.  No
// status 2; status 1 only when the structure pass found no path or xtot is 0.
template <bool EXT>
__global__ __launch_bounds__(1024) void exact_site_posteriors(ExactArgs a, SiteArgs s) {
  const int lane = threadIdx.x & (WAVE - 1), wave = threadIdx.x / WAVE, nw = blockDim.x / WAVE;
  const int hl = a.head_len, NP = s.n_pairs;
  __shared__ uint32_t present[32];  // one bit per bin (NP <= 990)
  const bool sparse = NP > nw;      // block-uniform
  for (int q = blockIdx.x; q < a.n_order; q += gridDim.x) {
    const int bi = a.order[q];
    const unsigned long long s0 = s.site_off[bi], s1 = s.site_off[bi + 1];
    if (s0 == s1) continue;
    const QueryInd<EXT> ind(a, q);
    if (const int gu = ind.give_up_status()) {  // rows of zeros
      for (unsigned long long i = s0 * NP + threadIdx.x; i < s1 * NP; i += blockDim.x) s.post[i] = 0.0;
      for (unsigned long long i = s0 + threadIdx.x; i < s1; i += blockDim.x) s.site_status[i] = gu;
      continue;
    }
    PowScale<EXT> ps(ind);
    for (unsigned long long site = s0; site < s1; ++site) {
      const int k = s.site_locus[site];
      const bool head = k < hl - 1;  // alleles from the head patterns (head_len > 1 only)
      const int j = head ? hl : k + 1;
      const RecView R = ind.rec(j);
      const double *fw = ind.fwd(j), *bw = fw + R.F;
      ps.at_record(ind, (const int32_t *)(bw + R.F));  // ind.spare(j), from what is held
      auto bin_of = [&](int t) -> uint32_t {
        uint32_t xa, xb;
        state_alleles(a, R, head, k, t, xa, xb);
        return xpair_index(xa, xb);
      };
      double *out = s.post + site * NP;
      if (sparse) {
        if (threadIdx.x < 32) present[threadIdx.x] = 0u;
        __syncthreads();
        for (int t = threadIdx.x; t < R.F; t += blockDim.x) {
          const uint32_t b = bin_of(t);
          if (b < (uint32_t)NP) atomicOr(&present[b >> 5], 1u << (b & 31u));
        }
        __syncthreads();
      }
      for (int b = wave; b < NP; b += nw) {  // wave-uniform
        if (sparse && !((present[b >> 5] >> (b & 31)) & 1u)) {
          if (lane == 0) out[b] = 0.0;
          continue;
        }
        double part[1] = {0.0};
        for (int t = lane; t < R.F; t += WAVE)
          if (bin_of(t) == (uint32_t)b) part[0] += ps.term(fw[t], bw[t]);
        const double v = group_sum_fixed<WAVE>(part) / ps.pgs;
        if (lane == 0) out[b] = v;
      }
      if (threadIdx.x == 0) s.site_status[site] = 0;
      if (sparse) __syncthreads();  // the bitmap is cleared for the next site
    }
  }
}

hipError_t launch_exact_site_posteriors(const ExactArgs &a, const SiteArgs &s, int grid, hipStream_t st, int block) {
  if (a.n_order <= 0) return hipSuccess;
  if (block < WAVE || block > 1024 || block % WAVE || grid < 1 || s.n_pairs != a.width * (a.width + 1) / 2 || !s.site_off ||
      !s.post || !s.site_status)
    return hipErrorInvalidValue;
  if (a.extended) hipLaunchKernelGGL(exact_site_posteriors<true>, dim3(grid), dim3(block), 0, st, a, s);
  else hipLaunchKernelGGL(exact_site_posteriors<false>, dim3(grid), dim3(block), 0, st, a, s);
  return hipGetLastError();
}

// Switch posteriors (hmc_switch_posteriors): for every pair (a, b) of
// consecutive heterozygous loci of an individual, P(the lower-index alleles of
// a and b lie on the same haplotype | genotype) (cis) and P(on different ones)
// (trans), each a sum of its own.  One labelled forward sweep per individual
// (one block each) over the records exact_fb has filled: every state t carries
// two values g[0][t], g[1][t], the forward likelihood of the paths into t on
// which the anchor locus's lower allele sits on t's a side (0) or b side (1).
//   anchor    at record a + 1 (the states carry a's alleles): o(t) = 0 when
//             the a side holds the lower allele, else 1; g[o(t)][t] = fwd[t],
//             g[1 - o(t)][t] = 0;
//   propagate record j from j - 1: over t's contributions r in stored order,
//             g'[c ^ rev(r)][t] += g[c][state(r)] * tpv[t] — a reversed link
//             moves the a-side haplotype to the b side (walk_terms); the first
//             term assigns, later ones add, as exact_fb's forward does;
//   evaluate  at record b + 1: cis = sum_t g[o(t)][t] bwd[t] / P(genotype),
//             trans = sum_t g[1 - o(t)][t] bwd[t] / P(genotype); wavefront 0
//             owns cis, wavefront 1 trans: lane l adds states l, l + 64, ...
//             ascending, then the fixed butterfly.  Then b becomes the anchor.
// With head_len > 1 the head record's states carry loci 0 .. head_len - 1 in
// their two head patterns (a side plo, b side phi): a site inside the head is
// anchored and evaluated at the head record with no propagation between.
// The two frontiers (previous and current record, 2 doubles per state each)
// live in LDS when the individual's largest record has at most `tier` states,
// else in the block's slice of an HBM scratch: the same doubles in the same
// order either way.  A state's sums follow its record's contribution order and
// a site's sums the record's state order, so block size, grid, grouping, shard
// and tier do not change the bits; no floating-point atomics.
// Factors are scaled by cancelling powers of two as in exact_site_posteriors.
// EXT (ExactArgs::extended): as exact_site_posteriors; the label values are
// anchored from the scaled forward values of their record, so a propagation to
// record j multiplies them by 2^(E_j - E_(j-1)), the step exact_fb applied to
// the forward values there (ldexp: exact; g <= fs <= 1, so nothing overflows).
template <bool EXT>
__global__ __launch_bounds__(256) void exact_switch_posteriors(ExactArgs a, SwitchArgs s) {
  extern __shared__ double sw_lds[];  // [2 frontiers][tier states][2 labels]
  const int tid = threadIdx.x, NT = blockDim.x;
  const int hl = a.head_len;
  for (int q = blockIdx.x; q < a.n_order; q += gridDim.x) {
    const int bi = a.order[q];
    const unsigned long long s0 = s.site_off[bi], s1 = s.site_off[bi + 1];
    if (s0 == s1) continue;
    const QueryInd<EXT> ind(a, q);
    const int gu = ind.give_up_status();
    FrontierStore fr(a, ind.roff, ind.resolved(), sw_lds, s.tier, s.tier, s.scratch, s.scratch_states, 2);
    if (gu || !fr.fits) {  // rows of zeros
      for (unsigned long long i = s0 * 2 + tid; i < s1 * 2; i += NT) s.post[i] = 0.0;
      for (unsigned long long i = s0 + tid; i < s1; i += NT) s.site_status[i] = fr.fits ? gu : 1;
      continue;
    }
    PowScale<EXT> ps(ind);
    auto anchor = [&](int j, int k) {
      const RecView R = ind.rec(j);
      const double *fw = ind.fwd(j);
      for (int t = tid; t < R.F; t += NT) {
        const int o = low_side(a, R, k, t);
        fr.cur[2 * t + o] = fw[t];
        fr.cur[2 * t + (o ^ 1)] = 0.0;
      }
      __syncthreads();
    };
    int j = s.locus_a[s0] < hl ? hl : s.locus_a[s0] + 1;
    __syncthreads();  // the previous individual's last readers of the frontiers are done
    anchor(j, s.locus_a[s0]);
    for (unsigned long long site = s0; site < s1; ++site) {
      const int kb = s.locus_b[site];
      const int jb = kb < hl ? hl : kb + 1;
      while (j < jb) {  // record j + 1 from record j (j + 1 > head_len: never the head record)
        ++j;
        fr.swap();
        const int step = EXT ? ind.spare(j)[0] - ind.spare(j - 1)[0] : 0;
        propagate_labels<1, EXT, LabelPair8>(ind.rec(j), fr.prev, fr.cur, step, 1u);
      }
      {
        const RecView R = ind.rec(j);
        ps.at_record(ind, ind.spare(j));
        ps.label_sums(  // 0 cis, 1 trans
            R.F, ind.bwd(j), [&](int t, int w) { return fr.cur[2 * t + (low_side(a, R, kb, t) ^ w)]; },
            [&](int w, double v) { s.post[site * 2 + w] = v / ps.pgs; });
        if (tid == 0) s.site_status[site] = 0;
      }
      __syncthreads();  // the sums have read the frontier the next anchor overwrites
      if (site + 1 < s1) anchor(j, kb);
    }
  }
}

hipError_t launch_exact_switch_posteriors(const ExactArgs &a, const SwitchArgs &s, int grid, hipStream_t st, int block) {
  if (a.n_order <= 0) return hipSuccess;
  if (block < WAVE || block > 256 || block % WAVE || grid < 1 || s.tier < 1 || s.tier > SWITCH_TIER_MAX || !s.site_off ||
      !s.locus_a || !s.locus_b || !s.post || !s.site_status || (s.scratch && s.scratch_states < 1))
    return hipErrorInvalidValue;
  if (a.extended) hipLaunchKernelGGL(exact_switch_posteriors<true>, dim3(grid), dim3(block), (size_t)s.tier * 32, st, a, s);
  else hipLaunchKernelGGL(exact_switch_posteriors<false>, dim3(grid), dim3(block), (size_t)s.tier * 32, st, a, s);
  return hipGetLastError();
}

// Pair posteriors (hmc_pair_posteriors): cis and trans as in
// exact_switch_posteriors, for pairs (a, b) of heterozygous loci any distance
// apart, with several anchors live in one labelled forward sweep.  A state t
// carries 2 NS doubles g[slot][0..1][t]; a slot holds one anchor locus from
// its record to the record of the farthest b asked for it.  The three steps
// are the switch kernel's, per slot:
//   anchor    slot s at record a + 1 from fwd: g[s][o(t)][t] = fwd[t], the
//             other label 0;
//   propagate record j from j - 1: a state's contribution words and tpv[t]
//             are read once, and every live slot takes the switch kernel's two
//             running sums in the record's contribution order (the first term
//             assigns, later ones add); dead slots are neither read nor
//             written;
//   evaluate  query (a, b) at record b + 1 from a's slot: wavefront 0 owns
//             cis, wavefront 1 trans, lane l adds states l, l + 64, ...
//             ascending, the fixed butterfly, one division by the scaled
//             P(genotype).
// The host turns an individual's queries into an event list in execution
// order (PairEvent, exact.hpp): the kernel never searches the queries.  Between
// events it propagates up to the next event's record while a slot is live and
// jumps there when none is, which is also how a later round (the anchors that
// found no free slot among NS) starts again from an earlier record.
// A query's two doubles are a function of the records, the forward and
// backward values and (a, b) alone: the slot only names where the anchor's
// labelled values are kept, so NS, slot, round, the other queries, block size,
// grid, grouping, shard and tier do not change the bits, and a query whose b
// is the next heterozygous locus after a repeats exact_switch_posteriors'
// operations for that site.  No floating-point atomics, no cross-wave sums.
// The frontiers (32 NS bytes per state for the two) live in LDS when the
// individual's largest record has at most `tier` states, else in the block's
// slice of an HBM scratch.
// EXT (ExactArgs::extended): as exact_switch_posteriors, every live slot's
// two sums times the record's forward exponent step.
template <int NS, bool EXT>
__global__ __launch_bounds__(256) void exact_pair_posteriors(ExactArgs a, PairArgs s) {
  extern __shared__ __attribute__((aligned(16))) double pr_lds[];  // [2 frontiers][lds_states][NS slots][2 labels]
  const int tid = threadIdx.x, NT = blockDim.x;
  const int L = a.L, hl = a.head_len;
  for (int q = blockIdx.x; q < a.n_order; q += gridDim.x) {
    const int bi = a.order[q];
    const unsigned long long s0 = s.row_off[bi], s1 = s.row_off[bi + 1];
    if (s0 == s1) continue;
    const QueryInd<EXT> ind(a, q);
    const int gu = ind.give_up_status();
    FrontierStore fr(a, ind.roff, ind.resolved(), pr_lds, min(s.tier, s.lds_states), s.lds_states, s.scratch, s.scratch_states,
                     2 * NS);
    if (gu || !fr.fits) {  // rows of zeros
      for (unsigned long long i = s0 * 2 + tid; i < s1 * 2; i += NT) s.post[i] = 0.0;
      for (unsigned long long i = s0 + tid; i < s1; i += NT) s.row_status[i] = fr.fits ? gu : 1;
      continue;
    }
    PowScale<EXT> ps(ind);
    __syncthreads();  // the previous individual's last readers of the frontiers are done
    const unsigned long long e0 = s.ev_off[ind.bi], e1 = s.ev_off[ind.bi + 1];
    unsigned live = 0;     // slots that hold an anchor (block-uniform, as everything the events decide)
    int j = hl;            // the record `cur` belongs to
    bool unread = false;   // evaluations since the last barrier may still be reading `cur`
    for (unsigned long long e = e0; e < e1; ++e) {
      const PairEvent ev = s.ev[e];
      const int kind = ev.op & 3, slot = ev.op >> 2;
      if (ev.rec < hl || ev.rec > L || slot >= NS) continue;  // (the host builds none such)
      if (live == 0u || ev.rec < j) {  // nothing to carry: the next round, or a gap between intervals
        j = ev.rec;
        live = 0u;
      }
      while (j < ev.rec) {  // record j + 1 from record j (j + 1 > head_len: never the head record)
        ++j;
        fr.swap();
        const int step = EXT ? ind.spare(j)[0] - ind.spare(j - 1)[0] : 0;
        propagate_labels<NS, EXT, double2>(ind.rec(j), fr.prev, fr.cur, step, live);
        unread = false;
      }
      const RecView R = ind.rec(j);
      if (kind == PAIR_EV_EVAL) {
        if (!((live >> slot) & 1u) || ev.row < 0 || s0 + (unsigned long long)ev.row >= s1) continue;  // (none such)
        const unsigned long long row = s0 + (unsigned long long)ev.row;
        ps.at_record(ind, ind.spare(j));
        ps.label_sums(  // 0 cis, 1 trans
            R.F, ind.bwd(j), [&](int t, int w) { return fr.cur[((size_t)t * NS + slot) * 2 + (low_side(a, R, ev.locus, t) ^ w)]; },
            [&](int w, double v) { s.post[row * 2 + w] = v / ps.pgs; });
        if (tid == 0) s.row_status[row] = 0;
        unread = true;
      } else if (kind == PAIR_EV_FREE) {
        live &= ~(1u << slot);
      } else if (kind == PAIR_EV_ANCHOR) {
        if (unread) __syncthreads();  // the sums have read the slot this anchor overwrites
        const double *fw = ind.fwd(j);
        for (int t = tid; t < R.F; t += NT) {
          const int o = low_side(a, R, ev.locus, t);
          double *g = fr.cur + ((size_t)t * NS + slot) * 2;
          g[o] = fw[t];
          g[o ^ 1] = 0.0;
        }
        __syncthreads();
        unread = false;
        live |= 1u << slot;
      }
    }
  }
}

template <int NS>
static hipError_t launch_pair(const ExactArgs &a, const PairArgs &s, int grid, hipStream_t st, int block) {
  if (a.extended)
    hipLaunchKernelGGL((exact_pair_posteriors<NS, true>), dim3(grid), dim3(block), (size_t)s.lds_states * 32 * NS, st, a, s);
  else
    hipLaunchKernelGGL((exact_pair_posteriors<NS, false>), dim3(grid), dim3(block), (size_t)s.lds_states * 32 * NS, st, a, s);
  return hipGetLastError();
}

hipError_t launch_exact_pair_posteriors(const ExactArgs &a, const PairArgs &s, int ns, int grid, hipStream_t st, int block) {
  if (a.n_order <= 0) return hipSuccess;
  if (block < WAVE || block > 256 || block % WAVE || grid < 1 || !pair_slots_ok(ns) || s.tier < 1 || s.lds_states < 1 ||
      s.lds_states > pair_tier_max(ns) || !s.row_off || !s.ev_off || !s.ev || !s.post || !s.row_status ||
      (s.scratch && s.scratch_states < 1))
    return hipErrorInvalidValue;
  return ns == 1   ? launch_pair<1>(a, s, grid, st, block)
         : ns == 2 ? launch_pair<2>(a, s, grid, st, block)
         : ns == 4 ? launch_pair<4>(a, s, grid, st, block)
                   : launch_pair<8>(a, s, grid, st, block);
}

// Haplotype dosages (hmc_haplotype_dosages): for caller-given patterns p — a
// window start .. start + len - 1 with two rows of allele codes A, B (an allele
// index, DOSE_ANY or DOSE_ABSENT) — d = sum over unordered pairs {h0, h1} of
// post({h0, h1}) ([M(h0, h1)] + [M(h1, h0)]), M(x, y) true when x matches row A
// and y row B at every locus of the window.  A sibling of
// exact_pair_posteriors: one block per individual, a state t carries 2 NS
// doubles g[slot][c][t], c = 0 when the haplotype held against row A lies on
// t's a side (hdr & 0xFF), c = 1 when on its b side; a slot holds one pattern
// from its first record to its last.  With xa, xb the state's alleles of locus
// k: ok0 = match(xa, A[k]) && match(xb, B[k]), ok1 = match(xb, A[k]) &&
// match(xa, B[k]).
//   anchor    slot s at the record of `start` from fwd: g[s][0][t] = ok0 ?
//             fwd[t] : 0, g[s][1][t] = ok1 ? fwd[t] : 0 (a homozygous matching
//             state takes both);
//   propagate record j from j - 1 as exact_switch_posteriors does — over t's
//             contributions r in stored order g'[c ^ rev(r)][t] += g[c][state(r)]
//             tpv[t], the first term assigns, later ones add — then a label
//             whose ok is false at locus j - 1 is stored as 0.0; a slot with
//             both false at t takes no sums.  Contribution words and tpv[t] are
//             read once per state for all live slots;
//   evaluate  at the record of the window's last locus: S_c = sum_t g[c][t]
//             bwd[t]; wavefront 0 owns S_0, wavefront 1 S_1, lane l adds states
//             l, l + 64, ... ascending, then the fixed butterfly; one thread
//             forms d = (S_0 + S_1) / P(genotype) (scaled as in
//             exact_site_posteriors).
// Loci below head_len (head_len > 1) are matched at the head record from the
// states' two head patterns, all of the window's head loci at the anchor, with
// no propagation between them.
// Why the lattice gives the definition (the path-to-pair bookkeeping of
// hmc_posterior_draws): a path ends with its a-side and b-side haplotype, and
// both labels are summed, so a path of posterior w adds w ([M(a, b)] + [M(b,
// a)]).  A heterozygous head state carries its factor 2 and is the pair's only
// path; a heterozygous pair behind a homozygous prefix is two paths of half
// its posterior each, one per orientation, and both add the same two-term sum;
// a homozygous pair is one path whose two labels coincide.  In every case the
// pair adds post ([M(h0, h1)] + [M(h1, h0)]).
// The host gives one event list for the call (DoseEvent, exact.hpp), the same
// for every individual, in execution order: the kernel never searches the
// patterns, propagates while a slot is live and jumps to the next event's
// record when none is (also how a later round starts again).  A pattern's
// double is a function of the records, the forward and backward values and its
// own (start, len, A, B): the slot only names where its labelled values are
// kept, so NS, slot, round, the other patterns, block size, grid, grouping,
// shard and tier do not change the bits.  No floating-point atomics, no
// cross-wave sums beyond S_0 + S_1.
// The frontiers (32 NS bytes per state for the two) live in LDS when the
// individual's largest record has at most `tier` states, else in the block's
// slice of an HBM scratch: the same doubles in the same order.
// EXT (ExactArgs::extended): as exact_switch_posteriors, every live slot's sums
// times the record's forward exponent step; evaluation cancels E_j + G_j
// against E_L.
template <int NS, bool EXT>
__global__ __launch_bounds__(256) void exact_haplotype_dosages(ExactArgs a, DoseArgs s) {
  extern __shared__ __attribute__((aligned(16))) double ds_lds[];  // [2 frontiers][lds_states][NS slots][2 labels]
  __shared__ double s_sum[PAIR_SLOTS_MAX][2];  // S_0, S_1 of the evaluations not yet written out
  __shared__ int s_col[PAIR_SLOTS_MAX];        // their patterns
  const int tid = threadIdx.x, NT = blockDim.x;
  const int L = a.L, hl = a.head_len, P = s.n_patterns, ML = s.maxlen;
  for (int q = blockIdx.x; q < a.n_order; q += gridDim.x) {
    const QueryInd<EXT> ind(a, q);
    double *out = s.dosage + (size_t)q * P;
    const int gu = ind.give_up_status();
    FrontierStore fr(a, ind.roff, ind.resolved(), ds_lds, min(s.tier, s.lds_states), s.lds_states, s.scratch, s.scratch_states,
                     2 * NS);
    if (gu || !fr.fits) {  // a row of zeros
      for (int i = tid; i < P; i += NT) out[i] = 0.0;
      if (tid == 0) s.status[q] = fr.fits ? gu : 1;
      continue;
    }
    PowScale<EXT> ps(ind);
    auto match = [](uint32_t x, uint32_t code) { return code == DOSE_ANY || code == x; };
    __syncthreads();  // the previous individual's last readers of the frontiers are done
    unsigned live = 0;   // slots that hold a pattern (block-uniform, as everything the events decide)
    unsigned pend = 0;   // slots whose S_0, S_1 wait in s_sum
    int j = hl;          // the record `cur` belongs to
    long long cbase[NS]; // per slot: the pattern's row A in s.codes, less its start (row B: + maxlen)
#pragma unroll
    for (int u = 0; u < NS; ++u) cbase[u] = 0;
    // the sums of the evaluations since the last barrier, one thread per slot (after a barrier)
    auto flush = [&]() {
      if (tid < NS && ((pend >> tid) & 1u)) out[s_col[tid]] = (s_sum[tid][0] + s_sum[tid][1]) / ps.pgs;
      pend = 0u;
    };
    for (int e = 0; e < s.n_events; ++e) {
      const DoseEvent ev = s.ev[e];
      const int kind = ev.op & 3, slot = ev.op >> 2;
      if (ev.rec < hl || ev.rec > L || slot < 0 || slot >= NS || ev.pat < 0 || ev.pat >= P || ev.start < 0 ||
          ev.start >= L)
        continue;  // (the host builds none such)
      if (live == 0u || ev.rec < j) {  // nothing to carry: the next round, or a gap between windows
        j = ev.rec;
        live = 0u;
      }
      while (j < ev.rec) {  // record j + 1 from record j (j + 1 > head_len: never the head record)
        if (pend) {
          __syncthreads();
          flush();
        }
        ++j;
        fr.swap();
        const RecView R = ind.rec(j);
        const int step = EXT ? ind.spare(j)[0] - ind.spare(j - 1)[0] : 0;
        uint32_t ca[NS], cb[NS];  // the live slots' codes of locus j - 1
#pragma unroll
        for (int u = 0; u < NS; ++u) {
          const bool on = (live >> u) & 1u;
          ca[u] = on ? s.codes[cbase[u] + (j - 1)] : DOSE_ABSENT;
          cb[u] = on ? s.codes[cbase[u] + ML + (j - 1)] : DOSE_ABSENT;
        }
        // propagate_labels' step with the match masks: a label whose side does not match the slot's codes of
        // locus j - 1 is stored as 0.0, a slot with neither takes no sums.  (Through the helper and a mask
        // functor the NS = 8 sweep measured 6-8 % slower: profiles/query_kernels/README.md.)
        const double *prev = fr.prev;
        double *cur = fr.cur;
        for (int t = tid; t < R.F; t += NT) {
          const uint32_t h = R.hdr[t], xa = h & 0xFFu, xb = (h >> 8) & 0xFFu;
          unsigned k0 = 0u, k1 = 0u;  // per slot: ok0, ok1
#pragma unroll
          for (int u = 0; u < NS; ++u)
            if ((live >> u) & 1u) {
              if (match(xa, ca[u]) && match(xb, cb[u])) k0 |= 1u << u;
              if (match(xb, ca[u]) && match(xa, cb[u])) k1 |= 1u << u;
            }
          const unsigned need = k0 | k1;
          double n0[NS], n1[NS];
#pragma unroll
          for (int u = 0; u < NS; ++u) n0[u] = n1[u] = 0.0;
          if (need) {
            const double tpv = R.tpv[t];
            const uint32_t r0 = R.cb[t], r1 = R.cb[t + 1];
            for (uint32_t r = r0; r < r1; ++r) {
              const uint32_t w = R.ct[r];
              const bool rv = cw_rev(w);
              const double2 *p = (const double2 *)(prev + (size_t)cw_state(w) * 2 * NS);
#pragma unroll
              for (int u = 0; u < NS; ++u)
                if ((need >> u) & 1u) {
                  const double2 g = p[u];
                  const double v0 = (rv ? g.y : g.x) * tpv, v1 = (rv ? g.x : g.y) * tpv;
                  n0[u] = r == r0 ? v0 : n0[u] + v0;
                  n1[u] = r == r0 ? v1 : n1[u] + v1;
                }
            }
          }
          double2 *o = (double2 *)(cur + (size_t)t * 2 * NS);
#pragma unroll
          for (int u = 0; u < NS; ++u)
            if ((live >> u) & 1u) {
              const double g0 = (k0 >> u) & 1u ? (EXT ? ldexp(n0[u], step) : n0[u]) : 0.0;
              const double g1 = (k1 >> u) & 1u ? (EXT ? ldexp(n1[u], step) : n1[u]) : 0.0;
              o[u] = make_double2(g0, g1);
            }
        }
        __syncthreads();
      }
      const RecView R = ind.rec(j);
      if (kind == DOSE_EV_EVAL) {
        if (!((live >> slot) & 1u)) continue;  // (none such)
        ps.at_record(ind, ind.spare(j));
        ps.label_sums(  // S_0, S_1
            R.F, ind.bwd(j), [&](int t, int w) { return fr.cur[((size_t)t * NS + slot) * 2 + w]; },
            [&](int w, double v) {
              s_sum[slot][w] = v;
              if (w == 0) s_col[slot] = ev.pat;
            });
        pend |= 1u << slot;
        live &= ~(1u << slot);
      } else if (kind == DOSE_EV_ANCHOR) {
        if (pend) {  // (the barrier also lets the sums finish reading the slot this anchor overwrites)
          __syncthreads();
          flush();
        }
        const long long base = (long long)ev.pat * 2 * ML - ev.start;
#pragma unroll
        for (int u = 0; u < NS; ++u)
          if (u == slot) cbase[u] = base;
        const double *fw = ind.fwd(j);
        const bool head = j == hl && hl > 1;  // the window's loci below head_len, from the head patterns
        const int k0 = ev.start, k1 = head ? min(ev.start + ev.len, hl) : ev.start + 1;
        for (int t = tid; t < R.F; t += NT) {
          bool ok0 = true, ok1 = true;
          for (int k = k0; k < k1; ++k) {
            uint32_t xa, xb;
            state_alleles(a, R, head, k, t, xa, xb);
            const uint32_t cA = s.codes[base + k], cB = s.codes[base + ML + k];
            ok0 = ok0 && match(xa, cA) && match(xb, cB);
            ok1 = ok1 && match(xb, cA) && match(xa, cB);
          }
          const double f = fw[t];
          double *g = fr.cur + ((size_t)t * NS + slot) * 2;
          g[0] = ok0 ? f : 0.0;
          g[1] = ok1 ? f : 0.0;
        }
        __syncthreads();
        live |= 1u << slot;
      }
    }
    if (pend) {
      __syncthreads();
      flush();
    }
    if (tid == 0) s.status[q] = 0;
  }
}

template <int NS>
static hipError_t launch_dosage(const ExactArgs &a, const DoseArgs &s, int grid, hipStream_t st, int block) {
  if (a.extended)
    hipLaunchKernelGGL((exact_haplotype_dosages<NS, true>), dim3(grid), dim3(block), (size_t)s.lds_states * 32 * NS, st, a, s);
  else
    hipLaunchKernelGGL((exact_haplotype_dosages<NS, false>), dim3(grid), dim3(block), (size_t)s.lds_states * 32 * NS, st, a, s);
  return hipGetLastError();
}

hipError_t launch_exact_haplotype_dosages(const ExactArgs &a, const DoseArgs &s, int ns, int grid, hipStream_t st, int block) {
  if (a.n_order <= 0 || s.n_events <= 0) return hipSuccess;
  if (block < WAVE || block > 256 || block % WAVE || grid < 1 || !pair_slots_ok(ns) || s.tier < 1 || s.lds_states < 1 ||
      s.lds_states > pair_tier_max(ns) || !s.ev || !s.codes || !s.dosage || !s.status || s.n_patterns < 1 || s.maxlen < 1 ||
      (s.scratch && s.scratch_states < 1))
    return hipErrorInvalidValue;
  return ns == 1   ? launch_dosage<1>(a, s, grid, st, block)
         : ns == 2 ? launch_dosage<2>(a, s, grid, st, block)
         : ns == 4 ? launch_dosage<4>(a, s, grid, st, block)
                   : launch_dosage<8>(a, s, grid, st, block);
}

// Posterior draws (hmc_posterior_draws): whole haplotype pairs sampled from
// the exact posterior by backward sampling through the forward values of
// exact_fb.  A state's forward value is tpv[t] times the sum of its
// predecessors' forward values over its contributions, so a path is drawn with
// its posterior probability by choosing the final state in proportion to
// fwd_L and then, record by record down to the head, one contribution of the
// current state in proportion to the predecessor's forward value.
// One lane per draw, 64 consecutive draws of one individual per wavefront,
// four wavefronts per block; the grid runs over (individual of the group,
// chunk of 256 draws).  Every choice takes the first index whose running sum
// exceeds u x (the full sum), else the last index with a positive term:
//   final record   the F states in chunks of 64: chunk c's sum is the fixed
//                  butterfly over states 64 c .. 64 c + 63 (zeros past F), the
//                  chunk prefix S_c = S_c-1 + chunk c's sum in chunk order,
//                  the full sum S_last.  The block computes the prefix once per
//                  individual (LDS, or its slice of a device scratch for
//                  records past DRAW_LDS_CHUNKS chunks — the same doubles); a
//                  lane searches it for the first chunk with S_c > target and
//                  then adds that chunk's states to S_c-1 one by one in state
//                  order;
//   contributions  of state t at record j, in record order (the order exact_fb
//                  adds them in): one pass for the full sum, one for the choice.
// u = draw_uniform(seed, panel index, draw, step) (philox.hpp), step 0 for the
// final record and 1 + (L - j) at record j: nothing about the launch enters.
// Haplotypes as estep_traceback spells a candidate: a side parity, flipped by
// the chosen contribution's rev flag after the state's two alleles are written.
// prob = ((tpv of the states from record L down to the head, multiplied in
// that order) x 2 if the two haplotypes differ) / P(genotype).
// EXT (ExactArgs::extended): every choice compares running sums within one
// record, all of whose values carry the same power of two, so the scaled
// forward values give the same choices.  The running product of tpv is kept
// as a mantissa in [0.5, 1) and a count of the powers of two taken out
// (frexp: exact), the count cancels against the total's exponent E_L, and prob
// is rounded by the division and, if subnormal, once more by the final ldexp.
template <bool EXT>
__global__ __launch_bounds__(DRAW_BLOCK) void exact_posterior_draws(ExactArgs a, DrawArgs s) {
  __shared__ double cs_lds[DRAW_LDS_CHUNKS];
  const int tid = threadIdx.x, lane = tid & (WAVE - 1), wave = tid / WAVE;
  constexpr int NW = DRAW_BLOCK / WAVE;
  const int L = a.L, hl = a.head_len, D = s.draws;
  const int ndc = (D + DRAW_BLOCK - 1) / DRAW_BLOCK;  // chunks of draws per individual
  const long long items = (long long)a.n_order * ndc;
  for (long long it = blockIdx.x; it < items; it += gridDim.x) {  // block-uniform
    const int q = (int)(it / ndc), dc = (int)(it % ndc);
    const int d = dc * DRAW_BLOCK + tid;
    const QueryInd<EXT> ind(a, q);
    if (const int gu = ind.give_up_status()) {  // the host writes the input genotype
      if (tid == 0 && dc == 0) s.status[q] = gu;
      continue;
    }
    const double *fwL = ind.fwd(L);
    const int F = ind.F(L), nc = (F + WAVE - 1) / WAVE;
    const bool in_lds = nc <= s.lds_chunks && nc <= DRAW_LDS_CHUNKS;
    if (!in_lds && (!s.csum || nc > s.csum_stride)) {  // (cannot occur: the host sizes the scratch from the group's fmax)
      if (tid == 0 && dc == 0) s.status[q] = 1;
      continue;
    }
    double *cs = in_lds ? cs_lds : s.csum + (size_t)blockIdx.x * s.csum_stride;
    __syncthreads();  // the previous item's lanes have read its prefix
    for (int c = wave; c < nc; c += NW) {
      const int t = c * WAVE + lane;
      double part[1] = {t < F ? fwL[t] : 0.0};
      const double v = group_sum_fixed<WAVE>(part);
      if (lane == 0) cs[c] = v;
    }
    __syncthreads();
    if (tid == 0) {
      double r = 0.0;
      for (int c = 0; c < nc; ++c) {
        r += cs[c];
        cs[c] = r;
      }
    }
    __syncthreads();
    if (d >= D) continue;  // (the barriers above are passed by every thread of the block)
    const uint32_t pi = (uint32_t)(s.indiv0 + ind.bi), du = (uint32_t)d;
    PathSpeller<EXT> sp(s.al, q, L, D, d, s.al != nullptr);  // (regular range: the raw product)
    int t;
    {  // the final state
      const double target = draw_uniform(s.seed, pi, du, 0u) * cs[nc - 1];
      int lo = 0, hi = nc - 1;  // S_last > target: u < 1
      while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (cs[mid] > target) hi = mid;
        else lo = mid + 1;
      }
      double run = lo > 0 ? cs[lo - 1] : 0.0;
      const int t1 = min(F, (lo + 1) * WAVE);
      int pick = -1, last = lo * WAVE;
      for (int x = lo * WAVE; x < t1; ++x) {
        const double v = fwL[x];
        run += v;
        if (v > 0.0) last = x;
        if (run > target) {
          pick = x;
          break;
        }
      }
      t = pick >= 0 ? pick : last;
    }
    bool dead = false;
    for (int j = L; j > hl; --j) {
      const RecView R = ind.rec(j);
      const uint32_t r0 = R.cb[t], r1 = R.cb[t + 1];
      const double *fp = ind.fwd(j - 1);
      sp.enter(R, j, t);
      // the full sum: four contributions at a time, their words, then their
      // predecessors' forward values, then the terms in record order
      double tot = 0.0;
      for (uint32_t r = r0; r < r1; r += 4) {
        uint32_t wv[4];
        double fv[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) wv[k] = r + k < r1 ? R.ct[r + k] : 0u;
#pragma unroll
        for (int k = 0; k < 4; ++k) fv[k] = r + k < r1 ? fp[cw_state(wv[k])] : 0.0;
#pragma unroll
        for (int k = 0; k < 4; ++k) tot += fv[k];
      }
      const double target = draw_uniform(s.seed, pi, du, (uint32_t)(1 + (L - j))) * tot;
      double run = 0.0;
      uint32_t wsel = 0u, wlast = 0u;
      bool got = false, any = false;
      for (uint32_t r = r0; r < r1; ++r) {
        const uint32_t w = R.ct[r];
        const double v = fp[cw_state(w)];
        run += v;
        if (v > 0.0) {
          wlast = w;
          any = true;
        }
        if (run > target) {
          wsel = w;
          got = true;
          break;
        }
      }
      if (!got) {
        if (!any) {  // (a state no path reaches: a zero term is never chosen, so no draw arrives here;
                     // if one did, the individual counts as unresolved and the host writes its input genotype)
          dead = true;
          s.status[q] = 1;
          break;
        }
        wsel = wlast;
      }
      sp.follow(wsel);
      t = (int)cw_state(wsel);
    }
    if (!dead) sp.head(a, ind.rec(hl), t);
    if (s.prob) s.prob[(size_t)q * D + d] = dead ? 0.0 : sp.prob(ind.pg, ind.pge);
  }
}

hipError_t launch_exact_posterior_draws(const ExactArgs &a, const DrawArgs &s, int grid, hipStream_t st) {
  if (a.n_order <= 0) return hipSuccess;
  if (grid < 1 || s.draws < 1 || !s.status || s.lds_chunks < 0 ||
      s.lds_chunks > DRAW_LDS_CHUNKS || (s.csum && s.csum_stride < 1))
    return hipErrorInvalidValue;
  if (a.extended) hipLaunchKernelGGL(exact_posterior_draws<true>, dim3(grid), dim3(DRAW_BLOCK), 0, st, a, s);
  else hipLaunchKernelGGL(exact_posterior_draws<false>, dim3(grid), dim3(DRAW_BLOCK), 0, st, a, s);
  return hipGetLastError();
}

// The draws' allele indices al[slot][side][locus][draw] (bytes, as the lanes
// of exact_posterior_draws store them) into the caller's layout
// hap[slot][draw][side][locus] as symbols of sym[locus][width]: tiles of 64
// loci x 64 draws through LDS, read along the draws and written along the
// loci.  A byte that is no allele index (an individual the draw kernel left
// unwritten: status 1 or 2) becomes -1; the host overwrites those rows.
__global__ __launch_bounds__(256) void draws_to_symbols(const uint8_t *al, const int32_t *sym, int32_t *hap, int L, int D, int W) {
  __shared__ uint8_t tile[64][65];
  const size_t us = blockIdx.x;  // slot * 2 + side
  const int l0 = blockIdx.y * 64, d0 = blockIdx.z * 64;
  for (int k = threadIdx.x; k < 64 * 64; k += 256) {
    const int l = k / 64, d = k % 64;
    if (l0 + l < L && d0 + d < D) tile[l][d] = al[(us * L + l0 + l) * D + d0 + d];
  }
  __syncthreads();
  const size_t slot = us >> 1, side = us & 1;
  for (int k = threadIdx.x; k < 64 * 64; k += 256) {
    const int d = k / 64, l = k % 64;
    if (l0 + l < L && d0 + d < D) {
      const int x = tile[l][d];
      hap[((slot * D + d0 + d) * 2 + side) * L + l0 + l] = x < W ? sym[(size_t)(l0 + l) * W + x] : -1;
    }
  }
}

hipError_t launch_draws_to_symbols(const uint8_t *al, const int32_t *sym, int32_t *hap, int slots, int L, int D, int W,
                                   hipStream_t st) {
  if (slots <= 0) return hipSuccess;
  const int gy = (L + 63) / 64, gz = (D + 63) / 64;
  if (!al || !sym || !hap || L < 1 || D < 1 || W < 1 || gy > 65535 || gz > 65535) return hipErrorInvalidValue;
  hipLaunchKernelGGL(draws_to_symbols, dim3(2u * (unsigned)slots, gy, gz), dim3(256), 0, st, al, sym, hap, L, D, W);
  return hipGetLastError();
}

// MAP phasing (hmc_map_phase): the haplotype pair of largest exact posterior
// and that posterior, by a max-product sweep over the records exact_fb sweeps
// with sums, and a traceback in the same launch.
// A pair's value is the product of its path's tpv, doubled if its two
// haplotypes differ anywhere (the draws' prob rule): a pair behind a
// homozygous prefix is two mirror paths of half each, and one state is reached
// by all-homozygous prefixes and by heterozygous ones (variable-order contexts
// forget history), so a state carries two values:
//   Vh[t]  the best product over paths to t whose haplotypes are equal so far,
//   Vd[t]  the best pair value (the 2 inside) over paths that differ already.
// Head record: homozygous state (Vh, Vd) = (tpv, 0), heterozygous (0, 2 tpv).
// Record j above it, state t with alleles (xa, xb), contributions r in record
// order, primes for record j - 1:
//   xa == xb   Vh = tpv max_r Vh'[pred r]    Vd = tpv max_r Vd'[pred r]
//   else       Vh = 0                        Vd = tpv max_r max(Vd'[pred r], 2 Vh'[pred r])
// One multiplication per state and label, after the maximum, so a power of two
// on a whole record changes no choice.  Vh sits where exact_fb keeps fwd, Vd
// where it keeps bwd: exact_fb has run forward-only over the group before (it
// lays out x_off, flags the underflow that sends an individual through the
// pruned records, and in extended range leaves the divisor xtot 2^-xtot_exp),
// and this sweep overwrites its slots.  EXT: every record's 2 F values are
// rescaled by the maximum over both labels (rescale_record; an entry more than
// 2^1021 below the maximum loses bits — a path that far behind), the
// cumulative exponent in the record's first spare word.  Regular range: raw
// doubles; a best path is far less probable than the genotype, so on a long
// panel its product leaves the doubles where P(genotype) is still normal — an
// individual whose raw sweep meets a value below DBL_MIN is swept again at
// once with rescaled records (the same choices wherever the raw values kept
// their bits, by the line above), instead of being given up.  For the same
// reason the traced product is kept as mantissa and power-of-two count in
// both ranges: the same bits as the raw product wherever that stays normal.
// No back-pointers: wave 0 re-derives each choice from the stored values.
//   Final record: candidates (t, label) with index 2 t + label (h = 0, d = 1);
//   the largest value, among equals the lowest index — a rule, so that neither
//   the block size nor the reduction order enters.
//   Going down from state t with label l: the contributions in record order,
//   the first that attains the maximum of the sweep; l = h reads Vh', l = d at
//   xa == xb reads Vd', l = d at xa != xb reads per contribution Vd' and then
//   2 Vh' (taking the latter switches the label to h).  The lanes of wave 0
//   take the candidates 64 at a time under the same (value, lowest index) rule.
// Haplotypes and prob exactly as exact_posterior_draws spells and multiplies
// them, in DrawArgs' byte layout with one draw per individual.

// The sweep of one individual (every thread of the block).  SCALE: every
// record's 2 F values rescaled by the maximum over both labels, the cumulative
// exponent in the record's first spare word.  Otherwise raw doubles, and *flag
// is raised when a value that should be positive comes out below DBL_MIN: it
// has lost bits or all of them, and a comparison above it could go wrong.
// Ends on a barrier.
template <bool SCALE>
__device__ inline void map_sweep(const ExactArgs &a, const unsigned long long *roff, const unsigned long long *xo, int *flag) {
  const int tid = threadIdx.x, NT = blockDim.x;
  const int L = a.L, hl = a.head_len;
  int ex = 0, Fp = 0;  // SCALE: the cumulative exponent (block-uniform); the states of the record below
  {
    const RecView R(a.rec + roff[hl], true);
    double *vh = (double *)(a.x + xo[hl]), *vd = vh + R.F;
    double m = 0.0;
    for (int t = tid; t < R.F; t += NT) {
      const bool homo = (R.hdr[t] >> 24) & 1u;
      const double tpv = R.tpv[t];
      vh[t] = homo ? tpv : 0.0;
      vd[t] = homo ? 0.0 : tpv * 2.0;
      if constexpr (SCALE) m = fmax(m, homo ? tpv : tpv * 2.0);
    }
    if constexpr (SCALE) {
      ex += rescale_record(vh, 2 * R.F, m);
      if (tid == 0) ((int32_t *)(vh + 2 * (size_t)R.F))[0] = ex;
    } else {
      __syncthreads();
    }
    Fp = R.F;
  }
  for (int j = hl + 1; j <= L; ++j) {
    const RecView R(a.rec + roff[j], false);
    const double *ph = (const double *)(a.x + xo[j - 1]), *pd = ph + Fp;
    double *vh = (double *)(a.x + xo[j]), *vd = vh + R.F;
    double m = 0.0;
    for (int t = tid; t < R.F; t += NT) {
      const uint32_t hd = R.hdr[t];
      const bool homo = (hd & 0xFFu) == ((hd >> 8) & 0xFFu);
      double mh = 0.0, md = 0.0;
      for (uint32_t r = R.cb[t]; r < R.cb[t + 1]; ++r) {
        const uint32_t p = cw_state(R.ct[r]);
        const double h = ph[p], d = pd[p];
        if (homo) {
          mh = fmax(mh, h);
          md = fmax(md, d);
        } else {
          md = fmax(md, fmax(d, 2.0 * h));
        }
      }
      const double tpv = R.tpv[t];
      const double h = homo ? tpv * mh : 0.0, d = tpv * md;
      vh[t] = h;
      vd[t] = d;
      if constexpr (SCALE) m = fmax(m, fmax(h, d));
      else if ((mh > 0.0 && homo && h < SITE_PG_MIN) || (md > 0.0 && d < SITE_PG_MIN)) *flag = 1;
    }
    if constexpr (SCALE) {
      ex += rescale_record(vh, 2 * R.F, m);
      if (tid == 0) ((int32_t *)(vh + 2 * (size_t)R.F))[0] = ex;
    } else {
      __syncthreads();
    }
    Fp = R.F;
  }
}

// The traceback of a max sweep by wave 0 (wave-uniform), from candidate bkey = 2 t
// + label of the final record down to the head state, spelled into sp.  No
// back-pointers: each choice is re-derived from the stored values — the
// contributions in record order, 64 at a time, the first that attains the
// maximum under wave_best's (value, lowest index) rule; an earlier batch wins a
// tie.  GIVEN: the records' kinds choose what a contribution offers (the table
// above exact_map_phase_given); else every record is plain: modes 2 and 3.
// Returns false if a state no path reaches was met (never chosen; if one were,
// the individual counts as unresolved).
template <bool GIVEN, bool EXT>
__device__ inline bool max_traceback(const ExactArgs &a, const QueryInd<EXT> &ind, unsigned bkey, PathSpeller<true> &sp) {
  const int lane = threadIdx.x & (WAVE - 1);
  const int L = a.L, hl = a.head_len;
  int t = (int)(bkey >> 1);
  unsigned lab = bkey & 1u;  // plain record: h = 0, d = 1; span record: c
  for (int j = L; j > hl; --j) {
    const RecView R = ind.rec(j);
    const uint32_t hd = R.hdr[t], xa = hd & 0xFFu, xb = (hd >> 8) & 0xFFu;
    const uint32_t r0 = R.cb[t], r1 = R.cb[t + 1];
    const double *p0 = ind.fwd(j - 1), *p1 = p0 + ind.F(j - 1);
    const int kj = GIVEN ? ind.spare(j)[1] : 0;
    const bool cont = kj & 2, labels = kj & 1, below = GIVEN && (ind.spare(j - 1)[1] & 1);
    sp.enter(R, j, t);
    // 0 inside; 1 over a span record; 2 Vd' then 2 Vh'; 3 the label's own value
    const int mode = cont ? 0 : below ? 1 : (labels || (lab == 1u && xa != xb)) ? 2 : 3;
    double cv = -1.0;
    unsigned ck = 0xFFFFFFFFu, cw = 0u;
    for (uint32_t rb = r0; rb < r1; rb += WAVE) {
      const uint32_t r = rb + (uint32_t)lane;
      double v = -1.0;
      unsigned k = 0xFFFFFFFFu;
      uint32_t w = 0u;
      if (r < r1) {
        w = R.ct[r];
        const uint32_t ps = cw_state(w);
        k = 2u * (unsigned)lane;
        if (mode == 0) {
          v = (lab ^ (cw_rev(w) ? 1u : 0u)) ? p1[ps] : p0[ps];
        } else if (mode == 1) {
          if (!labels && lab == 0u) {
            v = 0.0;  // (Vh is 0 above a span: never chosen)
          } else {
            const double d0 = p0[ps], d1 = p1[ps];
            v = d0;
            if (d1 > d0) {
              v = d1;
              k += 1u;
            }
          }
        } else if (mode == 2) {
          const double d = p1[ps], h2 = 2.0 * p0[ps];
          v = d;
          if (h2 > d) {
            v = h2;
            k += 1u;
          }
        } else {
          v = lab ? p1[ps] : p0[ps];
        }
      }
      wave_best(v, k);
      if (v > cv) {
        cv = v;
        ck = k;
        cw = __shfl(w, (int)(k >> 1));
      }
    }
    if (!(cv > 0.0)) return false;
    if (mode == 0) lab ^= cw_rev(cw) ? 1u : 0u;
    else if (mode == 1) lab = ck & 1u;
    else if (mode == 2) lab = (ck & 1u) ? 0u : 1u;
    sp.follow(cw);
    t = (int)cw_state(cw);
  }
  sp.head(a, ind.rec(hl), t);
  return true;
}

template <bool EXT>
__global__ __launch_bounds__(256) void exact_map_phase(ExactArgs a, MapArgs s) {
  __shared__ int flag;
  const int tid = threadIdx.x, lane = tid & (WAVE - 1), wave = tid / WAVE;
  const int L = a.L;
  for (int q = blockIdx.x; q < a.n_order; q += gridDim.x) {  // block-uniform
    const QueryInd<EXT> ind(a, q);
    if (const int gu = ind.give_up_status()) {  // the host writes the input genotype
      if (tid == 0) s.status[q] = gu;
      continue;
    }
    // the sweep: raw doubles in the regular range, and again with rescaled records if those underflow
    if constexpr (EXT) {
      map_sweep<true>(a, ind.roff, ind.xo, &flag);
    } else {
      if (tid == 0) flag = 0;  // (every thread has read the previous individual's flag before the barrier of its final reduction)
      __syncthreads();
      map_sweep<false>(a, ind.roff, ind.xo, &flag);
      if (flag != 0) map_sweep<true>(a, ind.roff, ind.xo, &flag);  // block-uniform: read behind the sweep's last barrier
    }
    double best;
    unsigned bkey;
    block_best_candidate(ind.fwd(L), ind.F(L), best, bkey);
    if (wave != 0) continue;  // (wave 0 passes the next individual's barriers after its traceback)
    if (!(best > 0.0)) {      // (no path with a positive product: the host writes the input genotype)
      if (lane == 0) s.status[q] = 1;
      continue;
    }
    PathSpeller<true> sp(s.al, q, L, 1, 0, s.al && lane == 0);
    const bool ok = max_traceback<false>(a, ind, bkey, sp);
    if (lane == 0) {
      if (!ok) s.status[q] = 1;
      if (s.prob) s.prob[q] = ok ? sp.prob(ind.pg, ind.pge) : 0.0;
    }
  }
}

hipError_t launch_exact_map_phase(const ExactArgs &a, const MapArgs &s, int grid, hipStream_t st, int block) {
  if (a.n_order <= 0) return hipSuccess;
  if (grid < 1 || !s.status || block < WAVE || block > 256 || block % WAVE) return hipErrorInvalidValue;
  if (a.extended) hipLaunchKernelGGL(exact_map_phase<true>, dim3(grid), dim3(block), 0, st, a, s);
  else hipLaunchKernelGGL(exact_map_phase<false>, dim3(grid), dim3(block), 0, st, a, s);
  return hipGetLastError();
}

// MAP phasing given phase sets (hmc_map_phase_given): exact_map_phase over the
// pairs consistent with the individual's evidence, and P(evidence | genotype).
// The host plan (evidence_plan.hpp) gives the constrained loci ascending, each
// with the allele index on its set's first haplotype, a set's first locus
// marked as anchor and its last as last; sets do not overlap.  The record of
// locus k is k + 1, or head_len for k < head_len.
// A set needs an orientation label c: its first haplotype lies on the state's
// a side (c = 0) or b side (c = 1); a predecessor's label c arrives as
// c ^ rev(r) (exact_haplotype_dosages' rule).  Every path through a set's first
// locus is heterozygous from there on, so inside a span Vh is 0, and outside
// any span there is no label: two values per state still hold everything.
//   span record (from the record of a set's first locus to that of its last,
//   when these differ): (V[0], V[1]) by label;
//   plain record: (Vh, Vd) as map_sweep.
// Max sweep, record j above the head, state t with alleles (xa, xb) of locus
// j - 1, primes for the record below:
//   anchor   m = max_r max(Vd'[p], 2 Vh'[p]) over a plain record below, max_r
//            max(V'[0][p], V'[1][p]) over a span record below (adjacent sets);
//            V[0] = tpv m if xa is the first allele, V[1] = tpv m if xb is, the
//            other label 0;
//   inside   V[c] = tpv max_r V'[c ^ rev(r)][p]; at a locus of the set a label
//            whose side does not carry the first allele is stored as 0, at any
//            other locus both labels pass;
//   plain    map_sweep's recurrence; over a span record below it reads Vd' =
//            max(V'[0], V'[1]) and Vh' = 0.
// Head record: the constrained loci below head_len are matched from the states'
// two head patterns (head_len = 1: from the state's alleles); a state that
// fails a set wholly inside the head is 0, and when a set continues above the
// head the head record is a span record with the state's value under the
// label(s) that match.  Scaling and the regular range's second, rescaled sweep
// as exact_map_phase.
// Sum sweep: the same with ordered sums in place of maxima (contributions in
// record order, the first assigns; two labels of one predecessor as V'[0] +
// V'[1]) and one value per plain state, every record rescaled in both ranges.
// The final record summed in state order from 0.0 (a span record: V[0][t] +
// V[1][t] per state) is P(evidence and genotype): a heterozygous pair behind a
// homozygous prefix is two mirror paths of half each, and both pass or both
// fail every set, since a set constrains relative orientation only.  Divided by
// the range's P(genotype) it is `evidence`; a sum of exactly 0 is status 3 and
// no max sweep runs.
// The sweeps leave each record's kind in its second spare word (bit 0: span
// record, bit 1: inside, i.e. reads label by label) for the traceback, which is
// exact_map_phase's: candidates of the final record by index 2 t + label (h = 0,
// d = 1; on a span record the label is c), largest value, lowest index.  Going
// down from state t with label l, contributions in record order, the first that
// attains the maximum, 64 at a time under (value, lowest index):
//   inside                  V'[l ^ rev(r)], the label becomes l ^ rev(r);
//   over a span record      V'[0] and then V'[1] per contribution (index 2
//   (anchor or plain d)     lane + c), the label becomes that c;
//   anchor over plain, and  Vd' and then 2 Vh' per contribution, the label
//   plain d at xa != xb     becomes d or h;
//   otherwise               Vh' for h, Vd' for d.
// A label stored as 0 is never chosen: only positive values are.
template <bool SUM, bool SCALE>
__device__ inline int given_sweep(const ExactArgs &a, const unsigned long long *roff, const unsigned long long *xo,
                                  const GivenEvent *ev, int ne, int *flag, bool &top_labels) {
  const int tid = threadIdx.x, NT = blockDim.x;
  const int L = a.L, hl = a.head_len;
  int ex = 0, Fp = 0, ec = 0;        // the cumulative exponent; the states of the record below; the next event
  bool open = false, below = false;  // a set continues above this record; the record below is a span record (block-uniform)
  {
    const RecView R(a.rec + roff[hl], true);
    double *v0 = (double *)(a.x + xo[hl]), *v1 = v0 + R.F;
    while (ec < ne && ev[ec].locus < hl) ++ec;  // the head's events: [0, ec)
    const int nh = ec;
    open = nh > 0 && !(ev[nh - 1].code & GIVEN_EV_LAST);
    double m = 0.0;
    for (int t = tid; t < R.F; t += NT) {
      const uint32_t hd = R.hdr[t];
      const bool homo = (hd >> 24) & 1u;
      bool ok = true, c0 = true, c1 = true;
      for (int e = 0; e < nh; ++e) {
        const int k = ev[e].locus, code = ev[e].code;
        const uint32_t first = (uint32_t)(code >> 8);
        uint32_t xa, xb;
        state_alleles(a, R, hl > 1, k, t, xa, xb);
        if (code & GIVEN_EV_ANCHOR) c0 = c1 = true;
        c0 = c0 && xa == first;
        c1 = c1 && xb == first;
        if (code & GIVEN_EV_LAST) ok = ok && (c0 || c1);
      }
      const double tpv = R.tpv[t], val = homo ? tpv : tpv * 2.0;
      double o0, o1;
      if (open) {
        o0 = ok && c0 ? val : 0.0;
        o1 = ok && c1 ? val : 0.0;
      } else if (SUM) {
        o0 = ok ? val : 0.0;
        o1 = 0.0;
      } else {
        o0 = ok && homo ? val : 0.0;
        o1 = ok && !homo ? val : 0.0;
      }
      v0[t] = o0;
      v1[t] = o1;
      if constexpr (SCALE) m = fmax(m, fmax(o0, o1));
    }
    if constexpr (SCALE) ex += rescale_record(v0, 2 * R.F, m);
    else __syncthreads();
    if (tid == 0) {
      int32_t *sp = (int32_t *)(v0 + 2 * (size_t)R.F);
      sp[0] = ex;
      sp[1] = open ? 1 : 0;
    }
    Fp = R.F;
    below = open;
  }
  for (int j = hl + 1; j <= L; ++j) {
    const RecView R(a.rec + roff[j], false);
    const double *p0 = (const double *)(a.x + xo[j - 1]), *p1 = p0 + Fp;
    double *v0 = (double *)(a.x + xo[j]), *v1 = v0 + R.F;
    const bool has = ec < ne && ev[ec].locus == j - 1;
    const int code = has ? ev[ec].code : 0;
    const uint32_t first = (uint32_t)(code >> 8);
    const bool cont = open, labels = open || (code & GIVEN_EV_ANCHOR);
    double m = 0.0;
    for (int t = tid; t < R.F; t += NT) {
      const uint32_t hd = R.hdr[t], xa = hd & 0xFFu, xb = (hd >> 8) & 0xFFu;
      const uint32_t r0 = R.cb[t], r1 = R.cb[t + 1];
      double a0 = 0.0, a1 = 0.0;
      if (cont) {  // label by label
        for (uint32_t r = r0; r < r1; ++r) {
          const uint32_t w = R.ct[r], p = cw_state(w);
          const bool rv = cw_rev(w);
          const double s0 = rv ? p1[p] : p0[p], s1 = rv ? p0[p] : p1[p];
          if constexpr (SUM) {
            a0 = r == r0 ? s0 : a0 + s0;
            a1 = r == r0 ? s1 : a1 + s1;
          } else {
            a0 = fmax(a0, s0);
            a1 = fmax(a1, s1);
          }
        }
      } else if (labels || SUM) {  // one value per predecessor: an anchor, or a plain record of the sum sweep
        for (uint32_t r = r0; r < r1; ++r) {
          const uint32_t p = cw_state(R.ct[r]);
          if constexpr (SUM) {
            const double sv = below ? p0[p] + p1[p] : p0[p];
            a0 = r == r0 ? sv : a0 + sv;
          } else {
            a0 = fmax(a0, below ? fmax(p0[p], p1[p]) : fmax(p1[p], 2.0 * p0[p]));
          }
        }
        a1 = a0;
      } else {  // a plain record of the max sweep: map_sweep's recurrence
        const bool homo = xa == xb;
        for (uint32_t r = r0; r < r1; ++r) {
          const uint32_t p = cw_state(R.ct[r]);
          const double h = below ? 0.0 : p0[p], d = below ? fmax(p0[p], p1[p]) : p1[p];
          if (homo) {
            a0 = fmax(a0, h);
            a1 = fmax(a1, d);
          } else {
            a1 = fmax(a1, fmax(d, 2.0 * h));
          }
        }
      }
      const double tpv = R.tpv[t];
      const bool ok0 = labels ? !has || xa == first : true, ok1 = labels ? !has || xb == first : !SUM;
      const double o0 = ok0 ? tpv * a0 : 0.0, o1 = ok1 ? tpv * a1 : 0.0;
      v0[t] = o0;
      v1[t] = o1;
      if constexpr (SCALE) m = fmax(m, fmax(o0, o1));
      else if ((ok0 && a0 > 0.0 && o0 < SITE_PG_MIN) || (ok1 && a1 > 0.0 && o1 < SITE_PG_MIN)) *flag = 1;
    }
    if constexpr (SCALE) ex += rescale_record(v0, 2 * R.F, m);
    else __syncthreads();
    if (tid == 0) {
      int32_t *sp = (int32_t *)(v0 + 2 * (size_t)R.F);
      sp[0] = ex;
      sp[1] = (labels ? 1 : 0) | (cont ? 2 : 0);
    }
    Fp = R.F;
    below = labels;
    open = labels && !(code & GIVEN_EV_LAST);
    if (has) ++ec;
  }
  top_labels = below;
  return ex;
}

template <bool EXT>
__global__ __launch_bounds__(256) void exact_map_phase_given(ExactArgs a, GivenArgs s) {
  __shared__ int flag;
  __shared__ double s_tot;
  const int tid = threadIdx.x, lane = tid & (WAVE - 1), wave = tid / WAVE;
  const int L = a.L;
  for (int q = blockIdx.x; q < a.n_order; q += gridDim.x) {  // block-uniform
    const QueryInd<EXT> ind(a, q);
    if (const int gu = ind.give_up_status()) {  // as exact_map_phase
      if (tid == 0) s.status[q] = gu;
      continue;
    }
    const GivenEvent *ev = s.ev + s.ev_off[ind.bi];
    const int ne = (int)(s.ev_off[ind.bi + 1] - s.ev_off[ind.bi]);
    // the sums: P(evidence and genotype) = tot 2^-es
    bool top = false;
    const int es = given_sweep<true, true>(a, ind.roff, ind.xo, ev, ne, &flag, top);
    if (tid == 0) {  // in state order from 0.0, as exact_fb sums its divisor
      const int F = ind.F(L);
      const double *v = ind.fwd(L);
      double tot = 0.0;
      for (int t = 0; t < F; ++t) tot += top ? v[t] + v[F + t] : v[t];
      s_tot = tot;
    }
    __syncthreads();
    const double tot = s_tot;  // (written again behind the next sweep's barriers only)
    if (!(tot > 0.0)) {        // no consistent path: the host writes the input genotype
      if (tid == 0) s.status[q] = 3;
      continue;
    }
    // the maxima: raw doubles in the regular range, and again with rescaled records if those underflow
    if constexpr (EXT) {
      given_sweep<false, true>(a, ind.roff, ind.xo, ev, ne, &flag, top);
    } else {
      if (tid == 0) flag = 0;
      __syncthreads();
      given_sweep<false, false>(a, ind.roff, ind.xo, ev, ne, &flag, top);
      if (flag != 0) given_sweep<false, true>(a, ind.roff, ind.xo, ev, ne, &flag, top);  // block-uniform: read behind the sweep's last barrier
    }
    double best;
    unsigned bkey;
    block_best_candidate(ind.fwd(L), ind.F(L), best, bkey);
    if (wave != 0) continue;  // (wave 0 passes the next individual's barriers after its traceback)
    if (!(best > 0.0)) {      // (the sums found a path, so the maxima do)
      if (lane == 0) s.status[q] = 1;
      continue;
    }
    PathSpeller<true> sp(s.al, q, L, 1, 0, s.al && lane == 0);
    const bool ok = max_traceback<true>(a, ind, bkey, sp);
    if (lane == 0) {
      if (!ok) s.status[q] = 1;
      if (s.prob) s.prob[q] = ok ? sp.prob(ind.pg, ind.pge) : 0.0;
      if (s.evidence) {
        int ge;
        const double gm = frexp(ind.pg, &ge);
        s.evidence[q] = ok ? ldexp(tot / gm, -es - ind.pge - ge) : 0.0;
      }
    }
  }
}

hipError_t launch_exact_map_phase_given(const ExactArgs &a, const GivenArgs &s, int grid, hipStream_t st, int block) {
  if (a.n_order <= 0) return hipSuccess;
  if (grid < 1 || !s.status || !s.ev_off || !s.ev || block < WAVE || block > 256 || block % WAVE) return hipErrorInvalidValue;
  if (a.extended) hipLaunchKernelGGL(exact_map_phase_given<true>, dim3(grid), dim3(block), 0, st, a, s);
  else hipLaunchKernelGGL(exact_map_phase_given<false>, dim3(grid), dim3(block), 0, st, a, s);
  return hipGetLastError();
}

// Ranked phasings (hmc_ranked_phasings): the k haplotype pairs of largest
// exact posterior, each once, with its posterior — exact_map_phase from
// max-product to list max-product.  State t of a record keeps two descending
// lists of at most KL values, Lh[t] (haplotypes equal so far) and Ld[t]
// (already different, the pair factor 2 inside); empty slots are 0.
//   Head record: homozygous state Lh = (tpv), Ld = (); heterozygous Lh = (),
//   Ld = (tpv * 2.0).
//   Record j above it, state t with alleles (xa, xb), contributions r in
//   record order, p = pred(r), primes for record j - 1; the candidates are
//     xa == xb   Lh[t]: (Lh'[p][q], key (r, q));  Ld[t]: (Ld'[p][q], key (r, q))
//     else       Lh[t] empty;  Ld[t]: (Ld'[p][q], key (r, 0, q)) and
//                (2.0 * Lh'[p][q], key (r, 1, q)) — the latter unless an
//                earlier contribution of t names the same predecessor p.
//   A heterozygous pair behind a homozygous prefix is two mirror paths of half
//   each (rev or not out of the state both haplotypes share); paths whose
//   haplotypes are equal so far share their contexts, so the two mirrors are
//   the two contributions of t from one predecessor, and the 2 h candidates of
//   the second would list every such pair twice.  (Ld' is read from both: once
//   the haplotypes differ the two orientations are two pairs.)
//   Candidates by value descending, then key ascending; the first KL with a
//   value > 0 are kept and then multiplied by tpv[t], one multiplication each.
//   The candidates arrive in key order and a predecessor's list is sorted, so
//   a list is left at its first entry that cannot enter (not above the running
//   KL-th value: an equal value with a later key loses).
// Every record is rescaled (rescale_record over its 2 F KL values); its
// largest value is a rank-0 entry, which is exact_map_phase's maximum, so the
// exponents and the rank-0 values are those of its rescaled sweep.
// The list store, of this call alone (the forward pass's x-store holds 2 F
// doubles per record): per individual from RankArgs::store_base, record j at
// 24 KL (states of the records below) + 8 (j - head_len) bytes — values
// [F][2][KL] doubles, back-pointers [F][2][KL] words (contribution offset in
// the state's range << 5 | source label d << 4 | source rank), the cumulative
// exponent and a pad word.  The states below a record come from the forward
// pass's x_off, which counts 4 F + 2 words per record.
//   Final record: candidates (t, label, q), key (2 t + label, q), the same
//   order; the first k are the rows — one block reduction per row, each taking
//   the first candidate behind the previous row's.
//   Traceback: lane r of wave 0 follows row r down its back-pointers; spelling
//   and prob exactly as exact_map_phase.  Neither the block size nor KL enters.
template <int KL>
__device__ inline void rank_insert(double (&v)[KL], uint32_t (&b)[KL], double x, uint32_t xb) {  // x > v[KL - 1]
#pragma unroll
  for (int i = KL - 1; i >= 0; --i) {
    if (v[i] < x) {  // entry i moves down; x lands here if the entry above stays
      const bool shift = i > 0 && v[i > 0 ? i - 1 : 0] < x;
      v[i] = shift ? v[i > 0 ? i - 1 : 0] : x;
      b[i] = shift ? b[i > 0 ? i - 1 : 0] : xb;
    }
  }
}

// the candidates of one predecessor list, x = scale * pv[q], into the running list
template <int KL>
__device__ inline void rank_take(double (&v)[KL], uint32_t (&b)[KL], const double *pv, double scale, uint32_t code) {
  for (int q = 0; q < KL; ++q) {
    const double x = scale * pv[q];
    if (!(x > v[KL - 1])) break;
    rank_insert<KL>(v, b, x, code | (uint32_t)q);
  }
}

__device__ inline size_t rank_rec_offset(const unsigned long long *xo, int hl, int j, int KL) {  // bytes from the individual's base
  const unsigned long long below = (xo[j] - xo[hl] - 2ull * (unsigned)(j - hl)) / 4ull;  // states of records hl .. j - 1
  return (size_t)24 * KL * below + (size_t)8 * (j - hl);
}

template <int KL, bool EXT>
__global__ __launch_bounds__(256) void exact_ranked_phasings(ExactArgs a, RankArgs s) {
  __shared__ double bv[2][4];
  __shared__ unsigned bk[2][4];
  const int tid = threadIdx.x, NT = blockDim.x, lane = tid & (WAVE - 1), wave = tid / WAVE, nw = NT / WAVE;
  const int L = a.L, hl = a.head_len, K = s.k;
  for (int q = blockIdx.x; q < a.n_order; q += gridDim.x) {  // block-uniform
    const QueryInd<EXT> ind(a, q);
    if (const int gu = ind.give_up_status()) {  // the host writes the input genotype
      if (tid == 0) s.status[q] = gu;
      continue;
    }
    const unsigned long long *xo = ind.xo;
    uint8_t *base = s.store + s.store_base[q];
    // ---- the sweep -------------------------------------------------------
    int ex = 0;
    {
      const RecView R = ind.rec(hl);
      double *vals = (double *)(base + rank_rec_offset(xo, hl, hl, KL));
      double m = 0.0;
      for (int t = tid; t < R.F; t += NT) {
        const bool homo = (R.hdr[t] >> 24) & 1u;
        const double tpv = R.tpv[t];
        double *o = vals + (size_t)t * 2 * KL;
#pragma unroll
        for (int i = 0; i < 2 * KL; ++i) o[i] = 0.0;
        const double v = homo ? tpv : tpv * 2.0;
        o[homo ? 0 : KL] = v;
        m = fmax(m, v);
      }
      ex += rescale_record(vals, 2 * R.F * KL, m);
      if (tid == 0) ((int32_t *)(vals + (size_t)3 * R.F * KL))[0] = ex;
    }
    for (int j = hl + 1; j <= L; ++j) {
      const RecView R = ind.rec(j);
      const double *pvals = (const double *)(base + rank_rec_offset(xo, hl, j - 1, KL));
      double *vals = (double *)(base + rank_rec_offset(xo, hl, j, KL));
      uint32_t *bps = (uint32_t *)(vals + (size_t)2 * R.F * KL);
      double m = 0.0;
      for (int t = tid; t < R.F; t += NT) {
        const uint32_t hd = R.hdr[t];
        const bool homo = (hd & 0xFFu) == ((hd >> 8) & 0xFFu);
        double lh[KL], ld[KL];
        uint32_t bh[KL], bd[KL];
#pragma unroll
        for (int i = 0; i < KL; ++i) {
          lh[i] = ld[i] = 0.0;
          bh[i] = bd[i] = 0u;
        }
        const uint32_t r0 = R.cb[t], r1 = R.cb[t + 1];
        for (uint32_t r = r0; r < r1; ++r) {
          const uint32_t p = cw_state(R.ct[r]);
          const double *pv = pvals + (size_t)p * 2 * KL;
          const uint32_t code = (r - r0) << 5;
          if (homo) {
            rank_take<KL>(lh, bh, pv, 1.0, code);
            rank_take<KL>(ld, bd, pv + KL, 1.0, code | 16u);
          } else {
            rank_take<KL>(ld, bd, pv + KL, 1.0, code | 16u);
            if (2.0 * pv[0] > ld[KL - 1]) {  // (h values are rare: only states whose two contexts are one)
              bool mirror = false;
              for (uint32_t e = r0; e < r; ++e) mirror |= cw_state(R.ct[e]) == p;
              if (!mirror) rank_take<KL>(ld, bd, pv, 2.0, code);
            }
          }
        }
        const double tpv = R.tpv[t];
        double *o = vals + (size_t)t * 2 * KL;
        uint32_t *ob = bps + (size_t)t * 2 * KL;
#pragma unroll
        for (int i = 0; i < KL; ++i) {
          o[i] = homo ? tpv * lh[i] : 0.0;
          o[KL + i] = tpv * ld[i];
          ob[i] = bh[i];
          ob[KL + i] = bd[i];
        }
        m = fmax(m, fmax(homo ? tpv * lh[0] : 0.0, tpv * ld[0]));
      }
      ex += rescale_record(vals, 2 * R.F * KL, m);
      if (tid == 0) ((int32_t *)(vals + (size_t)3 * R.F * KL))[0] = ex;
    }
    // ---- the final record's first K candidates: row r in lane r of every wave
    const int FL = ind.F(L);
    const double *vL = (const double *)(base + rank_rec_offset(xo, hl, L, KL));
    double pv = 0.0;
    unsigned pk = 0u, rowk = 0u;
    int cnt = 0;
    for (int r = 0; r < K; ++r) {  // block-uniform
      double best = -1.0;
      unsigned bkey = 0xFFFFFFFFu;
      for (int t = tid; t < FL; t += NT) {  // keys ascending: strictly larger only
        for (int lab = 0; lab < 2; ++lab) {
          const double *l = vL + ((size_t)t * 2 + lab) * KL;
          for (int i = 0; i < KL; ++i) {
            const double v = l[i];
            if (!(v > 0.0)) break;
            const unsigned key = (2u * (unsigned)t + (unsigned)lab) * KL + (unsigned)i;
            if (r == 0 || v < pv || (v == pv && key > pk)) {  // the list's first entry behind the previous row
              if (v > best) {
                best = v;
                bkey = key;
              }
              break;
            }
          }
        }
      }
      wave_best(best, bkey);
      if (lane == 0) {
        bv[r & 1][wave] = best;
        bk[r & 1][wave] = bkey;
      }
      __syncthreads();  // (the other buffer is rewritten only behind the next row's barrier)
      best = bv[r & 1][0];
      bkey = bk[r & 1][0];
      for (int w = 1; w < nw; ++w)
        if (bv[r & 1][w] > best || (bv[r & 1][w] == best && bk[r & 1][w] < bkey)) {
          best = bv[r & 1][w];
          bkey = bk[r & 1][w];
        }
      if (!(best > 0.0)) break;
      pv = best;
      pk = bkey;
      if (lane == r) rowk = bkey;
      ++cnt;
    }
    if (wave != 0) continue;  // (wave 0 passes the next individual's barriers after its tracebacks)
    if (lane == 0) {
      if (s.count) s.count[q] = cnt;
      if (cnt == 0) s.status[q] = 1;  // (no path with a positive product: the host writes the input genotype)
    }
    const bool mine = lane < cnt;  // ---- traceback of row `lane` (no divergent way to the next individual's barriers)
    PathSpeller<true> sp(s.al, q, L, K, lane, s.al != nullptr);
    int t = (int)(rowk / (2u * KL));
    uint32_t lab = (rowk / KL) & 1u, rk = rowk % KL;
    bool dead = false;
    for (int j = L; mine && j > hl; --j) {
      const RecView R = ind.rec(j);
      const uint32_t r0 = R.cb[t], r1 = R.cb[t + 1];
      sp.enter(R, j, t);
      const uint32_t *bps = (const uint32_t *)(base + rank_rec_offset(xo, hl, j, KL) + (size_t)16 * R.F * KL);
      const uint32_t bp = bps[((size_t)t * 2 + lab) * KL + rk];
      const uint32_t r = r0 + (bp >> 5);
      if (r >= r1 || (bp & 15u) >= (uint32_t)KL) {  // (never: an entry with a positive value has a contribution behind it)
        dead = true;
        break;
      }
      const uint32_t w = R.ct[r];
      lab = (bp >> 4) & 1u;
      rk = bp & 15u;
      sp.follow(w);
      t = (int)cw_state(w);
    }
    if (mine && !dead) sp.head(a, ind.rec(hl), t);
    if (mine && s.prob) s.prob[(size_t)q * K + lane] = dead ? 0.0 : sp.prob(ind.pg, ind.pge);
  }
}

// total states of the records of every individual of the group (what sizes its list store)
__global__ void exact_state_totals(ExactArgs a, unsigned long long *total) {
  const int q = blockIdx.x * blockDim.x + threadIdx.x;
  if (q >= a.n_order) return;
  const int bi = a.order[q], L = a.L, hl = a.head_len;
  if (!fb_laid_out(a.status[bi])) {  // (exact_fb laid out no x_off: the kernel leaves the individual at once)
    total[q] = 0;
    return;
  }
  const unsigned long long *xo = a.x_off + (size_t)bi * (L + 1);
  total[q] = (xo[L] - xo[hl] - 2ull * (unsigned)(L - hl)) / 4ull + a.rec[a.rec_off[(size_t)bi * (L + 1) + L]];
}

hipError_t launch_exact_state_totals(const ExactArgs &a, unsigned long long *total, hipStream_t st) {
  if (a.n_order <= 0) return hipSuccess;
  if (!total) return hipErrorInvalidValue;
  hipLaunchKernelGGL(exact_state_totals, dim3((a.n_order + 255) / 256), dim3(256), 0, st, a, total);
  return hipGetLastError();
}

template <int KL>
static hipError_t launch_ranked(const ExactArgs &a, const RankArgs &s, int grid, hipStream_t st, int block) {
  if (a.extended) hipLaunchKernelGGL((exact_ranked_phasings<KL, true>), dim3(grid), dim3(block), 0, st, a, s);
  else hipLaunchKernelGGL((exact_ranked_phasings<KL, false>), dim3(grid), dim3(block), 0, st, a, s);
  return hipGetLastError();
}

hipError_t launch_exact_ranked_phasings(const ExactArgs &a, const RankArgs &s, int kl, int grid, hipStream_t st, int block) {
  if (a.n_order <= 0) return hipSuccess;
  if (grid < 1 || !s.status || !s.store || !s.store_base || s.k < 1 || s.k > kl || block < WAVE || block > 256 || block % WAVE)
    return hipErrorInvalidValue;
  switch (kl) {
    case 2: return launch_ranked<2>(a, s, grid, st, block);
    case 4: return launch_ranked<4>(a, s, grid, st, block);
    case 8: return launch_ranked<8>(a, s, grid, st, block);
    case 16: return launch_ranked<16>(a, s, grid, st, block);
  }
  return hipErrorInvalidValue;  // a width that is not built is an error, never another kernel
}

// Window phasings (hmc_window_phasings): for every window of a call the
// distinct haplotype pairs the individual can carry over the window's loci,
// each with its posterior summed over everything outside the window, the k
// most probable in order.  The sum-product sibling of exact_ranked_phasings and
// the discovering sibling of exact_haplotype_dosages: one block per individual,
// one labelled forward sweep per window over the window's records only.  A
// state t carries one double per ordered configuration c — the a-side and
// b-side allele strings over the window's branching loci seen so far, as a
// mixed-radix code (window_plan.hpp) that grows by a digit at each branching
// locus, the first locus most significant.
//   anchor    at the record of the window's first locus (a head record of
//             head_len > 1 spells all of the window's head loci at once):
//             g[c][t] = fwd[t] for the one c state t spells, 0 for the others;
//   propagate record j from j - 1: c = (p, d), p the code so far and d the
//             digit of locus j - 1 (no d at a fixed locus); where d is the
//             digit t's own alleles spell, over t's contributions r in stored
//             order g'[c][t] += g[rev(r) ? swap(p) : p][state(r)] * tpv[t], the
//             first term assigns, later ones add; elsewhere 0.  swap, the code
//             with the two sides exchanged, comes from a table in LDS that is
//             rebuilt when the code grows;
//   evaluate  at the record of the window's last locus: S_c = sum_t g[c][t]
//             bwd[t], a wavefront per c in PowScale::label_sums' order;
//   select    the row of the unordered pair {x, y} is the orientation with the
//             smaller code (its a side is the smaller string); prob = (S_c +
//             S_swap(c)) / P(genotype), S_c / P(genotype) when c = swap(c).
//             Row c's rank is the number of rows that precede it — larger prob,
//             or equal prob and the smaller (a string, b string) — counted by
//             one thread per row, so nothing about the launch enters; ranks
//             below k are written.
// These are exact_haplotype_dosages' operations for the two-sided pattern the
// row spells: its g[0] is g[c], its g[1] is g[swap(c)], and the terms it adds
// beyond these are exact zeros.  So a row's prob is that call's double (half of
// it when the two strings are equal), and depends on the records, the forward
// and backward values and the window alone: NC, the other windows, k, block
// size, grid, grouping, shard and tier do not change the bits.  No
// floating-point atomics, no cross-wave sums beyond S_c + S_swap(c).
// A state's configurations lie an odd number of doubles (the window's C rounded
// up) apart from the next state's, so the lanes of an evaluating wavefront
// (consecutive states, one c) and of a propagating one (one state, consecutive
// c) both spread over the LDS banks.  The two frontiers of a window live in LDS
// when its largest record's fit there at that stride — always when the
// individual's largest record has at most `tier` states — else in the
// individual's slice of an HBM scratch: the same doubles in the same order.
// EXT (ExactArgs::extended): as exact_haplotype_dosages.
template <int NC, bool EXT>
__global__ __launch_bounds__(256) void exact_window_phasings(ExactArgs a, WindowArgs s) {
  extern __shared__ __attribute__((aligned(16))) double wn_lds[];  // 2 (NC + 1) lds_states doubles: a window's two frontiers
  constexpr int NCS = NC + 1;
  __shared__ double s_sum[NC], s_prob[NC];  // S_c; the rows' probs
  __shared__ uint16_t s_swp[NC], s_list[NC];  // swap of the codes so far; the rows of positive prob
  __shared__ WinDigit s_dig[WIN_DIGITS_MAX];
  __shared__ int s_n, s_f;  // rows of positive prob; the window's largest record
  const int tid = threadIdx.x, NT = blockDim.x, lane = tid & (WAVE - 1), wave = tid / WAVE, nw = NT / WAVE;
  const int L = a.L, hl = a.head_len, W = s.n_windows, K = s.k;
  for (int q = blockIdx.x; q < a.n_order; q += gridDim.x) {
    const QueryInd<EXT> ind(a, q);
    const int gu = ind.give_up_status();
    // (the individual's largest record against the tier; the windows place their own frontiers below)
    FrontierStore fr(a, ind.roff, ind.resolved(), wn_lds, min(s.tier, s.lds_states), s.lds_states, s.scratch, 0x7FFFFFFF, NCS);
    const unsigned long long sc0 = s.scratch ? s.scratch_off[q] : 0ull, sc1 = s.scratch ? s.scratch_off[q + 1] : 0ull;
    if (gu || !fr.fits) {  // no rows: the caller's zeros stand
      if (tid == 0) s.status[q] = fr.fits ? gu : 1;
      continue;
    }
    PowScale<EXT> ps(ind);
    for (int w = 0; w < W; ++w) {
      const WinItem it = s.item[(size_t)q * W + w];
      const int k0 = s.start[w], k1 = k0 + s.len[w];
      if (it.C < 1 || it.C > NC || it.nd < 0 || it.nd > WIN_DIGITS_MAX || k0 < 0 || k1 <= k0 || k1 > L) continue;  // over the cap
      __syncthreads();  // the previous window's last readers of the tables and the frontiers are done
      if (tid < it.nd) s_dig[tid] = s.dig[it.dig0 + tid];
      if (tid == 0) s_n = s_f = 0;
      __syncthreads();
      int j = k0 < hl ? hl : k0 + 1;               // the record `cur` belongs to
      const int jl = k1 - 1 < hl ? hl : k1;        // the record of the window's last locus
      const bool head = j == hl && hl > 1;         // the window's loci below head_len, from the head patterns
      const int ka = head ? min(k1, hl) : k0 + 1;  // the anchor spells the loci [k0, ka)
      int m = 0, cc = 1;                           // digits in the code so far, and its range (block-uniform)
      while (m < it.nd && s_dig[m].rel < ka - k0) cc *= win_radix(s_dig[m++]);
      if (cc > NC) continue;  // (the host builds none such)
      // The window's own stride and store: its C rounded up to an odd count of doubles per state, and LDS when
      // its largest record's two frontiers fit there at that stride, else the individual's slice of the scratch —
      // a narrow window of a wide individual neither strides nor spills like its widest one.
      const int ncs = (it.C + 1) | 1;
      for (int r = j + tid; r <= jl; r += NT) atomicMax(&s_f, ind.F(r));
      __syncthreads();
      const size_t fwin = (size_t)s_f, need = 2 * fwin * ncs;
      const bool in_lds = need <= (size_t)2 * NCS * s.lds_states;
      if (!in_lds && need > sc1 - sc0) continue;  // (none such: the host sizes the slice from the largest record and C)
      double *cur = in_lds ? wn_lds : s.scratch + sc0, *prev = cur + fwin * ncs;
      {
        const RecView R = ind.rec(j);
        const double *fw = ind.fwd(j);
        for (int t = tid; t < R.F; t += NT) {
          int code = 0;
          for (int i = 0; i < m && code >= 0; ++i) {
            uint32_t xa, xb;
            state_alleles(a, R, head, k0 + s_dig[i].rel, t, xa, xb);
            const int d = win_encode(s_dig[i], xa, xb);
            code = d < 0 ? -1 : code * win_radix(s_dig[i]) + d;
          }
          double *g = cur + (size_t)t * ncs;
          for (int c = 0; c < cc; ++c) g[c] = 0.0;
          if (code >= 0) g[code] = fw[t];
        }
      }
      for (int c = tid; c < cc; c += NT) s_swp[c] = (uint16_t)win_swap_code(s_dig, m, c);
      __syncthreads();
      while (j < jl) {  // record j + 1 from record j (j + 1 > head_len: never the head record)
        ++j;
        {
          double *x = prev;
          prev = cur;
          cur = x;
        }
        const RecView R = ind.rec(j);
        const int step = EXT ? ind.spare(j)[0] - ind.spare(j - 1)[0] : 0;
        const bool br = m < it.nd && s_dig[m].rel == j - 1 - k0;  // locus j - 1 branches: the code takes its digit
        const WinDigit dg = s_dig[br ? m : 0];
        const int rad = br ? win_radix(dg) : 1, cn = cc * rad;
        if (cn > NC) break;  // (none such)
        int sh = 0;  // items (t, p) by a power of two that holds the new range
        while ((1 << sh) < cn) ++sh;
        const int items = R.F << sh;
        for (int idx = tid; idx < items; idx += NT) {
          const int t = idx >> sh, p = idx & ((1 << sh) - 1);
          if (p >= cn) continue;
          int pp = p;
          bool on = true;
          if (br) {
            const uint32_t h = R.hdr[t];
            pp = p / rad;
            on = p - pp * rad == win_encode(dg, h & 0xFFu, (h >> 8) & 0xFFu);
          }
          double v = 0.0;
          if (on) {
            const double tpv = R.tpv[t];
            const int sp = s_swp[pp];
            const uint32_t r0 = R.cb[t], r1 = R.cb[t + 1];
            for (uint32_t r = r0; r < r1; ++r) {
              const uint32_t cw = R.ct[r];
              const double x = prev[(size_t)cw_state(cw) * ncs + (cw_rev(cw) ? sp : pp)] * tpv;
              v = r == r0 ? x : v + x;
            }
            if (EXT) v = ldexp(v, step);
          }
          cur[(size_t)t * ncs + p] = v;
        }
        __syncthreads();
        if (br) {
          ++m;
          cc = cn;
          for (int c = tid; c < cc; c += NT) s_swp[c] = (uint16_t)win_swap_code(s_dig, m, c);
          __syncthreads();
        }
      }
      if (j != jl || m != it.nd) continue;  // (none such)
      {
        const RecView R = ind.rec(j);
        const double *bw = ind.bwd(j);
        ps.at_record(ind, ind.spare(j));
        for (int c = wave; c < cc; c += nw) {  // wave-uniform
          const double v = ps.ordered_sum(R.F, bw, [&](int t) { return cur[(size_t)t * ncs + c]; });
          if (lane == 0) s_sum[c] = v;
        }
      }
      __syncthreads();
      for (int c = tid; c < cc; c += NT) {
        const int sc = s_swp[c];
        if (c > sc) continue;  // the other orientation spells the row
        const double pr = c == sc ? s_sum[c] / ps.pgs : (s_sum[c] + s_sum[sc]) / ps.pgs;
        s_prob[c] = pr;
        if (pr > 0.0) s_list[atomicAdd(&s_n, 1)] = (uint16_t)c;  // (the list's order does not enter a rank)
      }
      __syncthreads();
      const int n = s_n;
      const size_t base = (size_t)q * W + w;
      for (int i = tid; i < n; i += NT) {
        const int c = s_list[i];
        const double pc = s_prob[c];
        int rank = 0;
        for (int u = 0; u < n; ++u) {
          const int d = s_list[u];
          const double pd = s_prob[d];
          if (pd > pc || (pd == pc && d != c && win_order_less(s_dig, m, d, c))) ++rank;
        }
        if (rank < K) {
          s.code[base * K + rank] = c;
          s.prob[base * K + rank] = pc;
        }
      }
      if (tid == 0) {
        s.count[base] = min(n, K);
        s.n_config[base] = n;
      }
    }
  }
}

template <int NC>
static hipError_t launch_window(const ExactArgs &a, const WindowArgs &s, int grid, hipStream_t st, int block) {
  const size_t lds = (size_t)s.lds_states * 16 * (NC + 1);
  if (a.extended) hipLaunchKernelGGL((exact_window_phasings<NC, true>), dim3(grid), dim3(block), lds, st, a, s);
  else hipLaunchKernelGGL((exact_window_phasings<NC, false>), dim3(grid), dim3(block), lds, st, a, s);
  return hipGetLastError();
}

hipError_t launch_exact_window_phasings(const ExactArgs &a, const WindowArgs &s, int nc, int grid, hipStream_t st, int block) {
  if (a.n_order <= 0 || s.n_windows <= 0) return hipSuccess;
  if (block < WAVE || block > 256 || block % WAVE || grid < 1 || !win_width_ok(nc) || s.k < 1 || s.k > WIN_K_MAX || s.tier < 1 ||
      s.lds_states < 1 || s.lds_states > win_tier_max(nc) || !s.start || !s.len || !s.item || !s.dig || !s.code || !s.prob ||
      !s.count || !s.n_config || !s.status || (s.scratch && !s.scratch_off))
    return hipErrorInvalidValue;
  switch (nc) {
    case 4: return launch_window<4>(a, s, grid, st, block);
    case 16: return launch_window<16>(a, s, grid, st, block);
    case 64: return launch_window<64>(a, s, grid, st, block);
    case 256: return launch_window<256>(a, s, grid, st, block);
    case 1024: return launch_window<1024>(a, s, grid, st, block);
  }
  return hipErrorInvalidValue;  // a width that is not built is an error, never another kernel
}

}  // namespace hmc
