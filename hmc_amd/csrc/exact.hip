// exact.hip — the exact M-step (--exact-estimate) of the HaploModel EM on CDNA4.
//
// PatternManager::estimatePatterns (PatternManager.cpp:364-410) re-estimates
// pattern frequencies as expected counts under the current model instead of
// re-mining the sampled haplotypes.  Per individual, HaploBuilder::
// estimateFrequency (HaploBuilder.cpp:274-332) resolves the genotype, runs the
// backward pass over the forward links (calcBackwardLikelihood, :263-272,
// HaploPair.cpp:126-136) and, for every start locus, walks the candidates'
// ForwardPatternTree (PatternTree.cpp:179-212) carrying three state -> weight
// lists: both haplotypes of the pair match the pattern so far / only the a-side
// / only the b-side (:334-450).  A node's frequency is sum(weight * backward) /
// P(genotype); its pattern gains that frequency and, as prefix frequency, the
// parent node's.
//
// Here the structure pass (estep_split.hip) supplies the states, their
// incoming contributions in add order and, in exact mode, every locus's
// contributions in extendAll order (the forward links in push order):
//   exact_fb    one block per individual: forward likelihoods (the ordered sums
//               of HaploPair.cpp:42,66) and backward likelihoods (links[0]
//               then links[1], each in push order), stored per locus;
//   exact_walk  one wavefront per (individual, start locus): the trie walk,
//               depth first, with the three lists held densely per state of
//               the node's locus and gathered from each state's incoming
//               contributions (the reference scatters along forward links;
//               same terms).  Subtrees whose lists are all zero are skipped:
//               their nodes would add 0 to every frequency and prefix.
// Frequencies accumulate across individuals in 2^-44 fixed point with 64-bit
// integer atomics: the totals do not depend on the order in which waves or
// ranks add, so the result is deterministic and identical for any sharding.
// The reference sums its lists in std::map<HaploPair*, double> pointer order,
// which no restatement reproduces: the bar is 1e-6 relative (north star).
#include "hmc_internal.hpp"
#include "estep_common.hpp"
#include "exact.hpp"
#include "philox.hpp"

namespace hmc {

namespace {

// The sum of a wavefront's 64 virtual lanes in one fixed butterfly order
// (xor 32, 16, ..., 1), for groups of GL lanes that each carry WAVE / GL
// virtual lanes (virtual lane gl + GL k in p[k]): the in-lane steps first,
// then the shuffles within the group.  Every GL gives the same double, so a
// walk of four items per wavefront sums exactly as the one-item walk.
template <int GL>
__device__ inline double group_sum_fixed(double (&p)[WAVE / GL]) {
  constexpr int NV = WAVE / GL;
#pragma unroll
  for (int s = NV / 2; s > 0; s >>= 1) {
    double q[NV];
#pragma unroll
    for (int k = 0; k < NV; ++k) q[k] = p[k] + p[k ^ s];
#pragma unroll
    for (int k = 0; k < NV; ++k) p[k] = q[k];
  }
  double x = p[0];
#pragma unroll
  for (int o = GL / 2; o > 0; o >>= 1) x += __shfl_xor(x, o);
  return x;
}

struct RecView {  // one locus record of the structure pass
  int F, C, NCH, CF, NP;  // states, stored contributions, chains, contributions in extendAll order, allele pairs
  const double *tpv;
  const uint32_t *hdr, *cb, *ct, *out, *npo;
  __device__ RecView(const uint32_t *R, bool head) { set(R, (int)R[0], (int)R[1], (int)R[2], R[3], head); }
  // from header words the caller already holds (exact_walk's per-depth cache)
  __device__ RecView(const uint32_t *R, int f, int c, int nch, uint32_t cfnp, bool head) { set(R, f, c, nch, cfnp, head); }
  __device__ void set(const uint32_t *R, int f, int c, int nch, uint32_t cfnp, bool head) {
    F = f;
    C = c;
    NCH = nch;
    CF = (int)(cfnp >> 10);
    NP = (int)(cfnp & 1023u);
    tpv = (const double *)(R + 4);
    hdr = R + 4 + 2 * F;
    cb = hdr + F;
    ct = cb + F + 1;
    out = head ? nullptr : ct + C + NCH;
    npo = head ? nullptr : out + CF;
  }
};

}  // namespace

// Extended range: the values v[0, F) of one record (each thread has written
// the entries tid, tid + NT, ... and passes their maximum) times 2^k with k
// chosen so that the record's maximum lands in [0.5, 1): ldexp, so exact unless
// an entry is more than 2^1021 below the maximum.  A maximum is order-free, so
// any reduction gives the same k.  Returns k (block-uniform); 0 for a record of
// zeros.  Ends on a barrier: the scaled values are visible to the block.
__device__ inline int rescale_record(double *v, int F, double m) {
  __shared__ double wmax[16];
  const int tid = threadIdx.x, NT = blockDim.x, nw = NT / WAVE;
#pragma unroll
  for (int o = WAVE / 2; o > 0; o >>= 1) m = fmax(m, __shfl_xor(m, o));
  if ((tid & (WAVE - 1)) == 0) wmax[tid / WAVE] = m;
  __syncthreads();
  m = wmax[0];
  for (int w = 1; w < nw; ++w) m = fmax(m, wmax[w]);
  const int k = m > 0.0 && !isinf(m) ? -1 - ilogb(m) : 0;
  if (k != 0)
    for (int t = tid; t < F; t += NT) v[t] = ldexp(v[t], k);
  __syncthreads();
  return k;
}

// Forward and backward likelihoods of every state of every locus (block per individual).
// BACKWARD = false (ExactArgs::forward_only, the posterior draws) stops after the forward pass.
// EXT = true (ExactArgs::extended): every record rescaled by an exact power of
// two (rescale_record), the cumulative exponents in the record's spare words,
// the scaled total of the final record and its exponent per individual; no
// underflow flag, so no pruned re-run.  EXT = false is the raw-double pass the
// exact M-step (exact_walk) reads.
template <bool BACKWARD, bool EXT>
__global__ __launch_bounds__(256) void exact_fb(ExactArgs a) {
  const int tid = threadIdx.x, NT = blockDim.x;
  const int L = a.L, hl = a.head_len;
  __shared__ int flag;
  for (int q = blockIdx.x; q < a.n_order; q += gridDim.x) {
    const int bi = a.order[q];
    const int st0 = a.status[bi];
    if (st0 != EST_OK && st0 != EST_OK_PRUNED) continue;
    const bool pruned = st0 == EST_OK_PRUNED;  // zero forward likelihoods are expected (not extended)
    const unsigned long long *roff = a.rec_off + (size_t)bi * (L + 1);
    unsigned long long *xo = a.x_off + (size_t)bi * (L + 1);
    // x-store layout per locus: fwd[F] then bwd[F] (doubles), even word offsets
    unsigned long long cur = a.x_base[bi];
    for (int j = hl; j <= L; ++j) {
      const RecView R(a.rec + roff[j], j == hl);
      if (tid == 0) xo[j] = cur;
      cur += 4ull * R.F + 2;
    }
    if (tid == 0) flag = 0;
    __syncthreads();
    // forward (HaploPair.cpp:27-32 head, :42 / :66 extension and add)
    int ex = 0;  // EXT: the cumulative forward exponent E_j (block-uniform)
    {
      const RecView R(a.rec + roff[hl], true);
      double *fw = (double *)(a.x + xo[hl]);
      double m = 0.0;
      for (int t = tid; t < R.F; t += NT) {
        const bool homo = (R.hdr[t] >> 24) & 1u;
        fw[t] = homo ? R.tpv[t] : R.tpv[t] * 2.0;
        if constexpr (EXT) m = fmax(m, fw[t]);
      }
      if constexpr (EXT) {
        ex += rescale_record(fw, R.F, m);
        if (tid == 0) ((int32_t *)(fw + 2 * (size_t)R.F))[0] = ex;
      }
    }
    __syncthreads();
    for (int j = hl + 1; j <= L; ++j) {
      const RecView R(a.rec + roff[j], false);
      const double *fp = (const double *)(a.x + xo[j - 1]);
      double *fw = (double *)(a.x + xo[j]);
      double m = 0.0;
      for (int t = tid; t < R.F; t += NT) {
        const double tpv = R.tpv[t];
        double f = 0.0;
        for (uint32_t r = R.cb[t]; r < R.cb[t + 1]; ++r) {
          const double v = fp[cw_state(R.ct[r])] * tpv;
          f = r == R.cb[t] ? v : f + v;
        }
        fw[t] = f;
        if constexpr (EXT) m = fmax(m, f);
        else if (!(f > 0.0) && j < L && !pruned) flag = 1;  // extend() would skip this pair (HaploBuilder.cpp:237)
      }
      if constexpr (EXT) {
        ex += rescale_record(fw, R.F, m);
        if (tid == 0) ((int32_t *)(fw + 2 * (size_t)R.F))[0] = ex;
      } else {
        __syncthreads();
      }
    }
    if constexpr (EXT) {
      // the divisor: the final record's scaled values summed as the value pass sums
      // its total, sequentially in state order from 0.0, with the exponent E_L
      if (tid == 0) {
        const int F = (int)a.rec[roff[L]];
        const double *fw = (const double *)(a.x + xo[L]);
        double tot = 0.0;
        for (int t = 0; t < F; ++t) tot += fw[t];
        a.xtot[bi] = tot;
        a.xtot_exp[bi] = ex;
      }
    }
    // every thread reads the flag before any thread can reset it for the next
    // individual (the reset sits before the barrier at the top of the loop)
    if constexpr (!EXT) {
      const bool underflow = flag != 0;
      __syncthreads();
      if (underflow) {
        if (tid == 0) a.status[bi] = EST_NEEDS_EXACT;
        continue;
      }
    }
    if (!BACKWARD) continue;
    // backward: states of m_haplopairs[L] keep m_backward_likelihood = 1.0
    int gx = 0;  // EXT: the cumulative backward exponent G_j (block-uniform; G_L = 0)
    {
      const RecView R(a.rec + roff[L], L == hl);
      double *bw = (double *)(a.x + xo[L]) + R.F;
      for (int t = tid; t < R.F; t += NT) bw[t] = 1.0;
      if constexpr (EXT)
        if (tid == 0) ((int32_t *)(bw + R.F))[1] = 0;
    }
    __syncthreads();
    for (int j = L - 1; j >= hl; --j) {
      const RecView R(a.rec + roff[j], j == hl);       // states s at locus j
      const RecView N(a.rec + roff[j + 1], false);     // their forward links
      const double *bn = (const double *)(a.x + xo[j + 1]) + N.F;
      double *bw = (double *)(a.x + xo[j]) + R.F;
      double m = 0.0;
      for (int s = tid; s < R.F; s += NT) {
        double b = 0.0;
        for (int pass = 0; pass < 2; ++pass) {  // m_forward_links[0], then [1], each in push order
          uint32_t off = 0;
          for (int p = 0; p < N.NP; ++p) {
            const uint32_t no = N.npo[p];
            for (uint32_t o = 0; o < no; ++o) {
              const uint32_t w = N.out[off + (uint32_t)s * no + o];
              if (w != NONE && (uint32_t)cw_rev(w) == (uint32_t)pass) {
                const uint32_t t = cw_state(w);
                b += bn[t] * N.tpv[t];
              }
            }
            off += (uint32_t)R.F * no;
          }
        }
        bw[s] = b;
        if constexpr (EXT) m = fmax(m, b);
      }
      if constexpr (EXT) {
        gx += rescale_record(bw, R.F, m);
        if (tid == 0) ((int32_t *)(bw + R.F))[1] = gx;
      } else {
        __syncthreads();
      }
    }
  }
}

// The walk's largest per-item span (exact_walk's scratch layout): the states
// of records max(s + d, head_len), d = 0..max_depth + 1, over every start
// locus s of every individual of the group (block per individual).
__global__ __launch_bounds__(256) void exact_span(ExactArgs a) {
  const int tid = threadIdx.x, NT = blockDim.x;
  const int L = a.L, hl = a.head_len;
  for (int q = blockIdx.x; q < a.n_order; q += gridDim.x) {
    const int bi = a.order[q];
    const int st0 = a.status[bi];
    if (st0 != EST_OK && st0 != EST_OK_PRUNED) continue;
    const unsigned long long *roff = a.rec_off + (size_t)bi * (L + 1);
    unsigned sp = 0;
    for (int s0 = tid; s0 < L; s0 += NT) {
      unsigned long long sum = 0;
      for (int d = 0; d <= a.max_depth + 1; ++d) {
        const int r = s0 + d > hl ? s0 + d : hl;
        if (r > L) break;
        sum += a.rec[roff[r]];
      }
      const unsigned v = (unsigned)(sum < 0xFFFFFFFFull ? sum : 0xFFFFFFFFull);
      sp = v > sp ? v : sp;
    }
    atomicMax(a.span_max, sp);
  }
}

// One contribution's terms into a child list set (HaploBuilder.cpp:375-427):
// ma / mb = the child's allele is the pair's a / b allele at this locus.
__device__ inline void walk_terms(bool ma, bool mb, bool rev, double w0, double w1, double w2, double tp, double &n0,
                                  double &n1, double &n2) {
  if (ma && mb) n0 += w0 * tp;
  else if (ma) n1 += w0 * tp * 0.5;
  else n2 += w0 * tp * 0.5;
  // a-side list follows the a haplotype: links[0] keep it on a, links[1] move it to b
  if (!rev ? ma : mb) (!rev ? n1 : n2) += w1 * tp;
  if (!rev ? mb : ma) (!rev ? n2 : n1) += w2 * tp;
}

// The ForwardPatternTree walk of HaploBuilder::estimateFrequency (:296-308,
// :334-450), one wavefront per (individual, start locus), sparse like the
// reference's maps.  A node's children are computed together: the states
// its non-zero states link to (forward links of the record, marked in an
// LDS bitmap and compacted in state order) gather, over their incoming
// contributions in record order, the three lists of every child whose allele
// their pair carries — a heterozygous state feeds two children from one pass
// over its contributions.  The children's lists are kept per depth, one slot
// per allele, so the walk descends into them in allele order without
// recomputing.  Each child's frequency is sum(weight * backward) over the
// union of reached states in state order (zero entries add +0.0).  Scratch
// invariant: every dense entry not in a touched list is 0.0 (the host zeroes
// the scratch before the launch and every item clears what it wrote).
#ifndef HMC_XWALK_WPE
#define HMC_XWALK_WPE 4  // resident waves per SIMD the walk's registers allow (tuning builds vary it)
#endif
template <int GL>
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(HMC_XWALK_WPE))) void exact_walk(ExactArgs a) {
  extern __shared__ unsigned long long lds64[];  // per group: exact_walk_lds_bytes
  constexpr int NG = WAVE / GL;  // items walked at once by the wavefront, GL lanes each
  const int lane = threadIdx.x, g = lane / GL, gl = lane % GL;
  // this group's lanes of a wave ballot
  auto gballot = [&](bool p) -> unsigned long long {
    const unsigned long long b = __ballot(p);
    return GL == WAVE ? b : (b >> (g * GL)) & ((1ull << GL) - 1ull);
  };
  const int L = a.L, hl = a.head_len, W = a.width, maxd = a.max_depth;
  const int D = maxd + 2;
  unsigned long long *stk64 = lds64 + (size_t)g * (exact_walk_lds_bytes(maxd, a.fmax, a.width) / 8);
  unsigned long long *sdesc = stk64, *smask = stk64 + D;
  // per depth, read once per item: the record's offset, the x-store offset of its locus
  unsigned long long *droff = stk64 + 2 * D, *dxo = stk64 + 3 * D;
  // narrow tries (width <= XWALK_CACHE_W): per depth and slot, the non-zero
  // entries of the slot's lists among the first GL touched states (bit j), and the child ids
  const int wc = exact_walk_cache_w(W);
  unsigned long long *nzm = stk64 + 4 * D;
  int *snode = (int *)(nzm + (size_t)D * wc), *snext = snode + D, *sslot = snext + D, *tcnt = sslot + D;
  int *sF = tcnt + D, *soff = sF + D;        // per depth: the states of its locus, their first entry in the item's layout
  int *dC = soff + D, *dNCH = dC + D;        // per depth: the record's header words (RecView)
  uint32_t *dCFNP = (uint32_t *)(dNCH + D), *dnpo0 = dCFNP + D;  // ... and its first allele pair's out-degree
  int *dnzv = (int *)(dnpo0 + D);            // per depth: nzm holds its slots' masks
  int *schild = dnzv + D;                    // [D][wc]: the children of the node at depth d
  // per depth: the first GL entries of the touched list (u16 states; the rest,
  // and every entry when a locus has more than 65 536 states, in the scratch)
  uint16_t *tl16 = (uint16_t *)(schild + (size_t)D * wc);
  uint32_t *marks = (uint32_t *)(tl16 + (size_t)D * WAVE);  // [fmax/32 + 1] reached-state bitmap
  const int nwords = (a.fmax + 31) >> 5;
  const int tlc = a.fmax <= 65536 ? GL : 0;
  // one item per wave and at most 64 unordered allele pairs (width <= 10):
  // lane p holds pair p's alleles, and a node's pairs that carry an allele of
  // one of its children form one ballot, tested against the links' pair bits
  const bool pmk = GL == WAVE && W * (W + 1) / 2 <= WAVE;
  int px = 0;
  while ((px + 1) * (px + 2) / 2 <= lane) ++px;
  const int py = lane - px * (px + 1) / 2;
  const bool pin = lane < W * (W + 1) / 2;
  // The item's lists: per depth d, W slots of three lists over the F_d states
  // of d's locus (slot i of depth d at 3 (W soff[d] + i F_d)); the wave's
  // region holds the largest such span of any item (ExactArgs::span)
  double *lists = a.scratch + ((size_t)blockIdx.x * NG + g) * a.scratch_stride;  // [3 W span]
  double *cfreq = lists + (size_t)3 * W * a.span;                          // [maxd+2][W]
  uint32_t *touched = (uint32_t *)(cfreq + (size_t)(maxd + 2) * W);       // [span]: per depth at soff[d]
  auto slot = [&](int d, int i) { return lists + (size_t)3 * ((size_t)W * soff[d] + (size_t)i * sF[d]); };
  // entry j of depth d's touched list
  auto tget = [&](int d, int j) -> uint32_t { return j < tlc ? (uint32_t)tl16[d * WAVE + j] : touched[soff[d] + j]; };
  auto tput = [&](int d, int j, uint32_t t) {
    if (j < tlc) tl16[d * WAVE + j] = (uint16_t)t;
    else touched[soff[d] + j] = t;
  };
  for (int d = gl; d < D; d += GL) {
    tcnt[d] = 0;
    smask[d] = 0ull;
  }
  for (int w = gl; w < nwords; w += GL) marks[w] = 0u;
  __builtin_amdgcn_wave_barrier();
  __threadfence_block();
  const long long n_items = a.item1 < 0 ? (long long)a.n_order * L : a.item1;
  for (long long it = a.item0 + (long long)blockIdx.x * NG + g; it < n_items; it += (long long)gridDim.x * NG) {
    const int q = (int)(it / L), start = (int)(it % L);
    const int bi = a.order[q];
    const int root = a.tr_root[start];
    if (root < 0 || (a.status[bi] != EST_OK && a.status[bi] != EST_OK_PRUNED)) continue;
    const double pg = a.gprob[bi];  // P(genotype) of the last E-step (HaploModel.cpp:109, HaploBuilder.cpp:294)
    if (!(pg > 0.0)) continue;
    const unsigned long long *roff = a.rec_off + (size_t)bi * (L + 1);
    const unsigned long long *xo = a.x_off + (size_t)bi * (L + 1);
    const uint32_t *Rh = a.rec + roff[hl];
    const int Fh = (int)Rh[0];
    {  // the item's layout: depth d's states are those of record max(start + d, head_len);
       // each depth's record header and offsets are read here once
      int carry = 0;
      for (int d0 = 0; d0 < D; d0 += GL) {
        const int dd = d0 + gl;
        const int r = start + dd > hl ? start + dd : hl;
        const bool has = dd < D && r <= L;
        int f = 0;
        if (has) {
          const unsigned long long ro = roff[r];
          const uint32_t *R = a.rec + ro;
          const uint32_t hx = R[0], hy = R[1], hz = R[2], hw = R[3];  // F, C, NCH, CF << 10 | NP
          f = (int)hx;
          droff[dd] = ro;
          dxo[dd] = xo[r];
          dC[dd] = (int)hy;
          dNCH[dd] = (int)hz;
          dCFNP[dd] = hw;
          // out-degree of the first allele pair (npo[0]) of a non-head record
          dnpo0[dd] = r > hl && (hw & 1023u) > 0u ? R[4 + 4 * (size_t)f + 1 + hy + hz + (hw >> 10)] : 0u;
        }
        int incl = f;
#pragma unroll
        for (int o = 1; o < GL; o <<= 1) {
          const int y = __shfl_up(incl, o, GL);
          if (gl >= o) incl += y;
        }
        if (dd < D) {
          sF[dd] = f;
          soff[dd] = carry + incl - f;
        }
        carry += __shfl(incl, GL - 1, GL);
      }
    }
    __builtin_amdgcn_wave_barrier();
    __threadfence_block();
    // depth 0: every state after max(start, head_len) loci, weight = forward likelihood
    {
      const int F0 = sF[0];
      const double *fw = (const double *)(a.x + dxo[0]);
      double *S0 = slot(0, 0);
      for (int t = gl; t < F0; t += GL) {
        S0[3 * t] = fw[t];
        tput(0, t, (uint32_t)t);
      }
      if (gl == 0) {
        tcnt[0] = F0;
        smask[0] = 1ull;
        snode[0] = root;
        snext[0] = -1;  // children not computed yet
        sslot[0] = 0;
      }
    }
    __builtin_amdgcn_wave_barrier();
    __threadfence_block();
    int d = 0;
    while (d >= 0) {
      __builtin_amdgcn_wave_barrier();
      __threadfence_block();
      const int node = snode[d];
      if (snext[d] < 0) {  // ---- all children of this node, into depth d+1 ----
        unsigned long long cm = 0ull;  // alleles with a child
        // (one item per wave: lane i holds child i and its pattern, read here once)
        int chv = -1, patv = -1;
        if (d < maxd) {
          if constexpr (GL == WAVE) {
            chv = gl < W ? a.tr_child[(size_t)node * W + gl] : -1;
            cm = gballot(chv >= 0);
            patv = chv >= 0 ? a.tr_data[chv] : -1;
            if (gl < wc) schild[d * wc + gl] = chv;
          } else {
            for (int i0 = 0; i0 < W; i0 += GL) {
              const int i = i0 + gl;
              cm |= gballot(i < W && a.tr_child[(size_t)node * W + i] >= 0) << i0;
            }
          }
        }
        if (cm == 0ull) {  // node done
          --d;
          continue;
        }
        const int locus = start + d;  // the children's allele is at this locus
        const double last_freq = d == 0 ? 1.0 : cfreq[(size_t)d * W + sslot[d]];  // prefix freq (HaploBuilder.cpp:305)
        const double *P0 = slot(d, sslot[d]), *P1 = P0 + 1, *P2 = P0 + 2;  // [F][3]: n0 n1 n2 of a state together
        {  // the previous sibling's children at depth d+1 back to zero
          const int nc = tcnt[d + 1];
          const unsigned long long wm = smask[d + 1];
          for (int j = gl; j < nc; j += GL) {
            const uint32_t t = tget(d + 1, j);
            for (unsigned long long m = wm; m; m &= m - 1) {
              double *C0 = slot(d + 1, __builtin_ctzll(m));
              C0[3 * t] = 0.0;
              C0[3 * t + 1] = 0.0;
              C0[3 * t + 2] = 0.0;
            }
          }
        }
        int ntc = 0;
        const double *bw;
        // one reached state per lane (ntc <= GL, not the head): its children's
        // three weights stay in registers for the frequencies (4)
        bool regs = false;
        uint32_t rxa = 0, rxb = 0;
        bool rca = false, rcb = false;
        double ra0 = 0.0, ra1 = 0.0, ra2 = 0.0, rb0 = 0.0, rb1 = 0.0, rb2 = 0.0, rbw = 0.0;
        if (locus < hl) {  // head pairs: their patterns' alleles (HaploBuilder.cpp:340-367), same states
          const RecView R(Rh, true);
          const uint32_t *plo = R.cb + Fh + 1, *phi = plo + Fh;
          bw = (const double *)(a.x + xo[hl]) + Fh;
          for (int t = gl; t < Fh; t += GL) {
            uint32_t xa, xb;
            if (hl == 1) {
              xa = R.hdr[t] & 0xFFu;
              xb = (R.hdr[t] >> 8) & 0xFFu;
            } else {
              xa = a.head_al[(size_t)plo[t] * hl + locus];
              xb = a.head_al[(size_t)phi[t] * hl + locus];
            }
            const double w0 = P0[3 * t], w1 = P1[3 * t], w2 = P2[3 * t];
            for (unsigned long long m = cm; m; m &= m - 1) {
              const uint32_t i = (uint32_t)__builtin_ctzll(m);
              const bool ma = xa == i, mb = xb == i;
              double n0 = 0.0, n1 = 0.0, n2 = 0.0;
              if (ma) {
                if (mb) n0 = w0;
                else n1 = w0 * 0.5;
              } else if (mb) {
                n2 = w0 * 0.5;
              }
              if (ma) n1 += w1;
              if (mb) n2 += w2;
              double *C0 = slot(d + 1, (int)i);
              C0[3 * t] = n0;
              C0[3 * t + 1] = n1;
              C0[3 * t + 2] = n2;
            }
            tput(d + 1, t, (uint32_t)t);
          }
          ntc = Fh;
        } else {  // along the forward links into the states after `locus` (:369-427)
          // depth d's record is `locus`, depth d+1's `locus + 1` (both >= head_len)
          const RecView R(a.rec + droff[d + 1], sF[d + 1], dC[d + 1], dNCH[d + 1], dCFNP[d + 1], false);
          const uint32_t npo0 = dnpo0[d + 1];
          bw = (const double *)(a.x + dxo[d + 1]) + R.F;
          // (1) mark the states the parent's non-zero states link to and whose
          //     pair carries the allele of some child on either side
          const int np = tcnt[d];
          const int Fp = sF[d];  // states the links leave from
          const unsigned long long pm = pmk ? __ballot(pin && (((cm >> px) & 1ull) || ((cm >> py) & 1ull))) : 0ull;
          // the parent's non-zero entries among its first GL states, when its
          // parent computed them in registers (otherwise the lists are read)
          const bool nzk = wc > 0 && d > 0 && dnzv[d] != 0;
          const unsigned long long nzb = nzk ? nzm[d * wc + sslot[d]] : ~0ull;
          for (int j = gl; j < np; j += GL) {
            const uint32_t s = tget(d, j);
            if (nzk && j < GL) {
              if (!((nzb >> j) & 1ull)) continue;
            } else if (P0[3 * s] == 0.0 && P1[3 * s] == 0.0 && P2[3 * s] == 0.0) {
              continue;
            }
            uint32_t off = 0;
            for (int p = 0; p < R.NP; ++p) {
              const uint32_t no = p == 0 ? npo0 : R.npo[p];
              // four links at a time: their words, then their pairs' alleles, then the marks
              for (uint32_t o = 0; o < no; o += 4) {
                uint32_t wv[4], hv[4];
#pragma unroll
                for (int u = 0; u < 4; ++u) wv[u] = o + u < no ? R.out[off + s * no + o + u] : NONE;
#pragma unroll
                for (int u = 0; u < 4; ++u) hv[u] = !pmk && wv[u] != NONE ? R.hdr[cw_state(wv[u])] : 0u;
#pragma unroll
                for (int u = 0; u < 4; ++u)
                  if (wv[u] != NONE && (pmk ? ((pm >> cw_xpair(wv[u])) & 1ull) != 0ull
                                            : (((cm >> (hv[u] & 0xFFu)) & 1ull) || ((cm >> ((hv[u] >> 8) & 0xFFu)) & 1ull)))) {
                    const uint32_t t = cw_state(wv[u]);
                    atomicOr(&marks[t >> 5], 1u << (t & 31u));
                  }
              }
              off += (uint32_t)Fp * no;
            }
          }
          __builtin_amdgcn_wave_barrier();
          __threadfence_block();
          // (2) the marked states in ascending order; the bitmap back to zero
          const int nw = (R.F + 31) >> 5;
          for (int w0 = 0; w0 < nw; w0 += GL) {
            const int w = w0 + gl;
            uint32_t bits = w < nw ? marks[w] : 0u;
            const int c = __popc(bits);
            int incl = c;
#pragma unroll
            for (int dd = 1; dd < GL; dd <<= 1) {
              const int y = __shfl_up(incl, dd);
              if (gl >= dd) incl += y;
            }
            int at = ntc + incl - c;
            while (bits) {
              const int b = __builtin_ctz(bits);
              bits &= bits - 1u;
              tput(d + 1, at++, (uint32_t)(w * 32 + b));
            }
            if (w < nw) marks[w] = 0u;
            ntc += __shfl(incl, g * GL + GL - 1);
          }
          __builtin_amdgcn_wave_barrier();
          __threadfence_block();
          regs = GL == WAVE && ntc <= GL;
          // (3) each reached state gathers over its incoming contributions, for
          //     the children of its a allele and of its b allele in one pass
          //     (contributions two at a time: both words, then both weight sets,
          //     then the terms in record order)
          for (int j = gl; j < ntc; j += GL) {
            const uint32_t t = tget(d + 1, j);
            const uint32_t hd = R.hdr[t];
            const uint32_t xa = hd & 0xFFu, xb = (hd >> 8) & 0xFFu;
            const bool ca = (cm >> xa) & 1ull, cb = xb != xa && ((cm >> xb) & 1ull);
            double a0 = 0.0, a1 = 0.0, a2 = 0.0, b0 = 0.0, b1 = 0.0, b2 = 0.0;
            const double tp = R.tpv[t];
            const uint32_t r0 = R.cb[t], r1 = R.cb[t + 1];
            if (regs) rbw = bw[t];
            for (uint32_t r = r0; r < r1; r += 2) {
              const bool two = r + 1 < r1;
              const uint32_t wA = R.ct[r], wB = two ? R.ct[r + 1] : 0u;
              const uint32_t sA = cw_state(wA), sB = cw_state(wB);
              const double u0 = P0[3 * sA], u1 = P1[3 * sA], u2 = P2[3 * sA];
              double v0 = 0.0, v1 = 0.0, v2 = 0.0;
              if (two) {
                v0 = P0[3 * sB];
                v1 = P1[3 * sB];
                v2 = P2[3 * sB];
              }
              if (ca) walk_terms(true, xb == xa, cw_rev(wA), u0, u1, u2, tp, a0, a1, a2);
              if (cb) walk_terms(false, true, cw_rev(wA), u0, u1, u2, tp, b0, b1, b2);
              if (two) {
                if (ca) walk_terms(true, xb == xa, cw_rev(wB), v0, v1, v2, tp, a0, a1, a2);
                if (cb) walk_terms(false, true, cw_rev(wB), v0, v1, v2, tp, b0, b1, b2);
              }
            }
            if (ca) {
              double *C0 = slot(d + 1, (int)xa);
              C0[3 * t] = a0;
              C0[3 * t + 1] = a1;
              C0[3 * t + 2] = a2;
            }
            if (cb) {
              double *C0 = slot(d + 1, (int)xb);
              C0[3 * t] = b0;
              C0[3 * t + 1] = b1;
              C0[3 * t + 2] = b2;
            }
            rxa = xa;
            rxb = xb;
            rca = ca;
            rcb = cb;
            ra0 = a0;
            ra1 = a1;
            ra2 = a2;
            rb0 = b0;
            rb1 = b1;
            rb2 = b2;
          }
        }
        __builtin_amdgcn_wave_barrier();
        __threadfence_block();
        // (4) every child's frequency: hp->setFrequency(+freq), setPrefixFreq(+last_freq) (:437-441)
        unsigned long long desc = 0ull;
        for (unsigned long long m = cm; m; m &= m - 1) {
          const int i = __builtin_ctzll(m);
          double part[NG];  // virtual lane gl + GL k of a 64-lane sum (group_sum_fixed)
#pragma unroll
          for (int k = 0; k < NG; ++k) part[k] = 0.0;
          bool any = false;
          if (regs) {  // this lane's state (if any) from (3): the same terms the scratch holds
            if (gl < ntc) {
              const bool isa = rca && rxa == (uint32_t)i, isb = rcb && rxb == (uint32_t)i;
              const double n0 = isa ? ra0 : (isb ? rb0 : 0.0), n1 = isa ? ra1 : (isb ? rb1 : 0.0),
                           n2 = isa ? ra2 : (isb ? rb2 : 0.0);
              part[0] += ((n0 + n1) + n2) * rbw;
              any = (n0 != 0.0) | (n1 != 0.0) | (n2 != 0.0);
            }
          } else {
            const double *C0 = slot(d + 1, i);
            for (int j = gl; j < ntc; j += GL) {
              const uint32_t t = tget(d + 1, j);
              const double n0 = C0[3 * t], n1 = C0[3 * t + 1], n2 = C0[3 * t + 2];
              const double v = ((n0 + n1) + n2) * bw[t];
              if constexpr (NG == 1) {
                part[0] += v;
              } else {
                const int k = (j / GL) & (NG - 1);
#pragma unroll
                for (int u = 0; u < NG; ++u)
                  if (u == k) part[u] += v;
              }
              any |= (n0 != 0.0) | (n1 != 0.0) | (n2 != 0.0);
            }
          }
          const double freq = group_sum_fixed<GL>(part) / pg;
          int pat;
          if constexpr (GL == WAVE) {
            pat = __shfl(patv, i);
          } else {
            const int child = a.tr_child[(size_t)node * W + i];
            pat = a.tr_data[child];
          }
          if (gl == 0) {
            cfreq[(size_t)(d + 1) * W + i] = freq;
            if (pat >= 0) {
              atomicAdd(&a.acc_freq[pat], (unsigned long long)__double2ll_rn(freq * EXACT_FIXED_SCALE));
              atomicAdd(&a.acc_prefix[pat], (unsigned long long)__double2ll_rn(last_freq * EXACT_FIXED_SCALE));
            }
          }
          const unsigned long long anym = gballot(any);
          if (anym != 0ull && d + 1 <= maxd) desc |= 1ull << i;
          if (gl == 0 && i < wc) nzm[(d + 1) * wc + i] = anym;  // (bit j = touched entry j when regs)
        }
        if (gl == 0) {
          if (wc > 0) dnzv[d + 1] = regs ? 1 : 0;
          tcnt[d + 1] = ntc;
          smask[d + 1] = cm;
          sdesc[d] = desc;
          snext[d] = 0;
        }
        __builtin_amdgcn_wave_barrier();
        __threadfence_block();
      }
      // ---- descend into the next child whose lists are not all zero ----
      const unsigned long long left = sdesc[d] & ~((1ull << snext[d]) - 1ull);
      if (left == 0ull) {  // node done
        --d;
        continue;
      }
      const int i = __builtin_ctzll(left);
      const int child = GL == WAVE && wc > 0 ? schild[d * wc + i] : a.tr_child[(size_t)node * W + i];
      __builtin_amdgcn_wave_barrier();
      if (gl == 0) {
        snext[d] = i + 1;
        snode[d + 1] = child;
        snext[d + 1] = -1;
        sslot[d + 1] = i;
      }
      ++d;
    }
    // the item's entries back to zero (scratch invariant)
    __builtin_amdgcn_wave_barrier();
    __threadfence_block();
    for (int dd = 0; dd <= maxd; ++dd) {
      const int nc = tcnt[dd];
      const unsigned long long wm = smask[dd];
      for (int j = gl; j < nc; j += GL) {
        const uint32_t t = tget(dd, j);
        for (unsigned long long m = wm; m; m &= m - 1) {
          double *D0 = slot(dd, __builtin_ctzll(m));
          D0[3 * t] = 0.0;
          D0[3 * t + 1] = 0.0;
          D0[3 * t + 2] = 0.0;
        }
      }
    }
    __builtin_amdgcn_wave_barrier();
    __threadfence_block();
    for (int dd = gl; dd < D; dd += GL) {
      tcnt[dd] = 0;
      smask[dd] = 0ull;
    }
    __builtin_amdgcn_wave_barrier();
    __threadfence_block();
  }
}


#ifdef HMC_VARIANTS  // (the breadth-first walk: measured slower, the variants library only)
// ---- breadth-first walk ----------------------------------------------------
// The depth-first walk above spends a wavefront and a dozen dependent,
// barriered steps on every trie node, while a node's lists hold a handful of
// non-zero states (300 x 200 panel, restatement counts: 14.9 M live nodes, 5.0
// non-zero entries each).  Here a lane takes a whole node (a work unit,
// XWalkArgs): it scatters the node's entries along their forward links
// (HaploBuilder.cpp:369-427 scatters the same way) into private accumulators —
// per reached state the lists of its a-allele child and of its b-allele child —
// then adds every child's frequency (states ascending) and prefix term
// (:437-441) and emits the children with non-zero lists that have children of
// their own.  The host runs the levels depth by depth over batches of items;
// a wave reserves its outputs with one atomic pair, and units whose outputs do
// not fit are deferred and re-run once the deeper levels are done.
__device__ inline unsigned long long wave_excl_u64(unsigned long long v, unsigned long long &total) {
  const int lane = (int)(threadIdx.x & 63);
  unsigned long long incl = v;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const unsigned long long y = __shfl_up(incl, o);
    if (lane >= o) incl += y;
  }
  total = __shfl(incl, 63);
  return incl - v;
}

__global__ __launch_bounds__(256) void exact_walk_units(ExactArgs a, XWalkArgs x) {
  const int gtid = blockIdx.x * blockDim.x + threadIdx.x, nthr = gridDim.x * blockDim.x;
  const int lane = (int)(threadIdx.x & 63);
  const int L = a.L, hl = a.head_len, W = a.width, fmax = a.fmax;
  double *acc = x.lacc + (size_t)gtid * x.lacc_stride;  // [a side | b side][3][fmax]
  uint32_t *bits = x.lbits + (size_t)gtid * x.lbits_stride;
  const double *ew0 = x.e_w, *ew1 = x.e_w + x.e_cap, *ew2 = x.e_w + 2 * x.e_cap;
  double *ow0 = x.e_w, *ow1 = x.e_w + x.e_cap, *ow2 = x.e_w + 2 * x.e_cap;
  const int rounds = (x.n_in + nthr - 1) / nthr;  // wave-uniform: every lane joins its wave's reservation
  for (int it = 0; it < rounds; ++it) {
    const int j = it * nthr + gtid;
    bool live = j < x.n_in;
    unsigned long long u = 0;
    int q = 0, start = 0, node = -1, bi = 0;
    double pg = 0.0, pfreq = 1.0;
    if (live) {
      if (x.roots) {  // item j of the batch: its start locus's trie root, every state with its forward likelihood
        const long long item = (long long)x.in_base + (x.idx ? x.idx[j] : j);
        q = (int)(item / L);
        start = (int)(item % L);
        node = a.tr_root[start];
      } else {
        u = x.idx ? (unsigned long long)x.idx[j] : x.in_base + (unsigned long long)j;
        node = x.u.node[u];
        if (node >= 0) {
          q = x.u.q[u];
          start = x.u.start[u];
          pfreq = x.u.freq[u];
        }
      }
      live = node >= 0;
    }
    if (live) {
      bi = a.order[q];
      const int s0 = a.status[bi];
      pg = a.gprob[bi];  // P(genotype) of the last E-step (HaploModel.cpp:109, HaploBuilder.cpp:294)
      live = (s0 == EST_OK || s0 == EST_OK_PRUNED) && pg > 0.0;
    }
    unsigned long long cm = 0ull;  // alleles with a child
    if (live)
      for (int i = 0; i < W; ++i) cm |= (a.tr_child[(size_t)node * W + i] >= 0 ? 1ull : 0ull) << i;
    live = live && cm != 0ull;
    const int locus = start + x.depth;  // the children's allele is at this locus
    const bool head = locus < hl;       // head pairs: their patterns' alleles, same states (HaploBuilder.cpp:340-367)
    int FT = 0;
    const double *bw = nullptr;
    const uint32_t *thdr = nullptr, *plo = nullptr, *phi = nullptr;
    // the children's two alleles of state t (a side, b side)
    auto alleles = [&](uint32_t t, uint32_t &xa, uint32_t &xb) {
      if (!head || hl == 1) {
        xa = thdr[t] & 0xFFu;
        xb = (thdr[t] >> 8) & 0xFFu;
      } else {
        xa = a.head_al[(size_t)plo[t] * hl + locus];
        xb = a.head_al[(size_t)phi[t] * hl + locus];
      }
    };
    if (live) {
      const unsigned long long *roff = a.rec_off + (size_t)bi * (L + 1);
      const unsigned long long *xo = a.x_off + (size_t)bi * (L + 1);
      const int tix = head ? hl : locus + 1, pix = head ? hl : locus;  // the children's / the node's states
      const RecView R(a.rec + roff[tix], head);
      FT = R.F;
      thdr = R.hdr;
      if (head) {
        plo = R.cb + FT + 1;
        phi = plo + FT;
      }
      bw = (const double *)(a.x + xo[tix]) + FT;
      const int FP = (int)a.rec[roff[pix]];
      const double *fwp = (const double *)(a.x + xo[pix]);
      const unsigned long long e0 = x.roots ? 0ull : x.u.e0[u];
      const int ne = x.roots ? FP : (int)x.u.ne[u];
      for (int k = 0; k < ne; ++k) {
        const uint32_t s = x.roots ? (uint32_t)k : x.e_t[e0 + k];
        const double w0 = x.roots ? fwp[s] : ew0[e0 + k];
        const double w1 = x.roots ? 0.0 : ew1[e0 + k], w2 = x.roots ? 0.0 : ew2[e0 + k];
        if (w0 == 0.0 && w1 == 0.0 && w2 == 0.0) continue;
        if (head) {
          uint32_t xa, xb;
          alleles(s, xa, xb);
          const bool ca = (cm >> xa) & 1ull, cb = xb != xa && ((cm >> xb) & 1ull);
          if (!ca && !cb) continue;
          bits[s >> 5] |= 1u << (s & 31u);
          if (ca) {  // child xa: both sides when xb == xa, else the a side
            double *A = acc + s;
            if (xb == xa) {
              A[0] = w0;
              A[fmax] = w1;
              A[2 * fmax] = w2;
            } else {
              A[fmax] = w0 * 0.5 + w1;
            }
          }
          if (cb) acc[3 * (size_t)fmax + 2 * (size_t)fmax + s] = w0 * 0.5 + w2;  // child xb: the b side
          continue;
        }
        uint32_t off = 0;
        for (int p = 0; p < R.NP; ++p) {  // m_forward_links of the pair, in push order
          const uint32_t no = R.npo[p];
          for (uint32_t o = 0; o < no; ++o) {
            const uint32_t w = R.out[off + s * no + o];
            if (w == NONE) continue;
            const uint32_t t = cw_state(w);
            const bool rev = cw_rev(w);
            uint32_t xa, xb;
            alleles(t, xa, xb);
            const bool ca = (cm >> xa) & 1ull, cb = xb != xa && ((cm >> xb) & 1ull);
            if (!ca && !cb) continue;
            bits[t >> 5] |= 1u << (t & 31u);
            const double tp = R.tpv[t];
            if (ca) {
              double *A = acc + t;
              walk_terms(true, xb == xa, rev, w0, w1, w2, tp, A[0], A[fmax], A[2 * fmax]);
            }
            if (cb) {
              double *B = acc + 3 * (size_t)fmax + t;
              walk_terms(false, true, rev, w0, w1, w2, tp, B[0], B[fmax], B[2 * fmax]);
            }
          }
          off += (uint32_t)FP * no;
        }
      }
    }
    const int nwT = (FT + 31) >> 5;
    // child i's lists at state t: the a-side accumulators when t's a allele is i, else the b side's
    auto side = [&](uint32_t t, uint32_t i) -> const double * {
      uint32_t xa, xb;
      alleles(t, xa, xb);
      return xa == i ? acc + t : (xb == i ? acc + 3 * (size_t)fmax + t : nullptr);
    };
    auto has_children = [&](int c) {
      bool g = false;
      for (int i = 0; i < W; ++i) g = g || a.tr_child[(size_t)c * W + i] >= 0;
      return g;
    };
    // pass 1: the children this node emits and their entries
    unsigned long long nu = 0, nent = 0;
    if (live)
      for (unsigned long long m = cm; m; m &= m - 1) {
        const uint32_t i = (uint32_t)__builtin_ctzll(m);
        const int child = a.tr_child[(size_t)node * W + i];
        if (!has_children(child)) continue;
        unsigned long long cnt = 0;
        for (int w = 0; w < nwT; ++w)
          for (uint32_t b = bits[w]; b; b &= b - 1u) {
            const uint32_t t = (uint32_t)w * 32u + (uint32_t)__builtin_ctz(b);
            const double *n = side(t, i);
            if (n && (n[0] != 0.0 || n[fmax] != 0.0 || n[2 * fmax] != 0.0)) ++cnt;
          }
        if (cnt) {
          ++nu;
          nent += cnt;
        }
      }
    // one reservation per wave
    unsigned long long tu = 0, te = 0;
    const unsigned long long xu = wave_excl_u64(nu, tu), xe = wave_excl_u64(nent, te);
    unsigned long long bu = 0, be = 0;
    if (lane == 0 && (tu | te)) {
      bu = atomicAdd(x.cursor, tu);
      be = atomicAdd(x.cursor + 1, te);
    }
    bu = __shfl(bu, 0) + xu;
    be = __shfl(be, 0) + xe;
    const bool ok = live && bu + nu <= x.u_cap && be + nent <= x.e_cap;
    if (live && !ok) {  // re-run later: nothing of this node is added now
      const int d = atomicAdd(x.n_defer, 1);
      x.defer[d] = x.roots ? (x.idx ? x.idx[j] : (int32_t)j) : (int32_t)u;
      for (unsigned long long k = bu; k < bu + nu && k < x.u_cap; ++k) x.u.node[k] = -1;  // holes
    }
    // pass 2: frequencies (hp->setFrequency, setPrefixFreq, HaploBuilder.cpp:437-441) and the emitted children
    if (ok)
      for (unsigned long long m = cm; m; m &= m - 1) {
        const uint32_t i = (uint32_t)__builtin_ctzll(m);
        const int child = a.tr_child[(size_t)node * W + i];
        const bool gk = has_children(child);
        double f = 0.0;
        unsigned long long cnt = 0;
        for (int w = 0; w < nwT; ++w)
          for (uint32_t b = bits[w]; b; b &= b - 1u) {
            const uint32_t t = (uint32_t)w * 32u + (uint32_t)__builtin_ctz(b);
            const double *n = side(t, i);
            if (!n) continue;
            const double n0 = n[0], n1 = n[fmax], n2 = n[2 * fmax];
            if (n0 == 0.0 && n1 == 0.0 && n2 == 0.0) continue;
            f += ((n0 + n1) + n2) * bw[t];
            if (gk) {
              x.e_t[be + cnt] = t;
              ow0[be + cnt] = n0;
              ow1[be + cnt] = n1;
              ow2[be + cnt] = n2;
            }
            ++cnt;
          }
        const double freq = f / pg;
        const int pat = a.tr_data[child];
        if (pat >= 0) {
          atomicAdd(&a.acc_freq[pat], (unsigned long long)__double2ll_rn(freq * EXACT_FIXED_SCALE));
          atomicAdd(&a.acc_prefix[pat], (unsigned long long)__double2ll_rn(pfreq * EXACT_FIXED_SCALE));
        }
        if (gk && cnt) {
          x.u.q[bu] = q;
          x.u.start[bu] = start;
          x.u.node[bu] = child;
          x.u.freq[bu] = freq;
          x.u.e0[bu] = be;
          x.u.ne[bu] = (uint32_t)cnt;
          ++bu;
          be += cnt;
        }
      }
    // the accumulators and the bitmap back to zero
    if (live)
      for (int w = 0; w < nwT; ++w) {
        for (uint32_t b = bits[w]; b; b &= b - 1u) {
          const uint32_t t = (uint32_t)w * 32u + (uint32_t)__builtin_ctz(b);
          for (int c = 0; c < 6; ++c) acc[(size_t)c * fmax + t] = 0.0;
        }
        bits[w] = 0u;
      }
  }
}

hipError_t launch_exact_walk_units(const ExactArgs &a, const XWalkArgs &x, int grid, hipStream_t st) {
  if (x.n_in <= 0) return hipSuccess;
  if (a.width < 1 || a.width > 64 || grid < 1) return hipErrorInvalidValue;
  hipLaunchKernelGGL(exact_walk_units, dim3(grid), dim3(256), 0, st, a, x);
  return hipGetLastError();
}
#else
hipError_t launch_exact_walk_units(const ExactArgs &, const XWalkArgs &, int, hipStream_t) { return hipErrorNotSupported; }
#endif

size_t exact_walk_scratch_doubles(int max_depth, long long span, int width) {
  return (size_t)3 * width * (size_t)span + (size_t)(max_depth + 2) * width + ((size_t)span + 1) / 2;
}


hipError_t launch_exact_fb(const ExactArgs &a, int grid, hipStream_t st) {
  if (a.n_order <= 0) return hipSuccess;
  if (a.extended) {
    if (!a.xtot || !a.xtot_exp) return hipErrorInvalidValue;
    if (a.forward_only) hipLaunchKernelGGL((exact_fb<false, true>), dim3(grid), dim3(256), 0, st, a);
    else hipLaunchKernelGGL((exact_fb<true, true>), dim3(grid), dim3(256), 0, st, a);
    return hipGetLastError();
  }
  if (a.forward_only) hipLaunchKernelGGL((exact_fb<false, false>), dim3(grid), dim3(256), 0, st, a);
  else hipLaunchKernelGGL((exact_fb<true, false>), dim3(grid), dim3(256), 0, st, a);
  return hipGetLastError();
}

hipError_t launch_exact_span(const ExactArgs &a, int grid, hipStream_t st) {
  if (a.n_order <= 0) return hipSuccess;
  if (!a.span_max) return hipErrorInvalidValue;
  hipLaunchKernelGGL(exact_span, dim3(grid), dim3(256), 0, st, a);
  return hipGetLastError();
}

hipError_t launch_exact_walk(const ExactArgs &a, int grid, hipStream_t st, int items_per_wave) {
  if (a.n_order <= 0) return hipSuccess;
  if (a.width < 1 || a.width > 64 || (items_per_wave != 1 && items_per_wave != 4)) return hipErrorInvalidValue;
  const size_t lds = exact_walk_lds_bytes(a.max_depth, a.fmax, a.width) * (size_t)items_per_wave;
  if (lds > EXACT_WALK_LDS_MAX) return hipErrorInvalidValue;  // the host reports it (exact_walk_group)
#ifdef HMC_VARIANTS
  void (*k)(ExactArgs) = items_per_wave == 4 ? exact_walk<16> : exact_walk<WAVE>;
#else
  if (items_per_wave != 1) return hipErrorNotSupported;  // (four items per wave: the variants library only)
  void (*k)(ExactArgs) = exact_walk<WAVE>;
#endif
  if (lds > 65536) {  // wide frontiers: a larger reached-state bitmap, fewer waves per CU (set per launch: per device)
    hipError_t e = hipFuncSetAttribute((const void *)k, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return e;
  }
  hipLaunchKernelGGL(k, dim3(grid), dim3(WAVE), lds, st, a);
  return hipGetLastError();
}

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
  const int L = a.L, hl = a.head_len, NP = s.n_pairs;
  __shared__ uint32_t present[32];  // one bit per bin (NP <= 990)
  const bool sparse = NP > nw;      // block-uniform
  for (int q = blockIdx.x; q < a.n_order; q += gridDim.x) {
    const int bi = a.order[q];
    const unsigned long long s0 = s.site_off[bi], s1 = s.site_off[bi + 1];
    if (s0 == s1) continue;
    const int st0 = a.status[bi];
    const double pg = EXT ? a.xtot[bi] : a.gprob[bi];
    const bool resolved = (st0 == EST_OK || st0 == EST_OK_PRUNED) && pg > 0.0 && !isinf(pg);
    if (!resolved || (!EXT && pg < SITE_PG_MIN)) {  // rows of zeros: unresolved (1), or P(genotype) subnormal (2)
      for (unsigned long long i = s0 * NP + threadIdx.x; i < s1 * NP; i += blockDim.x) s.post[i] = 0.0;
      for (unsigned long long i = s0 + threadIdx.x; i < s1; i += blockDim.x) s.site_status[i] = resolved ? 2 : 1;
      continue;
    }
    const unsigned long long *roff = a.rec_off + (size_t)bi * (L + 1);
    const unsigned long long *xo = a.x_off + (size_t)bi * (L + 1);
    // On long panels P(genotype) is tiny and a product fwd * bwd of two normal
    // numbers would be subnormal or 0: both factors and the divisor are scaled
    // by powers of two that cancel (fwd * bwd <= P(genotype), so nothing
    // overflows).  Exact, so wherever the plain formula stays in the normal
    // range this gives its bits.
    int sc = EXT ? 0 : -ilogb(pg), sa = sc / 2, sb = sc - sa;
    const double pgs = EXT ? pg : ldexp(pg, sc);
    const int EL = EXT ? a.xtot_exp[bi] : 0;
    for (unsigned long long site = s0; site < s1; ++site) {
      const int k = s.site_locus[site];
      const bool head = k < hl - 1;  // alleles from the head patterns (head_len > 1 only)
      const int j = head ? hl : k + 1;
      const RecView R(a.rec + roff[j], j == hl);
      const double *fw = (const double *)(a.x + xo[j]), *bw = fw + R.F;
      if constexpr (EXT) {
        const int32_t *ex = (const int32_t *)(bw + R.F);  // E_j, G_j
        sc = EL - ex[0] - ex[1];
        sa = sc / 2;
        sb = sc - sa;
      }
      const uint32_t *plo = R.cb + R.F + 1, *phi = plo + R.F;  // head record: the states' two head patterns
      auto bin_of = [&](int t) -> uint32_t {
        if (head) return xpair_index(a.head_al[(size_t)plo[t] * hl + k], a.head_al[(size_t)phi[t] * hl + k]);
        const uint32_t h = R.hdr[t];
        return xpair_index(h & 0xFFu, (h >> 8) & 0xFFu);
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
          if (bin_of(t) == (uint32_t)b) part[0] += ldexp(fw[t], sa) * ldexp(bw[t], sb);
        const double v = group_sum_fixed<WAVE>(part) / pgs;
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
  __shared__ int fmx;
  const int tid = threadIdx.x, NT = blockDim.x;
  const int lane = tid & (WAVE - 1), wave = tid / WAVE, nw = NT / WAVE;
  const int L = a.L, hl = a.head_len;
  for (int q = blockIdx.x; q < a.n_order; q += gridDim.x) {
    const int bi = a.order[q];
    const unsigned long long s0 = s.site_off[bi], s1 = s.site_off[bi + 1];
    if (s0 == s1) continue;
    const int st0 = a.status[bi];
    const double pg = EXT ? a.xtot[bi] : a.gprob[bi];
    const bool resolved = (st0 == EST_OK || st0 == EST_OK_PRUNED) && pg > 0.0 && !isinf(pg);
    const unsigned long long *roff = a.rec_off + (size_t)bi * (L + 1);
    const unsigned long long *xo = a.x_off + (size_t)bi * (L + 1);
    // the individual's largest record (block-uniform after the barrier)
    int fbig = 0;
    if (resolved) {
      __syncthreads();  // every thread has read the previous individual's maximum
      if (tid == 0) fmx = 0;
      __syncthreads();
      int f = 0;
      for (int j = hl + tid; j <= L; j += NT) f = max(f, (int)a.rec[roff[j]]);
      atomicMax(&fmx, f);
      __syncthreads();
      fbig = fmx;
    }
    const bool in_lds = fbig <= s.tier;
    // (a frontier neither store holds cannot occur: the host sizes the scratch from the group's fmax)
    const bool fits = in_lds || (s.scratch && fbig <= s.scratch_states);
    if (!resolved || (!EXT && pg < SITE_PG_MIN) || !fits) {  // rows of zeros: unresolved (1), or P(genotype) subnormal (2)
      for (unsigned long long i = s0 * 2 + tid; i < s1 * 2; i += NT) s.post[i] = 0.0;
      for (unsigned long long i = s0 + tid; i < s1; i += NT) s.site_status[i] = resolved && fits ? 2 : 1;
      continue;
    }
    const size_t cap = in_lds ? (size_t)s.tier : (size_t)s.scratch_states;
    double *cur = in_lds ? sw_lds : s.scratch + (size_t)blockIdx.x * 4 * cap;
    double *prev = cur + 2 * cap;
    int sc = EXT ? 0 : -ilogb(pg), sa = sc / 2, sb = sc - sa;
    const double pgs = EXT ? pg : ldexp(pg, sc);
    const int EL = EXT ? a.xtot_exp[bi] : 0;
    // the exponents exact_fb left with record j (EXT): E_j, G_j
    auto rec_exp = [&](int j) { return (const int32_t *)(a.x + xo[j] + 4ull * a.rec[roff[j]]); };
    // o(t): the side of state t of record j that carries the lower allele of locus k
    // (k < head_len: j is the head record; its hdr word carries locus 0 when head_len is 1)
    auto low_side = [&](const RecView &R, int k, int t) -> int {
      uint32_t xa, xb;
      if (k < hl && hl > 1) {
        const uint32_t *plo = R.cb + R.F + 1, *phi = plo + R.F;
        xa = a.head_al[(size_t)plo[t] * hl + k];
        xb = a.head_al[(size_t)phi[t] * hl + k];
      } else {
        const uint32_t h = R.hdr[t];
        xa = h & 0xFFu;
        xb = (h >> 8) & 0xFFu;
      }
      return xa < xb ? 0 : 1;
    };
    auto anchor = [&](int j, int k) {
      const RecView R(a.rec + roff[j], j == hl);
      const double *fw = (const double *)(a.x + xo[j]);
      for (int t = tid; t < R.F; t += NT) {
        const int o = low_side(R, k, t);
        cur[2 * t + o] = fw[t];
        cur[2 * t + (o ^ 1)] = 0.0;
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
        double *x = prev;
        prev = cur;
        cur = x;
        const RecView R(a.rec + roff[j], false);
        const int step = EXT ? rec_exp(j)[0] - rec_exp(j - 1)[0] : 0;
        for (int t = tid; t < R.F; t += NT) {
          const double tpv = R.tpv[t];
          double n0 = 0.0, n1 = 0.0;
          const uint32_t r0 = R.cb[t], r1 = R.cb[t + 1];
          for (uint32_t r = r0; r < r1; ++r) {
            const uint32_t w = R.ct[r];
            const uint32_t sp = cw_state(w), rv = cw_rev(w) ? 1u : 0u;
            const double v0 = prev[2 * sp + rv] * tpv, v1 = prev[2 * sp + (rv ^ 1u)] * tpv;
            n0 = r == r0 ? v0 : n0 + v0;
            n1 = r == r0 ? v1 : n1 + v1;
          }
          cur[2 * t] = EXT ? ldexp(n0, step) : n0;
          cur[2 * t + 1] = EXT ? ldexp(n1, step) : n1;
        }
        __syncthreads();
      }
      {
        const RecView R(a.rec + roff[j], j == hl);
        const double *bw = (const double *)(a.x + xo[j]) + R.F;
        if constexpr (EXT) {
          sc = EL - rec_exp(j)[0] - rec_exp(j)[1];
          sa = sc / 2;
          sb = sc - sa;
        }
        for (int w = wave; w < 2; w += nw) {  // wave-uniform: 0 cis, 1 trans
          double part[1] = {0.0};
          for (int t = lane; t < R.F; t += WAVE)
            part[0] += ldexp(cur[2 * t + (low_side(R, kb, t) ^ w)], sa) * ldexp(bw[t], sb);
          const double v = group_sum_fixed<WAVE>(part) / pgs;
          if (lane == 0) s.post[site * 2 + w] = v;
        }
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
  __shared__ int fmx;
  const int tid = threadIdx.x, NT = blockDim.x;
  const int lane = tid & (WAVE - 1), wave = tid / WAVE, nw = NT / WAVE;
  const int L = a.L, hl = a.head_len;
  for (int q = blockIdx.x; q < a.n_order; q += gridDim.x) {
    const int bi = a.order[q];
    const unsigned long long s0 = s.row_off[bi], s1 = s.row_off[bi + 1];
    if (s0 == s1) continue;
    const int st0 = a.status[bi];
    const double pg = EXT ? a.xtot[bi] : a.gprob[bi];
    const bool resolved = (st0 == EST_OK || st0 == EST_OK_PRUNED) && pg > 0.0 && !isinf(pg);
    const unsigned long long *roff = a.rec_off + (size_t)bi * (L + 1);
    const unsigned long long *xo = a.x_off + (size_t)bi * (L + 1);
    // the individual's largest record (block-uniform after the barrier)
    int fbig = 0;
    if (resolved) {
      __syncthreads();  // every thread has read the previous individual's maximum
      if (tid == 0) fmx = 0;
      __syncthreads();
      int f = 0;
      for (int j = hl + tid; j <= L; j += NT) f = max(f, (int)a.rec[roff[j]]);
      atomicMax(&fmx, f);
      __syncthreads();
      fbig = fmx;
    }
    const bool in_lds = fbig <= s.tier && fbig <= s.lds_states;
    // (a frontier neither store holds cannot occur: the host sizes the scratch from the group's fmax)
    const bool fits = in_lds || (s.scratch && fbig <= s.scratch_states);
    if (!resolved || (!EXT && pg < SITE_PG_MIN) || !fits) {  // rows of zeros: unresolved (1), or P(genotype) subnormal (2)
      for (unsigned long long i = s0 * 2 + tid; i < s1 * 2; i += NT) s.post[i] = 0.0;
      for (unsigned long long i = s0 + tid; i < s1; i += NT) s.row_status[i] = resolved && fits ? 2 : 1;
      continue;
    }
    const size_t cap = in_lds ? (size_t)s.lds_states : (size_t)s.scratch_states;
    double *cur = in_lds ? pr_lds : s.scratch + (size_t)blockIdx.x * 4 * NS * cap;
    double *prev = cur + 2 * NS * cap;
    int sc = EXT ? 0 : -ilogb(pg), sa = sc / 2, sb = sc - sa;
    const double pgs = EXT ? pg : ldexp(pg, sc);
    const int EL = EXT ? a.xtot_exp[bi] : 0;
    // the exponents exact_fb left with record j (EXT): E_j, G_j
    auto rec_exp = [&](int j) { return (const int32_t *)(a.x + xo[j] + 4ull * a.rec[roff[j]]); };
    // o(t): the side of state t of record j that carries the lower allele of locus k
    // (k < head_len: j is the head record; its hdr word carries locus 0 when head_len is 1)
    auto low_side = [&](const RecView &R, int k, int t) -> int {
      uint32_t xa, xb;
      if (k < hl && hl > 1) {
        const uint32_t *plo = R.cb + R.F + 1, *phi = plo + R.F;
        xa = a.head_al[(size_t)plo[t] * hl + k];
        xb = a.head_al[(size_t)phi[t] * hl + k];
      } else {
        const uint32_t h = R.hdr[t];
        xa = h & 0xFFu;
        xb = (h >> 8) & 0xFFu;
      }
      return xa < xb ? 0 : 1;
    };
    __syncthreads();  // the previous individual's last readers of the frontiers are done
    const unsigned long long e0 = s.ev_off[bi], e1 = s.ev_off[bi + 1];
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
        double *x = prev;
        prev = cur;
        cur = x;
        const RecView R(a.rec + roff[j], false);
        const int step = EXT ? rec_exp(j)[0] - rec_exp(j - 1)[0] : 0;
        for (int t = tid; t < R.F; t += NT) {
          const double tpv = R.tpv[t];
          double n0[NS], n1[NS];
#pragma unroll
          for (int u = 0; u < NS; ++u) n0[u] = n1[u] = 0.0;
          const uint32_t r0 = R.cb[t], r1 = R.cb[t + 1];
          for (uint32_t r = r0; r < r1; ++r) {
            const uint32_t w = R.ct[r];
            const bool rv = cw_rev(w);
            const double2 *p = (const double2 *)(prev + (size_t)cw_state(w) * 2 * NS);
#pragma unroll
            for (int u = 0; u < NS; ++u)
              if ((live >> u) & 1u) {
                const double2 g = p[u];
                const double v0 = (rv ? g.y : g.x) * tpv, v1 = (rv ? g.x : g.y) * tpv;
                n0[u] = r == r0 ? v0 : n0[u] + v0;
                n1[u] = r == r0 ? v1 : n1[u] + v1;
              }
          }
          double2 *o = (double2 *)(cur + (size_t)t * 2 * NS);
#pragma unroll
          for (int u = 0; u < NS; ++u)
            if ((live >> u) & 1u) o[u] = EXT ? make_double2(ldexp(n0[u], step), ldexp(n1[u], step)) : make_double2(n0[u], n1[u]);
        }
        __syncthreads();
        unread = false;
      }
      const RecView R(a.rec + roff[j], j == hl);
      if (kind == PAIR_EV_EVAL) {
        if (!((live >> slot) & 1u) || ev.row < 0 || s0 + (unsigned long long)ev.row >= s1) continue;  // (none such)
        const unsigned long long row = s0 + (unsigned long long)ev.row;
        const double *bw = (const double *)(a.x + xo[j]) + R.F;
        if constexpr (EXT) {
          sc = EL - rec_exp(j)[0] - rec_exp(j)[1];
          sa = sc / 2;
          sb = sc - sa;
        }
        for (int w = wave; w < 2; w += nw) {  // wave-uniform: 0 cis, 1 trans
          double part[1] = {0.0};
          for (int t = lane; t < R.F; t += WAVE)
            part[0] += ldexp(cur[((size_t)t * NS + slot) * 2 + (low_side(R, ev.locus, t) ^ w)], sa) * ldexp(bw[t], sb);
          const double v = group_sum_fixed<WAVE>(part) / pgs;
          if (lane == 0) s.post[row * 2 + w] = v;
        }
        if (tid == 0) s.row_status[row] = 0;
        unread = true;
      } else if (kind == PAIR_EV_FREE) {
        live &= ~(1u << slot);
      } else if (kind == PAIR_EV_ANCHOR) {
        if (unread) __syncthreads();  // the sums have read the slot this anchor overwrites
        const double *fw = (const double *)(a.x + xo[j]);
        for (int t = tid; t < R.F; t += NT) {
          const int o = low_side(R, ev.locus, t);
          double *g = cur + ((size_t)t * NS + slot) * 2;
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
  __shared__ int fmx;
  __shared__ double s_sum[PAIR_SLOTS_MAX][2];  // S_0, S_1 of the evaluations not yet written out
  __shared__ int s_col[PAIR_SLOTS_MAX];        // their patterns
  const int tid = threadIdx.x, NT = blockDim.x;
  const int lane = tid & (WAVE - 1), wave = tid / WAVE, nw = NT / WAVE;
  const int L = a.L, hl = a.head_len, P = s.n_patterns, ML = s.maxlen;
  for (int q = blockIdx.x; q < a.n_order; q += gridDim.x) {
    const int bi = a.order[q];
    double *out = s.dosage + (size_t)q * P;
    const int st0 = a.status[bi];
    const double pg = EXT ? a.xtot[bi] : a.gprob[bi];
    const bool resolved = (st0 == EST_OK || st0 == EST_OK_PRUNED) && pg > 0.0 && !isinf(pg);
    const unsigned long long *roff = a.rec_off + (size_t)bi * (L + 1);
    const unsigned long long *xo = a.x_off + (size_t)bi * (L + 1);
    // the individual's largest record (block-uniform after the barrier)
    int fbig = 0;
    if (resolved) {
      __syncthreads();  // every thread has read the previous individual's maximum
      if (tid == 0) fmx = 0;
      __syncthreads();
      int f = 0;
      for (int j = hl + tid; j <= L; j += NT) f = max(f, (int)a.rec[roff[j]]);
      atomicMax(&fmx, f);
      __syncthreads();
      fbig = fmx;
    }
    const bool in_lds = fbig <= s.tier && fbig <= s.lds_states;
    // (a frontier neither store holds cannot occur: the host sizes the scratch from the group's fmax)
    const bool fits = in_lds || (s.scratch && fbig <= s.scratch_states);
    if (!resolved || (!EXT && pg < SITE_PG_MIN) || !fits) {  // a row of zeros: unresolved (1), or P(genotype) subnormal (2)
      for (int i = tid; i < P; i += NT) out[i] = 0.0;
      if (tid == 0) s.status[q] = resolved && fits ? 2 : 1;
      continue;
    }
    const size_t cap = in_lds ? (size_t)s.lds_states : (size_t)s.scratch_states;
    double *cur = in_lds ? ds_lds : s.scratch + (size_t)blockIdx.x * 4 * NS * cap;
    double *prev = cur + 2 * NS * cap;
    int sc = EXT ? 0 : -ilogb(pg), sa = sc / 2, sb = sc - sa;
    const double pgs = EXT ? pg : ldexp(pg, sc);
    const int EL = EXT ? a.xtot_exp[bi] : 0;
    // the exponents exact_fb left with record j (EXT): E_j, G_j
    auto rec_exp = [&](int j) { return (const int32_t *)(a.x + xo[j] + 4ull * a.rec[roff[j]]); };
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
      if (tid < NS && ((pend >> tid) & 1u)) out[s_col[tid]] = (s_sum[tid][0] + s_sum[tid][1]) / pgs;
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
        double *x = prev;
        prev = cur;
        cur = x;
        const RecView R(a.rec + roff[j], false);
        const int step = EXT ? rec_exp(j)[0] - rec_exp(j - 1)[0] : 0;
        uint32_t ca[NS], cb[NS];  // the live slots' codes of locus j - 1
#pragma unroll
        for (int u = 0; u < NS; ++u) {
          const bool on = (live >> u) & 1u;
          ca[u] = on ? s.codes[cbase[u] + (j - 1)] : DOSE_ABSENT;
          cb[u] = on ? s.codes[cbase[u] + ML + (j - 1)] : DOSE_ABSENT;
        }
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
      const RecView R(a.rec + roff[j], j == hl);
      if (kind == DOSE_EV_EVAL) {
        if (!((live >> slot) & 1u)) continue;  // (none such)
        const double *bw = (const double *)(a.x + xo[j]) + R.F;
        if constexpr (EXT) {
          sc = EL - rec_exp(j)[0] - rec_exp(j)[1];
          sa = sc / 2;
          sb = sc - sa;
        }
        for (int w = wave; w < 2; w += nw) {  // wave-uniform: S_0, S_1
          double part[1] = {0.0};
          for (int t = lane; t < R.F; t += WAVE) part[0] += ldexp(cur[((size_t)t * NS + slot) * 2 + w], sa) * ldexp(bw[t], sb);
          const double v = group_sum_fixed<WAVE>(part);
          if (lane == 0) {
            s_sum[slot][w] = v;
            if (w == 0) s_col[slot] = ev.pat;
          }
        }
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
        const double *fw = (const double *)(a.x + xo[j]);
        const bool head = j == hl && hl > 1;  // the window's loci below head_len, from the head patterns
        const int k0 = ev.start, k1 = head ? min(ev.start + ev.len, hl) : ev.start + 1;
        const uint32_t *plo = R.cb + R.F + 1, *phi = plo + R.F;
        for (int t = tid; t < R.F; t += NT) {
          bool ok0 = true, ok1 = true;
          for (int k = k0; k < k1; ++k) {
            uint32_t xa, xb;
            if (head) {
              xa = a.head_al[(size_t)plo[t] * hl + k];
              xb = a.head_al[(size_t)phi[t] * hl + k];
            } else {
              const uint32_t h = R.hdr[t];
              xa = h & 0xFFu;
              xb = (h >> 8) & 0xFFu;
            }
            const uint32_t cA = s.codes[base + k], cB = s.codes[base + ML + k];
            ok0 = ok0 && match(xa, cA) && match(xb, cB);
            ok1 = ok1 && match(xb, cA) && match(xa, cB);
          }
          const double f = fw[t];
          double *g = cur + ((size_t)t * NS + slot) * 2;
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
    const int bi = a.order[q];
    const int st0 = a.status[bi];
    const double pg = EXT ? a.xtot[bi] : a.gprob[bi];
    const bool resolved = (st0 == EST_OK || st0 == EST_OK_PRUNED) && pg > 0.0 && !isinf(pg);
    if (!resolved || (!EXT && pg < SITE_PG_MIN)) {  // the host writes the input genotype: unresolved (1), P(genotype) subnormal (2)
      if (tid == 0 && dc == 0) s.status[q] = resolved ? 2 : 1;
      continue;
    }
    const unsigned long long *roff = a.rec_off + (size_t)bi * (L + 1);
    const unsigned long long *xo = a.x_off + (size_t)bi * (L + 1);
    const RecView RL(a.rec + roff[L], L == hl);
    const double *fwL = (const double *)(a.x + xo[L]);
    const int F = RL.F, nc = (F + WAVE - 1) / WAVE;
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
    const uint32_t pi = (uint32_t)(s.indiv0 + bi), du = (uint32_t)d;
    auto put = [&](int k, int side, uint32_t x) {
      if (s.al) s.al[(((size_t)q * 2 + side) * L + k) * D + d] = (uint8_t)x;
    };
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
    int par = 0;
    bool het = false, dead = false;
    double p = 1.0;
    int pe = 0;  // EXT: the true product is p 2^pe
    auto renorm = [&]() {
      if constexpr (EXT) {
        int e;
        p = frexp(p, &e);
        pe += e;
      }
    };
    for (int j = L; j > hl; --j) {
      const RecView R(a.rec + roff[j], false);
      const uint32_t hd = R.hdr[t], xa = hd & 0xFFu, xb = (hd >> 8) & 0xFFu;
      const uint32_t r0 = R.cb[t], r1 = R.cb[t + 1];
      const double tpv = R.tpv[t];
      const double *fp = (const double *)(a.x + xo[j - 1]);
      put(j - 1, par, xa);
      put(j - 1, par ^ 1, xb);
      het |= xa != xb;
      p = j == L ? tpv : p * tpv;
      renorm();
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
      if (cw_rev(wsel)) par ^= 1;
      t = (int)cw_state(wsel);
    }
    if (!dead) {  // the head state: loci below head_len
      const RecView H(a.rec + roff[hl], true);
      const double tpv = H.tpv[t];
      p = L == hl ? tpv : p * tpv;
      renorm();
      if (hl == 1) {
        const uint32_t hd = H.hdr[t], xa = hd & 0xFFu, xb = (hd >> 8) & 0xFFu;
        put(0, par, xa);
        put(0, par ^ 1, xb);
        het |= xa != xb;
      } else {
        const uint32_t *plo = H.cb + H.F + 1, *phi = plo + H.F;
        const uint8_t *pa = a.head_al + (size_t)plo[t] * hl, *pb = a.head_al + (size_t)phi[t] * hl;
        for (int k = 0; k < hl; ++k) {
          put(k, par, pa[k]);
          put(k, par ^ 1, pb[k]);
          het |= pa[k] != pb[k];
        }
      }
    }
    if constexpr (EXT) {
      if (s.prob) s.prob[(size_t)q * D + d] = dead ? 0.0 : ldexp((het ? p * 2.0 : p) / pg, pe + a.xtot_exp[bi]);
    } else {
      if (s.prob) s.prob[(size_t)q * D + d] = dead ? 0.0 : (het ? p * 2.0 : p) / pg;
    }
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
__device__ inline void wave_best(double &v, unsigned &k) {  // the largest v, then the lowest k, in every lane
#pragma unroll
  for (int o = WAVE / 2; o > 0; o >>= 1) {
    const double ov = __shfl_xor(v, o);
    const unsigned ok = __shfl_xor(k, o);
    if (ov > v || (ov == v && ok < k)) {
      v = ov;
      k = ok;
    }
  }
}

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

template <bool EXT>
__global__ __launch_bounds__(256) void exact_map_phase(ExactArgs a, MapArgs s) {
  __shared__ double bv[4];
  __shared__ unsigned bk[4];
  __shared__ int flag;
  const int tid = threadIdx.x, NT = blockDim.x, lane = tid & (WAVE - 1), wave = tid / WAVE, nw = NT / WAVE;
  const int L = a.L, hl = a.head_len;
  for (int q = blockIdx.x; q < a.n_order; q += gridDim.x) {  // block-uniform
    const int bi = a.order[q];
    const int st0 = a.status[bi];
    const double pg = EXT ? a.xtot[bi] : a.gprob[bi];
    const int pge = EXT ? -a.xtot_exp[bi] : 0;  // P(genotype) = pg 2^pge
    const bool resolved = (st0 == EST_OK || st0 == EST_OK_PRUNED) && pg > 0.0 && !isinf(pg);
    if (!resolved || (!EXT && pg < SITE_PG_MIN)) {  // the host writes the input genotype: unresolved (1), P(genotype) subnormal (2)
      if (tid == 0) s.status[q] = resolved ? 2 : 1;
      continue;
    }
    const unsigned long long *roff = a.rec_off + (size_t)bi * (L + 1);
    const unsigned long long *xo = a.x_off + (size_t)bi * (L + 1);
    // the sweep: raw doubles in the regular range, and again with rescaled records if those underflow
    if constexpr (EXT) {
      map_sweep<true>(a, roff, xo, &flag);
    } else {
      if (tid == 0) flag = 0;  // (every thread has read the previous individual's flag before the barrier of its final reduction)
      __syncthreads();
      map_sweep<false>(a, roff, xo, &flag);
      if (flag != 0) map_sweep<true>(a, roff, xo, &flag);  // block-uniform: read behind the sweep's last barrier
    }
    // the final record's best candidate
    const RecView RL(a.rec + roff[L], L == hl);
    const double *vL = (const double *)(a.x + xo[L]);
    double best = -1.0;
    unsigned bkey = 0xFFFFFFFFu;
    for (int t = tid; t < RL.F; t += NT) {  // ascending: strictly larger only
      const double h = vL[t], d = vL[RL.F + t];
      if (h > best) {
        best = h;
        bkey = 2u * (unsigned)t;
      }
      if (d > best) {
        best = d;
        bkey = 2u * (unsigned)t + 1u;
      }
    }
    wave_best(best, bkey);
    if (lane == 0) {
      bv[wave] = best;
      bk[wave] = bkey;
    }
    __syncthreads();
    if (wave != 0) continue;  // (wave 0 passes the next individual's barriers after its traceback)
    best = bv[0];
    bkey = bk[0];
    for (int w = 1; w < nw; ++w)
      if (bv[w] > best || (bv[w] == best && bk[w] < bkey)) {
        best = bv[w];
        bkey = bk[w];
      }
    if (!(best > 0.0)) {  // (no path with a positive product: the host writes the input genotype)
      if (lane == 0) s.status[q] = 1;
      continue;
    }
    auto put = [&](int k, int side, uint32_t x) {
      if (s.al && lane == 0) s.al[((size_t)q * 2 + side) * L + k] = (uint8_t)x;
    };
    int t = (int)(bkey >> 1);
    bool lab_d = bkey & 1u;
    int par = 0;
    bool het = false, dead = false;
    double p = 1.0;
    int pe = 0;  // the true product is p 2^pe (a raw product of a long panel's path underflows where its quotient does not)
    auto renorm = [&]() {
      int e;
      p = frexp(p, &e);
      pe += e;
    };
    for (int j = L; j > hl; --j) {  // wave-uniform
      const RecView R(a.rec + roff[j], false);
      const uint32_t hd = R.hdr[t], xa = hd & 0xFFu, xb = (hd >> 8) & 0xFFu;
      const uint32_t r0 = R.cb[t], r1 = R.cb[t + 1];
      const double tpv = R.tpv[t];
      const int Fq = (int)a.rec[roff[j - 1]];
      const double *ph = (const double *)(a.x + xo[j - 1]), *pd = ph + Fq;
      put(j - 1, par, xa);
      put(j - 1, par ^ 1, xb);
      het |= xa != xb;
      p = j == L ? tpv : p * tpv;
      renorm();
      const bool both = lab_d && xa != xb;
      double cv = -1.0;
      unsigned ck = 0xFFFFFFFFu, cw = 0u;
      for (uint32_t rb = r0; rb < r1; rb += WAVE) {  // 64 contributions at a time; an earlier batch wins a tie
        const uint32_t r = rb + (uint32_t)lane;
        double v = -1.0;
        unsigned k = 0xFFFFFFFFu;
        uint32_t w = 0u;
        if (r < r1) {
          w = R.ct[r];
          const uint32_t ps = cw_state(w);
          k = 2u * (unsigned)lane;
          if (both) {
            const double d = pd[ps], h2 = 2.0 * ph[ps];
            v = d;
            if (h2 > d) {
              v = h2;
              k += 1u;
            }
          } else {
            v = lab_d ? pd[ps] : ph[ps];
          }
        }
        wave_best(v, k);
        if (v > cv) {
          cv = v;
          ck = k;
          cw = __shfl(w, (int)(k >> 1));
        }
      }
      if (!(cv > 0.0)) {  // (a state no path reaches is never chosen; if one were, the individual counts as unresolved)
        dead = true;
        break;
      }
      if (ck & 1u) lab_d = false;
      if (cw_rev(cw)) par ^= 1;
      t = (int)cw_state(cw);
    }
    if (!dead) {  // the head state: loci below head_len
      const RecView H(a.rec + roff[hl], true);
      const double tpv = H.tpv[t];
      p = L == hl ? tpv : p * tpv;
      renorm();
      if (hl == 1) {
        const uint32_t hd = H.hdr[t], xa = hd & 0xFFu, xb = (hd >> 8) & 0xFFu;
        put(0, par, xa);
        put(0, par ^ 1, xb);
        het |= xa != xb;
      } else {
        const uint32_t *plo = H.cb + H.F + 1, *phi = plo + H.F;
        const uint8_t *pa = a.head_al + (size_t)plo[t] * hl, *pb = a.head_al + (size_t)phi[t] * hl;
        for (int k = 0; k < hl; ++k) {
          put(k, par, pa[k]);
          put(k, par ^ 1, pb[k]);
          het |= pa[k] != pb[k];
        }
      }
    }
    if (lane == 0) {
      if (dead) s.status[q] = 1;
      if (s.prob) s.prob[q] = dead ? 0.0 : ldexp((het ? p * 2.0 : p) / pg, pe - pge);
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
    const uint32_t *plo = R.cb + R.F + 1, *phi = plo + R.F;
    double m = 0.0;
    for (int t = tid; t < R.F; t += NT) {
      const uint32_t hd = R.hdr[t];
      const bool homo = (hd >> 24) & 1u;
      bool ok = true, c0 = true, c1 = true;
      for (int e = 0; e < nh; ++e) {
        const int k = ev[e].locus, code = ev[e].code;
        const uint32_t first = (uint32_t)(code >> 8);
        uint32_t xa, xb;
        if (hl == 1) {
          xa = hd & 0xFFu;
          xb = (hd >> 8) & 0xFFu;
        } else {
          xa = a.head_al[(size_t)plo[t] * hl + k];
          xb = a.head_al[(size_t)phi[t] * hl + k];
        }
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
  __shared__ double bv[4];
  __shared__ unsigned bk[4];
  __shared__ int flag;
  __shared__ double s_tot;
  const int tid = threadIdx.x, NT = blockDim.x, lane = tid & (WAVE - 1), wave = tid / WAVE, nw = NT / WAVE;
  const int L = a.L, hl = a.head_len;
  for (int q = blockIdx.x; q < a.n_order; q += gridDim.x) {  // block-uniform
    const int bi = a.order[q];
    const int st0 = a.status[bi];
    const double pg = EXT ? a.xtot[bi] : a.gprob[bi];
    const int pge = EXT ? -a.xtot_exp[bi] : 0;  // P(genotype) = pg 2^pge
    const bool resolved = (st0 == EST_OK || st0 == EST_OK_PRUNED) && pg > 0.0 && !isinf(pg);
    if (!resolved || (!EXT && pg < SITE_PG_MIN)) {  // as exact_map_phase: unresolved (1), P(genotype) subnormal (2)
      if (tid == 0) s.status[q] = resolved ? 2 : 1;
      continue;
    }
    const unsigned long long *roff = a.rec_off + (size_t)bi * (L + 1);
    const unsigned long long *xo = a.x_off + (size_t)bi * (L + 1);
    const GivenEvent *ev = s.ev + s.ev_off[bi];
    const int ne = (int)(s.ev_off[bi + 1] - s.ev_off[bi]);
    // the sums: P(evidence and genotype) = tot 2^-es
    bool top = false;
    const int es = given_sweep<true, true>(a, roff, xo, ev, ne, &flag, top);
    if (tid == 0) {  // in state order from 0.0, as exact_fb sums its divisor
      const int F = (int)a.rec[roff[L]];
      const double *v = (const double *)(a.x + xo[L]);
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
      given_sweep<false, true>(a, roff, xo, ev, ne, &flag, top);
    } else {
      if (tid == 0) flag = 0;
      __syncthreads();
      given_sweep<false, false>(a, roff, xo, ev, ne, &flag, top);
      if (flag != 0) given_sweep<false, true>(a, roff, xo, ev, ne, &flag, top);  // block-uniform: read behind the sweep's last barrier
    }
    auto kind = [&](int j) { return ((const int32_t *)(a.x + xo[j] + 4ull * a.rec[roff[j]]))[1]; };
    // the final record's best candidate
    const RecView RL(a.rec + roff[L], L == hl);
    const double *vL = (const double *)(a.x + xo[L]);
    double best = -1.0;
    unsigned bkey = 0xFFFFFFFFu;
    for (int t = tid; t < RL.F; t += NT) {  // ascending: strictly larger only
      const double h = vL[t], d = vL[RL.F + t];
      if (h > best) {
        best = h;
        bkey = 2u * (unsigned)t;
      }
      if (d > best) {
        best = d;
        bkey = 2u * (unsigned)t + 1u;
      }
    }
    wave_best(best, bkey);
    if (lane == 0) {
      bv[wave] = best;
      bk[wave] = bkey;
    }
    __syncthreads();
    if (wave != 0) continue;  // (wave 0 passes the next individual's barriers after its traceback)
    best = bv[0];
    bkey = bk[0];
    for (int w = 1; w < nw; ++w)
      if (bv[w] > best || (bv[w] == best && bk[w] < bkey)) {
        best = bv[w];
        bkey = bk[w];
      }
    if (!(best > 0.0)) {  // (the sums found a path, so the maxima do)
      if (lane == 0) s.status[q] = 1;
      continue;
    }
    auto put = [&](int k, int side, uint32_t x) {
      if (s.al && lane == 0) s.al[((size_t)q * 2 + side) * L + k] = (uint8_t)x;
    };
    int t = (int)(bkey >> 1);
    unsigned lab = bkey & 1u;  // plain record: h = 0, d = 1; span record: c
    int par = 0;
    bool het = false, dead = false;
    double p = 1.0;
    int pe = 0;  // the true product is p 2^pe
    auto renorm = [&]() {
      int e;
      p = frexp(p, &e);
      pe += e;
    };
    for (int j = L; j > hl; --j) {  // wave-uniform
      const RecView R(a.rec + roff[j], false);
      const uint32_t hd = R.hdr[t], xa = hd & 0xFFu, xb = (hd >> 8) & 0xFFu;
      const uint32_t r0 = R.cb[t], r1 = R.cb[t + 1];
      const double tpv = R.tpv[t];
      const int Fq = (int)a.rec[roff[j - 1]];
      const double *p0 = (const double *)(a.x + xo[j - 1]), *p1 = p0 + Fq;
      const int kj = kind(j);
      const bool cont = kj & 2, labels = kj & 1, below = kind(j - 1) & 1;
      put(j - 1, par, xa);
      put(j - 1, par ^ 1, xb);
      het |= xa != xb;
      p = j == L ? tpv : p * tpv;
      renorm();
      // 0 inside; 1 over a span record; 2 Vd' then 2 Vh'; 3 the label's own value
      const int mode = cont ? 0 : below ? 1 : (labels || (lab == 1u && xa != xb)) ? 2 : 3;
      double cv = -1.0;
      unsigned ck = 0xFFFFFFFFu, cw = 0u;
      for (uint32_t rb = r0; rb < r1; rb += WAVE) {  // 64 contributions at a time; an earlier batch wins a tie
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
      if (!(cv > 0.0)) {  // (a state no path reaches is never chosen; if one were, the individual counts as unresolved)
        dead = true;
        break;
      }
      if (mode == 0) lab ^= cw_rev(cw) ? 1u : 0u;
      else if (mode == 1) lab = ck & 1u;
      else if (mode == 2) lab = (ck & 1u) ? 0u : 1u;
      if (cw_rev(cw)) par ^= 1;
      t = (int)cw_state(cw);
    }
    if (!dead) {  // the head state: loci below head_len
      const RecView H(a.rec + roff[hl], true);
      const double tpv = H.tpv[t];
      p = L == hl ? tpv : p * tpv;
      renorm();
      if (hl == 1) {
        const uint32_t hd = H.hdr[t], xa = hd & 0xFFu, xb = (hd >> 8) & 0xFFu;
        put(0, par, xa);
        put(0, par ^ 1, xb);
        het |= xa != xb;
      } else {
        const uint32_t *plo = H.cb + H.F + 1, *phi = plo + H.F;
        const uint8_t *pa = a.head_al + (size_t)plo[t] * hl, *pb = a.head_al + (size_t)phi[t] * hl;
        for (int k = 0; k < hl; ++k) {
          put(k, par, pa[k]);
          put(k, par ^ 1, pb[k]);
          het |= pa[k] != pb[k];
        }
      }
    }
    if (lane == 0) {
      if (dead) s.status[q] = 1;
      if (s.prob) s.prob[q] = dead ? 0.0 : ldexp((het ? p * 2.0 : p) / pg, pe - pge);
      if (s.evidence) {
        int ge;
        const double gm = frexp(pg, &ge);
        s.evidence[q] = dead ? 0.0 : ldexp(tot / gm, -es - pge - ge);
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
    const int bi = a.order[q];
    const int st0 = a.status[bi];
    const double pg = EXT ? a.xtot[bi] : a.gprob[bi];
    const int pge = EXT ? -a.xtot_exp[bi] : 0;  // P(genotype) = pg 2^pge
    const bool resolved = (st0 == EST_OK || st0 == EST_OK_PRUNED) && pg > 0.0 && !isinf(pg);
    if (!resolved || (!EXT && pg < SITE_PG_MIN)) {  // the host writes the input genotype: unresolved (1), P(genotype) subnormal (2)
      if (tid == 0) s.status[q] = resolved ? 2 : 1;
      continue;
    }
    const unsigned long long *roff = a.rec_off + (size_t)bi * (L + 1);
    const unsigned long long *xo = a.x_off + (size_t)bi * (L + 1);
    uint8_t *base = s.store + s.store_base[q];
    // ---- the sweep -------------------------------------------------------
    int ex = 0;
    {
      const RecView R(a.rec + roff[hl], true);
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
      const RecView R(a.rec + roff[j], false);
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
    const RecView RL(a.rec + roff[L], L == hl);
    const double *vL = (const double *)(base + rank_rec_offset(xo, hl, L, KL));
    double pv = 0.0;
    unsigned pk = 0u, rowk = 0u;
    int cnt = 0;
    for (int r = 0; r < K; ++r) {  // block-uniform
      double best = -1.0;
      unsigned bkey = 0xFFFFFFFFu;
      for (int t = tid; t < RL.F; t += NT) {  // keys ascending: strictly larger only
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
    auto put = [&](int locus, int side, uint32_t x) {
      if (s.al) s.al[(((size_t)q * 2 + side) * L + locus) * K + lane] = (uint8_t)x;
    };
    int t = (int)(rowk / (2u * KL));
    uint32_t lab = (rowk / KL) & 1u, rk = rowk % KL;
    int par = 0;
    bool het = false, dead = false;
    double p = 1.0;
    int pe = 0;  // the true product is p 2^pe
    auto renorm = [&]() {
      int e;
      p = frexp(p, &e);
      pe += e;
    };
    for (int j = L; mine && j > hl; --j) {
      const RecView R(a.rec + roff[j], false);
      const uint32_t hd = R.hdr[t], xa = hd & 0xFFu, xb = (hd >> 8) & 0xFFu;
      const uint32_t r0 = R.cb[t], r1 = R.cb[t + 1];
      const double tpv = R.tpv[t];
      put(j - 1, par, xa);
      put(j - 1, par ^ 1, xb);
      het |= xa != xb;
      p = j == L ? tpv : p * tpv;
      renorm();
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
      if (cw_rev(w)) par ^= 1;
      t = (int)cw_state(w);
    }
    if (mine && !dead) {  // the head state: loci below head_len
      const RecView H(a.rec + roff[hl], true);
      const double tpv = H.tpv[t];
      p = L == hl ? tpv : p * tpv;
      renorm();
      if (hl == 1) {
        const uint32_t hd = H.hdr[t], xa = hd & 0xFFu, xb = (hd >> 8) & 0xFFu;
        put(0, par, xa);
        put(0, par ^ 1, xb);
        het |= xa != xb;
      } else {
        const uint32_t *plo = H.cb + H.F + 1, *phi = plo + H.F;
        const uint8_t *pa = a.head_al + (size_t)plo[t] * hl, *pb = a.head_al + (size_t)phi[t] * hl;
        for (int k = 0; k < hl; ++k) {
          put(k, par, pa[k]);
          put(k, par ^ 1, pb[k]);
          het |= pa[k] != pb[k];
        }
      }
    }
    if (mine && s.prob) s.prob[(size_t)q * K + lane] = dead ? 0.0 : ldexp((het ? p * 2.0 : p) / pg, pe - pge);
  }
}

// total states of the records of every individual of the group (what sizes its list store)
__global__ void exact_state_totals(ExactArgs a, unsigned long long *total) {
  const int q = blockIdx.x * blockDim.x + threadIdx.x;
  if (q >= a.n_order) return;
  const int bi = a.order[q], L = a.L, hl = a.head_len;
  const int st0 = a.status[bi];
  if (st0 != EST_OK && st0 != EST_OK_PRUNED) {  // (exact_fb laid out no x_off: the kernel leaves the individual at once)
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

}  // namespace hmc
