// exact_dev.hpp — device code shared by the exact M-step (exact.hip) and the
// posterior queries (exact_query.hip).  Device-only: include from .hip files.
// First what both use (group_sum_fixed, RecView, rescale_record, wave_best),
// then the pieces the query kernels are built from.
#pragma once
#include "hmc_internal.hpp"
#include "exact.hpp"

namespace hmc {

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
  // head record only: behind cb[F + 1] come the states' two head patterns (a side, b side)
  __device__ const uint32_t *plo() const { return ct; }
  __device__ const uint32_t *phi() const { return ct + F; }
};

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

// the largest v, then the lowest k, in every lane
__device__ inline void wave_best(double &v, unsigned &k) {
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


// ---- what the posterior queries share -------------------------------------
// Each piece exists once; DESIGN.md ("The query kernels' shared device code")
// says which kernel uses which.  Helpers that hold a barrier or static LDS say
// so: every thread of the block calls them, under block-uniform control flow.

// The two alleles (a side, b side) of state t of record R at locus k.  head: R
// is the head record and holds several loci (head_len > 1), so they come from
// the state's two head patterns; else from the state's hdr word, which carries
// the record's own locus (locus 0 in a head record of head_len 1).
__device__ inline void state_alleles(const ExactArgs &a, const RecView &R, bool head, int k, int t, uint32_t &xa, uint32_t &xb) {
  if (head) {
    xa = a.head_al[(size_t)R.plo()[t] * a.head_len + k];
    xb = a.head_al[(size_t)R.phi()[t] * a.head_len + k];
  } else {
    const uint32_t h = R.hdr[t];
    xa = h & 0xFFu;
    xb = (h >> 8) & 0xFFu;
  }
}

// o(t): the side of state t of record R that carries the lower allele of locus k
// (k < head_len: R is the head record)
__device__ inline int low_side(const ExactArgs &a, const RecView &R, int k, int t) {
  uint32_t xa, xb;
  state_alleles(a, R, k < a.head_len && a.head_len > 1, k, t, xa, xb);
  return xa < xb ? 0 : 1;
}

// exact_fb lays out the x-store of an individual (and the queries may read its
// records) only under these E-step statuses
__device__ inline bool fb_laid_out(int st0) { return st0 == EST_OK || st0 == EST_OK_PRUNED; }

// One individual of a query launch: its divisor, the rule that gives it up, its
// records and its x-store.  EXT (ExactArgs::extended): P(genotype) = pg 2^pge
// from exact_fb's scaled total; else the E-step's raw double, pge = 0.
template <bool EXT>
struct QueryInd {
  const ExactArgs &a;
  int bi, st0, pge;
  double pg;
  const unsigned long long *roff, *xo;
  __device__ QueryInd(const ExactArgs &a_, int q) : a(a_), bi(a_.order[q]) {
    st0 = a.status[bi];
    pg = EXT ? a.xtot[bi] : a.gprob[bi];
    pge = EXT ? -a.xtot_exp[bi] : 0;
    roff = a.rec_off + (size_t)bi * (a.L + 1);
    xo = a.x_off + (size_t)bi * (a.L + 1);
  }
  __device__ bool resolved() const { return fb_laid_out(st0) && pg > 0.0 && !isinf(pg); }
  // 0 to go on; else the status of the individual's rows: 1 unresolved, 2 P(genotype)
  // subnormal (regular range only: its likelihoods have lost their bits)
  __device__ int give_up_status() const { return !resolved() ? 1 : (!EXT && pg < SITE_PG_MIN) ? 2 : 0; }
  __device__ int F(int j) const { return (int)a.rec[roff[j]]; }
  __device__ RecView rec(int j) const { return RecView(a.rec + roff[j], j == a.head_len); }
  __device__ double *fwd(int j) const { return (double *)(a.x + xo[j]); }
  __device__ double *bwd(int j) const { return fwd(j) + F(j); }
  // the two int32 words behind record j's 2 F values: exact_fb's E_j, G_j; the
  // sweeps' cumulative exponent and record kind
  __device__ int32_t *spare(int j) const { return (int32_t *)(a.x + xo[j] + 4ull * a.rec[roff[j]]); }
};

// The individual's largest record and the store of its two frontiers (current
// and previous record, `per_state` doubles per state each): LDS when the largest
// record has at most lds_limit states, else the block's slice of a device
// scratch — the same doubles in the same order.  lds_cap / scratch_states: the
// states each store was sized for.  !fits: neither holds the frontier (cannot
// occur: the host sizes the scratch from the group's fmax).
// Three barriers when `resolved` (block-uniform) and static LDS: every thread
// of the block constructs it.
struct FrontierStore {
  double *cur, *prev;
  bool fits;
  __device__ FrontierStore(const ExactArgs &a, const unsigned long long *roff, bool resolved, double *lds, int lds_limit,
                           int lds_cap, double *scratch, int scratch_states, int per_state) {
    __shared__ int fmx;
    const int tid = threadIdx.x, NT = blockDim.x;
    int fbig = 0;  // block-uniform after the barrier
    if (resolved) {
      __syncthreads();  // every thread has read the previous individual's maximum
      if (tid == 0) fmx = 0;
      __syncthreads();
      int f = 0;
      for (int j = a.head_len + tid; j <= a.L; j += NT) f = max(f, (int)a.rec[roff[j]]);
      atomicMax(&fmx, f);
      __syncthreads();
      fbig = fmx;
    }
    const bool in_lds = fbig <= lds_limit;
    fits = in_lds || (scratch && fbig <= scratch_states);
    cur = prev = nullptr;
    if (fits) {  // (no arithmetic on a scratch that is not there)
      const size_t cap = in_lds ? (size_t)lds_cap : (size_t)scratch_states;
      cur = in_lds ? lds : scratch + (size_t)blockIdx.x * 2 * per_state * cap;
      prev = cur + per_state * cap;
    }
  }
  __device__ void swap() {
    double *x = prev;
    prev = cur;
    cur = x;
  }
};

// fwd * bwd / P(genotype) without underflow: on long panels P(genotype) is tiny
// and a product of two normal numbers would be subnormal or 0, so both factors
// and the divisor are scaled by powers of two that cancel (fwd * bwd <=
// P(genotype): nothing overflows).  Exact, so wherever the plain formula stays
// in the normal range this gives its bits.  Regular range: sc = -ilogb(pg) split
// in two, the divisor pgs = pg 2^sc.  EXT: the x-store holds exact_fb's scaled
// values, the divisor is the scaled total, and the split is per record
// (at_record): sc = E_L - E_j - G_j, since the sum over a record of
// fs bs 2^(E_L - E_j - G_j) is xtot.
template <bool EXT>
struct PowScale {
  int sa, sb;
  double pgs;
  __device__ explicit PowScale(const QueryInd<EXT> &ind) {
    const int sc = EXT ? 0 : -ilogb(ind.pg);
    sa = sc / 2;
    sb = sc - sa;
    pgs = EXT ? ind.pg : ldexp(ind.pg, sc);
  }
  // ex: the record's spare words E_j, G_j (QueryInd::spare(j), or formed from what the caller holds)
  __device__ void at_record(const QueryInd<EXT> &ind, const int32_t *ex) {
    if constexpr (EXT) {
      const int sc = -ind.pge - ex[0] - ex[1];
      sa = sc / 2;
      sb = sc - sa;
    }
  }
  __device__ double term(double f, double b) const { return ldexp(f, sa) * ldexp(b, sb); }
  // One label's sum by the calling wavefront, in label_sums' order: lane l adds
  // term(g(t), bw[t]) over the states l, l + 64, ... ascending, then the fixed
  // butterfly; every lane gets the sum.  No barrier.
  template <class G>
  __device__ double ordered_sum(int F, const double *bw, G g) const {
    const int lane = threadIdx.x & (WAVE - 1);
    double part[1] = {0.0};
    for (int t = lane; t < F; t += WAVE) part[0] += term(g(t), bw[t]);
    return group_sum_fixed<WAVE>(part);
  }
  // The two-wave evaluation: wavefront 0 owns label 0, wavefront 1 label 1 (a
  // block of one wave takes both in turn); lane l adds term(g(t, label), bw[t])
  // over the states l, l + 64, ... ascending, then the fixed butterfly; lane 0
  // hands the sum to out(label, sum).  No barrier.
  template <class G, class O>
  __device__ void label_sums(int F, const double *bw, G g, O out) const {
    const int lane = threadIdx.x & (WAVE - 1), wave = threadIdx.x / WAVE, nw = blockDim.x / WAVE;
    for (int w = wave; w < 2; w += nw) {  // wave-uniform
      double part[1] = {0.0};
      for (int t = lane; t < F; t += WAVE) part[0] += term(g(t, w), bw[t]);
      const double v = group_sum_fixed<WAVE>(part);
      if (lane == 0) out(w, v);
    }
  }
};

struct LabelPair8 {  // a state's two labels where the frontier is only 8-byte aligned (the switch sweep's LDS)
  double x, y;
};

// The labelled propagate step: frontier `cur` of record R from `prev` of the
// record below, NS slots of two labels per state.  Over state t's contributions
// r in stored order g'[c ^ rev(r)][t] += g[c][state(r)] * tpv[t]: a reversed
// link moves the a-side haplotype to the b side; the first term assigns, later
// ones add, as exact_fb's forward does.  EXT: times 2^step, the exponent step
// exact_fb applied to the forward values of this record.
// live: the slots that hold something; dead ones are neither read nor written.
// V: the load and store unit of a slot's two labels.  Contribution words and
// tpv[t] are read once per state for all slots.  Ends on a barrier.
// (exact_haplotype_dosages keeps this step with its match masks in its own loop.)
template <int NS, bool EXT, class V>
__device__ inline void propagate_labels(const RecView &R, const double *prev, double *cur, int step, unsigned live) {
  for (int t = threadIdx.x; t < R.F; t += blockDim.x) {
    const double tpv = R.tpv[t];
    double n0[NS], n1[NS];
#pragma unroll
    for (int u = 0; u < NS; ++u) n0[u] = n1[u] = 0.0;
    const uint32_t r0 = R.cb[t], r1 = R.cb[t + 1];
    for (uint32_t r = r0; r < r1; ++r) {
      const uint32_t w = R.ct[r];
      const bool rv = cw_rev(w);
      const V *p = (const V *)(prev + (size_t)cw_state(w) * 2 * NS);
#pragma unroll
      for (int u = 0; u < NS; ++u)
        if ((live >> u) & 1u) {
          const V g = p[u];
          const double v0 = (rv ? g.y : g.x) * tpv, v1 = (rv ? g.x : g.y) * tpv;
          n0[u] = r == r0 ? v0 : n0[u] + v0;
          n1[u] = r == r0 ? v1 : n1[u] + v1;
        }
    }
    V *o = (V *)(cur + (size_t)t * 2 * NS);
#pragma unroll
    for (int u = 0; u < NS; ++u)
      if ((live >> u) & 1u) {
        V g;
        g.x = EXT ? ldexp(n0[u], step) : n0[u];
        g.y = EXT ? ldexp(n1[u], step) : n1[u];
        o[u] = g;
      }
  }
  __syncthreads();
}

// A traced path spelled as a haplotype pair, and its probability.  Allele x of
// locus k on side `side` goes to al[((q * 2 + side) * L + k) * stride + column]
// when `write` holds: the draws' ... * D + d, MAP's row of lane 0 (stride 1),
// the ranked ... * K + lane.  The a side parity `par` is flipped by a chosen
// contribution's rev flag after the state's two alleles are written
// (estep_traceback's rule).  The product of the path's tpv runs from record L
// down to the head.  RENORM: kept as mantissa p in [0.5, 1) and power-of-two
// count pe (frexp: exact), since a raw product of a long panel's path underflows
// where its quotient does not; else raw doubles (the draws' regular range).
template <bool RENORM>
struct PathSpeller {
  uint8_t *al;
  size_t q, stride, column;
  bool write;
  int L, par = 0, pe = 0;
  bool het = false;
  double p = 1.0;
  __device__ PathSpeller(uint8_t *al_, size_t q_, int L_, size_t stride_, size_t column_, bool write_)
      : al(al_), q(q_), stride(stride_), column(column_), write(write_), L(L_) {}
  __device__ void put(int k, int side, uint32_t x) const {
    if (write) al[((q * 2 + side) * L + k) * stride + column] = (uint8_t)x;
  }
  __device__ void times(double tpv, bool first) {
    p = first ? tpv : p * tpv;
    if constexpr (RENORM) {
      int e;
      p = frexp(p, &e);
      pe += e;
    }
  }
  __device__ void spell(int k, uint32_t xa, uint32_t xb) {
    put(k, par, xa);
    put(k, par ^ 1, xb);
    het |= xa != xb;
  }
  // state t of record j > head_len: the alleles of locus j - 1 and the state's tpv
  __device__ void enter(const RecView &R, int j, int t) {
    const uint32_t hd = R.hdr[t];
    spell(j - 1, hd & 0xFFu, (hd >> 8) & 0xFFu);
    times(R.tpv[t], j == L);
  }
  // the path went over contribution word w to the record below
  __device__ void follow(uint32_t w) {
    if (cw_rev(w)) par ^= 1;
  }
  // the head state t of head record H: its tpv and the loci below head_len
  __device__ void head(const ExactArgs &a, const RecView &H, int t) {
    times(H.tpv[t], L == a.head_len);
    for (int k = 0; k < a.head_len; ++k) {
      uint32_t xa, xb;
      state_alleles(a, H, a.head_len > 1, k, t, xa, xb);
      spell(k, xa, xb);
    }
  }
  // (the product, doubled if the two haplotypes differ) / P(genotype), P(genotype) = pg 2^pge
  __device__ double prob(double pg, int pge) const {
    const double v = (het ? p * 2.0 : p) / pg;
    if constexpr (RENORM) return ldexp(v, pe - pge);
    else return v;
  }
};

// The best candidate of a record of 2 F values v[label][t], index 2 t + label:
// the largest value, among equals the lowest index — a rule, so that neither
// the block size nor the reduction order enters.  Every wave gets the answer.
// One barrier and static LDS: every thread of the block calls it; the LDS is
// rewritten by the next call only, so whatever barrier the caller passes before
// then protects wave 0's reads.
__device__ inline void block_best_candidate(const double *v, int F, double &best, unsigned &bkey) {
  __shared__ double bv[4];
  __shared__ unsigned bk[4];
  const int tid = threadIdx.x, NT = blockDim.x, lane = tid & (WAVE - 1), wave = tid / WAVE, nw = NT / WAVE;
  best = -1.0;
  bkey = 0xFFFFFFFFu;
  for (int t = tid; t < F; t += NT) {  // ascending: strictly larger only
    const double h = v[t], d = v[F + t];
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
  best = bv[0];
  bkey = bk[0];
  for (int w = 1; w < nw; ++w)
    if (bv[w] > best || (bv[w] == best && bk[w] < bkey)) {
      best = bv[w];
      bkey = bk[w];
    }
}

}  // namespace hmc
