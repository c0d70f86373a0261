// coop_select.hpp — the libstdc++ (GCC 11) std::nth_element of select.hpp,
// run by a wavefront on several lists at once.  The wave is cut into
// segments of SW = 2S lanes; segment g holds one list, element k in lane
// g*SW + k.  Every step is evaluated for all segments together with ballots,
// lane shuffles and small LDS exchanges, and produces exactly the element
// permutation of the sequential algorithm (select.hpp).
//
// Partition (std::__unguarded_partition, stl_algo.h:1878-1896; comp =
// greater, pivot at `first`): the left scan stops at positions p in
// [first+1,last) with !(v[p] > pivot) ("left stops"), the right scan at p in
// [first,last) with !(pivot > v[p]) ("right stops"; `first` itself is one).
// Let l_k be the k-th left stop from the left and r_k the k-th right stop
// from the right, on the values the partition starts from.  A swapped value
// is only met again where the scans cross, and there it stops the scan at once
// (a value moved right came from a left stop and vice versa), so the loop
// swaps l_k <-> r_k exactly for the k with l_k < r_k — a prefix k < K, both
// sequences being monotone — and returns cut = min(l_K, r_{K-1}) (r_{-1} =
// infinity).  No position takes part in two swaps.  Each segment therefore
// numbers its stops (ballot + popcount), the stops publish their positions in
// two small LDS arrays, and every stop reads its partner: one shuffle then
// moves all swapped elements.
//
// Which stops swap follows from the stop counts alone, before any position is
// published.  With Lw / Rw the stop masks, kL(x) = |Lw below x| and
// above(x) = |Rw strictly above x|:
//   a left stop at x (it is l_kL) swaps   iff  above(x) > kL(x)
//   a right stop at x (it is r_above) swaps iff  kL(x) > above(x)
// since l_kL < r_kL says that more than kL right stops lie strictly above x,
// and l_above < x says that more than above(x) left stops lie strictly below
// x.  (In the loop's older names, kR = nR - 1 - |Rw below x| is above(x) +
// [x in Rw], which gives lsw = isL && kR - isR >= kL, rsw = isR && kL > kR.)
// `first` is always a right stop, the last one (r_{nR-1}); no left stop lies
// below it, so it never swaps and no swapping left stop is paired with it:
// the loops leave it out of Rw, which changes no above(x) for x > first.
// K = the number of swapping left stops, known before the LDS exchange; the
// right stops are published behind a sentinel (rp[0] = 64 = r_{-1}, rp[k + 1]
// = r_k), so the partner positions and the two cut candidates lp[K], rp[K] are
// read in one batch with indices that need no clamp (all are < the segment's
// slot count: kL < x, above <= |Rw| <= slots - 1, K <= |Lw| <= slots - 1).
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

#include "select.hpp"

namespace hmc {

__device__ inline double rl_f64(double x, int lane) {
  const unsigned long long b = (unsigned long long)__double_as_longlong(x);
  const int lo = __builtin_amdgcn_readlane((int)(uint32_t)b, lane);
  const int hi = __builtin_amdgcn_readlane((int)(uint32_t)(b >> 32), lane);
  return __longlong_as_double((long long)(((unsigned long long)(uint32_t)hi << 32) | (uint32_t)lo));
}
__device__ inline uint32_t rl_u32(uint32_t x, int lane) { return (uint32_t)__builtin_amdgcn_readlane((int)x, lane); }

// Lane gather over the whole wave (ds_bpermute); src is taken modulo 64.
__device__ inline uint32_t gat_u32(uint32_t x, int src) {
  return (uint32_t)__builtin_amdgcn_ds_bpermute(src << 2, (int)x);
}
__device__ inline double gat_f64(double x, int src) {
  const unsigned long long b = (unsigned long long)__double_as_longlong(x);
  const uint32_t lo = gat_u32((uint32_t)b, src), hi = gat_u32((uint32_t)(b >> 32), src);
  return __longlong_as_double((long long)(((unsigned long long)hi << 32) | lo));
}

// Cross-lane LDS exchange inside one wavefront: the LDS executes a wave's
// instructions in order, so only the compiler must keep the accesses in
// program order (no s_barrier, no wait on outstanding HBM stores).
__device__ inline void wave_lds_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// Keeps a batch of LDS reads where it is written: the values count as used
// here, so no read is sunk behind the branch of the one select that consumes
// it (which would put it after the others in an exec-masked block of its own).
__device__ inline void lds_batch(int &a, int &b, int &c, int &d) {
  asm volatile("" : "+v"(a), "+v"(b), "+v"(c), "+v"(d));
}
__device__ inline void lds_batch(int &a, int &b, int &c, int &d, int &e, int &f) {
  asm volatile("" : "+v"(a), "+v"(b), "+v"(c), "+v"(d), "+v"(e), "+v"(f));
}

// This lane's place in the segmentation (SW lanes per segment, G segments).
struct Seg {
  int g;          // segment index (>= G: lane outside every segment)
  int base;       // first lane of the segment
  int k;          // element index inside the segment
  int sw;         // segment width
  uint64_t mask;  // lanes of the segment
  uint64_t lt;    // lanes of the segment below this lane
  uint32_t wm;    // segment-relative: all SW bits (0 outside every segment)
  uint32_t ltk;   // segment-relative: bits below k
};

// Lane mask of a predicate; unlike __ballot(int) the predicate stays a mask
// (no 0/1 materialisation and re-compare).
__device__ inline uint64_t wave_ballot(bool p) { return __builtin_amdgcn_ballot_w64(p); }

// A wave ballot seen from this lane's segment (bit k = element k).
__device__ inline uint32_t seg_bits(uint64_t ballot, const Seg &sg) { return (uint32_t)(ballot >> sg.base) & sg.wm; }

__device__ inline Seg make_seg(int SW) {
  Seg s;
  const int lane = (int)(threadIdx.x & 63);
  const int G = 64 / SW;
  s.g = lane / SW;
  s.base = s.g * SW;
  s.k = lane - s.base;
  s.sw = SW;
  const uint64_t w = SW >= 64 ? ~0ull : ((1ull << SW) - 1ull);
  s.mask = s.g < G ? (w << s.base) : 0ull;
  s.lt = s.mask & ((1ull << lane) - 1ull);
  s.wm = s.g < G ? (SW >= 32 ? ~0u : ((1u << SW) - 1u)) : 0u;
  s.ltk = s.k < 32 ? (1u << s.k) - 1u : ~0u;
  return s;
}

// Lowest set element of a segment-relative mask (64 if none).
__device__ inline int seg_lowest(uint32_t bits) {
  return bits ? __builtin_ctz(bits) : 64;
}

// LDS scratch of the segmented selection, one entry per lane (segment g uses
// [base, base+SW)): left-stop and right-stop positions (rpos: a sentinel,
// then the stops), per-lane junk slots that absorb the writes of lanes that
// are not stops (the selections use the first 64: the slots are never read,
// and each write instruction hits a lane's slot once), and a spill list for
// the heap-select path.
struct SegScratch {
  int *lpos;      // [64]
  int *rpos;      // [64]
  int *junk;      // [128]
  double *slik;   // [64]
  uint32_t *smeta;
};

// The final window [first, last) of 2 or 3 elements (std::__insertion_sort,
// stl_algo.h:1819-1849, comp = greater) as a placement: where each element of
// the window ends up, from the three comparisons the sequential code can make.
// With a, b, c the values at first, first + 1, first + 2 and s = b > a,
// ca = c > a, cb = c > b (ca = cb = false in a window of 2):
//   i = 1: b goes before a iff s; call the pair (p, q) = s ? (b, a) : (a, b).
//   i = 2: c goes to the front iff c > p (cp = s ? cb : ca); else
//          __unguarded_linear_insert passes q iff c > q and then stops at p
//          (c > p is known false), so c passes q iff t = ca || cb.
// End offsets:  c: 2 - cp - t    p: cp    q: 1 + t, i.e.
//   a: s ? 1 + t : ca        b: s ? cb : 1 + t        c: 2 - cp - t
// On a weak ordering this is the stable descending rank, offset(x_j) =
// #{i : x_i > x_j} + #{i < j : x_i equivalent to x_j} (s && cb implies ca, and
// so on); the case form above is also what the sequential code does on values
// that are no weak ordering (NaN compares false both ways), which the rank
// count is not.  The offsets of all eight outcomes are packed two bits each
// into one 48-bit constant (bits [16 j + 2 idx, +2): the element at window
// offset j under idx = 4 s + 2 ca + cb), so a lane owns the element at its
// position and gets that element's end offset with one shift; a window of 2 is
// a window of 3 whose c is NaN (ca = cb = false).  A lane whose position is
// outside a live window writes its element back to its own slot, so the writes
// need no exec mask.  No swap network, no 3-way select, no branch.
constexpr uint64_t small_window_table() {
  uint64_t T = 0;
  for (int idx = 0; idx < 8; ++idx) {
    const int s = (idx >> 2) & 1, ca = (idx >> 1) & 1, cb = idx & 1;
    const int t = ca | cb, cp = s ? cb : ca;
    const uint64_t a = s ? 1 + t : ca, b = s ? cb : 1 + t, c = 2 - cp - t;
    T |= a << (2 * idx) | b << (16 + 2 * idx) | c << (32 + 2 * idx);
  }
  return T;
}
// (a, b, c) end offsets for idx = 0 .. 7, written out from the sequential code:
// (0,1,2) (0,2,1) (1,2,0) (1,2,0) (1,0,2) (2,1,0) (2,0,1) (2,1,0)
// (tests/test_small_window_rank.py holds the same constant)
static_assert(small_window_table() == 0x120644a9a950ull, "small-window placement table");
struct SmallWindow {
  int idx2;  // 2 * (4 s + 2 ca + cb)
  int len;   // 2 or 3; 0 where the segment does not run the sort
  __device__ SmallWindow(double a, double b, double c, int len_, bool live) : len(live ? len_ : 0) {
    const double c3 = len_ > 2 ? c : __builtin_nan("");
    idx2 = (b > a ? 8 : 0) | (c3 > a ? 4 : 0) | (c3 > b ? 2 : 0);
  }
  // destination of the element at position p
  __device__ int dest(int p, int first) const {
    constexpr uint64_t T = small_window_table();
    const int j = p - first;
    const int off = (int)(uint32_t)(T >> ((idx2 + 16 * j) & 63)) & 3;
    return (unsigned)j < (unsigned)len ? first + off : p;
  }
};

// std::nth_element(v, v+nth, v+n, greater) on every segment's list, in
// place in the LDS slots slik/smeta (segment g's element k in slot
// g*SW + k; n, nth uniform inside a segment, n <= SW <= 64; n == 0 marks an
// idle segment).  Whole-wave call, branch-free per lane for SW <= 32.
//
// One partition costs two dependent LDS round trips: one batch that reads the
// median candidates, the value at `first` and every lane's own element, and
// one batch behind the stops' position writes that reads the partner
// positions together with the two cut candidates (the swap decisions and K
// come from the stop counts, so nothing in that batch waits on another read;
// the cut used to be a third trip behind a ballot of the partner test).  Each
// lane then writes its element straight into its destination slot (the LDS
// executes a wave's accesses in order, so no wait).  The median
// swap (std::__move_median_to_first) is not executed as a data move: the
// ballots are taken over *positions* (lane p evaluates the value position p
// holds after the swap: the pivot at `first`, first's value at r), and each
// lane's element enters the partition at x = tau(lane), tau = (first r).
__device__ inline void seg_nth_slots(int n, int nth, const Seg &sg, const SegScratch &ss) {
  const int lane = (int)(threadIdx.x & 63);
  const int k = sg.k;
  if (sg.sw > 32) {  // lists of up to 64 (S > 16): one per wave, the sequential algorithm on its first lane
    if (n > 0 && nth != n && sg.mask != 0ull && k == 0) {
      const LinkList wl{ss.slik + sg.base, ss.smeta + sg.base, 1};
      nth_element_greater(wl, n, nth);
    }
    wave_lds_sync();
    return;
  }
  int first = 0, last = n, depth = n > 0 ? lg2_floor(n) * 2 : 0;
  const bool act = n > 0 && nth != n && sg.mask != 0ull;
  double *sl = ss.slik + sg.base;
  uint32_t *sm = ss.smeta + sg.base;
  int *lp = ss.lpos + sg.base, *rp = ss.rpos + sg.base;
  int *jk = ss.junk + lane;  // never read: absorbs the writes of lanes that are not stops
  const int kmax = sg.sw - 1;
  const uint64_t b_act = wave_ballot(act);
  if (k == 0) rp[0] = 64;  // r_{-1}: stays for the whole call (stops go to rp[1 ..])
  while (true) {
    // a segment whose depth budget is spent stops here with > 3 elements left
    // and finishes with the heap select below (its range no longer changes)
    const bool part = act && last - first > 3 && depth > 0;
    // each ballot of a single comparison stays a lane mask; the conjunctions
    // are scalar ANDs (a ballot of a && b would be materialised and re-compared)
    const uint64_t b_part = b_act & wave_ballot(last - first > 3) & wave_ballot(depth > 0);
    if (!b_part) break;
    depth -= part ? 1 : 0;
    // std::__move_median_to_first(first, first+1, mid, last-1) (stl_algo.h:79-102)
    const int a = first + 1, b = first + ((last - first) >> 1), c = last > 0 ? last - 1 : 0;
    const double va = sl[a], vb = sl[b], vc = sl[c], vf = sl[first];
    const double v = sl[k];
    const uint32_t m = sm[k];
    // which of a (0), b (1), c (2) is the median, as a table over the three
    // comparisons (index ab*4 + bc*2 + ac) so it compiles to selects; `first`
    // (the identity) in a segment that sits this round out
    const int idx = (va > vb ? 4 : 0) | (vb > vc ? 2 : 0) | (va > vc ? 1 : 0);
    const int w = (22561 >> (2 * idx)) & 3;
    const int r = !part ? first : (w == 0 ? a : (w == 1 ? b : c));
    const double pivot = w == 0 ? va : (w == 1 ? vb : vc);
    // stops by position (std::__unguarded_partition, stl_algo.h:1878-1896):
    // left scan over [first+1, last) stops at !(x > pivot), right scan over
    // [first, last) at !(pivot > x); `first`, always a right stop, never swaps
    // and is left out of Rw
    const double pv = k == first ? pivot : (k == r ? vf : v);
    const uint64_t b_in = b_part & wave_ballot(k > first) & wave_ballot(k < last);
    const uint32_t Lw = seg_bits(b_in & wave_ballot(!(pv > pivot)), sg);
    const uint32_t Rw = seg_bits(b_in & wave_ballot(!(pivot > pv)), sg);
    const int nL = __popc(Lw);
    // this lane's element is at position x once the median is at first
    const int x = k == first ? r : (k == r ? first : k);
    const bool isL = (Lw >> x) & 1u, isR = (Rw >> x) & 1u;
    // left stops below x and right stops above x: the pair index of a stop of
    // either kind, and the swap decision (header comment)
    const int kL = __popc(Lw & ((1u << x) - 1u));
    const int kR = __popc((Rw >> 1) >> x);
    const bool lsw = isL && kR > kL, rsw = isR && kL > kR;
    const int K = __popcll(wave_ballot(isL) & wave_ballot(kR > kL) & sg.mask);
    *(isL ? lp + kL : jk) = x;
    *(isR ? rp + 1 + kR : jk) = x;
    wave_lds_sync();
    // one batch: the partners and the cut = min(l_K, r_{K-1}), the first left
    // stop that does not swap and the lowest right stop that does.  Every
    // index is inside the segment (kL < x, kR and K < sw); a lane that does
    // not swap reads a slot it does not use.
    int qR = rp[1 + kL], qL = lp[kR];
    int lKs = lp[K], rK = rp[K];
    lds_batch(qR, qL, lKs, rK);
    const int dest = lsw ? qR : (rsw ? qL : x);
    sl[dest] = v;
    sm[dest] = m;
    const int lK = K < nL ? lKs : 64;
    const int cut = lK < rK ? lK : rK;
    wave_lds_sync();
    first = part && cut <= nth ? cut : first;
    last = part && cut > nth ? cut : last;
  }
  // Depth limit reached (std::__heap_select + iter_swap, stl_algo.h:1973-1979):
  // rare; the segment's first lane runs the sequential code on the slots.
  const bool heap = act && last - first > 3;
  if (wave_ballot(heap)) {
    if (heap && k == 0) {
      const LinkList wl{sl, sm, 1};
      heap_select(wl, first, nth + 1, last);
      wl.swap(first, nth);
    }
    wave_lds_sync();
  }
  // std::__insertion_sort of the <= 3 remaining elements (stl_algo.h:1819-1849)
  // as a rank placement (header comment): reads, then writes, then visible
  const bool ins = act && !heap && last - first > 1;
  if (wave_ballot(ins)) {
    const int f0 = first < kmax ? first : kmax;
    const int f1 = first + 1 < kmax ? first + 1 : kmax, f2 = first + 2 < kmax ? first + 2 : kmax;
    const double y0 = sl[f0], y1 = sl[f1], y2 = sl[f2];
    const double v = sl[k];
    const uint32_t m = sm[k];
    const SmallWindow sw3(y0, y1, y2, last - first, ins);
    const int d = sw3.dest(k, first);
    wave_lds_sync();
    sl[d] = v;
    sm[d] = m;
    wave_lds_sync();
  }
}

// The same selection with two elements per lane: segment g of W = S lanes
// holds a list of up to 2S <= 32 links in its slots [g*2W, g*2W + 2W); lane k
// of the segment carries positions k (element 0) and k + W (element 1), so a
// wavefront works on 64 / W lists (S = 10: 6) instead of 64 / 2W.  The
// per-segment work of a partition (median, stop masks, cut) is shared by the
// two elements; only the per-element compares, ranks and moves double.  The
// permutation is the one of seg_nth_slots (the stop masks are assembled from
// the two elements' ballots, bit p = position p).  sg = make_seg(W); the
// scratch arrays hold (64 / W + 1) x 2W slots: lanes past the last segment
// address a dead segment of their own.
__device__ inline void seg2_nth_slots(int n, int nth, const Seg &sg, const SegScratch &ss) {
  const int lane = (int)(threadIdx.x & 63);
  const int W = sg.sw, k = sg.k;
  int first = 0, last = n, depth = n > 0 ? lg2_floor(n) * 2 : 0;
  const bool act = n > 0 && nth != n && sg.mask != 0ull;
  const int sb = sg.g * 2 * W;  // the segment's first slot
  double *sl = ss.slik + sb;
  uint32_t *sm = ss.smeta + sb;
  int *lp = ss.lpos + sb, *rp = ss.rpos + sb;
  int *jk = ss.junk + lane;  // never read: one slot per lane serves all four writes
  const int kmax = 2 * W - 1;
  const int p0 = k, p1 = k + W;  // this lane's positions
  const uint64_t b_act = wave_ballot(act);
  if (k == 0) rp[0] = 64;  // r_{-1}: stays for the whole call (stops go to rp[1 ..])
  while (true) {
    const bool part = act && last - first > 3 && depth > 0;
    if (!(b_act & wave_ballot(last - first > 3) & wave_ballot(depth > 0))) break;
    depth -= part ? 1 : 0;
    // std::__move_median_to_first(first, first+1, mid, last-1) (stl_algo.h:79-102)
    const int a = first + 1, b = first + ((last - first) >> 1), c = last > 0 ? last - 1 : 0;
    const double va = sl[a], vb = sl[b], vc = sl[c], vf = sl[first];
    const double v0 = sl[p0], v1 = sl[p1];
    const uint32_t m0 = sm[p0], m1 = sm[p1];
    const int idx = (va > vb ? 4 : 0) | (vb > vc ? 2 : 0) | (va > vc ? 1 : 0);
    const int w = (22561 >> (2 * idx)) & 3;
    // where the median comes from; `first` (the identity) in a segment that sits this round out
    const int r = !part ? first : (w == 0 ? a : (w == 1 ? b : c));
    const double pivot = w == 0 ? va : (w == 1 ? vb : vc);
    // the value each position holds once the median is at first
    const double pv0 = p0 == first ? pivot : (p0 == r ? vf : v0);
    const double pv1 = p1 == first ? pivot : (p1 == r ? vf : v1);
    // stop masks over positions: ballot bits of element 0 at [0, W), element 1 at [W, 2W)
    const uint32_t le = seg_bits(wave_ballot(!(pv0 > pivot)), sg) | seg_bits(wave_ballot(!(pv1 > pivot)), sg) << W;
    const uint32_t ge = seg_bits(wave_ballot(!(pivot > pv0)), sg) | seg_bits(wave_ballot(!(pivot > pv1)), sg) << W;
    const uint32_t in = part ? (2u << c) - (2u << first) : 0u;  // (first, last): first < c = last - 1 <= 31
    const uint32_t Lw = le & in, Rw = ge & in;                  // Rw: the right stops but `first`
    const int nL = __popc(Lw);
    // each element's position once the median is at first
    const int x0 = p0 == first ? r : (p0 == r ? first : p0);
    const int x1 = p1 == first ? r : (p1 == r ? first : p1);
    const bool isL0 = (Lw >> x0) & 1u, isR0 = (Rw >> x0) & 1u;
    const bool isL1 = (Lw >> x1) & 1u, isR1 = (Rw >> x1) & 1u;
    // left stops below and right stops above each element: its pair index as a
    // stop of either kind, and the swap decision (header comment)
    const int kL0 = __popc(Lw & ((1u << x0) - 1u)), kL1 = __popc(Lw & ((1u << x1) - 1u));
    const int kR0 = __popc((Rw >> 1) >> x0), kR1 = __popc((Rw >> 1) >> x1);
    const uint64_t b_lsw0 = wave_ballot(isL0) & wave_ballot(kR0 > kL0);
    const uint64_t b_lsw1 = wave_ballot(isL1) & wave_ballot(kR1 > kL1);
    const bool lsw0 = isL0 && kR0 > kL0, lsw1 = isL1 && kR1 > kL1;
    const bool rsw0 = isR0 && kL0 > kR0, rsw1 = isR1 && kL1 > kR1;
    const int K = __popc(seg_bits(b_lsw0, sg) | seg_bits(b_lsw1, sg) << W);
    *(isL0 ? lp + kL0 : jk) = x0;
    *(isL1 ? lp + kL1 : jk) = x1;
    *(isR0 ? rp + 1 + kR0 : jk) = x0;
    *(isR1 ? rp + 1 + kR1 : jk) = x1;
    wave_lds_sync();
    // one batch: the partners and the cut = min(l_K, r_{K-1}).  Every index
    // is inside the segment's 2W slots (kL < x, kR and K < 2W); a lane that
    // does not swap reads a slot it does not use.
    int qR0 = rp[1 + kL0], qR1 = rp[1 + kL1];
    int qL0 = lp[kR0], qL1 = lp[kR1];
    int lKs = lp[K], rK = rp[K];
    lds_batch(qR0, qR1, qL0, qL1, lKs, rK);
    const int d0 = lsw0 ? qR0 : (rsw0 ? qL0 : x0), d1 = lsw1 ? qR1 : (rsw1 ? qL1 : x1);
    sl[d0] = v0;
    sm[d0] = m0;
    sl[d1] = v1;
    sm[d1] = m1;
    const int lK = K < nL ? lKs : 64;
    const int cut = lK < rK ? lK : rK;
    wave_lds_sync();
    first = part && cut <= nth ? cut : first;
    last = part && cut > nth ? cut : last;
  }
  // depth limit: std::__heap_select + iter_swap on the segment's first lane
  const bool heap = act && last - first > 3;
  if (wave_ballot(heap)) {
    if (heap && k == 0) {
      const LinkList wl{sl, sm, 1};
      heap_select(wl, first, nth + 1, last);
      wl.swap(first, nth);
    }
    wave_lds_sync();
  }
  // std::__insertion_sort of the <= 3 remaining elements (stl_algo.h:1819-1849)
  // as a rank placement (header comment): reads, then writes, then visible
  const bool ins = act && !heap && last - first > 1;
  if (wave_ballot(ins)) {
    const int f0 = first < kmax ? first : kmax;
    const int f1 = first + 1 < kmax ? first + 1 : kmax, f2 = first + 2 < kmax ? first + 2 : kmax;
    const double y0 = sl[f0], y1 = sl[f1], y2 = sl[f2];
    const double v0 = sl[p0], v1 = sl[p1];
    const uint32_t m0 = sm[p0], m1 = sm[p1];
    const SmallWindow sw3(y0, y1, y2, last - first, ins);
    const int d0 = sw3.dest(p0, first), d1 = sw3.dest(p1, first);
    wave_lds_sync();
    sl[d0] = v0;
    sm[d0] = m0;
    sl[d1] = v1;
    sm[d1] = m1;
    wave_lds_sync();
  }
}

// Value-only top-S of every segment's list (slots [0, n), n <= SW): each
// element's rank is the number of elements greater than it plus the equal ones
// in lower slots, and the S best are written to slots [0, S) in rank order.
// Returns, on the lane that finds one, the non-zero value straddling the
// S-cut (the element ranked S equals one ranked above it), else 0: only such
// a tie can make the retained set depend on the order libstdc++ would have
// left the list in — and only if it is still at the cut when the list is
// complete (a later, larger cut evicts both tied elements anyway).  Segments
// with n <= S are left untouched.  Whole-wave call.
__device__ inline double seg_rank_select(int n, int S, const Seg &sg, const SegScratch &ss) {
  const int k = sg.k;
  const double *sl = ss.slik + (sg.mask != 0ull ? sg.base : 0);
  const bool mine = sg.mask != 0ull && n > S && k < n;
  const double v = mine ? sl[k] : 0.0;
  const uint32_t m = mine ? ss.smeta[sg.base + k] : 0u;
  int gt = 0, eq = 0;
  for (int q = 0; q < sg.sw; q += 2) {  // two slots per read; segment lanes read the same address
    const double2 y = *(const double2 *)(sl + q);
    gt += (q < n && y.x > v) ? 1 : 0;
    eq += (q < k && y.x == v) ? 1 : 0;
    gt += (q + 1 < n && y.y > v) ? 1 : 0;
    eq += (q + 1 < k && y.y == v) ? 1 : 0;
  }
  const int rank = gt + eq;
  wave_lds_sync();
  if (mine && rank < S) {
    ss.slik[sg.base + rank] = v;
    ss.smeta[sg.base + rank] = m;
  }
  wave_lds_sync();
  return mine && rank == S && eq > 0 ? v : 0.0;
}

// Register interface: lane g*SW+k holds element k of segment g's list.
__device__ inline void seg_nth_element(double &v, uint32_t &m, int n, int nth, const Seg &sg,
                                       const SegScratch &ss) {
  const int lane = (int)(threadIdx.x & 63);
  ss.slik[lane] = v;
  ss.smeta[lane] = m;
  wave_lds_sync();
  seg_nth_slots(n, nth, sg, ss);
  v = ss.slik[lane];
  m = ss.smeta[lane];
}

}  // namespace hmc
