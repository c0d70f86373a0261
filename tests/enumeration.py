"""Exhaustive enumeration of the haplotype model in exact rational arithmetic.

An independent reference for the E-step, the pattern mining and the exact
M-step at sizes where every phasing of a genotype can be listed: no dynamic
programme, no k-best lists, no traceback, no trie.  Every double is an exact
rational, so `fractions.Fraction` carries the tables' numbers without error
and every sum, product and quotient below is exact; the comparison helpers
then bound the implementation's rounding error from operation counts.

Derived from the reference's source (cited per function), not from
oracle/hmc_oracle.cpp; this module imports neither the product nor the
restatement.  A haplotype is a tuple of allele symbols, a pattern's key is
(start, tuple of symbols), a table is the dict `patterns()` returns.

What it cannot pin: the order among candidates of equal prior, individuals
with a missing allele at a head locus (HEAD_QUIRK below), which S candidates
of an individual with a homozygous phasing survive the cuts (HOMOZYGOUS_CUT
below), and anything larger than MAX_PHASINGS ordered phasings per individual.
"""
from __future__ import annotations

import hashlib
import itertools
import math
from fractions import Fraction

import numpy as np

U = Fraction(1, 2 ** 53)  # unit roundoff of IEEE double
MAX_PHASINGS = 4096       # ordered phasings per individual the enumeration accepts
FIXED_QUANTUM = Fraction(1, 2 ** 44)  # exact.hpp EXACT_FIXED_SCALE = 2^44

# HEAD_QUIRK: for an individual with a missing allele at a locus < head_len the
# reference's initHeadList (HaploBuilder.cpp:153-224) pairs every head pattern
# that matches the genotype with every completion of the *other* haplotype,
# including pairs that are not phasings of the genotype; the model below does
# not describe it.  Such individuals are left out (`head_quirk`).
#
# HOMOZYGOUS_CUT: a k-best link that is still homozygous carries P(h)^2, one
# that is heterozygous carries P(h0) P(h1), half its prior; the per-state cut
# (HaploPair.cpp:85-88) compares the two as they are, while the final list
# doubles the heterozygous ones before its cut (HaploBuilder.cpp:98-103).  The
# links of one state share every later factor, so the two scales meet only for
# an individual that has a homozygous phasing (no locus with two different
# known alleles): before a heterozygous locus every link is doubled in the end,
# after it none is homozygous.  For such an individual with more positive
# phasings than S the reference's candidates are therefore not always the S
# largest priors.  What the cuts do guarantee, and check_estep asserts there:
# the candidates are distinct phasings with their enumerated priors, in
# descending order, and every phasing left out has a score (its prior, halved
# if heterozygous) no larger than the last kept prior, since at the cut that
# dropped it S links of no smaller score stayed, and a prior is at least its
# score.  With at most S positive phasings nothing is cut and all are listed.

_memo: dict = {}


def gamma(k: int) -> Fraction:
    """Higham's gamma_k = k u / (1 - k u): the relative error bound of a
    result that k roundings separate from the exact value."""
    k = int(k)
    return k * U / (1 - k * U)


def _digest(*arrays) -> str:
    h = hashlib.sha1()
    for a in arrays:
        a = np.ascontiguousarray(a)
        h.update(str(a.dtype).encode() + str(a.shape).encode() + a.tobytes())
    return h.hexdigest()


def memo(key, fn):
    if key not in _memo:
        _memo[key] = fn()
    return _memo[key]


# ------------------------------------------------------------------ panel ----
def allele_table(alleles: np.ndarray):
    """GenoData.cpp:78-118: per locus the distinct non-missing symbols sorted
    by value, each with count / non-missing count."""
    N, _, L = alleles.shape
    out = []
    for k in range(L):
        col = [int(a) for a in alleles[:, :, k].ravel() if a >= 0]
        out.append([(s, Fraction(col.count(s), len(col))) for s in sorted(set(col))])
    return out


def head_quirk(alleles: np.ndarray, head_len: int) -> np.ndarray:
    """Individuals with a missing allele at a head locus (see HEAD_QUIRK)."""
    return (alleles[:, :, :head_len] < 0).any(axis=(1, 2))


def locus_options(g: np.ndarray, k: int, syms) -> list:
    """Ordered allele pairs of genotype g[2][L] at locus k (HaploBuilder.cpp:
    47-79): both alleles missing gives every ordered pair, one missing every
    allele against the known one in both orders; `syms` = symbols of positive
    allele frequency."""
    a, b = int(g[0, k]), int(g[1, k])
    if a < 0 and b < 0:
        return [(x, y) for x in syms for y in syms]
    if a < 0 or b < 0:
        kn = b if a < 0 else a
        return sorted({(x, kn) for x in syms} | {(kn, x) for x in syms})
    return [(a, a)] if a == b else [(a, b), (b, a)]


def phasing_count(g: np.ndarray, table_of_alleles) -> int:
    n = 1
    for k in range(g.shape[1]):
        n *= len(locus_options(g, k, [s for s, f in table_of_alleles[k] if f > 0]))
    return n


def phasings(g: np.ndarray, table_of_alleles):
    """Every ordered pair (h0, h1) consistent with genotype g."""
    opts = [locus_options(g, k, [s for s, f in table_of_alleles[k] if f > 0]) for k in range(g.shape[1])]
    n = math.prod(len(o) for o in opts)
    assert n <= MAX_PHASINGS, n
    for combo in itertools.product(*opts):
        yield tuple(c[0] for c in combo), tuple(c[1] for c in combo)


# ------------------------------------------------------------------ table ----
class Table:
    """A pattern table indexed by (start, symbols), numbers as Fractions."""

    def __init__(self, pt: dict):
        self.n = len(pt["start"])
        self.start = [int(x) for x in pt["start"]]
        self.len = [int(x) for x in pt["len"]]
        self.al = [tuple(int(a) for a in pt["alleles"][i, :self.len[i]]) for i in range(self.n)]
        self.freq = [Fraction(float(x)) for x in pt["freq"]]
        self.tp = [Fraction(float(x)) for x in pt["tp"]]
        self.index = {(self.start[i], self.al[i]): i for i in range(self.n)}
        assert len(self.index) == self.n, "duplicate patterns"
        self.key = _digest(pt["start"], pt["len"], pt["alleles"], pt["freq"], pt["tp"])
        self._chain: dict = {}
        self._global: dict = {}

    def longest(self, h, end: int, min_start: int):
        """Longest stored pattern ending at `end` (exclusive) that equals
        h[start:end] with start >= min_start, or None."""
        for s in range(min_start, end):
            i = self.index.get((s, tuple(h[s:end])))
            if i is not None:
                return i
        return None

    def chain_prob(self, h, head_len: int, global_match: bool = False) -> Fraction:
        """P(h) by the variable-order chain: the head pattern's frequency
        (HaploPair.cpp:14-33), then per further locus the transition
        probability of the successor (PatternManager.cpp:308-317: the longest
        stored pattern ending there that matches h and starts no earlier than
        the current pattern).  `global_match` drops the start constraint — the
        longest match of HaploBuilder.cpp:128-146."""
        cache = self._global if global_match else self._chain
        h = tuple(h)
        if (h, head_len) in cache:
            return cache[h, head_len]
        cur = self.index.get((0, h[:head_len]))
        p = Fraction(0)
        if cur is not None:
            p = self.freq[cur]
            for e in range(head_len + 1, len(h) + 1):
                cur = self.longest(h, e, 0 if global_match else self.start[cur])
                if cur is None:
                    p = Fraction(0)
                    break
                p *= self.tp[cur]
        cache[h, head_len] = p
        return p


def rebuild_successors(pt: dict, table_of_alleles, L: int) -> np.ndarray:
    """succ[P][A] by the successor rule (PatternManager.cpp:308-317): for
    pattern p ending before L and allele index j of locus p.end, the longest
    stored pattern ending at p.end + 1 that equals p's symbols followed by the
    allele, with start >= p.start; -1 where none."""
    t = Table(pt)
    A = max(len(x) for x in table_of_alleles)
    succ = np.full((t.n, A), -1, np.int32)
    for i in range(t.n):
        end = t.start[i] + t.len[i]
        if end >= L:
            continue
        for j, (s, _) in enumerate(table_of_alleles[end]):
            ext = (None,) * t.start[i] + t.al[i] + (s,)
            q = t.longest(ext, end + 1, t.start[i])
            succ[i, j] = -1 if q is None else q
    return succ


# ----------------------------------------------------------------- E-step ----
def estep(alleles: np.ndarray, pt: dict, head_len: int):
    """Per individual (None for HEAD_QUIRK ones): total = sum over ordered
    phasings of P(h0) P(h1) (HaploBuilder.cpp:87-91), M = their number,
    priors[{h0, h1}] = 2 P(h0) P(h1), or P(h)^2 for h0 == h1 (HaploPair.cpp:
    14-89), marg[h] = sum over phasings with h0 == h of P(h0) P(h1)."""
    t = Table(pt)

    def run():
        ta = allele_table(alleles)
        skip = head_quirk(alleles, head_len)
        out = []
        for i in range(alleles.shape[0]):
            if skip[i]:
                out.append(None)
                continue
            total, M, priors, marg = Fraction(0), 0, {}, {}
            for h0, h1 in phasings(alleles[i], ta):
                p = t.chain_prob(h0, head_len) * t.chain_prob(h1, head_len)
                total += p
                M += 1
                k = (h0, h1) if h0 <= h1 else (h1, h0)
                priors[k] = priors.get(k, 0) + p  # both orders of a heterozygous pair land here
                marg[h0] = marg.get(h0, 0) + p
            out.append(dict(total=total, M=M, priors=priors, marg=marg))
        return out

    return memo(("estep", _digest(alleles), t.key, head_len), run)


# ----------------------------------------------------------------- mining ----
def matcher(alleles: np.ndarray, samples=None):
    """The matching state of a mining candidate and its extension by one
    symbol, shared by `mine` and set_enumeration.find_patterns_by_num.

    Frequencies: from the genotypes (getMatchingFrequency, PatternManager.cpp:
    267-291) the sum over individuals that match at every locus (an allele
    missing or equal) of the product over loci of half the sum, over the two
    alleles, of 1 if equal or the allele's frequency if missing, divided by N;
    from `samples` = (haplotypes[H][L], weights[H]) the matching weights over
    all weights (checkFrequencyWithExtension, :195-265).

    Returns (root, extend): root = the state of the empty string, [(item,
    factor)]; extend(state, k, a, af) = (state, frequency) of the string with
    symbol a (allele frequency af) appended at locus k."""
    N = alleles.shape[0]
    if samples is None:
        def extend(state, k, a, af):
            nxt = []
            for i, f in state:
                b0, b1 = int(alleles[i, 0, k]), int(alleles[i, 1, k])
                if b0 < 0 or b1 < 0 or b0 == a or b1 == a:
                    x = (af if b0 < 0 else int(b0 == a)) + (af if b1 < 0 else int(b1 == a))
                    nxt.append((i, f * x / 2))
            return nxt, sum((f for _, f in nxt), Fraction(0)) / N

        return [(i, Fraction(1)) for i in range(N)], extend
    sal = np.asarray(samples[0])
    sw = [Fraction(float(w)) for w in samples[1]]
    tw = sum(sw)

    def extend(state, k, a, af):
        nxt = [(i, f) for i, f in state if sal[i, k] == a]
        return nxt, sum((f for _, f in nxt), Fraction(0)) / tw

    return [(i, sw[i]) for i in range(len(sw))], extend


def mine(alleles: np.ndarray, min_freq: Fraction, min_len: int, max_len: int, samples=None):
    """PatternManager::searchPattern (PatternManager.cpp:100-144): per start
    locus a depth-first search from the empty string.  A string is extended by
    every allele of positive frequency if (freq >= min_freq or len < min_len),
    its end < L and len < max_len; it is stored if (freq >= min_freq or
    len <= min_len) and len >= max(min_len, 1).  Frequencies: `matcher`.

    Returns (stored, visited): stored[(start, symbols)] = (freq, prefix) with
    prefix the frequency without the last symbol (1 for length 1), visited =
    the frequency of every candidate the search looked at."""
    N, _, L = alleles.shape
    ta = allele_table(alleles)
    min_len = max(min_len, 1)
    max_len = max(L if max_len <= 0 else max_len, min_len)
    root, extend = matcher(alleles, samples)
    stored, visited = {}, []
    for s in range(L):
        stack = [((), root, Fraction(1), None)]
        while stack:
            al, state, freq, prefix = stack.pop()
            ln, end = len(al), s + len(al)
            if ln:
                visited.append(freq)
            if (freq >= min_freq or ln < min_len) and end < L and ln < max_len:
                for a, af in ta[end]:
                    if af > 0:
                        st2, f2 = extend(state, end, a, af)
                        stack.append((al + (a,), st2, f2, freq))
            if (freq >= min_freq or ln <= min_len) and ln >= min_len:
                stored[(s, al)] = (freq, prefix)
    return stored, visited


def threshold_margin(visited, min_freq: Fraction):
    """(candidates whose frequency equals min_freq, smallest relative distance
    of any other candidate's frequency from min_freq)."""
    if min_freq <= 0:
        return 0, math.inf
    eq = sum(1 for f in visited if f == min_freq)
    d = [abs(f - min_freq) / min_freq for f in visited if f != min_freq]
    return eq, float(min(d)) if d else math.inf


# ----------------------------------------------------------- exact M-step ----
def mstep(alleles: np.ndarray, prev: dict, head_len: int, keys):
    """HaploBuilder.cpp:274-332, 334-450 without the walk: for every key
    (start, symbols), f = sum over individuals of E[(1{h0 matches} +
    1{h1 matches}) / 2 | genotype] under P(h0) P(h1) / total of the previous
    table, pre = the same for the key without its last symbol (N for length
    1).  Returns {key: (f, pre)} before the clamp and the division by N.
    The ordered phasings are symmetric, so the expectation is the h0 marginal."""
    N = alleles.shape[0]
    en = estep(alleles, prev, head_len)
    assert all(e is not None for e in en), "the exact M-step sums over every individual: no HEAD_QUIRK ones"

    cache = memo(("expect", _digest(alleles), Table(prev).key, head_len), dict)  # shared by every call on this E-step

    def expect(s, al):
        if not al:
            return Fraction(N)
        if (s, al) not in cache:
            tot = Fraction(0)
            for e in en:
                tot += sum((p for h, p in e["marg"].items() if h[s:s + len(al)] == al), Fraction(0)) / e["total"]
            cache[s, al] = tot
        return cache[s, al]

    return {(s, al): (expect(s, al), expect(s, al[:-1])) for s, al in keys}


# ------------------------------------------------------------ comparisons ----
def within(got: float, exact: Fraction, rel: Fraction, absolute: Fraction = Fraction(0)) -> bool:
    return abs(Fraction(float(got)) - exact) <= rel * abs(exact) + absolute


def relerr(got: float, exact: Fraction) -> float:
    if exact == 0:
        return 0.0 if got == 0 else math.inf
    return float(abs(Fraction(float(got)) - exact) / abs(exact))


def check_estep(view: dict, alleles: np.ndarray, pt: dict, head_len: int, S: int, max_excluded: float = 0.25):
    """The E-step of an implementation against enumeration.

    view: ll, total[N], ncand[N], prior/posterior/weight[N][>=ncand],
    haps[i] = [(h0, h1)] per candidate, resolutions[N][2][L].

    Bounds, u = 2^-53, every term positive so no cancellation:
      prior      a chain of at most 2L+2 multiplications (per locus the two
                 transition probabilities multiplied, then into the running
                 likelihood; the final doubling is exact): gamma(2L+2);
      total      a sum of M_i terms of that kind, M_i the enumerator's count of
                 ordered phasings: gamma(2L+2+M_i);
      posterior  prior / total: the two bounds and one division;
      weight     posterior over the sum of at most S kept posteriors: twice
                 the posterior's bound, S additions, one division;
      LL         per individual the total's relative error (d log x = dx / x)
                 and a faithfully rounded log (2 u |log|), N additions, and
                 the same again for the float logs of this reference.
    Returns the largest observed errors relative to their bounds' unit u."""
    N, _, L = alleles.shape
    en = estep(alleles, pt, head_len)
    excluded = sum(e is None for e in en)
    assert excluded <= max_excluded * N, (excluded, N)
    kp = 2 * L + 2
    worst = dict(total=0.0, prior=0.0, posterior=0.0, weight=0.0)
    ll_ref, ll_abs, sum_abs_log, quirk_cut = [], Fraction(0), 0.0, 0
    for i, e in enumerate(en):
        if e is None:  # HEAD_QUIRK: the LL check below takes the implementation's own total
            ll_ref.append(math.log(float(view["total"][i])))
            sum_abs_log += abs(ll_ref[-1])
            continue
        assert e["M"] <= MAX_PHASINGS
        kt = kp + e["M"]
        assert e["total"] > 0
        assert within(view["total"][i], e["total"], gamma(kt)), (i, relerr(view["total"][i], e["total"]))
        worst["total"] = max(worst["total"], relerr(view["total"][i], e["total"]))
        positive = sorted((p for p in e["priors"].values() if p > 0), reverse=True)
        npos = min(S, len(positive))
        nc = int(view["ncand"][i])
        assert npos <= nc <= S, (i, nc, npos)
        # HOMOZYGOUS_CUT applies: a homozygous phasing exists and the lists are cut
        mixed_cut = len(positive) > S and all(a < 0 or b < 0 or a == b for a, b in zip(*alleles[i].tolist()))
        seen = set()
        cov = sum(e["priors"].get(k, 0) for k in _cand_keys(view, i, npos)) / e["total"]  # the kept posteriors
        for c in range(nc):
            pr, po, w = (float(view[k][i][c]) for k in ("prior", "posterior", "weight"))
            if c >= npos:  # reversed-homozygous links zeroed at HaploPair.cpp:53-60
                assert pr == 0.0 and w == 0.0, (i, c, pr, w)
                continue
            if not mixed_cut:
                # the S largest positive priors, in descending order (ties: equal values)
                assert within(pr, positive[c], gamma(kp)), (i, c, relerr(pr, positive[c]))
            h0, h1 = view["haps"][i][c]
            key = (h0, h1) if h0 <= h1 else (h1, h0)
            assert key in e["priors"], (i, c, "not a phasing of the genotype")
            assert key not in seen, (i, c, "candidate listed twice")
            seen.add(key)
            assert within(pr, e["priors"][key], gamma(kp)), (i, c, relerr(pr, e["priors"][key]))
            ex_po = e["priors"][key] / e["total"]
            assert within(po, ex_po, gamma(kp + kt + 1)), (i, c, relerr(po, ex_po))
            ex_w = ex_po / cov
            assert within(w, ex_w, gamma(2 * (kp + kt + 1) + S + 1)), (i, c, relerr(w, ex_w))
            worst["prior"] = max(worst["prior"], relerr(pr, e["priors"][key]))
            worst["posterior"] = max(worst["posterior"], relerr(po, ex_po))
            worst["weight"] = max(worst["weight"], relerr(w, ex_w))
        reported = [Fraction(float(view["prior"][i][c])) for c in range(npos)]
        assert all(x >= y * (1 - gamma(kp)) for x, y in zip(reported, reported[1:])), (i, "not in descending order")
        if mixed_cut:  # every phasing left out scores no more than the last one kept
            left_out = max(p if k[0] == k[1] else p / 2 for k, p in e["priors"].items() if k not in seen)
            assert reported[-1] >= left_out * (1 - gamma(2 * kp)), (i, float(reported[-1]), float(left_out))
            quirk_cut += 1
        # the selected pair is the first candidate (HaploBuilder.cpp:115)
        r = view["resolutions"][i]
        assert (tuple(int(a) for a in r[0]), tuple(int(a) for a in r[1])) == view["haps"][i][0], i
        lg = math.log(float(e["total"]))
        ll_ref.append(lg)
        sum_abs_log += abs(lg)
        ll_abs += gamma(kt) + U
    ref = math.fsum(ll_ref)
    bound = float(ll_abs) + float((4 + N) * U) * sum_abs_log
    assert abs(view["ll"] - ref) <= bound, (view["ll"], ref, bound)
    out = {k: v / float(U) for k, v in worst.items()}
    out["ll_abs"], out["ll_bound"], out["excluded"] = abs(view["ll"] - ref), bound, excluded
    out["homozygous_cut"] = quirk_cut
    return out


def _cand_keys(view, i, npos):
    out = []
    for c in range(npos):
        h0, h1 = view["haps"][i][c]
        out.append((h0, h1) if h0 <= h1 else (h1, h0))
    return out


def check_chain_equals_global(alleles: np.ndarray, pt: dict, head_len: int) -> int:
    """Number of enumerated haplotypes whose chain P(h) differs from the
    global-longest-match P(h) (0 on a mined table)."""
    t = Table(pt)
    ta = allele_table(alleles)
    skip = head_quirk(alleles, head_len)
    haps = set()
    for i in range(alleles.shape[0]):
        if not skip[i]:
            for h0, _ in phasings(alleles[i], ta):
                haps.add(h0)
    return sum(1 for h in haps if t.chain_prob(h, head_len) != t.chain_prob(h, head_len, global_match=True))


def check_mined_table(pt: dict, alleles: np.ndarray, min_freq: Fraction, min_len: int, max_len: int,
                      samples=None, allow_equal: bool = False):
    """A mined table against enumeration: the pattern set exactly, freq /
    prefix / tp within the bound, every successor.

    Bounds: from the genotypes an addend is a product over at most L loci of
    0.5 * (x0 + x1) with a rounded allele frequency: three roundings per
    locus, N positive addends, one division: gamma(3L + N + 2); from H
    samples the weights are data, H additions each for the matching and the
    total weight and one division: gamma(2H + 1); tp = freq / prefix: twice
    that and one division.

    Condition for comparing the set exactly: no visited candidate within 1e-9
    relative of min_freq, except exactly equal where `allow_equal` (genotype
    mining without missing data: every term is dyadic and the two sides are
    one correctly rounded division of the same rational)."""
    N, _, L = alleles.shape
    ta = allele_table(alleles)
    stored, visited = memo(("mine", _digest(alleles), min_freq, min_len, max_len,
                            None if samples is None else _digest(samples[0], samples[1])),
                           lambda: mine(alleles, min_freq, min_len, max_len, samples))
    eq, margin = threshold_margin(visited, min_freq)
    assert margin > 1e-9, margin
    assert eq == 0 or allow_equal, eq
    t = Table(pt)
    assert set(t.index) == set(stored), (sorted(set(t.index) ^ set(stored))[:5], t.n, len(stored))
    k = 3 * L + N + 2 if samples is None else 2 * len(samples[1]) + 1
    worst = 0.0
    for key, i in t.index.items():
        f, pre = stored[key]
        pre = Fraction(1) if pre is None or len(key[1]) == 1 else pre
        tp = f / pre if pre > 0 else f
        assert within(pt["freq"][i], f, gamma(k)), (key, relerr(pt["freq"][i], f))
        assert within(pt["prefix"][i], pre, gamma(k)), (key, relerr(pt["prefix"][i], pre))
        assert within(pt["tp"][i], min(tp, 1), gamma(2 * k + 1)), (key, relerr(pt["tp"][i], tp))
        worst = max(worst, relerr(pt["freq"][i], f), relerr(pt["tp"][i], tp))
    check_successors(pt, ta, L)
    return dict(worst_u=worst / float(U), equal_to_threshold=eq, margin=margin, patterns=t.n)


def check_successors(pt: dict, table_of_alleles, L: int):
    """Every successor of the table equals the rule's (rebuild_successors)."""
    t = Table(pt)
    succ = rebuild_successors(pt, table_of_alleles, L)
    got = np.asarray(pt["succ"])
    for i in range(t.n):
        end = t.start[i] + t.len[i]
        n = len(table_of_alleles[end]) if end < L else 0
        assert np.array_equal(got[i, :n], succ[i, :n]), (i, t.start[i], t.al[i], got[i], succ[i])


def check_mstep(new: dict, alleles: np.ndarray, prev: dict, head_len: int, fixed_point: bool):
    """The table of one exact M-step against enumeration.

    Floating-point part, per individual i (every term positive): the genotype
    probability carries gamma(2L+2+M_i); a pattern's numerator is a sum over
    pairs of states of forward likelihood x transition probabilities x
    backward likelihood, at most 4L+4 multiplications and, the forward and
    the backward sums each merging at most M_i phasings, 2 M_i additions; one
    division: k_i = 6L + 8 + 3 M_i.  Over N individuals N additions, then the
    division by N: gamma(max k_i + N + 1) relative on freq and prefix.

    Fixed-point part (`fixed_point`: the library and the device-order
    restatement): each individual's term is rounded to a multiple of 2^-44
    before it is added (exact.hpp:9 EXACT_FIXED_SCALE, exact.hip:604-605 and
    :891-892 __double2ll_rn(freq * 2^44), one addend per individual and
    pattern; hmc_oracle.cpp xwalk llrint), the integer total converts exactly
    (N 2^44 < 2^53) and is divided by N (ctx_exact.cpp:160-164): at most
    N * 2^-45 on f and pre, 2^-45 absolute on freq and prefix.

    tp = f / pre with errors a_f, a_p: |tp' - tp| <= (a_f + tp a_p) /
    (pre - a_p) + u tp.  Returns the worst errors and the loosest relative
    bound met at a non-zero frequency."""
    N, _, L = alleles.shape
    t = Table(new)
    en = estep(alleles, prev, head_len)
    assert all(e is not None for e in en), "the exact M-step sums over every individual: no HEAD_QUIRK ones"
    ex = memo(("mstep", _digest(alleles), Table(prev).key, head_len, tuple(sorted(t.index))),
              lambda: mstep(alleles, prev, head_len, list(t.index)))
    k = max(6 * L + 8 + 3 * e["M"] for e in en) + N + 1
    q = FIXED_QUANTUM / 2 if fixed_point else Fraction(0)  # per individual, absolute, on f and pre
    worst = dict(freq=0.0, prefix=0.0, tp=0.0, loosest_rel_bound=0.0)
    for key, i in t.index.items():
        f, pre = ex[key]
        f = min(f, pre, N)
        a_f, a_p = gamma(k) * f + N * q, gamma(k) * pre + N * q
        if len(key[1]) == 1:
            assert pre == N
        assert abs(Fraction(float(new["freq"][i])) - f / N) <= a_f / N, (key, relerr(new["freq"][i], f / N))
        assert abs(Fraction(float(new["prefix"][i])) - pre / N) <= a_p / N, (key, relerr(new["prefix"][i], pre / N))
        tp = f / pre if pre > 0 else f / N
        if pre > a_p:
            b_tp = (a_f + tp * a_p) / (pre - a_p) + U * tp
            assert abs(Fraction(float(new["tp"][i])) - min(tp, 1)) <= b_tp, (key, relerr(new["tp"][i], tp))
            if tp > 0:
                worst["loosest_rel_bound"] = max(worst["loosest_rel_bound"], float(b_tp / tp))
        if f > 0:
            worst["loosest_rel_bound"] = max(worst["loosest_rel_bound"], float(a_f / f))
            worst["freq"] = max(worst["freq"], relerr(new["freq"][i], f / N))
            worst["tp"] = max(worst["tp"], relerr(new["tp"][i], tp))
        if pre > 0:
            worst["prefix"] = max(worst["prefix"], relerr(new["prefix"][i], pre / N))
    return worst
