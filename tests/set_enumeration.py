"""Which patterns the exact M-step and findPatternByNum keep, and in which
order, by the reference's selection rules on enumerated frequencies.

enumeration.mstep gives freq / prefix of whatever keys it is handed, and
enumeration.mine covers findPatternByFreq; the two selections that neither
states are stated here, in exact rational arithmetic and without a trie, a
lattice or a walk:

  estimate_patterns_set  PatternManager::estimatePatterns + extendPatterns
                         (PatternManager.cpp:364-438): seeds, four-level
                         extension rounds on inherited frequencies, the final
                         filter, creation order;
  find_patterns_by_num   PatternManager::findPatternByNum (:44-70): rounds of
                         searchPattern(true) (:100-144) at thresholds 1.0,
                         x 0.9, ... with reserved candidates, the last
                         round's tail sorted by frequency and cut.

check_pattern_set holds a table to such a list: set, order, successors, and
the conditions under which a set decided by exact frequencies can be demanded
of an implementation that decides in doubles.  Like enumeration.py this module
imports neither the product nor the restatement.
"""
from __future__ import annotations

import math
from fractions import Fraction

import numpy as np

import enumeration as en

MARGIN = 1e-9  # the relative distance from a threshold that check_mined_table demands


def table_keys(pt: dict) -> list:
    """(start, symbols) of every pattern, in table order."""
    t = en.Table(pt)
    return [(t.start[i], t.al[i]) for i in range(t.n)]


def _lengths(L: int, min_len: int, max_len: int):
    """PatternManager.cpp:30-32 / :48-50."""
    min_len = max(min_len, 1)
    return min_len, max(L if max_len <= 0 else max_len, min_len)


# ------------------------------------------------------------ exact M-step ----
def estimate_patterns_set(alleles: np.ndarray, prev: dict, head_len: int, min_freq: Fraction, min_len: int,
                          max_len: int):
    """The table of PatternManager::estimatePatterns (PatternManager.cpp:
    364-410) after the E-step on `prev`, as an ordered list of keys.

    min_freq < 0 (:369-370): estimateFrequency, the same patterns in place.
    Otherwise, walking `prev` in table order (:373-389): every pattern is a
    candidate, and behind it, if its end < L and its length < max_len, comes
    its extension by every allele index j of the locus at its end whose
    successor (the rule of :308-317, rebuilt here, not read from prev["succ"])
    is missing or starts elsewhere; those extensions are the seeds.  Then
    rounds (:390-395) until one has nothing to estimate: the new candidates
    get their frequency, min(f, pre, N) / N of enumeration.mstep
    (HaploBuilder.cpp:317-331), and extendPatterns (:412-438) runs four
    levels: a seed with end < L, length < max_len and frequency >= min_freq is
    extended by every allele index of the next locus — alleles of zero
    frequency too —, the extension inherits the seed's frequency (:428), is a
    candidate, and is a seed of the next level; so levels 2-4 extend on the
    frequency of the level-1 seed, not on their own, and only the last level's
    extensions seed the next round.  At the end (:397-406) a candidate stays
    if its frequency >= min_freq or its length <= min_len, in creation order.

    Returns (kept, info): rounds (estimations with something to estimate),
    added (candidates each round's extendPatterns created), candidates, kept,
    equal (candidates whose frequency equals min_freq) and margin (smallest
    relative distance of any other candidate's frequency from min_freq)."""
    N, _, L = alleles.shape
    ta = en.allele_table(alleles)
    t = en.Table(prev)
    prev_keys = [(t.start[i], t.al[i]) for i in range(t.n)]
    if min_freq < 0:
        return prev_keys, dict(rounds=1, added=[], candidates=t.n, kept=t.n, equal=0, margin=math.inf)
    min_len, max_len = _lengths(L, min_len, max_len)
    succ = en.rebuild_successors(prev, ta, L)
    freq = {}  # a candidate's frequency as extendPatterns reads it: inherited, then estimated

    def estimate(keys):
        for key, (f, pre) in en.mstep(alleles, prev, head_len, keys).items():
            freq[key] = min(f, pre, N) / N

    def extensible(key):
        return key[0] + len(key[1]) < L and len(key[1]) < max_len

    cands, seeds = [], []
    for i, key in enumerate(prev_keys):
        cands.append(key)
        if extensible(key):
            for j, (sym, _) in enumerate(ta[key[0] + len(key[1])]):
                if succ[i, j] < 0 or t.start[succ[i, j]] != key[0]:
                    cands.append((key[0], key[1] + (sym,)))
                    seeds.append(cands[-1])
    begin, added = 0, []
    while begin < len(cands):
        estimate(cands[begin:])
        begin = len(cands)
        for _ in range(4):
            nxt = []
            for key in seeds:
                if extensible(key) and freq[key] >= min_freq:
                    for sym, _ in ta[key[0] + len(key[1])]:
                        new = (key[0], key[1] + (sym,))
                        freq[new] = freq[key]
                        cands.append(new)
                        nxt.append(new)
            seeds = nxt
        added.append(len(cands) - begin)
    assert len(set(cands)) == len(cands), "a candidate created twice"
    kept = [k for k in cands if freq[k] >= min_freq or len(k[1]) <= min_len]
    eq, margin = en.threshold_margin([freq[k] for k in cands], min_freq)
    return kept, dict(rounds=len(added), added=added, candidates=len(cands), kept=len(kept), equal=eq, margin=margin)


# -------------------------------------------------------- findPatternByNum ----
def thresholds():
    """m_min_freq of the successive searches (PatternManager.cpp:55, :60): 1.0
    and its repeated products with 0.9, rounded to double each time."""
    theta = 1.0
    while True:
        yield theta
        theta *= 0.9


def find_patterns_by_num(alleles: np.ndarray, max_num: int, min_len: int, max_len: int, samples=None):
    """PatternManager::findPatternByNum (PatternManager.cpp:44-70).

    One candidate stack for all start loci (generateCandidates, :90-98: the
    empty strings of start 0 .. L-1, popped from the back).  A search at
    threshold theta (searchPattern(true), :100-144) pops until the stack is
    empty: a candidate with (freq >= theta or len < min_len), end < L and
    len < max_len pushes its extension by every allele of positive frequency;
    then, if (freq >= theta or len <= min_len), it is stored when 0 < len and
    len >= min_len and is gone either way — so a string of length exactly
    min_len below the threshold is stored without ever being extended —, and
    otherwise it is reserved: the reserved ones, in pop order, are the next
    search's stack.  The first search runs at 1.0; max_num becomes
    max(max_num, size); while size < max_num and theta > 1e-38, last_size =
    size, theta *= 0.9, search.  If size > max_num the patterns from last_size
    on are sorted by descending frequency and the list is cut at max_num.
    Frequencies are enumeration.matcher's, the ones `mine` uses.

    Returns (patterns, info): patterns = [((start, symbols), freq)] in table
    order; info = rounds, last_size, last_threshold (the double the exact
    M-step after this search filters by), sorted_from (last_size if the tail
    was sorted, else None), visited, equal_at_one / equal (visited candidates
    equal to the threshold of the search that popped them, at 1.0 / below),
    margin (smallest relative distance of any other visited candidate from
    that threshold), cut_gap (relative frequency gap across the cut) and
    tail_gap (smallest relative gap between different frequencies next to
    each other in the sorted tail)."""
    N, _, L = alleles.shape
    ta = en.allele_table(alleles)
    min_len, max_len = _lengths(L, min_len, max_len)
    root, extend = en.matcher(alleles, samples)
    stack = [(s, (), root, Fraction(1)) for s in range(L)]
    pats, seen = [], []

    def search(theta):
        nonlocal stack
        reserved = []
        while stack:
            s, al, state, freq = stack.pop()
            ln, end = len(al), s + len(al)
            if ln:
                seen.append((freq, theta))
            if (freq >= theta or ln < min_len) and end < L and ln < max_len:
                for a, af in ta[end]:
                    if af > 0:
                        st2, f2 = extend(state, end, a, af)
                        stack.append((s, al + (a,), st2, f2))
            if freq >= theta or ln <= min_len:
                if ln > 0 and ln >= min_len:
                    pats.append(((s, al), freq))
            else:
                reserved.append((s, al, state, freq))
        stack = reserved

    th = thresholds()
    theta, rounds, last_size = next(th), 1, 0
    search(Fraction(theta))
    max_num = max(max_num, len(pats))
    while len(pats) < max_num and theta > 1e-38:
        last_size, theta, rounds = len(pats), next(th), rounds + 1
        search(Fraction(theta))
    cut_gap = tail_gap = sorted_from = None
    if len(pats) > max_num:
        pats[last_size:] = sorted(pats[last_size:], key=lambda x: -x[1])  # ties: check_pattern_set compares them as sets
        sorted_from = last_size
        lo, hi = pats[max_num][1], pats[max_num - 1][1]
        cut_gap = float((hi - lo) / hi) if hi > 0 else 0.0
        pats = pats[:max_num]
        gaps = [(x[1] - y[1]) / x[1] for x, y in zip(pats[last_size:], pats[last_size + 1:]) if x[1] != y[1]]
        tail_gap = float(min(gaps)) if gaps else math.inf
    other = [abs(f - th_) / th_ for f, th_ in seen if f != th_]
    return pats, dict(rounds=rounds, last_size=last_size, last_threshold=theta, sorted_from=sorted_from,
                      patterns=len(pats), visited=len(seen),
                      equal_at_one=sum(1 for f, th_ in seen if f == th_ == 1),
                      equal=sum(1 for f, th_ in seen if f == th_ and th_ != 1),
                      margin=float(min(other)) if other else math.inf, cut_gap=cut_gap, tail_gap=tail_gap)


# ------------------------------------------------------------- comparison ----
def check_pattern_set(pt: dict, expected, info: dict, alleles: np.ndarray, allow_equal: bool = False):
    """A table's pattern set and order against an enumerated list.

    expected: keys, or (key, freq) pairs from find_patterns_by_num.

    Conditions on the enumeration alone, for demanding the set of an
    implementation that compares doubles (the margin of check_mined_table,
    far above the 4.1e-12 loosest relative bound of check_mstep):
      no candidate within 1e-9 relative of the threshold it was compared with;
      none equal to it — for the exact M-step never, since there the
      fixed-point walk decides; for findPatternByNum at threshold 1.0 (a
      candidate every item matches: the sum is N / N or W / W exactly) and
      under `allow_equal` (genotype mining without missing data, as in
      check_mined_table);
      the frequencies on the two sides of the cut, and any two different
      ones next to each other in the sorted tail, more than 1e-9 relative
      apart.
    Then: the same set; the same order, where inside the sorted tail a run of
    exactly equal enumerated frequencies is compared as a set (std::sort is
    not stable); every successor by the rule (check_successors)."""
    assert info["margin"] > MARGIN, info["margin"]
    assert info["equal"] == 0 or allow_equal, info["equal"]
    if info.get("cut_gap") is not None:
        assert info["cut_gap"] > MARGIN, info["cut_gap"]
        assert info["tail_gap"] > MARGIN, info["tail_gap"]
    pairs = [x if len(x) == 2 and isinstance(x[1], Fraction) else (x, None) for x in expected]
    keys = [k for k, _ in pairs]
    got = table_keys(pt)
    assert set(got) == set(keys), (sorted(set(got) ^ set(keys))[:5], len(got), len(keys))
    assert len(got) == len(keys), (len(got), len(keys))
    cut = info.get("sorted_from")
    cut = len(keys) if cut is None else cut
    first = next((i for i in range(cut) if got[i] != keys[i]), None)
    assert first is None, (first, got[first], keys[first])
    i = cut
    while i < len(keys):  # runs of equal frequency in the sorted tail
        j = i
        while j < len(keys) and pairs[j][1] == pairs[i][1]:
            j += 1
        assert set(got[i:j]) == set(keys[i:j]), (i, j, got[i:j], keys[i:j])
        i = j
    en.check_successors(pt, en.allele_table(alleles), alleles.shape[2])
    return dict(patterns=len(keys), margin=info["margin"], equal=info["equal"])
