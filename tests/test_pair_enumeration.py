"""The enumerated pair posteriors (tests/pair_enumeration.py) on the panels of
tests/test_enumeration_oracle.py, with the table the CPU restatement mines from
the genotypes (M0), over *all* pairs of heterozygous loci of every individual:
what tests/test_gpu_pair_posteriors.py holds the library against must itself
be a distribution over {cis, trans}, must not depend on the order of an
individual's two input rows, must agree with the consecutive enumerator
(tests/switch_enumeration.py) on span-1 queries, and must reach the shapes the
GPU test relies on — queries anchored in the head, queries inside it, queries
over homozygous or missing loci, queries three or more heterozygous loci
apart, and at least one individual with three or more anchor intervals open at
once (so that a sweep forced to two slots takes more than one round).

Known answer (test_three_locus_known_answer), one individual, three loci,
alleles 1 and 2 at each, head_len 1.  Table: (0, "1") and (0, "2") with
frequency 1/2; transition probabilities of the patterns of length two
11: 3/4, 12: 1/4, 22: 1/2, 21: 1/2, and of length three 111: 1/2, 112: 1/2,
121: 1/4, 122: 3/4, 221: 1/4, 222: 3/4, 211: 3/4, 212: 1/4.  So
  P(111) = 1/2 x 3/4 x 1/2 = 3/16    P(112) = 3/16
  P(121) = 1/2 x 1/4 x 1/4 = 1/32    P(122) = 3/32
  P(221) = 1/2 x 1/2 x 1/4 = 1/16    P(222) = 3/16
  P(211) = 1/2 x 1/2 x 3/4 = 3/16    P(212) = 1/16        (they sum to 1).
The genotype {1, 2} at all three loci has four phasings, priors 2 P(h0) P(h1):
  {111, 222} 18/256   {112, 221} 6/256   {121, 212} 1/256   {122, 211} 9/256,
total 34/256.  The haplotype with the lower allele (1) at the first locus of a
query has the lower allele at the second one (cis) in
  (0, 1): {111, 222}, {112, 221}   cis 24/34 = 12/17, trans 5/17;
  (1, 2): {111, 222}, {122, 211}   cis 27/34,         trans 7/34;
  (0, 2): {111, 222}, {121, 212}   cis 19/34,         trans 15/34.
The consecutive answers do not multiply to the distant one: 12/17 x 27/34 +
5/17 x 7/34 = 359/578 = 0.62, not 19/34 = 0.56 — the switches are not
independent under a variable-order chain.
"""
import os
import sys
from fractions import Fraction

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import enumeration as en  # noqa: E402
import pair_enumeration as pe  # noqa: E402
import switch_enumeration as se  # noqa: E402
from test_enumeration_oracle import PANELS, build_panel, head_len, make_oracle  # noqa: E402

NAMES = ["a3", "a4", "hom", "mc", "minlen2", "short", "snp"]  # the seven panels of test_switch_enumeration.COUNTS
# panel: all-pairs queries; those of the individuals the enumeration covers (not HEAD_QUIRK); among these: a inside
# the head and b outside it, both inside it, a homozygous or missing locus between a and b, b at least three
# heterozygous loci after a; and the largest number of anchor intervals of one individual open at once
COUNTS = {"a3": (68, 65, 20, 0, 28, 22, 6), "a4": (27, 27, 13, 0, 19, 3, 3), "hom": (63, 63, 17, 0, 34, 20, 5),
          "mc": (62, 61, 30, 5, 44, 17, 5), "minlen2": (56, 56, 28, 2, 19, 18, 7), "short": (101, 100, 24, 0, 62, 37, 6),
          "snp": (96, 96, 26, 0, 59, 36, 7)}


def counts(a, hl):
    quirk = en.head_quirk(a, hl)
    q = pe.all_pairs(a)
    e = [x for x in q if not quirk[x[0]]]
    het = {i: pe.het_loci(a[i]) for i in range(a.shape[0])}
    return (len(q), len(e), sum(1 for _, x, y in e if x < hl <= y), sum(1 for _, x, y in e if y < hl),
            sum(1 for i, x, y in e if any(k not in het[i] for k in range(x + 1, y))),
            sum(1 for i, x, y in e if het[i].index(y) - het[i].index(x) >= 3), pe.max_overlap(q))


def test_span_lists():
    a = build_panel("a3")
    assert pe.span_list(a, 1) == se.sites(a)
    most = max(len(pe.het_loci(a[i])) for i in range(a.shape[0]))
    assert pe.span_list(a, most) == pe.span_list(a, most + 5) == pe.all_pairs(a)
    s2 = pe.span_list(a, 2)
    assert s2 == sorted(s2) and len(set(s2)) == len(s2) and set(se.sites(a)) < set(s2) < set(pe.all_pairs(a))
    # three heterozygous loci with a homozygous one and a half-missing one between
    g = np.array([[[1, 1, 1, -1, 1], [2, 1, 2, 2, 2]]], np.int32)
    assert pe.span_list(g, 1) == [(0, 0, 2), (0, 2, 4)]
    assert pe.span_list(g, 2) == [(0, 0, 2), (0, 0, 4), (0, 2, 4)]
    assert pe.max_overlap(pe.span_list(g, 1)) == 1 and pe.max_overlap(pe.span_list(g, 2)) == 2


@pytest.mark.parametrize("name", NAMES)
def test_enumerated_pair_posteriors(oracle_mod, name):
    a = build_panel(name)
    hl = head_len(name)
    o = make_oracle(oracle_mod, name, PANELS[name]["S"][0], a)
    o.find_patterns()
    assert o.head_len() == hl
    pt = o.patterns()
    queries = pe.all_pairs(a)
    post = pe.pair_posteriors(a, pt, hl, queries)
    quirk = en.head_quirk(a, hl)
    assert sorted(post) == [q for q in queries if not quirk[q[0]]]
    c = counts(a, hl)
    print(name, "all-pairs queries", c[0], "largest number of overlapping anchor intervals of an individual", c[6], "counts", c)
    assert c == COUNTS[name]
    for (i, x, y), (cis, trans) in post.items():
        assert cis + trans == 1, (i, x, y)
        assert 0 < cis < 1, (i, x, y, cis)  # mixed: no query passes on a trivial 0 or 1
    # an individual's two input rows swapped: the same numbers
    assert pe.pair_posteriors(np.ascontiguousarray(a[:, ::-1]), pt, hl, queries) == post
    # span-1 queries are the consecutive enumerator's sites and answers
    sw = se.switch_posteriors(a, pt, hl)
    assert pe.pair_posteriors(a, pt, hl, pe.span_list(a, 1)) == sw
    assert all(post[k] == v for k, v in sw.items())


def test_panels_overlap_enough_for_rounds():
    """test_gpu_pair_posteriors forces two slots and asserts more than one
    round: some individual must have three or more intervals open at once."""
    assert set(COUNTS) == set(NAMES)
    assert max(c[6] for c in COUNTS.values()) >= 3
    assert all(c[6] >= 3 for c in COUNTS.values())  # (every panel does)
    assert sum(c[3] for c in COUNTS.values()) > 0 and all(c[2] > 0 and c[4] > 0 and c[5] > 0 for c in COUNTS.values())


def test_three_locus_known_answer():
    one, two = ord("1"), ord("2")
    a = np.array([[[one, one, one], [two, two, two]]], np.int32)
    pats = [((one,), 0.5, 1.0), ((two,), 0.5, 1.0), ((one, one), 0.0, 0.75), ((one, two), 0.0, 0.25),
            ((two, two), 0.0, 0.5), ((two, one), 0.0, 0.5),
            ((one, one, one), 0.0, 0.5), ((one, one, two), 0.0, 0.5), ((one, two, one), 0.0, 0.25),
            ((one, two, two), 0.0, 0.75), ((two, two, one), 0.0, 0.25), ((two, two, two), 0.0, 0.75),
            ((two, one, one), 0.0, 0.75), ((two, one, two), 0.0, 0.25)]
    al = np.full((len(pats), 3), -1, np.int32)
    for i, (s, _, _) in enumerate(pats):
        al[i, :len(s)] = s
    pt = dict(start=np.zeros(len(pats), np.int32), len=np.array([len(s) for s, _, _ in pats], np.int32), alleles=al,
              freq=np.array([f for _, f, _ in pats]), tp=np.array([t for _, _, t in pats]))
    queries = [(0, 0, 1), (0, 1, 2), (0, 0, 2)]
    assert pe.all_pairs(a) == sorted(queries)
    want = {(0, 0, 1): (Fraction(12, 17), Fraction(5, 17)), (0, 1, 2): (Fraction(27, 34), Fraction(7, 34)),
            (0, 0, 2): (Fraction(19, 34), Fraction(15, 34))}
    assert pe.pair_posteriors(a, pt, 1, queries) == want
    assert pe.pair_posteriors(a[:, ::-1].copy(), pt, 1, queries) == want
    c01, t01 = want[0, 0, 1]
    c12, t12 = want[0, 1, 2]
    assert c01 * c12 + t01 * t12 == Fraction(359, 578) != want[0, 0, 2][0]  # the consecutive answers do not multiply
