"""The enumerated switch posteriors (tests/switch_enumeration.py) on the
panels of tests/test_enumeration_oracle.py, with the table the CPU restatement
mines from the genotypes (M0): what tests/test_gpu_switch_posteriors.py holds
the library against must itself be a distribution over {cis, trans}, must not
depend on the order of an individual's two input rows, must reach sites with a
gap and sites anchored in the head, and must not be trivial (0 or 1).

Known answer (test_two_locus_known_answer), one individual, two loci, alleles
1 and 2 at both, head_len 1.  Table: (0, "1") and (0, "2") with frequency 1/2;
transition probabilities of the patterns of length two (0, "11") 3/4,
(0, "12") 1/4, (0, "22") 1/2, (0, "21") 1/2.  So P(11) = 1/2 x 3/4 = 3/8,
P(12) = 1/8, P(22) = 1/4, P(21) = 1/4.  The genotype {1, 2} {1, 2} has the
phasings {11, 22}, the lower alleles together (cis), of prior 2 x 3/8 x 1/4 =
3/16, and {12, 21} (trans) of prior 2 x 1/8 x 1/4 = 1/16: cis = 3/4, trans =
1/4.
"""
import os
import sys
from fractions import Fraction

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import enumeration as en  # noqa: E402
import switch_enumeration as se  # noqa: E402
from test_enumeration_oracle import PANELS, build_panel, head_len, make_oracle  # noqa: E402

# panel: sites, sites of the individuals the enumeration covers (not HEAD_QUIRK), sites with
# a < head_len, sites with b - a > 1 (the last two among the enumerated ones)
COUNTS = {"snp": (34, 34, 6, 15), "a3": (27, 25, 6, 10), "a4": (15, 15, 5, 7), "mc": (27, 26, 11, 13),
          "short": (37, 36, 5, 13), "minlen2": (23, 23, 9, 9), "hom": (25, 25, 4, 9)}


def counts(a, hl):
    quirk = en.head_quirk(a, hl)
    s = se.sites(a)
    e = [x for x in s if not quirk[x[0]]]
    return len(s), len(e), sum(1 for _, x, _ in e if x < hl), sum(1 for _, x, y in e if y - x > 1)


@pytest.mark.parametrize("name", sorted(COUNTS))
def test_enumerated_switch_posteriors(oracle_mod, name):
    a = build_panel(name)
    hl = head_len(name)
    o = make_oracle(oracle_mod, name, PANELS[name]["S"][0], a)
    o.find_patterns()
    assert o.head_len() == hl
    pt = o.patterns()
    post = se.switch_posteriors(a, pt, hl)
    quirk = en.head_quirk(a, hl)
    want = [s for s in se.sites(a) if not quirk[s[0]]]
    assert sorted(post) == want
    assert counts(a, hl) == COUNTS[name]
    for (i, x, y), (cis, trans) in post.items():
        assert x < y and all(a[i, 0, k] < 0 or a[i, 1, k] < 0 or a[i, 0, k] == a[i, 1, k] for k in range(x + 1, y))
        assert cis + trans == 1, (i, x, y)
        assert 0 < cis < 1, (i, x, y, cis)  # mixed: no site passes on a trivial 0 or 1
    # an individual's two input rows swapped: the same sites, the same numbers
    swapped = se.switch_posteriors(np.ascontiguousarray(a[:, ::-1]), pt, hl)
    assert swapped == post
    small = [min(c, t) for c, t in post.values()]
    print(name, len(want), "sites; the smaller of cis and trans from", float(min(small)), "to", float(max(small)))
    assert Fraction(4, 100) < min(small) and max(small) <= Fraction(1, 2)


def test_two_locus_known_answer():
    a = np.array([[[ord("1"), ord("1")], [ord("2"), ord("2")]]], np.int32)
    one, two = ord("1"), ord("2")
    pats = [((one,), 0.5, 1.0), ((two,), 0.5, 1.0), ((one, one), 0.0, 0.75), ((one, two), 0.0, 0.25),
            ((two, two), 0.0, 0.5), ((two, one), 0.0, 0.5)]
    al = np.full((len(pats), 2), -1, np.int32)
    for i, (s, _, _) in enumerate(pats):
        al[i, :len(s)] = s
    pt = dict(start=np.zeros(len(pats), np.int32), len=np.array([len(s) for s, _, _ in pats], np.int32), alleles=al,
              freq=np.array([f for _, f, _ in pats]), tp=np.array([t for _, _, t in pats]))
    assert se.sites(a) == [(0, 0, 1)]
    assert se.switch_posteriors(a, pt, 1) == {(0, 0, 1): (Fraction(3, 4), Fraction(1, 4))}
    # the rows swapped, and the table's two transition pairs swapped: the answer follows the alleles
    assert se.switch_posteriors(a[:, ::-1].copy(), pt, 1) == {(0, 0, 1): (Fraction(3, 4), Fraction(1, 4))}
    pt["tp"] = np.array([1.0, 1.0, 0.25, 0.75, 0.5, 0.5])
    assert se.switch_posteriors(a, pt, 1) == {(0, 0, 1): (Fraction(1, 4), Fraction(3, 4))}
