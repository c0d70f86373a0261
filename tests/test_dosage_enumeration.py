"""The dosage enumerator (tests/dosage_enumeration.py) against what is already
pinned, on the CPU restatement's M0 table of every enumeration panel: what
tests/test_gpu_haplotype_dosages.py holds the library against must itself be
right.

  one-sided length-1 dosages over a locus's alleles sum to exactly 2, and at a
      locus typed in the input each allele's dosage is its count in the genotype;
  a two-sided spec on two heterozygous loci with -1 between them is
      pair_enumeration's cis / trans, exactly;
  a fully specified spec is draw_enumeration.pair_posteriors_exact's posterior
      of that pair, exactly (twice it for a homozygous pair: two terms always);
  an absent symbol gives 0, the all -1 pattern 2.

It also asserts the non-vacuity condition of the GPU test: on every panel the
pattern set dosage_enumeration.panel_patterns has at least 100 exact values in
(0.05, 0.95) or (1.05, 1.95), spread over at least 5 individuals.
"""
from fractions import Fraction

import pytest

import dosage_enumeration as dn
import draw_enumeration as de
import enumeration as en
import pair_enumeration as pe
from test_enumeration_oracle import PANELS, build_panel, head_len, make_oracle

MIN_MIXED, MIN_MIXED_INDIVIDUALS = 100, 5


def m0_table(oracle_mod, name):
    a = build_panel(name)
    hl = head_len(name)
    o = make_oracle(oracle_mod, name, PANELS[name]["S"][0], a)
    o.find_patterns()
    assert o.head_len() == hl
    return a, hl, o.patterns()


@pytest.mark.parametrize("name", sorted(PANELS))
def test_enumerated_dosages(oracle_mod, name):
    a, hl, pt = m0_table(oracle_mod, name)
    N, _, L = a.shape
    ta = en.allele_table(a)
    covered = [i for i in range(N) if not en.head_quirk(a, hl)[i]]
    # one-sided, one locus: the alleles' dosages sum to 2; a typed locus gives the genotype's counts
    single = [(k, (s,), None) for k in range(L) for s, _ in ta[k]]
    d = dn.dosages_exact(a, pt, hl, single)
    assert [row is None for row in d] == en.head_quirk(a, hl).tolist()
    for i in covered:
        at = 0
        for k in range(L):
            vals = d[i][at:at + len(ta[k])]
            assert sum(vals) == 2 and all(0 <= v <= 2 for v in vals)
            if (a[i, :, k] >= 0).all():
                assert vals == [Fraction(int((a[i, :, k] == s).sum())) for s, _ in ta[k]]
            at += len(ta[k])
    # two heterozygous loci, -1 between: cis and trans
    queries = [q for q in pe.all_pairs(a) if q[0] in covered]
    exact = pe.pair_posteriors(a, pt, hl, queries)
    specs = []
    for i, x, y in queries:
        lx, hx, ly, hy = (int(v) for v in (a[i, :, x].min(), a[i, :, x].max(), a[i, :, y].min(), a[i, :, y].max()))
        gap = (dn.ANY,) * (y - x - 1)
        specs += [(x, (lx,) + gap + (ly,), (hx,) + gap + (hy,)), (x, (lx,) + gap + (hy,), (hx,) + gap + (ly,))]
    d = dn.dosages_exact(a, pt, hl, specs)
    assert len(queries) >= 10
    for q, (i, x, y) in enumerate(queries):
        assert (d[i][2 * q], d[i][2 * q + 1]) == exact[i, x, y], (i, x, y)
    # every locus given: the posterior of that whole pair
    post = de.pair_posteriors_exact(a, pt, hl)
    for i in covered:
        pairs = sorted(post[i])
        d = dn.dosages_exact(a, pt, hl, [(0, h0, h1) for h0, h1 in pairs])
        for (h0, h1), v in zip(pairs, d[i]):
            assert v == post[i][h0, h1] * (2 if h0 == h1 else 1), (i, h0, h1)
        swapped = dn.dosages_exact(a, pt, hl, [(0, h1, h0) for h0, h1 in pairs])
        assert swapped[i] == d[i]  # which row is A carries no information
    # an absent symbol; the all -1 pattern
    d = dn.dosages_exact(a, pt, hl, [(0, (dn.ABSENT,), None), (L - 2, (dn.ANY, dn.ABSENT), None), (0, (dn.ANY,) * L, None),
                                    (1, (dn.ANY,) * 2, (dn.ANY,) * 2), (0, (dn.ANY, dn.ABSENT), (dn.ANY, dn.ANY))])
    for i in covered:
        assert d[i] == [0, 0, 2, 2, 0]
    # the GPU test's value comparison is not vacuous
    pats = dn.panel_patterns(a, pt, hl)
    mixed, who = dn.mixed_values(dn.dosages_exact(a, pt, hl, pats))
    print(name, len(pats), "patterns;", mixed, "mixed values over", who, "individuals")
    assert mixed >= MIN_MIXED and who >= MIN_MIXED_INDIVIDUALS


def test_two_locus_known_answer():
    """Two SNP loci, one double heterozygote and a table that makes the cis
    phasing three times as likely as the trans one (the panel of
    test_pair_enumeration's known answer, rebuilt here by hand)."""
    import numpy as np

    one, two = 1, 2
    a = np.array([[[one, one], [two, two]]], np.int32)  # genotype 1/2, 1/2
    # patterns of length 2 at start 0 with freq as joint probabilities: P(11) = P(22) = 3/8, P(12) = P(21) = 1/8
    pt = dict(start=np.zeros(4, np.int32), len=np.full(4, 2, np.int32),
              alleles=np.array([[one, one], [one, two], [two, one], [two, two]], np.int32),
              freq=np.array([0.375, 0.125, 0.125, 0.375]), tp=np.ones(4), succ=np.full((4, 2), -1, np.int32))
    d = dn.dosages_exact(a, pt, 2, [(0, (one, one), None), (0, (one, two), None), (0, (one, one), (two, two)),
                                    (0, (one, two), (two, one)), (0, (one,), None), (0, (dn.ANY, dn.ANY), None)])
    # pairs {11, 22}: 2 * 9/64, {12, 21}: 2 * 1/64: posteriors 9/10 and 1/10
    assert d[0] == [Fraction(9, 10), Fraction(1, 10), Fraction(9, 10), Fraction(1, 10), 1, 2]
