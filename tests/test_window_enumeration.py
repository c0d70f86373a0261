"""The window enumerator (tests/window_enumeration.py) against what is already
pinned, on the CPU restatement's M0 table of the enumeration panels: what
tests/test_gpu_window_phasings.py holds the library against must itself be
right.

  every window's posteriors sum to exactly 1;
  a window equal to the whole panel is ranked_enumeration.ranked_exact, pair
      for pair in the same order;
  a window whose only branching loci are two heterozygous ones has two rows,
      pair_enumeration's cis and trans, exactly;
  every enumerated window pair is a restriction of a phasing of the genotype,
      and no more pairs have a positive posterior than C allows.

It also asserts that the panels give the GPU test its cases: windows with three
or more heterozygous loci, a missing allele inside a window, a window pair of
positive posterior whose two haplotypes are equal, and exact ties.
"""
from fractions import Fraction

import pytest

import enumeration as en
import pair_enumeration as pe
import ranked_enumeration as re_
import window_enumeration as wn
from test_dosage_enumeration import m0_table

NAMES = ["snp", "a3", "a4", "short", "mc", "minlen2"]


@pytest.mark.parametrize("name", NAMES)
def test_enumerated_windows(oracle_mod, name):
    a, hl, pt = m0_table(oracle_mod, name)
    N, _, L = a.shape
    ta = en.allele_table(a)
    wins = wn.windows_of(L)
    assert {n for _, n in wins} == {1, 2, 3, (L + 1) // 2, L}
    exact = wn.window_exact(a, pt, hl, wins)
    assert [e is None for e in exact] == en.head_quirk(a, hl).tolist()
    ranked = re_.ranked_exact(a, pt, hl)
    het3 = missing = equal = ties = two_het = 0
    for i, per in enumerate(exact):
        if per is None:
            continue
        g = a[i]
        het = pe.het_loci(g)
        for (s, n), rows in per.items():
            assert sum(p for _, p in rows) == 1 and all(rows[r][1] >= rows[r + 1][1] for r in range(len(rows) - 1))
            assert all(x <= y for (x, y), _ in rows) and len({k for k, _ in rows}) == len(rows)
            C = wn.config_count(g, ta, s, n)
            assert {k for k, _ in rows} <= wn.restrictions(g, ta, s, n) and wn.positive(rows) <= len(rows) <= C
            inside = [k for k in het if s <= k < s + n]
            het3 += len(inside) >= 3
            missing += bool((g[:, s:s + n] < 0).any())
            equal += any(x == y and p > 0 for (x, y), p in rows)
            ties += any(rows[r][1] == rows[r + 1][1] > 0 for r in range(len(rows) - 1))
            if n == L:  # the whole panel: the ranked enumeration
                assert rows == ranked[i]
            fixed = [k for k in range(s, s + n) if k not in inside]
            if len(inside) == 2 and all(g[0, k] == g[1, k] >= 0 for k in fixed):  # two heterozygous loci and fixed ones
                x, y = inside
                cis, trans = pe.pair_posteriors(a, pt, hl, [(i, x, y)])[i, x, y]
                got = {(h0[x - s] < h1[x - s]) == (h0[y - s] < h1[y - s]): p for (h0, h1), p in rows}
                assert len(rows) == 2 and got[True] == cis and got[False] == trans, (i, s, n)
                two_het += 1
    print(name, dict(windows=len(wins), het3=het3, missing=missing, equal=equal, ties=ties, two_het=two_het))
    assert het3 >= 1 and two_het >= 1 and equal >= 1
    if (a < 0).any():
        assert missing >= 1


def test_panels_give_the_gpu_test_its_cases(oracle_mod):
    """snp, a3, a4 and short: individuals with up to 8 heterozygous loci and 1 to 4 missing alleles."""
    most_het, miss = 0, set()
    for name in ("snp", "a3", "a4", "short"):
        a, hl, pt = m0_table(oracle_mod, name)
        for g in a:
            most_het = max(most_het, len(pe.het_loci(g)))
            if (g < 0).any():
                miss.add(int((g < 0).sum()))
    assert most_het == 8 and {1, 4} <= miss and min(miss) == 1, (most_het, miss)


def test_two_locus_known_answer():
    """test_dosage_enumeration's hand-made table: cis three times as likely as trans."""
    import numpy as np

    one, two = 1, 2
    a = np.array([[[one, one], [two, two]]], np.int32)
    pt = dict(start=np.zeros(4, np.int32), len=np.full(4, 2, np.int32),
              alleles=np.array([[one, one], [one, two], [two, one], [two, two]], np.int32),
              freq=np.array([0.375, 0.125, 0.125, 0.375]), tp=np.ones(4), succ=np.full((4, 2), -1, np.int32))
    per = wn.window_exact(a, pt, 2, [(0, 2), (0, 1), (1, 1)])[0]
    assert per[0, 2] == [(((one, one), (two, two)), Fraction(9, 10)), (((one, two), (two, one)), Fraction(1, 10))]
    assert per[0, 1] == per[1, 1] == [(((one,), (two,)), Fraction(1))]
    assert wn.config_count(a[0], en.allele_table(a), 0, 2) == 4
