"""The enumerated genotype posteriors (tests/posterior_enumeration.py) on the
panels of tests/test_enumeration_oracle.py, with the table the CPU restatement
mines from the genotypes (M0): what tests/test_gpu_posteriors.py holds the
library against must itself be a distribution, respect the known allele and
not be constant.
"""
import os
import sys
from fractions import Fraction

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import enumeration as en  # noqa: E402
import posterior_enumeration as pe  # noqa: E402
from test_enumeration_oracle import PANELS, build_panel, head_len, make_oracle  # noqa: E402

# sites of the individuals the enumeration covers, and those with both alleles missing
SITES = {"a3": (12, 0), "a4": (15, 2), "hom": (5, 2), "mc": (3, 0), "short": (9, 0)}


@pytest.mark.parametrize("name", sorted(SITES))
def test_enumerated_posteriors(oracle_mod, name):
    a = build_panel(name)
    hl = head_len(name)
    o = make_oracle(oracle_mod, name, PANELS[name]["S"][0], a)
    o.find_patterns()
    assert o.head_len() == hl
    post = pe.site_posteriors(a, o.patterns(), hl)
    quirk = en.head_quirk(a, hl)
    want = [(i, k) for i, k in pe.sites(a) if not quirk[i]]
    assert sorted(post) == want
    assert (len(want), sum(1 for i, k in want if a[i, 0, k] < 0 and a[i, 1, k] < 0)) == SITES[name]
    assert all(k >= hl for _, k in want), "a site at a head locus of a non-quirk individual"
    assert any(k == a.shape[2] - 1 for _, k in want), "no site at the last locus"
    spread = 0
    for (i, k), row in post.items():
        assert sum(row.values()) == 1, (i, k)
        assert all(p >= 0 for p in row.values())
        g = [int(a[i, 0, k]), int(a[i, 1, k])]
        known = [x for x in g if x >= 0]
        if known:  # one allele missing: every positive pair holds the known one
            assert all(known[0] in key for key, p in row.items() if p > 0), (i, k, row)
        spread += sum(1 for p in row.values() if p > 0) >= 2
    assert spread >= 1, "every site has a single positive pair"
    print(name, len(want), "sites,", spread, "with two or more positive pairs; smallest positive posterior",
          float(min((p for r in post.values() for p in r.values() if p > 0), default=Fraction(0))))
