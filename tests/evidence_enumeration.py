"""MAP phasing under phase evidence by exhaustive enumeration: the consistency
of a pair with caller-given phase sets, the exact constrained maximum, the
exact P(evidence | genotype), the acceptance predicate of a constrained MAP
phaser and a model of the host plan's checks.

Built on draw_enumeration.pair_posteriors_exact alone (exact rationals over
every phasing of an individual); this module imports neither the product nor
the restatement.

Evidence is a list of entries (individual, locus, set, first): in phase set
`set` (a name only) of the individual, the allele with symbol `first` at
`locus` lies on the set's first haplotype.  A pair {h0, h1} is consistent with
a set when one of its two haplotypes carries `first` at every locus of the set
(which of the two may differ from set to set), and with the evidence when it
is consistent with every set of the individual.

Acceptance is map_enumeration's argument unchanged: the filter is exact (a
label is kept or stored as 0, never rounded), and the sweep compares computed
path values of at most 2L + 2 roundings each, so the returned pair c is
accepted iff it is consistent and
    e_c >= e*_E (1 - g) / (1 + g),   g = gamma(2L + 2),
with e*_E the largest exact posterior of any consistent pair.

Bound of `evidence` = P(evidence | genotype) = (sum over consistent paths) /
P(genotype), every term positive, so relative errors compose:
  numerator    a path's product carries at most 2L + 2 roundings (as above);
               the ordered sums that bring it to the total are additions of
               non-negative numbers, and every addition a path's value passes
               through merges in at least one other lattice path, distinct for
               distinct additions, so at most M - 1 of them (M = the
               individual's ordered phasings, which bounds its lattice paths);
               the two labels of a state are added once wherever a span record
               is read as one value: at most once per record, L in all; the
               rescaling by powers of two is exact:  2L + 2 + M + L;
  denominator  the genotype probability carries gamma(2L + 2 + M)
               (enumeration.check_mstep; the draws' bound uses the same);
  the division one more:
    evidence_k(L, M) = 5L + 5 + 2M.
Derived, not tuned.
"""
from __future__ import annotations

from fractions import Fraction

import draw_enumeration as de
import enumeration as en
import map_enumeration as me


def sets_of(entries, i) -> dict:
    """{set: [(locus, first)]} of individual i."""
    out = {}
    for ii, k, s, f in entries:
        if int(ii) == i:
            out.setdefault(int(s), []).append((int(k), int(f)))
    return out


def consistent(pair, entries, i) -> bool:
    """The pair (h0, h1) of individual i against its sets."""
    h0, h1 = pair
    for loci in sets_of(entries, i).values():
        if not (all(h0[k] == f for k, f in loci) or all(h1[k] == f for k, f in loci)):
            return False
    return True


def constrained_exact(post: dict, entries, i) -> dict:
    """post = {pair: exact posterior} of individual i -> dict(evidence = the sum
    over consistent pairs, best = the largest consistent posterior (0 if none),
    argmax = the consistent pairs that attain it, post = the consistent pairs)."""
    ok = {k: p for k, p in post.items() if consistent(k, entries, i)}
    best = max(ok.values(), default=Fraction(0))
    return dict(evidence=sum(ok.values(), Fraction(0)), best=best, argmax={k for k, p in ok.items() if p == best and p > 0},
                post=ok)


def accepts(pair, e_c, entries, i, best_given: Fraction, L: int) -> bool:
    """The predicate: the pair is consistent and its exact posterior e_c is
    within the sweep's comparison bound of the constrained maximum."""
    return consistent(pair, entries, i) and best_given > 0 and me.accepts(e_c, best_given, L)


def evidence_k(L: int, M: int) -> int:
    return 5 * L + 5 + 2 * M


def het_loci(g) -> list:
    return [k for k in range(g.shape[1]) if g[0, k] >= 0 and g[1, k] >= 0 and g[0, k] != g[1, k]]


def spell(pair, i, groups, first_set=0) -> list:
    """Entries that spell the phase of `pair` (h0, h1) of individual i over the
    groups of loci given, one set per group, h0 as every set's first haplotype."""
    return [(i, k, first_set + s, int(pair[0][k])) for s, loci in enumerate(groups) for k in loci]


def flipped(entries, alleles, which) -> list:
    """The entries with the sets of `which` = {(individual, set)} flipped wholesale."""
    out = []
    for i, k, s, f in entries:
        if (i, s) in which:
            a0, a1 = int(alleles[i, 0, k]), int(alleles[i, 1, k])
            f = a1 if f == a0 else a0
        out.append((i, k, s, f))
    return out


# The host plan's checks (hmc_amd/csrc/evidence_plan.hpp), restated: what the
# call answers for a table of entries when every individual is asked for.
OK, EARG, EUNSUPPORTED = 0, -1, -4  # include/hmc_amd.h


def plan_model(alleles, entries):
    """(code, offender): (OK, None), (EARG, the first offending entry) or
    (EUNSUPPORTED, the first individual with interleaving sets)."""
    N, _, L = alleles.shape
    seen = set()
    for e, (i, k, s, f) in enumerate(entries):
        if not 0 <= i < N:
            return EARG, e
        if not 0 <= k < L:
            return EARG, e
        a0, a1 = int(alleles[i, 0, k]), int(alleles[i, 1, k])
        if a0 < 0 or a1 < 0 or a0 == a1 or f not in (a0, a1) or (i, k) in seen:
            return EARG, e
        seen.add((i, k))
    for i in range(N):
        spans = sorted((min(k for k, _ in v), max(k for k, _ in v)) for v in sets_of(entries, i).values() if len(v) > 1)
        for (f0, l0), (f1, l1) in zip(spans, spans[1:]):
            if f1 < l0:
                return EUNSUPPORTED, i
    return OK, None
