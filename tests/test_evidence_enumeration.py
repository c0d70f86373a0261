"""What tests/test_gpu_map_phase_given.py holds hmc_map_phase_given against,
checked without a GPU: the enumerator of tests/evidence_enumeration.py against
itself on panels of tests/test_enumeration_oracle.py, and the host plan
(hmc_amd/csrc/evidence_plan.hpp through the device-free seam
hmc_test_evidence_plan) against its restatement, every HMC_EARG case and
interleaved sets included.  Also the coverage the GPU test relies on: on each
of its seven panels at least 60 % of the individuals have two or more
heterozygous loci outside the head quirk, one has at least four, and every
phasing of every covered individual has a positive posterior under the M0
table (so no committed panel has impossible evidence)."""
import ctypes as C
import os
import sys
from fractions import Fraction

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import draw_enumeration as de  # noqa: E402
import enumeration as en  # noqa: E402
import evidence_enumeration as ee  # noqa: E402
import map_enumeration as me  # noqa: E402
from test_enumeration_oracle import PANELS, build_panel, head_len, make_oracle  # noqa: E402

PANEL_S = [("snp", 2), ("a3", 3), ("a4", 6), ("hom", 2), ("mc", 4), ("short", 5), ("minlen2", 10)]  # test_gpu_posterior_draws


def m0_posteriors(oracle_mod, name, S):
    a = build_panel(name)
    o = make_oracle(oracle_mod, name, S, a)
    o.find_patterns()
    hl = head_len(name)
    assert o.head_len() == hl
    return a, hl, de.pair_posteriors_exact(a, o.patterns(), hl)


def plan(a, entries):
    """hmc_test_evidence_plan: (code, message, events kept, individuals with events, events[n, 2])."""
    import hmc_amd
    a = np.ascontiguousarray(a, np.int32)
    N, _, L = a.shape
    cols = [np.ascontiguousarray([e[c] for e in entries], np.int32) for c in range(4)]
    p = lambda x: x.ctypes.data_as(C.POINTER(C.c_int32))  # noqa: E731
    msg = C.create_string_buffer(512)
    ne, nc = C.c_int64(0), C.c_int(0)
    out = np.zeros((max(len(entries), 1), 2), np.int32)
    rc = hmc_amd.lib().hmc_test_evidence_plan(N, L, p(a), len(entries), p(cols[0]), p(cols[1]), p(cols[2]), p(cols[3]), msg, 512,
                                              C.byref(ne), C.byref(nc), p(out), len(out))
    return rc, msg.value.decode(), ne.value, nc.value, out[:ne.value]


@pytest.mark.parametrize("name", ["snp", "a3", "hom"])
def test_enumerator_against_itself(oracle_mod, name):
    a, hl, post = m0_posteriors(oracle_mod, name, PANELS[name]["S"][0])
    L = a.shape[2]
    checked = rejected = 0
    for i, d in enumerate(post):
        het = ee.het_loci(a[i])
        if d is None or len(het) < 2:
            continue
        checked += 1
        best = max(d.values())
        top = max((k for k, p in d.items() if p == best))
        # evidence taken from an exact maximiser returns that maximum
        ev = ee.spell(top, i, [het])
        c = ee.constrained_exact(d, ev, i)
        assert c["best"] == best and top in c["argmax"] and 0 < c["evidence"] <= 1
        assert ee.accepts(top, d[top], ev, i, c["best"], L)
        # both orientations of a two-locus set sum to 1
        x, y = het[0], het[1]
        cis = [(i, x, 0, int(a[i, 0, x])), (i, y, 0, int(a[i, 0, y]))]
        trans = [(i, x, 0, int(a[i, 0, x])), (i, y, 0, int(a[i, 1, y]))]
        assert ee.constrained_exact(d, cis, i)["evidence"] + ee.constrained_exact(d, trans, i)["evidence"] == 1
        # flipping a set wholesale changes nothing
        assert ee.constrained_exact(d, ee.flipped(ev, a, {(i, 0)}), i) == c
        # a single-locus set constrains nothing
        assert ee.constrained_exact(d, [(i, x, 5, int(a[i, 1, x]))], i)["evidence"] == 1
        # evidence from the second-best pair: below the unconstrained best, and rejected by the unconstrained predicate
        # wherever the two are further apart than the bound
        sb = me.second_best(dict(post=d, argmax={k for k, p in d.items() if p == best}))
        if sb is None:
            continue
        k2, p2 = sb
        ev2 = ee.spell(k2, i, [het])
        c2 = ee.constrained_exact(d, ev2, i)
        if not ee.consistent(top, ev2, i):  # (the two pairs differ in the phase of the heterozygous loci)
            assert c2["best"] == p2 < best and k2 in c2["argmax"]
            assert ee.accepts(k2, p2, ev2, i, c2["best"], L) and not ee.accepts(top, best, ev2, i, c2["best"], L)
            if p2 < me.map_floor(best, L):
                assert not me.accepts(p2, best, L)
                rejected += 1
    print(name, "individuals checked:", checked, "; second-best evidence rejected by the unconstrained predicate:", rejected)
    assert checked >= 3 and rejected >= 1


@pytest.mark.parametrize("name,S", PANEL_S)
def test_gpu_panels_cover_the_checks(oracle_mod, name, S):
    a, hl, post = m0_posteriors(oracle_mod, name, S)
    N = a.shape[0]
    quirk = en.head_quirk(a, hl)
    covered = [i for i in range(N) if not quirk[i] and len(ee.het_loci(a[i])) >= 2]
    assert len(covered) * 10 >= 6 * N, (name, covered)
    assert max(len(ee.het_loci(a[i])) for i in covered) >= 4
    for i in covered:  # every phasing has a positive posterior: no impossible evidence on this panel
        assert all(p > 0 for p in post[i].values())


def test_host_plan_recognises_every_case(oracle_mod):
    a = build_panel("a3")
    N, _, L = a.shape
    het = {i: ee.het_loci(a[i]) for i in range(N)}
    i4 = next(i for i in range(N) if len(het[i]) >= 4)
    h = het[i4]
    f = lambda i, k: int(a[i, 0, k])  # noqa: E731
    ihom, khom = next((i, k) for i in range(N) for k in range(L) if a[i, 0, k] >= 0 and a[i, 0, k] == a[i, 1, k])
    imis, kmis = next((i, k) for i in range(N) for k in range(L) if (a[i, :, k] < 0).any())
    good = [(i4, h[0], 7, f(i4, h[0])), (i4, h[1], 7, f(i4, h[1]))]
    cases = {
        "empty": [],
        "one set": good,
        "single-locus sets": [(i4, h[0], 1, f(i4, h[0])), (i4, h[2], 2, f(i4, h[2]))],
        "a single-locus set inside another": good[:1] + [(i4, h[2], 7, f(i4, h[2])), (i4, h[1], 9, f(i4, h[1]))],
        "adjacent": [(i4, h[0], 1, f(i4, h[0])), (i4, h[1], 1, f(i4, h[1])), (i4, h[2], 2, f(i4, h[2])), (i4, h[3], 2, f(i4, h[3]))],
        "interleaved": [(i4, h[0], 1, f(i4, h[0])), (i4, h[2], 1, f(i4, h[2])), (i4, h[1], 2, f(i4, h[1])), (i4, h[3], 2, f(i4, h[3]))],
        "nested": [(i4, h[0], 1, f(i4, h[0])), (i4, h[3], 1, f(i4, h[3])), (i4, h[1], 2, f(i4, h[1])), (i4, h[2], 2, f(i4, h[2]))],
        "individual outside the panel": good + [(N, 0, 0, 0)],
        "negative individual": [(-1, 0, 0, 0)] + good,
        "locus out of range": good + [(i4, L, 7, 0)],
        "negative locus": good + [(i4, -1, 7, 0)],
        "homozygous locus": good + [(ihom, khom, 0, int(a[ihom, 0, khom]))],
        "missing allele": good + [(imis, kmis, 0, int(a[imis, :, kmis].max()))],
        "neither allele": good[:1] + [(i4, h[1], 7, 9999)],
        "duplicate": good + [(i4, h[0], 8, f(i4, h[0]))],
        "two errors: the first entry is named": [(i4, L, 7, 0)] + good + [(N, 0, 0, 0)],
    }
    seen = set()
    for what, entries in cases.items():
        code, offender = ee.plan_model(a, entries)
        rc, msg, ne, nc, evs = plan(a, entries)
        assert rc == code, (what, rc, code, msg)
        seen.add(code)
        if code == ee.EARG:
            assert f"evidence entry {offender}:" in msg, (what, msg)
        elif code == ee.EUNSUPPORTED:
            assert f"individual {offender}:" in msg and "interleave" in msg, (what, msg)
        else:
            multi = [e for e in entries if sum(1 for x in entries if x[0] == e[0] and x[2] == e[2]) > 1]
            assert ne == len(multi) and nc == len({e[0] for e in multi}), (what, ne, nc)
            assert sorted(evs[:, 0].tolist()) == evs[:, 0].tolist() == sorted(e[1] for e in multi)
            assert ((evs[:, 1] & 1) != 0).sum() == ((evs[:, 1] & 2) != 0).sum() == len({(e[0], e[2]) for e in multi})
    assert seen == {ee.OK, ee.EARG, ee.EUNSUPPORTED}
    # the allele index the kernel compares against: the symbol's rank in the locus's allele table
    rc, msg, ne, nc, evs = plan(a, cases["one set"])
    ta = en.allele_table(a)
    for (i, k, s, sym), (locus, code) in zip(cases["one set"], evs.tolist()):
        assert locus == k and code >> 8 == [x for x, _ in ta[k]].index(sym)
    # entry order and set names do not enter
    perm = cases["adjacent"][::-1]
    renamed = [(i, k, 100 - s, x) for i, k, s, x in cases["adjacent"]]
    assert plan(a, perm)[4].tolist() == plan(a, renamed)[4].tolist() == plan(a, cases["adjacent"])[4].tolist()
