"""Every device k-best selection layout of the E-step's value pass
(hmc_amd/csrc/coop_select.hpp), driven directly through the library's test
hooks instead of through whole E-steps:

  one link per lane   seg_nth_slots, sw <= 32      hmc_test_coop_nth_element
  two links per lane  seg2_nth_slots, W at run time and W = 10 at compile time
  wide                seg_nth_slots, sw = 64: one list of up to 128 per wave
  value only          seg_rank_select and its tie-at-the-cut return value

The nth_element layouts must leave every list exactly as the real
std::nth_element(.., greater) of the CPU restatement's libstdc++ does: tags
equal, values equal bit for bit (NaN is among them).  The lists include the
committed heap-path inputs (tests/golden/heap_path_ranks.json), on which the
selection spends its 2 * floor(lg n) partitions and finishes with
std::__heap_select — a branch the random, tied, sorted and organ-pipe lists
practically never reach — as ranks, as likelihood-like magnitudes down to
1e-300 and as true subnormals, and the wavefronts are composed so that heap
segments sit next to each other, next to segments that are still
partitioning, next to 2- and 3-element insertion sorts, and next to idle and
no-op segments (select_inputs.compose; what each wavefront holds is read from
tests/introselect_model.py's path reports and asserted).
"""
import ctypes as C

import numpy as np
import pytest

import hmc_amd
import introselect_model as model
import select_inputs as si

pytestmark = pytest.mark.gpu

PAIR, PAIR10, WIDE, RANK = 0, 1, 2, 3
PAD_VALUE = 1e308       # behind every list: larger than any element, so a read past n changes the result
PAD_TAG = 0xA5000000


def _ptr(a, t):
    return a.ctypes.data_as(C.POINTER(t))


def _pad(count, stride):
    lik = np.full((count, stride), PAD_VALUE, np.float64)
    tag = (PAD_TAG + np.arange(stride, dtype=np.uint32))[None, :].repeat(count, 0)
    return lik, np.ascontiguousarray(tag)


def _run_strided(mode, width, stride, lik, tag, ns, nths, tie=None):
    """hmc_test_coop_select on copies of lik/tag[count, stride]."""
    l2, t2 = lik.copy(), tag.copy()
    n_a = np.asarray(ns, np.int32)
    nth_a = np.asarray(nths, np.int32)
    rc = hmc_amd.lib().hmc_test_coop_select(
        0, mode, width, _ptr(l2, C.c_double), _ptr(t2, C.c_uint32), _ptr(n_a, C.c_int32), _ptr(nth_a, C.c_int32),
        _ptr(tie, C.c_double) if tie is not None else None, len(n_a))
    assert rc == 0, rc
    return l2, t2


def _pack_strided(lists, stride, use_ref):
    lik, tag = _pad(len(lists), stride)
    for j, s in enumerate(lists):
        lik[j, :s.n] = s.ref_values if use_ref else s.values
        tag[j, :s.n] = s.ref_tags if use_ref else np.arange(s.n)
    return lik, tag


def _first_mismatch(got_l, got_t, exp_l, exp_t):
    """Index of the first list whose values (as bits) or tags differ, or None."""
    bad = (got_l.view(np.uint64) != exp_l.view(np.uint64)) | (got_t != exp_t)
    rows = np.flatnonzero(bad.reshape(len(bad), -1).any(axis=1)) if bad.ndim == 2 else np.flatnonzero(bad)
    return int(rows[0]) if len(rows) else None


def _describe(s):
    return dict(n=s.n, nth=s.nth, origin=s.origin, path=s.path, values=s.values.tolist())


def _check_strided(mode, width, stride, comp):
    lik, tag = _pack_strided(comp.lists, stride, use_ref=False)
    exp_l, exp_t = _pack_strided(comp.lists, stride, use_ref=True)
    got_l, got_t = _run_strided(mode, width, stride, lik, tag, [s.n for s in comp.lists], [s.nth for s in comp.lists])
    j = _first_mismatch(got_l, got_t, exp_l, exp_t)
    assert j is None, (j, j // comp.G, j % comp.G, _describe(comp.lists[j]), got_t[j].tolist(), exp_t[j].tolist())


@pytest.mark.parametrize("sw", [14, 20, 32])
def test_one_link_layout_with_heap_path_wavefronts(oracle_mod, sw):
    """seg_nth_slots through the existing hook, 64 / sw lists per wavefront."""
    name = f"one_link_sw{sw}"
    comp = si.layout_composition(oracle_mod, name)
    si.check_coverage(name, comp)
    ns = [s.n for s in comp.lists]
    off = np.cumsum([0] + ns[:-1]).astype(np.int32)
    lik = np.concatenate([s.values for s in comp.lists])
    tag = np.concatenate([np.arange(n, dtype=np.uint32) for n in ns])
    exp_l = np.concatenate([s.ref_values for s in comp.lists])
    exp_t = np.concatenate([s.ref_tags.astype(np.uint32) for s in comp.lists])
    n_a, nth_a = np.array(ns, np.int32), np.array([s.nth for s in comp.lists], np.int32)
    rc = hmc_amd.lib().hmc_test_coop_nth_element(
        0, _ptr(lik, C.c_double), _ptr(tag, C.c_uint32), _ptr(off, C.c_int32), _ptr(n_a, C.c_int32),
        _ptr(nth_a, C.c_int32), len(ns), len(lik), sw)
    assert rc == 0
    e = _first_mismatch(lik, tag, exp_l, exp_t)
    if e is not None:
        j = int(np.searchsorted(off, e, side="right")) - 1
        o, n = off[j], ns[j]
        raise AssertionError((j, _describe(comp.lists[j]), tag[o:o + n].tolist(), exp_t[o:o + n].tolist()))


@pytest.mark.parametrize("W", [1, 2, 3, 7, 10, 16])
def test_pair_layout_matches_libstdcxx(oracle_mod, W):
    """seg2_nth_slots with make_seg(W) at run time: 64 / W lists of up to 2W
    per wavefront, lane k carrying positions k and k + W; the lanes past the
    last segment address their dead segment (W = 3, 7, 10)."""
    name = f"pair_W{W}"
    comp = si.layout_composition(oracle_mod, name)
    si.check_coverage(name, comp)
    _check_strided(PAIR, W, 2 * W, comp)


def test_pair_layout_fixed_width_10_matches_libstdcxx(oracle_mod):
    """The same with the width a compile-time constant, as estep_values<..,
    PAIR, 10> has it (what the flagship runs at the reference's default S)."""
    comp = si.layout_composition(oracle_mod, "pair_W10")
    si.check_coverage("pair_W10", comp)
    _check_strided(PAIR10, 10, 20, comp)


def test_wide_layout_matches_libstdcxx(oracle_mod):
    """seg_nth_slots with make_seg(64): one list of up to 128 links per
    wavefront, lane k loading and storing positions k and k + 64, the
    sequential select.hpp code on the wave's first lane."""
    comp = si.layout_composition(oracle_mod, "wide")
    si.check_coverage("wide", comp)
    assert sum(1 for s in comp.lists if s.path.heap and s.n > 64) >= 8
    _check_strided(WIDE, 64, 128, comp)


def test_negative_control_wrong_nth_is_noticed(oracle_mod):
    """The comparison the tests above use fails when the device result at nth
    is held against the reference at another nth' whose arrangement differs."""
    v = si.map_values(next(e for e in si.heap_path_ranks() if (e["n"], e["nth"]) == (20, 9))["ranks"], "likelihoods")
    tags = list(range(20))
    at9 = model.nth_element(v.tolist(), tags, 9)[1]
    other = next(k for k in range(20) if model.nth_element(v.tolist(), tags, k)[1] != at9)
    run, wrong = si.reference(oracle_mod, [si.SelList(v, 9, "heap"), si.SelList(v, other, "heap")])
    assert run.ref_tags.tolist() != wrong.ref_tags.tolist()
    lik, tag = _pack_strided([run], 20, use_ref=False)
    got_l, got_t = _run_strided(PAIR, 10, 20, lik, tag, [20], [9])
    assert _first_mismatch(got_l, got_t, *_pack_strided([run], 20, use_ref=True)) is None
    assert _first_mismatch(got_l, got_t, *_pack_strided([wrong], 20, use_ref=True)) == 0


# ---- value-only lists --------------------------------------------------------
def rank_lists(S, seed):
    """Lists of n = 0..2S values >= 0 without NaN (likelihoods on this path are
    neither): distinct, heavily tied, all equal, all zero, a zero tie and a
    non-zero tie across the S-cut, subnormal ties, ties at 1e-300."""
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(max(6, 1500 // (8 * (2 * S + 1)))):  # 1500 lists or more
        for n in range(0, 2 * S + 1):
            cut = np.sort(rng.random(n))[::-1].copy()        # descending; a tie put across the cut
            if n > S:
                cut[S] = cut[S - 1]
            ztie = np.zeros(n)                                # at most S - 1 positive values, zeros across the cut
            npos = int(rng.integers(0, S)) if n else 0
            ztie[:min(npos, n)] = 1.0 + rng.random(min(npos, n))
            for kind, v in (("distinct", rng.random(n)),
                            ("ties", rng.integers(0, 3, n).astype(np.float64)),
                            ("equal", np.full(n, 0.25)),
                            ("zeros", np.zeros(n)),
                            ("cut_tie", rng.permutation(cut)),
                            ("zero_cut_tie", rng.permutation(ztie)),
                            ("subnormal_ties", np.ldexp(rng.integers(0, 4, n).astype(np.float64), -1074)),
                            ("tiny_ties", rng.integers(1, 4, n).astype(np.float64) * 1e-300)):
                out.append((kind, v))
    return out


def rank_reference(v, S):
    """Plain restatement: sort stably descending by value, ties by slot; the
    first S go to slots [0, S); a list of n <= S is untouched.  Tie value:
    v[S] when n > S, v[S] == v[S - 1] and the value is non-zero, else 0."""
    n = len(v)
    if n <= S:
        return None, None, 0.0
    order = sorted(range(n), key=lambda i: (-v[i], i))
    sv = [v[i] for i in order]
    tie = sv[S] if sv[S] == sv[S - 1] and sv[S] != 0.0 else 0.0
    return np.array(sv[:S]), np.array(order[:S], np.uint32), tie


@pytest.mark.parametrize("S", [1, 2, 3, 5, 10, 16])
def test_rank_select_and_tie_at_the_cut(S):
    """seg_rank_select(n, S, make_seg(2S)): 64 / 2S lists per wavefront."""
    lists = rank_lists(S, 700 + S)
    stride = 2 * S
    lik, tag = _pad(len(lists), stride)
    exp_l, exp_t = _pad(len(lists), stride)
    exp_tie = np.zeros(len(lists))
    seen = {}
    for j, (kind, v) in enumerate(lists):
        n = len(v)
        lik[j, :n] = v
        tag[j, :n] = np.arange(n)
        top_v, top_t, exp_tie[j] = rank_reference(v.tolist(), S)
        if top_v is not None:
            exp_l[j, :S], exp_t[j, :S] = top_v, top_t
        else:
            exp_l[j, :n], exp_t[j, :n] = v, np.arange(n)
        if exp_tie[j] != 0.0:
            seen[kind] = seen.get(kind, 0) + 1
    # the cases the tie value exists for are among the lists
    assert seen.get("cut_tie", 0) > 0 and seen.get("equal", 0) > 0 and seen.get("tiny_ties", 0) > 0
    assert S == 1 or seen.get("subnormal_ties", 0) > 0
    assert "zeros" not in seen and "zero_cut_tie" not in seen  # a zero tie at the cut must report 0
    tie = np.full(len(lists), -1.0)
    got_l, got_t = _run_strided(RANK, S, stride, lik, tag, [len(v) for _, v in lists], [0] * len(lists), tie=tie)
    print(f"rank select S={S}: {len(lists)} lists, {int(np.count_nonzero(exp_tie))} with a non-zero tie at the cut")
    # slots [0, S) hold the S best in rank order; everything behind the list is untouched
    # (slots [S, n) keep stale links the value pass overwrites with the next add)
    keep = np.ones((len(lists), stride), bool)
    for j, (_, v) in enumerate(lists):
        if len(v) > S:
            keep[j, S:len(v)] = False
    bad = ((got_l.view(np.uint64) != exp_l.view(np.uint64)) | (got_t != exp_t)) & keep
    rows = np.flatnonzero(bad.any(axis=1))
    assert len(rows) == 0, (int(rows[0]), lists[rows[0]], got_l[rows[0]].tolist(), got_t[rows[0]].tolist())
    wrong = np.flatnonzero(tie.view(np.uint64) != exp_tie.view(np.uint64))
    assert len(wrong) == 0, (int(wrong[0]), lists[wrong[0]], tie[wrong[0]], exp_tie[wrong[0]])
