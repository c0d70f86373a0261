"""Tie-dense lists through the cooperative partition (coop_select.hpp).

With many equal values a position is a left stop and a right stop at once —
the case in which the swap rule's two roles of one element meet (a left stop
at x swaps iff more right stops lie strictly above x than left stops below
it; tests/test_partition_swap_rule.py has the rule on masks).  The random
lists of tests/test_gpu_select_layouts.py reach it least, so here every list
is drawn from an alphabet of 1, 2, 3 or 5 non-negative values (zero among
them), a few with a NaN, as the E-step calls the selection: n = W+1 .. 2W
links, nth = W - 1.  Tied lists share their wavefronts with untied lists,
idle segments (n = 0) and no-op segments (n == nth).  Expected values and tags
are those of the CPU restatement's real std::nth_element, values compared as
bits and tags exactly; one launch per mode.
"""
import ctypes as C

import numpy as np
import pytest

import hmc_amd
import select_inputs as si

pytestmark = pytest.mark.gpu

PAIR, PAIR10 = 0, 1
PAD_VALUE = 1e308
PAD_TAG = 0xA5000000
ALPHABETS = (1, 2, 3, 5)
_LISTS = {}


def _ptr(a, t):
    return a.ctypes.data_as(C.POINTER(t))


def tie_lists(oracle_mod, W):
    """About a thousand lists for width W, with their references; built once."""
    if W in _LISTS:
        return _LISTS[W]
    rng = np.random.default_rng(4200 + W)
    nth = W - 1
    scales = (1.0, 1e-300, 2.0 ** -1074, 0.125)
    out = []
    rounds = max(3, 1000 // (W * (len(ALPHABETS) + 2)))
    for rnd in range(rounds):
        for n in range(W + 1, 2 * W + 1):
            for a in ALPHABETS:
                scale = scales[(rnd + a) % len(scales)]
                v = rng.integers(0, a, n).astype(np.float64) * scale   # zero included; a = 1: all zero
                if a == 1 and rnd % 2:
                    v = np.full(n, scale)                              # all equal and non-zero
                out.append(si.SelList(v, nth, f"ties{a}"))
            v = rng.integers(0, 3, n).astype(np.float64)
            v[rng.integers(0, n, 1 + rnd % 2)] = np.nan                # one or two NaN among ties
            out.append(si.SelList(v, nth, "nan"))
            out.append(si.SelList(rng.permutation(n).astype(np.float64) + 1.0, nth, "untied"))
        out.append(si.idle_list())
        out.append(si.SelList(rng.integers(0, 2, nth).astype(np.float64), nth, "noop"))  # n == nth: nothing to do
    order = rng.permutation(len(out))
    out = [out[i] for i in order]
    si.reference(oracle_mod, out)
    _LISTS[W] = out
    return out


def check_composition(lists, G):
    """What the wavefronts hold: tied, untied, idle and no-op segments together."""
    waves = [lists[i:i + G] for i in range(0, len(lists), G)]
    kinds = [{("tied" if s.origin.startswith("ties") or s.origin == "nan" else s.origin) for s in w} for w in waves]
    assert sum(1 for k in kinds if {"tied", "untied"} <= k) > 0
    if G >= 4:
        assert sum(1 for k in kinds if {"tied", "idle"} <= k) > 0
        assert sum(1 for k in kinds if {"tied", "noop"} <= k) > 0
    else:
        assert any("idle" in k for k in kinds) and any("noop" in k for k in kinds)
    # the lists are what the test is about: positions that are both stops exist
    assert sum(1 for s in lists if len(set(s.values.tolist())) < s.n) > len(lists) // 2
    assert any(s.n > 3 and len(set(s.values.tolist())) < s.n for s in lists)  # and some of them partition
    assert any(np.isnan(s.values).any() for s in lists)
    assert any(s.n > 0 and not s.values.any() for s in lists)


def _pack(lists, stride, use_ref):
    lik = np.full((len(lists), stride), PAD_VALUE, np.float64)
    tag = np.ascontiguousarray((PAD_TAG + np.arange(stride, dtype=np.uint32))[None, :].repeat(len(lists), 0))
    for j, s in enumerate(lists):
        lik[j, :s.n] = s.ref_values if use_ref else s.values
        tag[j, :s.n] = s.ref_tags if use_ref else np.arange(s.n)
    return lik, tag


def _check_pair(mode, W, lists):
    stride = 2 * W
    lik, tag = _pack(lists, stride, use_ref=False)
    exp_l, exp_t = _pack(lists, stride, use_ref=True)
    n_a = np.array([s.n for s in lists], np.int32)
    nth_a = np.array([s.nth for s in lists], np.int32)
    rc = hmc_amd.lib().hmc_test_coop_select(0, mode, W, _ptr(lik, C.c_double), _ptr(tag, C.c_uint32),
                                            _ptr(n_a, C.c_int32), _ptr(nth_a, C.c_int32), None, len(lists))
    assert rc == 0, rc
    bad = ((lik.view(np.uint64) != exp_l.view(np.uint64)) | (tag != exp_t)).any(axis=1)
    rows = np.flatnonzero(bad)
    if len(rows):
        j = int(rows[0])
        s = lists[j]
        raise AssertionError((len(rows), j, s.origin, s.n, s.nth, s.values.tolist(), tag[j].tolist(), exp_t[j].tolist()))


@pytest.mark.parametrize("W", [2, 3, 10, 16])
def test_pair_layout_on_tie_dense_lists(oracle_mod, W):
    """seg2_nth_slots, W at run time: 64 / W lists per wavefront (W = 3, 10:
    with the dead segment of the lanes past the last list)."""
    lists = tie_lists(oracle_mod, W)
    check_composition(lists, 64 // W)
    _check_pair(PAIR, W, lists)


def test_pair_layout_fixed_width_10_on_tie_dense_lists(oracle_mod):
    """The compile-time width of estep_values<.., PAIR, 10>."""
    lists = tie_lists(oracle_mod, 10)
    check_composition(lists, 6)
    _check_pair(PAIR10, 10, lists)


def test_one_link_layout_sw20_on_tie_dense_lists(oracle_mod):
    """seg_nth_slots at sw = 20 (three lists per wavefront) on the W = 10 lists."""
    lists = tie_lists(oracle_mod, 10)
    check_composition(lists, 3)
    ns = [s.n for s in lists]
    off = np.cumsum([0] + ns[:-1]).astype(np.int32)
    lik = np.concatenate([s.values for s in lists])
    tag = np.concatenate([np.arange(n, dtype=np.uint32) for n in ns])
    exp_l = np.concatenate([s.ref_values for s in lists])
    exp_t = np.concatenate([s.ref_tags.astype(np.uint32) for s in lists])
    n_a, nth_a = np.array(ns, np.int32), np.array([s.nth for s in lists], np.int32)
    rc = hmc_amd.lib().hmc_test_coop_nth_element(
        0, _ptr(lik, C.c_double), _ptr(tag, C.c_uint32), _ptr(off, C.c_int32), _ptr(n_a, C.c_int32),
        _ptr(nth_a, C.c_int32), len(ns), len(lik), 20)
    assert rc == 0, rc
    bad = np.flatnonzero((lik.view(np.uint64) != exp_l.view(np.uint64)) | (tag != exp_t))
    if len(bad):
        j = int(np.searchsorted(off, bad[0], side="right")) - 1
        o, n = off[j], ns[j]
        s = lists[j]
        raise AssertionError((j, s.origin, n, s.nth, s.values.tolist(), tag[o:o + n].tolist(), exp_t[o:o + n].tolist()))
