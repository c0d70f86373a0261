"""The final window of the device k-best selections (coop_select.hpp): the
2- or 3-element std::__insertion_sort every selection ends with, done on the
device as a placement (SmallWindow) instead of a compare-swap network.

Inputs are the smallest at which the placement can go wrong: every list over
{0.0, 1.0, 2.0} of length 2..7 with every nth (the whole list is a final
window, or reaches one after one or two partitions, ties inside it), and a few
thousand random lists of length up to 2W over three symbols, whose final
windows sit at every offset, the straddle of a lane's two positions (offsets
W - 1, W, W + 1) included.  The expected permutation is the real
std::nth_element(.., greater) of the CPU restatement's libstdc++; every slot of
every list is compared, tags and value bits.
"""
import ctypes as C
import itertools

import numpy as np
import pytest

import hmc_amd

pytestmark = pytest.mark.gpu

PAIR, PAIR10 = 0, 1
PAD_VALUE = 1e308
PAD_TAG = 0xA5000000
_REF = {}


def _ptr(a, t):
    return a.ctypes.data_as(C.POINTER(t))


def small_lists():
    """(values, nth): every list over {0, 1, 2} of length 2..7, nth = 0..n."""
    out = []
    for n in range(2, 8):
        for v in itertools.product((0.0, 1.0, 2.0), repeat=n):
            for nth in range(n + 1):
                out.append((np.array(v), nth))
    return out


def random_lists(cap, count, seed):
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(count):
        n = int(rng.integers(2, cap + 1))
        sym = rng.choice([0.0, 0.25, 1e-300, 3.0, 7.5], 3, replace=False)
        v = sym[rng.integers(0, 3, n)]
        half = cap // 2
        nth = half - 1 if n > half >= 1 and rng.random() < 0.5 else int(rng.integers(0, n + 1))
        out.append((v, nth))
    return out


def lists_for(cap, seed):
    """The lists a layout of up to `cap` elements runs, with their references
    (computed once per session and shared, never modified)."""
    if cap not in _REF:
        ls = [(v, nth) for v, nth in small_lists() if len(v) <= cap]
        if cap >= 2:
            ls += random_lists(cap, 3000, seed)
        _REF[cap] = ls
    return _REF[cap]


def reference(oracle_mod, ls, key):
    if ("ref", key) not in _REF:
        ref = []
        for v, nth in ls:
            rv, rt = oracle_mod.std_nth_element(v, np.arange(len(v), dtype=np.int32), nth)
            ref.append((rv, rt.astype(np.uint32)))
        _REF[("ref", key)] = ref
    return _REF[("ref", key)]


def _check_pair(oracle_mod, mode, W):
    cap, stride = 2 * W, 2 * W
    ls = lists_for(cap, 4100 + W)
    ref = reference(oracle_mod, ls, cap)
    lik = np.full((len(ls), stride), PAD_VALUE, np.float64)
    tag = np.ascontiguousarray((PAD_TAG + np.arange(stride, dtype=np.uint32))[None, :].repeat(len(ls), 0))
    exp_l, exp_t = lik.copy(), tag.copy()
    for j, ((v, _), (rv, rt)) in enumerate(zip(ls, ref)):
        n = len(v)
        lik[j, :n], tag[j, :n] = v, np.arange(n)
        exp_l[j, :n], exp_t[j, :n] = rv, rt
    n_a = np.array([len(v) for v, _ in ls], np.int32)
    nth_a = np.array([nth for _, nth in ls], np.int32)
    rc = hmc_amd.lib().hmc_test_coop_select(0, mode, W, _ptr(lik, C.c_double), _ptr(tag, C.c_uint32),
                                            _ptr(n_a, C.c_int32), _ptr(nth_a, C.c_int32), None, len(ls))
    assert rc == 0, rc
    bad = ((lik.view(np.uint64) != exp_l.view(np.uint64)) | (tag != exp_t)).any(axis=1)
    rows = np.flatnonzero(bad)
    print(f"W={W} mode={mode}: {len(ls)} lists, {len(rows)} differ")
    assert len(rows) == 0, (int(rows[0]), ls[rows[0]][0].tolist(), ls[rows[0]][1], tag[rows[0]].tolist(),
                            exp_t[rows[0]].tolist())


@pytest.mark.parametrize("W", [1, 2, 3, 7, 10, 16])
def test_pair_layout_final_windows(oracle_mod, W):
    """seg2_nth_slots, W at run time: 64 / W lists of up to 2W per wavefront."""
    _check_pair(oracle_mod, PAIR, W)


def test_pair_layout_fixed_width_10_final_windows(oracle_mod):
    """The compile-time width of estep_values<.., PAIR, 10>."""
    _check_pair(oracle_mod, PAIR10, 10)


@pytest.mark.parametrize("sw", [14, 20, 32])
def test_one_link_layout_final_windows(oracle_mod, sw):
    """seg_nth_slots at sw <= 32: 64 / sw lists per wavefront, one link per lane."""
    ls = lists_for(sw, 4200 + sw)
    ref = reference(oracle_mod, ls, sw)
    ns = [len(v) for v, _ in ls]
    off = np.cumsum([0] + ns[:-1]).astype(np.int32)
    lik = np.concatenate([v for v, _ in ls])
    tag = np.concatenate([np.arange(n, dtype=np.uint32) for n in ns])
    exp_l = np.concatenate([rv for rv, _ in ref])
    exp_t = np.concatenate([rt for _, rt in ref])
    n_a, nth_a = np.array(ns, np.int32), np.array([nth for _, nth in ls], np.int32)
    rc = hmc_amd.lib().hmc_test_coop_nth_element(0, _ptr(lik, C.c_double), _ptr(tag, C.c_uint32), _ptr(off, C.c_int32),
                                                 _ptr(n_a, C.c_int32), _ptr(nth_a, C.c_int32), len(ns), len(lik), sw)
    assert rc == 0, rc
    bad = np.flatnonzero((lik.view(np.uint64) != exp_l.view(np.uint64)) | (tag != exp_t))
    print(f"sw={sw}: {len(ls)} lists, {len(bad)} slots differ")
    if len(bad):
        j = int(np.searchsorted(off, bad[0], side="right")) - 1
        o, n = off[j], ns[j]
        raise AssertionError((j, ls[j][0].tolist(), ls[j][1], tag[o:o + n].tolist(), exp_t[o:o + n].tolist()))
