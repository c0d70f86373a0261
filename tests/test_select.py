"""The E-step's libstdc++-exact k-best selection (hmc_amd/csrc/select.hpp),
run on the host through the library's test hooks, against the real
std::nth_element / std::sort compiled into the CPU restatement."""
import ctypes as C

import numpy as np
import pytest

import hmc_amd


def _ours(fn, lik, tag, *extra):
    l = np.ascontiguousarray(lik, np.float64).copy()
    t = np.ascontiguousarray(tag, np.uint32).copy()
    fn(l.ctypes.data_as(C.POINTER(C.c_double)), t.ctypes.data_as(C.POINTER(C.c_uint32)), len(l), *extra)
    return l, t.astype(np.int32)


def _cases(rng, n):
    yield rng.random(n)
    yield rng.integers(0, 3, n).astype(np.float64)          # heavy ties
    yield np.zeros(n)                                        # all equal
    yield np.arange(n, dtype=np.float64)                     # ascending
    yield np.arange(n, dtype=np.float64)[::-1].copy()        # descending
    v = np.concatenate([np.arange(n // 2), np.arange(n - n // 2)[::-1]]).astype(np.float64)
    yield v                                                  # organ pipe
    w = rng.integers(0, 4, n).astype(np.float64) * 1e-300
    w[rng.integers(0, n)] = np.nan
    yield w                                                  # denormal-ish ties + NaN


@pytest.mark.parametrize("n", list(range(1, 21)) + [24, 32, 33, 64, 100, 257])
def test_nth_element_matches_libstdcxx(oracle_mod, n):
    L = hmc_amd.lib()
    rng = np.random.default_rng(n)
    for lik in _cases(rng, n):
        for nth in sorted({0, n // 2, n - 1, max(0, n - 2)}):
            tag = np.arange(n, dtype=np.int32)
            l1, t1 = _ours(L.hmc_test_nth_element, lik, tag, nth)
            l2, t2 = oracle_mod.std_nth_element(lik, tag, nth)
            assert np.array_equal(t1, t2), (n, nth, lik)


@pytest.mark.parametrize("n", list(range(1, 33)))
def test_mask_partition_nth_element_matches_libstdcxx(oracle_mod, n):
    """The stop-mask formulation of the Hoare partition (select.hpp,
    partition_pivot_masks) used by the E-step kernel gives the identical
    permutation."""
    L = hmc_amd.lib()
    rng = np.random.default_rng(500 + n)
    for rep in range(40):
        for lik in _cases(rng, n):
            nth = int(rng.integers(0, n))
            tag = np.arange(n, dtype=np.int32)
            _, t1 = _ours(L.hmc_test_nth_element_masks, lik, tag, nth)
            _, t2 = oracle_mod.std_nth_element(lik, tag, nth)
            assert np.array_equal(t1, t2), (n, nth, lik)


@pytest.mark.parametrize("n", range(0, 17))
def test_small_sort_matches_libstdcxx(oracle_mod, n):
    L = hmc_amd.lib()
    rng = np.random.default_rng(100 + n)
    for lik in _cases(rng, max(n, 1)):
        lik = lik[:n]
        tag = np.arange(n, dtype=np.int32)
        _, t1 = _ours(L.hmc_test_sort_small, lik, tag)
        _, t2 = oracle_mod.std_sort(lik, tag)
        assert np.array_equal(t1, t2)


@pytest.mark.parametrize("n", list(range(0, 70)) + [100, 257, 1000])
def test_sort_matches_libstdcxx(oracle_mod, n):
    """std::sort for any n (select.hpp sort_greater: introsort with the
    threshold 16, heap sort at depth 0, final insertion sort) — the final
    candidate order when sample_size > 16."""
    L = hmc_amd.lib()
    rng = np.random.default_rng(300 + n)
    for rep in range(4):
        for ci, lik in enumerate(_cases(rng, max(n, 1))):
            if ci == 6:  # NaN: std::sort's unguarded loops need a strict weak order
                continue
            lik = lik[:n]
            tag = np.arange(n, dtype=np.int32)
            _, t1 = _ours(L.hmc_test_sort, lik, tag)
            _, t2 = oracle_mod.std_sort(lik, tag)
            assert np.array_equal(t1, t2), (n, ci)


# ---- the depth-limit branch (std::__heap_select + iter_swap) -----------------
# Random, tied, sorted and organ-pipe lists of n <= 32 practically never spend
# the 2 * floor(lg n) partition budget; the committed heap-path lists
# (tests/golden/heap_path_ranks.json) do, which test_introselect_model.py
# asserts through a model pinned against the real std::nth_element.
def _heap_path_cases(max_n):
    import select_inputs as si

    for e in si.heap_path_ranks():
        if e["n"] <= max_n:
            for how in si.VALUE_MAPS:
                yield e, how, si.map_values(e["ranks"], how)


def _check_heap_path(oracle_mod, fn, max_n):
    count = 0
    for e, how, lik in _heap_path_cases(max_n):
        n, nth = e["n"], e["nth"]
        tag = np.arange(n, dtype=np.int32)
        l1, t1 = _ours(fn, lik, tag, nth)
        l2, t2 = oracle_mod.std_nth_element(lik, tag, nth)
        assert np.array_equal(t1, t2), (n, nth, how, e["ranks"])
        assert np.array_equal(l1.view(np.uint64), l2.view(np.uint64)), (n, nth, how)
        count += 1
    return count


def test_nth_element_heap_path_matches_libstdcxx(oracle_mod):
    """select.hpp's sequential nth_element on lists that end in the heap
    select, n = 13..128 (what one lane runs for the wide lists and for a
    segment whose budget is spent), as ranks, likelihood-like magnitudes down
    to 1e-300 and true subnormals."""
    assert _check_heap_path(oracle_mod, hmc_amd.lib().hmc_test_nth_element, 128) >= 3 * 100


def test_mask_partition_heap_path_matches_libstdcxx(oracle_mod):
    """The same lists of n <= 32 through the stop-mask partition."""
    assert _check_heap_path(oracle_mod, hmc_amd.lib().hmc_test_nth_element_masks, 32) >= 3 * 80


def test_coop_select_hook_refuses_shapes_the_value_pass_lacks():
    """hmc_test_coop_select checks its shapes before it touches a device: a
    width outside 1..16, a list longer than 2W or 128, nth > n, the fixed-10
    mode at another width and a missing tie array are HMC_EARG."""
    L = hmc_amd.lib()
    PAIR, PAIR10, WIDE, RANK = 0, 1, 2, 3

    def call(mode, width, n, nth, stride, tie=False):
        lik = np.zeros(stride, np.float64)
        tag = np.zeros(stride, np.uint32)
        na, ntha = np.array([n], np.int32), np.array([nth], np.int32)
        t = np.zeros(1, np.float64)
        return L.hmc_test_coop_select(
            0, mode, width, lik.ctypes.data_as(C.POINTER(C.c_double)), tag.ctypes.data_as(C.POINTER(C.c_uint32)),
            na.ctypes.data_as(C.POINTER(C.c_int32)), ntha.ctypes.data_as(C.POINTER(C.c_int32)),
            t.ctypes.data_as(C.POINTER(C.c_double)) if tie else None, 1)

    EARG = -1
    for mode in (PAIR, RANK):
        assert call(mode, 0, 0, 0, 2, tie=True) == EARG
        assert call(mode, 17, 4, 1, 34, tie=True) == EARG
        assert call(mode, 5, 11, 1, 10, tie=True) == EARG       # n > 2W
        assert call(mode, 5, -1, 0, 10, tie=True) == EARG
    assert call(PAIR, 5, 6, 7, 10) == EARG                      # nth > n
    assert call(PAIR10, 9, 4, 1, 18) == EARG
    assert call(PAIR10, 10, 21, 1, 20) == EARG
    assert call(WIDE, 32, 4, 1, 128) == EARG
    assert call(WIDE, 64, 129, 1, 128) == EARG
    assert call(RANK, 5, 6, 0, 10, tie=False) == EARG           # no tie array
    assert call(4, 5, 6, 0, 10) == EARG and call(-1, 5, 6, 0, 10) == EARG
