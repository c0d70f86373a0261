"""The final window of the cooperative selections as a placement
(hmc_amd/csrc/coop_select.hpp, SmallWindow): std::__insertion_sort with
comp = greater on a window [first, last) of 2 or 3 elements is a stable
descending sort, so the element at window offset j ends at

  first + #{i < len : x_i > x_j} + #{i < j : x_i equivalent to x_j}

and the kernel's case form over s = b > a, ca = c > a, cb = c > b gives the
same offsets on every weak ordering — and, unlike the rank count, also what
the sequential code does when the three comparisons are no weak ordering (NaN).

Checked on every weak ordering of 2 (3 of them) and 3 (13) elements with
distinct tags at several window offsets, on all 8 comparison outcomes against
insertion sort run on a comparison table, and through the host selection
(select.hpp, hmc_test_nth_element) on lists that end in such windows.
"""
import ctypes as C
import itertools

import numpy as np
import pytest

NAN = float("nan")


def gt(a, b):
    return a > b


def insertion_sort(v, first, last, comp=gt):
    """std::__insertion_sort (stl_algo.h:1819-1849) on v[first:last], in place;
    v holds (value, tag) records compared by value."""
    for i in range(first + 1, last):
        val = v[i]
        if comp(val[0], v[first][0]):
            v[first + 1:i + 1] = v[first:i]  # move_backward
            v[first] = val
        else:  # __unguarded_linear_insert
            nxt = i - 1
            pos = i
            while comp(val[0], v[nxt][0]):
                v[pos] = v[nxt]
                pos = nxt
                nxt -= 1
            v[pos] = val


def rank_offsets(x):
    """The stable descending rank of each window element."""
    n = len(x)
    return [sum(1 for i in range(n) if x[i] > x[j]) +
            sum(1 for i in range(j) if not x[i] > x[j] and not x[j] > x[i]) for j in range(n)]


def kernel_offsets(s, ca, cb, three):
    """SmallWindow::dest: [offset >= 1] + [offset >= 2] per window offset j."""
    ca, cb = three and ca, three and cb
    t = ca or cb
    cp = cb if s else ca
    ge1 = [s or ca, (not s) or cb, not cp]
    ge2 = [s and t, (not s) and t, not t]
    return [int(ge1[j]) + int(ge2[j]) for j in range(3 if three else 2)]


TABLE = 0x120644A9A950  # coop_select.hpp static_asserts small_window_table() against the same constant


def table_offset(idx, j):
    """SmallWindow::dest's arithmetic: two bits at 16 j + 2 idx of the packed constant."""
    return (TABLE >> ((2 * idx + 16 * j) & 63)) & 3


def test_packed_table_is_the_case_form():
    packed = 0
    for idx in range(8):
        s, ca, cb = bool(idx & 4), bool(idx & 2), bool(idx & 1)
        off = kernel_offsets(s, ca, cb, True)
        for j in range(3):
            assert table_offset(idx, j) == off[j], (idx, j)
            packed |= off[j] << (16 * j + 2 * idx)
    assert packed == TABLE
    # a window of 2 is a window of 3 whose c is NaN: idx 0 or 4, offsets of a and b only
    for s in (False, True):
        assert [table_offset(4 if s else 0, j) for j in range(2)] == kernel_offsets(s, False, False, False)


def kernel_place(v, first, last):
    """The kernel's tail on a list of (value, tag): every position inside the
    window writes its record to first + offset, every other one to itself."""
    n = last - first
    x = [v[first + j][0] for j in range(n)]
    three = n > 2
    c = x[2] if three else NAN
    idx = (4 if x[1] > x[0] else 0) | (2 if c > x[0] else 0) | (1 if c > x[1] else 0)
    off = [table_offset(idx, j) for j in range(n)]
    out = list(v)
    written = set()
    for p in range(len(v)):
        j = p - first
        d = first + off[j] if 0 <= j < n else p
        assert d not in written, "two elements placed on one slot"
        written.add(d)
        out[d] = v[p]
    return out


def weak_orderings(n):
    """One value tuple per weak ordering of n elements (3 for n = 2, 13 for n = 3)."""
    seen = {}
    for v in itertools.product(range(n), repeat=n):
        levels = sorted(set(v))
        canon = tuple(levels.index(a) for a in v)
        seen[canon] = tuple(float(a) for a in canon)
    return sorted(seen.values())


def test_counts_of_weak_orderings():
    assert len(weak_orderings(2)) == 3 and len(weak_orderings(3)) == 13


@pytest.mark.parametrize("n", [2, 3])
@pytest.mark.parametrize("first", [0, 1, 8, 9, 10, 17])
def test_placement_on_every_weak_ordering(n, first):
    # a 20-slot list as the pair layout at W = 10 has it: windows at the start,
    # across a lane's two positions (9 | 10) and at the end
    for x in weak_orderings(n):
        v = [(100.0 + p, 1000 + p) for p in range(20)]
        for j in range(n):
            v[first + j] = (x[j], first + j)
        seq = list(v)
        insertion_sort(seq, first, first + n)
        assert kernel_place(v, first, first + n) == seq, (x, first)
        by_rank = list(v)
        for j, r in enumerate(rank_offsets(x)):
            by_rank[first + r] = v[first + j]
        assert by_rank == seq, (x, first)


@pytest.mark.parametrize("three", [False, True])
def test_case_form_on_every_comparison_outcome(three):
    """All outcomes of (b > a, c > a, c > b), the non-transitive ones included:
    insertion sort driven by the table against the case form."""
    for s, ca, cb in itertools.product([False, True], repeat=3):
        table = {(1, 0): s, (2, 0): ca, (2, 1): cb}
        n = 3 if three else 2
        v = [(float(j), j) for j in range(n)]  # value = identity of the element

        def comp(a, b):  # only c > a, c > b and b > a are ever asked (KeyError otherwise)
            return table[(int(a), int(b))]

        insertion_sort(v, 0, n, comp)
        off = kernel_offsets(s, ca, cb, three)
        assert sorted(off) == list(range(n)), (s, ca, cb)
        assert [v[off[j]][1] for j in range(n)] == list(range(n)), (s, ca, cb, off, v)


def test_nan_windows_against_insertion_sort():
    for x in itertools.product([NAN, 0.0, 1.0, 2.0], repeat=3):
        for n in (2, 3):
            v = [(x[j], j) for j in range(n)] + [(5.0, 9)]
            seq = list(v)
            insertion_sort(seq, 0, n)
            got = kernel_place(v, 0, n)
            assert [t for _, t in got] == [t for _, t in seq], (x, n)


def test_host_selection_on_lists_ending_in_small_windows(oracle_mod):
    """select.hpp on the host against the real std::nth_element: every list
    over {0, 1, 2} of length 2..7 with every nth, and tied lists of 11..20."""
    import hmc_amd

    L = hmc_amd.lib()
    rng = np.random.default_rng(515)
    cases = []
    for n in range(2, 8):
        for v in itertools.product((0.0, 1.0, 2.0), repeat=n):
            cases += [(np.array(v), nth) for nth in range(n + 1)]
    for _ in range(2000):
        n = int(rng.integers(11, 21))
        cases.append((rng.integers(0, 3, n).astype(np.float64), 9))
    for v, nth in cases:
        lik = v.copy()
        tag = np.arange(len(v), dtype=np.uint32)
        L.hmc_test_nth_element(lik.ctypes.data_as(C.POINTER(C.c_double)), tag.ctypes.data_as(C.POINTER(C.c_uint32)),
                               len(v), nth)
        rv, rt = oracle_mod.std_nth_element(v, np.arange(len(v), dtype=np.int32), nth)
        assert tag.tolist() == rt.tolist() and np.array_equal(lik, rv), (v.tolist(), nth)
