"""libstdc++'s std::nth_element(first, first + nth, last, greater) on (value,
tag) records, restated in plain Python with a report of the path it took.

TEST INFRASTRUCTURE ONLY.  It is written from the algorithm's description
(introselect: median of three to `first`, unguarded Hoare partition, a budget
of 2 * floor(lg n) partitions, then heap select + swap; insertion sort of the
last <= 3 elements) and shares no code with hmc_amd/csrc/select.hpp.  Its
permutation is pinned against the real std::nth_element by
tests/test_introselect_model.py; the path report is trusted only because of
that equality.  Comparisons are Python float comparisons, which agree with
C++'s `>` on doubles (NaN compares false, subnormals are kept).
"""
from __future__ import annotations

from dataclasses import dataclass


@dataclass(frozen=True)
class Path:
    partitions: int      # partitions performed
    heap: bool           # the partition budget ran out with more than 3 elements left
    heap_len: int        # length of the range handed to the heap select (0 if not reached)
    insertion_len: int   # length handed to the final insertion sort (0 on the heap path / no-op)
    noop: bool           # n == 0 or nth == n: nothing is touched
    ranges: tuple = ()   # length of the range each partition started from


def _gt(a, b):
    """greater<Record>: compares the value only."""
    return a[0] > b[0]


def _median_to_first(r, result, a, b, c):
    if _gt(r[a], r[b]):
        if _gt(r[b], r[c]):
            pick = b
        elif _gt(r[a], r[c]):
            pick = c
        else:
            pick = a
    elif _gt(r[a], r[c]):
        pick = a
    elif _gt(r[b], r[c]):
        pick = c
    else:
        pick = b
    r[result], r[pick] = r[pick], r[result]


def _partition(r, first, last, pivot):
    while True:
        while _gt(r[first], r[pivot]):
            first += 1
        last -= 1
        while _gt(r[pivot], r[last]):
            last -= 1
        if not first < last:
            return first
        r[first], r[last] = r[last], r[first]
        first += 1


def _adjust_heap(r, first, hole, length, value):
    top = hole
    second = hole
    while second < (length - 1) // 2:
        second = 2 * (second + 1)
        if _gt(r[first + second], r[first + second - 1]):
            second -= 1
        r[first + hole] = r[first + second]
        hole = second
    if length % 2 == 0 and second == (length - 2) // 2:
        second = 2 * (second + 1)
        r[first + hole] = r[first + second - 1]
        hole = second - 1
    # __push_heap
    while hole > top:
        parent = (hole - 1) // 2
        if not _gt(r[first + parent], value):
            break
        r[first + hole] = r[first + parent]
        hole = parent
    r[first + hole] = value


def _heap_select(r, first, middle, last):
    length = middle - first
    if length >= 2:  # __make_heap
        parent = (length - 2) // 2
        while True:
            _adjust_heap(r, first, parent, length, r[first + parent])
            if parent == 0:
                break
            parent -= 1
    for i in range(middle, last):
        if _gt(r[i], r[first]):  # __pop_heap(first, middle, i)
            value = r[i]
            r[i] = r[first]
            _adjust_heap(r, first, 0, length, value)


def _insertion_sort(r, first, last):
    for i in range(first + 1, last):
        value = r[i]
        if _gt(value, r[first]):
            r[first + 1:i + 1] = r[first:i]
            r[first] = value
        else:  # __unguarded_linear_insert
            hole = i
            while _gt(value, r[hole - 1]):
                r[hole] = r[hole - 1]
                hole -= 1
            r[hole] = value


def nth_element(values, tags, nth):
    """Returns (values, tags, Path) after nth_element(v, v + nth, v + n, greater)."""
    r = list(zip(values, tags))
    n = len(r)
    if n == 0 or nth == n:
        return [x[0] for x in r], [x[1] for x in r], Path(0, False, 0, 0, True)
    first, last = 0, n
    depth = 2 * (n.bit_length() - 1)
    parts = 0
    heap, heap_len = False, 0
    ranges = []
    while last - first > 3:
        if depth == 0:
            heap, heap_len = True, last - first
            _heap_select(r, first, nth + 1, last)
            r[first], r[nth] = r[nth], r[first]
            break
        depth -= 1
        ranges.append(last - first)
        mid = first + (last - first) // 2
        _median_to_first(r, first, first + 1, mid, last - 1)
        cut = _partition(r, first + 1, last, first)
        parts += 1
        if cut <= nth:
            first = cut
        else:
            last = cut
    ins = 0
    if not heap:
        ins = last - first
        _insertion_sort(r, first, last)
    return [x[0] for x in r], [x[1] for x in r], Path(parts, heap, heap_len, ins, False, tuple(ranges))


def path(values, nth):
    return nth_element(values, range(len(values)), nth)[2]
