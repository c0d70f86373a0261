"""The swap rule of the cooperative partition (hmc_amd/csrc/coop_select.hpp):
which stops swap is a function of stop counts alone.

With Lw the left stops (subset of (first, last)), Rw the right stops (subset
of [first, last), `first` always one), l_k the k-th left stop from the left
and r_k the k-th right stop from the right, pair k swaps iff l_k < r_k.  For
a position x with kL = |Lw below x| and kR = |Rw| - 1 - |Rw below x|:

  a left stop at x swaps   iff  kR - [x in Rw] >= kL
  a right stop at x swaps  iff  kL > kR

and, as the kernel evaluates it (`first` never swaps, so it is left out of
the right stops; above = |Rw \\ {first} strictly above x|):

  a left stop at x swaps   iff  above > kL
  a right stop at x swaps  iff  kL > above     (x != first)

Checked exhaustively on every mask pair of ranges of up to 10 positions, on
random mask pairs at n = 20 and 32, and against a direct simulation of
std::__move_median_to_first + std::__unguarded_partition (comp = greater).
"""
import itertools
import random

import pytest

INF = 64


def bits(mask):
    return [p for p in range(mask.bit_length()) if (mask >> p) & 1]


def popc(x):
    return bin(x).count("1")


def paired(Lw, Rw, x):
    """The definition: the stop at x swaps iff its partner lies beyond it."""
    ls, rs = bits(Lw), bits(Rw)[::-1]
    nL, nR = len(ls), len(rs)
    below = (1 << x) - 1
    kL = popc(Lw & below)
    kR = nR - 1 - popc(Rw & below)
    isL, isR = bool((Lw >> x) & 1), bool((Rw >> x) & 1)
    lsw = isL and kL < nR and x < rs[kL]
    rsw = isR and kR < nL and ls[kR] < x
    return lsw, rsw


def closed(Lw, Rw, x):
    """The closed forms over the loop's own counts."""
    below = (1 << x) - 1
    kL = popc(Lw & below)
    kR = popc(Rw) - 1 - popc(Rw & below)
    isL, isR = bool((Lw >> x) & 1), bool((Rw >> x) & 1)
    return isL and kR - (1 if isR else 0) >= kL, isR and kL > kR


def kernel_form(Lw, Rw, first, x):
    """As seg_nth_slots / seg2_nth_slots evaluate it: right stops without
    `first`, counted strictly above x."""
    Rq = Rw & ~(1 << first)
    kL = popc(Lw & ((1 << x) - 1))
    above = popc((Rq >> 1) >> x)
    isL, isR = bool((Lw >> x) & 1), bool((Rq >> x) & 1)
    return isL and above > kL, isR and kL > above


def cut_of(Lw, Rw, K):
    ls, rs = bits(Lw), bits(Rw)[::-1]
    lK = ls[K] if K < len(ls) else INF
    rK = rs[K - 1] if K > 0 else INF
    return min(lK, rK)


def kernel_cut(Lw, Rw, first, K):
    """The kernel's LDS picture: rp[0] = 64, rp[k + 1] = r_k without `first`;
    lp[k] = l_k, anything at and behind nL."""
    ls, rs = bits(Lw), bits(Rw & ~(1 << first))[::-1]
    rp = [INF] + rs
    lK = ls[K] if K < len(ls) else INF
    return min(lK, rp[K])


def check_masks(Lw, Rw, first, last, n):
    want = [paired(Lw, Rw, x) for x in range(n)]
    assert [closed(Lw, Rw, x) for x in range(n)] == want
    assert [kernel_form(Lw, Rw, first, x) for x in range(n)] == want
    ls, rs = bits(Lw), bits(Rw)[::-1]
    K_def = sum(1 for k in range(min(len(ls), len(rs))) if ls[k] < rs[k])
    K = sum(1 for l, _ in want if l)
    assert K == K_def == sum(1 for _, r in want if r)
    # the swaps are a prefix of the pairs
    assert all(ls[k] < rs[k] for k in range(K))
    assert cut_of(Lw, Rw, K) == kernel_cut(Lw, Rw, first, K)
    return K, cut_of(Lw, Rw, K)


def mask_pairs(first, last):
    """Every Lw subset of (first, last) and Rw subset of [first, last) with bit first."""
    inner = list(range(first + 1, last))
    subsets = []
    for r in range(len(inner) + 1):
        for c in itertools.combinations(inner, r):
            subsets.append(sum(1 << p for p in c))
    for Lw in subsets:
        for Rq in subsets:
            yield Lw, Rq | (1 << first)


@pytest.mark.parametrize("n", [1, 2, 3, 4, 5, 6, 7])
def test_every_mask_pair_small(n):
    for Lw, Rw in mask_pairs(0, n):
        check_masks(Lw, Rw, 0, n, n)


def test_every_mask_pair_n10_inner_ranges():
    # ranges of up to 8 positions at every offset inside 10 positions, and the
    # full ranges of 9 and 10 positions on a stride of the left masks
    for first in range(0, 10):
        for last in range(first + 1, 11):
            if last - first <= 7:
                for Lw, Rw in mask_pairs(first, last):
                    check_masks(Lw, Rw, first, last, 10)


@pytest.mark.parametrize("span", [8, 9, 10])
def test_every_mask_pair_n10_wide(span):
    # all 4^(span-1) pairs of the widest ranges, vectorised by position
    import numpy as np

    first, last, n = 10 - span, 10, 10
    m = 1 << (span - 1)
    sub = (np.arange(m, dtype=np.int64) << (first + 1))
    Lw = np.repeat(sub, m)
    Rw = np.tile(sub, m) | (1 << first)
    pc = np.array([popc(i) for i in range(1 << 11)], dtype=np.int64)
    pos = np.arange(n)
    # l_k from the left and r_k from the right, INF-padded
    def stops(M, from_right):
        out = np.full((M.size, n + 1), INF, dtype=np.int64)
        cnt = np.zeros(M.size, dtype=np.int64)
        order = pos[::-1] if from_right else pos
        for p in order:
            has = ((M >> p) & 1).astype(bool)
            out[np.nonzero(has)[0], cnt[has]] = p
            cnt += has
        return out, cnt
    ls, nL = stops(Lw, False)
    rs, nR = stops(Rw, True)
    rows = np.arange(Lw.size)
    K_rule = np.zeros(Lw.size, dtype=np.int64)
    K_rsw = np.zeros(Lw.size, dtype=np.int64)
    for x in range(n):
        below = (1 << x) - 1
        kL = pc[Lw & below]
        kR = nR - 1 - pc[Rw & below]
        isL = ((Lw >> x) & 1).astype(bool)
        isR = ((Rw >> x) & 1).astype(bool)
        lsw_def = isL & (kL < nR) & (x < rs[rows, np.minimum(kL, n)])
        rsw_def = isR & (kR >= 0) & (kR < nL) & (ls[rows, np.clip(kR, 0, n)] < x)
        lsw = isL & (kR - isR >= kL)
        rsw = isR & (kL > kR)
        assert np.array_equal(lsw, lsw_def) and np.array_equal(rsw, rsw_def), x
        Rq = Rw & ~(1 << first)
        above = pc[(Rq >> 1) >> x]
        isRq = ((Rq >> x) & 1).astype(bool)
        assert np.array_equal(isL & (above > kL), lsw_def) and np.array_equal(isRq & (kL > above), rsw_def), x
        K_rule += lsw
        K_rsw += rsw
    K_def = np.zeros(Lw.size, dtype=np.int64)
    for k in range(n):
        K_def += (ls[:, k] < rs[:, k]) & (k < nL) & (k < nR)
    assert np.array_equal(K_rule, K_def) and np.array_equal(K_rsw, K_def)
    cut = np.minimum(ls[rows, K_def], np.where(K_def > 0, rs[rows, np.maximum(K_def - 1, 0)], INF))
    # the kernel's picture: right stops without `first` behind a sentinel
    rq, _ = stops(Rw & ~(1 << first), True)
    rp = np.concatenate([np.full((Lw.size, 1), INF, dtype=np.int64), rq], axis=1)
    assert np.array_equal(cut, np.minimum(ls[rows, K_def], rp[rows, K_def]))


@pytest.mark.parametrize("n", [20, 32])
def test_random_mask_pairs(n):
    rng = random.Random(1000 + n)
    for _ in range(4000):
        first = rng.randrange(1, n - 4)
        last = rng.randrange(first + 2, n)
        dens_l, dens_r = rng.choice([0.1, 0.5, 0.9, 1.0]), rng.choice([0.1, 0.5, 0.9, 1.0])
        Lw = sum(1 << p for p in range(first + 1, last) if rng.random() < dens_l)
        Rw = sum(1 << p for p in range(first + 1, last) if rng.random() < dens_r) | (1 << first)
        check_masks(Lw, Rw, first, last, n)


# ---- against the sequential algorithm -------------------------------------

def gt(a, b):
    return a > b


def move_median_to_first(v, result, a, b, c):
    """std::__move_median_to_first (stl_algo.h:79-102), comp = greater."""
    def swap(i, j):
        v[i], v[j] = v[j], v[i]
    if gt(v[a], v[b]):
        if gt(v[b], v[c]):
            swap(result, b); return b
        elif gt(v[a], v[c]):
            swap(result, c); return c
        else:
            swap(result, a); return a
    elif gt(v[a], v[c]):
        swap(result, a); return a
    elif gt(v[b], v[c]):
        swap(result, c); return c
    else:
        swap(result, b); return b


def unguarded_partition(v, first, last, pivot):
    """std::__unguarded_partition (stl_algo.h:1878-1896); returns the cut and
    the swapped position pairs."""
    swaps = []
    while True:
        while gt(v[first], v[pivot]):
            first += 1
        last -= 1
        while gt(v[pivot], v[last]):
            last -= 1
        if not first < last:
            return first, swaps
        v[first], v[last] = v[last], v[first]
        swaps.append((first, last))
        first += 1


def rule_partition(v, first, last):
    """The same step by the rule, on the list after the median move."""
    pivot = v[first]
    Lw = sum(1 << p for p in range(first + 1, last) if not gt(v[p], pivot))
    Rw = sum(1 << p for p in range(first, last) if not gt(pivot, v[p]))
    K, cut = check_masks(Lw, Rw, first, last, len(v))
    ls, rs = bits(Lw), bits(Rw)[::-1]
    lsw = [x for x in range(len(v)) if kernel_form(Lw, Rw, first, x)[0]]
    rsw = [x for x in range(len(v)) if kernel_form(Lw, Rw, first, x)[1]]
    assert lsw == ls[:K] and rsw == rs[:K][::-1]
    return cut, list(zip(ls[:K], rs[:K]))


@pytest.mark.parametrize("alphabet", [1, 2, 3, 30])
def test_sequential_partition(alphabet):
    rng = random.Random(77 + alphabet)
    for n in range(4, 21):
        for _ in range(150):
            pad_lo, pad_hi = rng.randrange(0, 3), rng.randrange(0, 3)
            v = [rng.randrange(alphabet) for _ in range(pad_lo + n + pad_hi)]
            first, last = pad_lo, pad_lo + n
            move_median_to_first(v, first, first + 1, first + (last - first) // 2, last - 1)
            seq = list(v)
            cut_seq, swaps_seq = unguarded_partition(seq, first + 1, last, first)
            cut, swaps = rule_partition(v, first, last)
            assert cut == cut_seq, (v, first, last)
            assert swaps == swaps_seq, (v, first, last)
            # and the moved list is the sequential one
            out = list(v)
            for l, r in swaps:
                out[l], out[r] = out[r], out[l]
            assert out == seq
