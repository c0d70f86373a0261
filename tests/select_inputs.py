"""Inputs of the k-best selection tests (test infrastructure): the committed
heap-path rank lists in three order-isomorphic value maps, the six input kinds
of the older selection tests, and wavefronts composed from them on purpose.

Everything here is deterministic and runs on the CPU.  `reference()` pairs
every list with the real std::nth_element's result and with the path report of
tests/introselect_model.py, and refuses a list on which the two disagree: a
path report is only used for a list the model permutes like libstdc++.
"""
from __future__ import annotations

import json
import os
from dataclasses import dataclass, field

import numpy as np

import introselect_model as model

_GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "heap_path_ranks.json")
VALUE_MAPS = ("ranks", "likelihoods", "subnormals")


def heap_path_ranks():
    """The committed lists: dicts with n, nth, kind ('estep', 'general', 'wide'), ranks."""
    with open(_GOLDEN) as f:
        return json.load(f)


def map_values(ranks, how):
    """Order-isomorphic images of a rank list: the algorithm only compares, so
    its path is the same on all three."""
    r = np.asarray(ranks, np.float64)
    n = len(r)
    if how == "ranks":
        return r.copy()
    if how == "likelihoods":  # products of many transition probabilities: 1e-300 .. 0.1
        return 10.0 ** (-300.0 + 299.0 * r / max(n - 1, 1))
    if how == "subnormals":   # rank * 2^-1074: FP64 denormals, kept by the kernels
        return np.ldexp(r, -1074)
    raise ValueError(how)


def six_kinds(rng, n, kind):
    """The input kinds of test_segmented_nth_element_matches_libstdcxx."""
    if kind == 0:
        return rng.random(n)
    if kind == 1:
        return rng.integers(0, 3, n).astype(np.float64)
    if kind == 2:
        return np.zeros(n)
    if kind == 3:
        return np.arange(n, dtype=np.float64)[:: (1 if rng.random() < 0.5 else -1)].copy()
    if kind == 4:
        return np.concatenate([np.arange(n // 2), np.arange(n - n // 2)[::-1]]).astype(np.float64)
    v = rng.integers(0, 4, n).astype(np.float64) * 1e-300
    v[rng.integers(0, n)] = np.nan
    return v


@dataclass
class SelList:
    values: np.ndarray
    nth: int
    origin: str                      # 'heap', 'kind0'..'kind5', 'idle', 'noop'
    path: model.Path = None
    ref_values: np.ndarray = None    # after the real std::nth_element
    ref_tags: np.ndarray = None

    @property
    def n(self):
        return len(self.values)


def reference(oracle_mod, lists):
    """Fills path / ref_* of every list; the model must permute it like libstdc++."""
    for s in lists:
        if s.path is not None:
            continue
        tags = np.arange(s.n, dtype=np.int32)
        s.ref_values, s.ref_tags = oracle_mod.std_nth_element(s.values, tags, s.nth)
        mv, mt, s.path = model.nth_element(s.values.tolist(), tags.tolist(), s.nth)
        assert mt == s.ref_tags.tolist(), ("model != std::nth_element", s.n, s.nth, s.values)
        assert np.array_equal(np.asarray(mv, np.float64).view(np.uint64), s.ref_values.view(np.uint64))
    return lists


def heap_lists(cap):
    """Every committed heap-path list with n <= cap, in the three value maps."""
    out = []
    for e in heap_path_ranks():
        if e["n"] <= cap:
            for how in VALUE_MAPS:
                out.append(SelList(map_values(e["ranks"], how), e["nth"], "heap"))
    return out


def generic_lists(rng, cap, total):
    """The six kinds at n = 1..cap, half with the E-step's call (nth = S - 1,
    n in S+1..2S, S = cap / 2) and half with nth drawn from [0, n]."""
    out = []
    S = cap // 2
    while len(out) < total:
        for n in range(1, cap + 1):
            kind = int(rng.integers(0, 6))
            v = six_kinds(rng, n, kind)
            estep = S >= 1 and n > S and rng.random() < 0.5
            nth = S - 1 if estep else int(rng.integers(0, n + 1))
            out.append(SelList(v, nth, "noop" if nth == n else f"kind{kind}"))
    return out


def idle_list():
    return SelList(np.zeros(0), 0, "idle")


@dataclass
class Composition:
    lists: list                       # list j runs in wave j // G, segment j % G
    G: int
    waves: dict = field(default_factory=dict)  # composed kind -> number of waves
    heap: int = 0                     # lists that take the heap path


def _classify(wave):
    """The composed kinds a wavefront of lists belongs to, from the model's reports."""
    heaps = [s for s in wave if s.path.heap]
    kinds = set()
    if len(heaps) >= 2:
        kinds.add("two_heaps")
    if heaps:
        spent = min(s.path.partitions for s in heaps)
        if any(s.path.partitions > spent for s in wave):
            kinds.add("heap_and_longer_partitioning")
        if any(s.path.insertion_len == 2 for s in wave):
            kinds.add("heap_and_insertion2")
        if any(s.path.insertion_len == 3 for s in wave):
            kinds.add("heap_and_insertion3")
        if any(s.n == 0 for s in wave) and any(s.n > 0 and s.path.noop for s in wave):
            kinds.add("heap_idle_noop")
    if any(s.n == 0 for s in wave) and any(s.n > 0 and s.path.noop for s in wave):
        kinds.add("idle_and_noop")
    return kinds


def compose(oracle_mod, seed, cap, G, total=2000):
    """Wavefronts of G lists of up to `cap` elements: composed on purpose where
    heap-path inputs of that length exist, then the generic lists shuffled."""
    rng = np.random.default_rng(seed)
    heaps = reference(oracle_mod, heap_lists(cap))
    gen = reference(oracle_mod, generic_lists(rng, cap, total))
    noops = [s for s in gen if s.n > 0 and s.path.noop]
    ins2 = [s for s in gen if s.path.insertion_len == 2]
    ins3 = [s for s in gen if s.path.insertion_len == 3]
    used = set()
    waves = []

    def clone(s):  # a list placed a second time is a record of its own
        return SelList(s.values, s.nth, s.origin, s.path, s.ref_values, s.ref_tags)

    def pick(pool, i):
        return clone(pool[i % len(pool)])

    def fill(wave):
        while len(wave) < G:
            wave.append(pick(gen, int(rng.integers(0, len(gen)))))
        order = rng.permutation(G)
        return [wave[i] for i in order]

    if heaps and G >= 2:
        by_parts = sorted(range(len(heaps)), key=lambda i: heaps[i].path.partitions)
        short, longest = heaps[by_parts[0]], heaps[by_parts[-1]]
        for i in range(0, len(heaps) - 1, 2):                      # two heap-path lists (G > 2: plus others)
            waves.append(fill([heaps[i], heaps[i + 1]]))
            used.update((i, i + 1))
        if longest.path.partitions > short.path.partitions:        # budget spent next to one still partitioning
            for i in by_parts[:4]:
                waves.append(fill([clone(heaps[i]), clone(longest)]))
        for i in range(4):                                         # next to 2- and 3-element insertion sorts
            if G >= 3:
                waves.append(fill([pick(heaps, i), pick(ins2, i), pick(ins3, i)]))
            else:
                waves.append(fill([pick(heaps, i), pick(ins2, i)]))
                waves.append(fill([pick(heaps, i + 1), pick(ins3, i)]))
        if G >= 3:                                                 # next to an idle segment and a no-op
            for i in range(4):
                waves.append(fill([pick(heaps, i), idle_list(), pick(noops, i)]))
    for i, s in enumerate(heaps):                                  # every heap-path list runs at least once
        if i not in used:
            waves.append(fill([s]))
    for i in range(4):                                             # idle and no-op lists without a heap list
        w = [idle_list(), pick(noops, i)] if G >= 2 else [idle_list()]
        waves.append(fill(w))
    rest = list(gen)
    order = rng.permutation(len(rest))
    rest = [rest[i] for i in order]
    while len(rest) % G:
        rest.append(idle_list())
    waves += [rest[i:i + G] for i in range(0, len(rest), G)]
    order = rng.permutation(len(waves))
    waves = [waves[i] for i in order]

    comp = Composition([s for w in waves for s in w], G)
    reference(oracle_mod, comp.lists)
    for w in waves:
        for k in _classify(w):
            comp.waves[k] = comp.waves.get(k, 0) + 1
    comp.heap = sum(1 for s in comp.lists if s.path.heap)
    return comp


def required_wave_kinds(cap, G):
    """The composed kinds a layout must run, given what its widths admit.

    A heap-path list needs n >= 13 (none is known below), whose budget is
    2 * floor(lg n) = 6 partitions for n <= 15 and 8 from n = 16 on.  A
    neighbour still partitioning after a heap list's budget is spent therefore
    needs cap >= 16; at cap = 14 every list's budget is at most 6.  A wave of
    one list (G = 1) has no neighbours, and a wave of two cannot hold a heap
    list, an idle segment and a no-op together."""
    if cap < 13 or G < 2:
        return set()
    req = {"two_heaps", "heap_and_insertion2", "heap_and_insertion3", "idle_and_noop"}
    if cap >= 16:
        req.add("heap_and_longer_partitioning")
    if G >= 3:
        req.add("heap_idle_noop")
    return req


# every layout the GPU tests run: name -> (longest list, lists per wavefront)
LAYOUTS = {f"one_link_sw{sw}": (sw, 64 // sw) for sw in (14, 20, 32)}
LAYOUTS.update({f"pair_W{W}": (2 * W, 64 // W) for W in (1, 2, 3, 7, 10, 16)})
LAYOUTS["wide"] = (128, 1)
_COMPOSED = {}


def layout_composition(oracle_mod, name):
    """The lists of one layout with their references, built once per session."""
    if name not in _COMPOSED:
        cap, G = LAYOUTS[name]
        seed = 9000 + list(LAYOUTS).index(name)
        _COMPOSED[name] = compose(oracle_mod, seed, cap, G, total=600 if cap > 32 else 2000)
    return _COMPOSED[name]


def check_coverage(name, comp):
    """The coverage conditions of the selection tests, from the model's reports:
    at least 8 heap-path lists at every width that admits them (n >= 13), at
    least one wavefront of every composed kind the width admits, idle and no-op
    lists, 2- and 3-element insertion sorts.  Below 13 elements no heap-path
    input is known: the count is printed and nothing is asserted about it."""
    cap, G = LAYOUTS[name]
    print(f"{name}: {len(comp.lists)} lists, {comp.heap} on the heap path, "
          f"composed waves {dict(sorted(comp.waves.items()))}")
    if cap >= 13:
        assert comp.heap >= 8, (name, comp.heap)
    missing = required_wave_kinds(cap, G) - {k for k, c in comp.waves.items() if c > 0}
    assert not missing, (name, missing)
    assert any(s.n == 0 for s in comp.lists) and any(s.n > 0 and s.path.noop for s in comp.lists)
    assert any(s.path.insertion_len == 2 for s in comp.lists)
    assert cap < 3 or any(s.path.insertion_len == 3 for s in comp.lists)
