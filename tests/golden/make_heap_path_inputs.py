"""Regenerates tests/golden/heap_path_ranks.json: permutations of 0..n-1 on
which std::nth_element(v, v + nth, v + n, greater) spends its whole partition
budget (2 * floor(lg n)) with more than 3 elements left and finishes with
std::__heap_select — the branch random, tied, sorted and organ-pipe inputs
practically never reach at n <= 32.

A seeded hill climb over permutations (swap two positions, keep the swap if
the path of tests/introselect_model.py got no shorter) maximises (heap
reached, partitions done, sum of the ranges partitioned).  The pairs are the
E-step's shape (nth = S - 1, n in S+1..2S) where such inputs exist, general
nth at n = 16, 24, 32, and the wide lists n = 66, 100, 128.

    python tests/golden/make_heap_path_inputs.py

Deterministic: the same file comes out of every run.  The tests assert
through the model that every committed list still reaches the heap select.
"""
import json
import os
import random
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
from introselect_model import path  # noqa: E402

# E-step shape: sample size S -> the n (S < n <= 2S) with a known heap-path input
ESTEP = {7: [13, 14], 8: [13, 14, 15, 16], 10: list(range(13, 21)),
         12: [14, 15] + list(range(17, 25)), 16: list(range(18, 33))}
GENERAL = {16: [7, 8, 9, 10, 11], 24: [4, 8, 11, 12, 17, 23], 32: [5, 10, 15, 16, 22, 31]}
WIDE = {66: [20, 32, 50], 100: [30, 49, 80], 128: [40, 63, 64, 100]}
PER_PAIR = 2  # distinct lists per (n, nth)


def score(v, nth):
    p = path(v, nth)
    return (p.heap, p.partitions, sum(p.ranges))


def climb(n, nth, rng, steps=6000, restarts=40):
    for _ in range(restarts):
        v = list(range(n))
        rng.shuffle(v)
        s = score(v, nth)
        for _ in range(steps):
            if s[0]:
                return v
            i, j = rng.randrange(n), rng.randrange(n)
            if i == j:
                continue
            v[i], v[j] = v[j], v[i]
            t = score(v, nth)
            if t >= s:
                s = t
            else:
                v[i], v[j] = v[j], v[i]
        if s[0]:
            return v
    return None


def main():
    pairs = [(n, S - 1, "estep") for S, ns in ESTEP.items() for n in ns]
    pairs += [(n, nth, "general") for n, nths in GENERAL.items() for nth in nths]
    pairs += [(n, nth, "wide") for n, nths in WIDE.items() for nth in nths]
    out, missing = [], []
    for n, nth, kind in pairs:
        seen = set()
        for rep in range(PER_PAIR):
            rng = random.Random(1000003 * n + 1009 * nth + rep)
            v = climb(n, nth, rng)
            if v is None or tuple(v) in seen:
                missing.append((n, nth, rep))
                continue
            seen.add(tuple(v))
            p = path(v, nth)
            out.append({"n": n, "nth": nth, "kind": kind, "partitions": p.partitions, "heap_len": p.heap_len,
                        "ranks": v})
        print(n, nth, kind, len(seen), flush=True)
    with open(os.path.join(HERE, "heap_path_ranks.json"), "w") as f:
        f.write("[\n" + ",\n".join(json.dumps(e, separators=(",", ":")) for e in out) + "\n]\n")
    print(f"{len(out)} lists; none found for {missing}")


if __name__ == "__main__":
    main()
