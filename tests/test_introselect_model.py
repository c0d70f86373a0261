"""tests/introselect_model.py (the path-reporting Python restatement of
std::nth_element) against the real libstdc++ algorithm compiled into the CPU
restatement, and the committed heap-path inputs against the model: the GPU
selection tests trust the model's path reports only because of these."""
import numpy as np
import pytest

import introselect_model as model
import select_inputs as si

# (n, nth) the heap-path fixture must hold: the E-step's shape nth = S - 1,
# n in S+1..2S where such inputs exist, general nth at 16, 24, 32, wide lists
ESTEP_SHAPES = {7: [13, 14], 8: [13, 14, 15, 16], 10: list(range(13, 21)),
                12: [14, 15] + list(range(17, 25)), 16: list(range(18, 33))}


def _inputs(rng, n):
    for kind in range(6):
        yield si.six_kinds(rng, n, kind)
    yield rng.permutation(n).astype(np.float64)
    yield rng.integers(0, max(2, n // 3), n).astype(np.float64)  # ties, more distinct values as n grows


@pytest.mark.parametrize("n", range(1, 129))
def test_model_matches_libstdcxx(oracle_mod, n):
    """Every nth in [0, n] (nth == n is a no-op) on the six kinds, a random
    permutation and a tied list: the same (value, tag) arrangement, values
    compared by their bits (NaN is among them)."""
    rng = np.random.default_rng(4000 + n)
    tags = np.arange(n, dtype=np.int32)
    for v in _inputs(rng, n):
        vl, tl = v.tolist(), tags.tolist()
        for nth in range(n + 1):
            rv, rt = oracle_mod.std_nth_element(v, tags, nth)
            mv, mt, p = model.nth_element(vl, tl, nth)
            assert mt == rt.tolist(), (n, nth, v)
            assert np.array_equal(np.asarray(mv, np.float64).view(np.uint64), rv.view(np.uint64)), (n, nth, v)
            assert p.noop == (nth == n)
            assert p.partitions <= 2 * (n.bit_length() - 1)
            assert p.heap == (p.heap_len > 3) and (p.heap or p.noop or p.insertion_len <= 3)


def test_model_path_of_the_issue_example():
    v = [0, 17, 12, 2, 16, 7, 13, 5, 15, 8, 10, 1, 9, 11, 3, 14, 18, 6, 4, 19]
    p = model.path(v, 9)
    assert p.heap and p.partitions == 8


def test_heap_path_fixture_reaches_the_heap_select(oracle_mod):
    """Every committed list, in each value map, spends the whole budget with
    more than 3 elements left, and the model permutes it like libstdc++; the
    fixture holds every required (n, nth)."""
    entries = si.heap_path_ranks()
    have = {(e["n"], e["nth"]) for e in entries}
    for S, ns in ESTEP_SHAPES.items():
        for n in ns:
            assert (n, S - 1) in have, (S, n)
    for n in (16, 24, 32, 66, 100, 128):
        assert any(e["n"] == n for e in entries), n
    for n in (16, 24, 32):  # general nth: more than the E-step's one
        assert len({e["nth"] for e in entries if e["n"] == n and e["kind"] == "general"}) >= 2, n
    lists = []
    for e in entries:
        assert sorted(e["ranks"]) == list(range(e["n"]))
        for how in si.VALUE_MAPS:
            lists.append(si.SelList(si.map_values(e["ranks"], how), e["nth"], "heap"))
    si.reference(oracle_mod, lists)
    for s in lists:
        assert s.path.heap and s.path.partitions == 2 * (s.n.bit_length() - 1) and s.path.heap_len > 3, (s.n, s.nth)
    assert len(set(np.ldexp(1.0, -1074) * np.arange(4))) == 4  # subnormals stay distinct on the host


def test_value_maps_are_order_isomorphic():
    r = np.random.default_rng(5).permutation(128)
    for how in si.VALUE_MAPS:
        v = si.map_values(r, how)
        assert np.array_equal(np.argsort(v), np.argsort(r)) and len(set(v.tolist())) == 128
    assert si.map_values(r, "likelihoods").min() == 1e-300
    sub = si.map_values(r, "subnormals")
    assert sub.max() < np.finfo(np.float64).tiny and sorted(sub.view(np.uint64).tolist()) == list(range(128))


@pytest.mark.parametrize("name", list(si.LAYOUTS))
def test_composed_wavefronts_cover_the_paths(oracle_mod, name):
    """The wavefronts the GPU tests run hold what they are meant to hold (the
    same check runs there on the same lists), and every list in them is one
    the model permutes like libstdc++ (select_inputs.reference)."""
    cap, G = si.LAYOUTS[name]
    comp = si.layout_composition(oracle_mod, name)
    si.check_coverage(name, comp)
    assert all(s.n <= cap for s in comp.lists) and len(comp.lists) % G == 0
