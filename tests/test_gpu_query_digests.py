"""The posterior queries (exact_query.hip) byte for byte against recorded
digests: tools/query_digest.py gives exactly tests/golden/query_digests.json —
every output and status array of every query, on the 60 x 120 mosaic (both
frontier stores in one launch), on the head_len 2 panel (the head-pattern
spelling) and on the 12 x 1 200 mixed panel (status 1 and 2 in the regular
range), in the regular and in the extended range.

The golden file was written by the tool from the library of the commit before
the query kernels were rewritten on exact_dev.hpp, and pins them since: a change
that is meant to move a byte regenerates it from the commit before that change
(python tools/query_digest.py --json tests/golden/query_digests.json), never
from the code under test.
"""
import importlib.util
import json
import os

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "query_digests.json")


def test_query_digests():
    spec = importlib.util.spec_from_file_location("query_digest", os.path.join(ROOT, "tools", "query_digest.py"))
    qd = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(qd)
    with open(GOLDEN) as f:
        want = json.load(f)
    got = qd.digests()
    assert got.keys() == want.keys() == {"mosaic", "mc", "mixed"}
    bad = []
    for panel in want:
        assert got[panel].keys() == want[panel].keys() == {"regular", "extended"}
        for rng in want[panel]:
            assert got[panel][rng].keys() == want[panel][rng].keys(), (panel, rng)
            assert len(want[panel][rng]) >= 40  # 13 calls, status arrays included
            bad += [(panel, rng, k) for k, h in want[panel][rng].items() if got[panel][rng][k] != h]
    assert not bad, bad
