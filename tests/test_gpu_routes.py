"""The same solver takes the same move: tests/golden/expansion_routes_v1.json, recorded on an MI355X before the routing of expansion
moves went into csrc/move_route.h, replayed on the library as built.  The oracle comparisons of test_gpu_parity.py pin WHAT a move
computes; this file pins WHO computed it (expansion_paths, the work counters, the launch counters), at the smallest shapes on either
side of every routing edge and under each routing switch.  Cases and recorded fields: tests/route_cases.py."""
import json
import os

import pytest

import route_cases

with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "expansion_routes_v1.json")) as f:
    GOLDEN = json.load(f)


def test_the_recording_covers_every_case_and_dropped_nothing_it_must_keep():
    assert sorted(GOLDEN["cases"]) == sorted(route_cases.cases())
    for entry in GOLDEN["header"]["dropped"]:
        assert not route_cases.must_keep(entry.split(":", 1)[1]), entry


@pytest.mark.gpu
@pytest.mark.parametrize("case_id", list(route_cases.cases()))
def test_route_replays(case_id):
    want = GOLDEN["cases"][case_id]
    got = route_cases.flatten(route_cases.run_case(case_id))
    assert set(want) <= set(got)
    differ = {k: (want[k], got[k]) for k in want if want[k] != got[k]}
    assert not differ, f"{case_id}: (recorded, now) {differ}"
