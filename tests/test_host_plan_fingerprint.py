"""The launch plans of the whole grid of tests/golden/make_plan_fingerprints.py (count backend, no GPU) are, operand for operand, the ones
recorded in tests/golden/plan_fingerprints.json: per bucket of points, the SHA-256 over every point's fingerprint (the SHA-256 of
host.Op.plan(full=True) plus the instruction / launch / byte totals, or the message of the exception where the code rejects the
combination).  The planner (host/src/Planner.cpp, the launch builder in host/src/Arch.cpp) may be restructured freely; a plan may not move."""
import importlib.util
import json
import os

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
_spec = importlib.util.spec_from_file_location("make_plan_fingerprints", os.path.join(HERE, "golden", "make_plan_fingerprints.py"))
gen = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(gen)

GOLDEN = json.load(open(gen.PATH))["groups"]


def test_the_golden_file_covers_the_grid_and_nothing_else():
    assert set(GOLDEN) == set(gen.GRID)
    for name, pts in gen.GRID.items():
        want = {}
        for p in pts:
            want[gen.bucket(p)] = want.get(gen.bucket(p), 0) + 1
        assert {b: d["points"] for b, d in GOLDEN[name].items()} == want, name
    # a rejection is recorded as such, never as a plan: rotations beyond what one op takes, and nothing else on this grid
    rejecting = {name for name, g in GOLDEN.items() if any("rejected" in d for d in g.values())}
    assert rejecting == {f"hrotate_hoisted rotations={gen.MAX_ROT + 1}"}


@pytest.mark.parametrize("group", list(gen.GRID))
def test_plans_are_the_recorded_ones(group):
    got = gen.digests(group)
    moved = [b for b in GOLDEN[group] if got.get(b) != GOLDEN[group][b]]
    assert not moved, f"plans moved in {len(moved)} of {len(got)} buckets of '{group}': {moved[:5]} (make_plan_fingerprints.py --points lists them)"
