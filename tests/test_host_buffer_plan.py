"""The buffer plan of every op on the count backend (no GPU) against tests/golden/buffer_plans.json (tests/golden/make_buffer_plans.py, recorded
from this project's own stage-graph builders): the CLI's `Malloc <name> from <first> to <last>` lines in order, and every named buffer of the op with
its limb count.  tests/test_host_structural.py holds the five original ops to the reference's Malloc lines; this also covers hrotate_hoisted,
hlintrans, hdot, hrotsum and hbsgs, the key product's three branches (beta = 1, 2, >= 3), a short last digit and alpha = 1."""
import importlib.util
import json
import os

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
_spec = importlib.util.spec_from_file_location("make_buffer_plans", os.path.join(HERE, "golden", "make_buffer_plans.py"))
gen = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(gen)

GOLD = json.load(open(gen.PATH))["points"]
POINTS, key, record = gen.POINTS, gen.key, gen.record


def test_fixture_covers_every_point():
    assert sorted(GOLD) == sorted(key(p) for p in POINTS) and len(GOLD) == 28 + 5 * 10   # ... and ten variants of the summing ops at five alphas
    assert sum("malloc" in g for g in GOLD.values()) == 10   # one readable point per op


@pytest.mark.parametrize("pt", POINTS, ids=key)
def test_buffer_plan_is_the_recorded_one(pt):
    gold = GOLD[key(pt)]
    got = record(pt, full="malloc" in gold)
    for k in ("malloc", "buffer_limbs"):     # the readable form first: a difference shows as lines, not as two hashes
        if k in gold:
            assert got[k] == gold[k]
    assert got == gold, f'compare: python tests/golden/make_buffer_plans.py --point "{key(pt)}"'
