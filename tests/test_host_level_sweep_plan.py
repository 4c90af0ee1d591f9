"""The grid of tests/test_gpu_level_sweep.py without a GPU (count backend): every point builds a plan, the ops that rescale refuse l = 1 and
nothing else is refused, and every point takes the route recorded in tests/golden/level_sweep_routes.json.  The recorded routes are then held to
the rules the sweep relies on, so that the GPU sweep cannot pass by running the plain plan:
  * the ops that switch one key of their own (hdot, hsquare, hmuladd, hdotadd, hreim) have no ModUp base-conversion launch and one second_pass_only
    inverse transform up to beta = 4 at N = 2^15, with digits of up to 28 limbs; at N = 2^16 a digit above 15 limbs keeps its conversion launch;
  * the ops that share one ModUp among several rotations (hrotate_hoisted, hlintrans, hrotsum, hbsgs) store the raised digits, so their plan keeps
    one conversion launch per shared ModUp at every shape and no second_pass_only transform;
  * up to beta = 4 the op's own launch kinds are there as often as the op's own test file asserts, from beta = 5 none of them is, the key products are
    element-wise and the rotating ops run automorphism launches."""
import importlib.util
import json
import os

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
_spec = importlib.util.spec_from_file_location("make_level_sweep_routes", os.path.join(HERE, "golden", "make_level_sweep_routes.py"))
gen = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(gen)

GOLDEN = json.load(open(gen.PATH))["routes"]
POINTS = gen.points()
REFUSAL = "Rescale needs at least two limbs"
OWN_MODUP = gen.OWN_MODUP


def test_the_golden_file_covers_the_grid_and_nothing_else():
    keys = [gen.key(p) for p in POINTS]
    assert len(set(keys)) == len(keys) and set(GOLDEN) == set(keys)
    # grid A: 14 rows x 4 digit widths x 13 levels; grid B: 14 rows x 4 levels and the three N = 2^16 points
    assert sum(p[0] == "A" for p in POINTS) == len(gen.ROWS) * len(gen.A_ALPHAS) * gen.A_L == 728
    assert sum(p[0] == "B" for p in POINTS) == len(gen.ROWS) * len(gen.B_LEVELS) == 56 and sum(p[0] == "B16" for p in POINTS) == 3
    assert {a for a, _ in gen.A_RUNS} == set(gen.A_ALPHAS)


@pytest.mark.parametrize("name", list(gen.ROWS) + list(gen.ELEMENTWISE) + ["hmodraise"])
def test_plans_are_the_recorded_ones(name):
    """the planner against the file, point by point; the file regenerates byte for byte when nothing moved"""
    pts = [p for p in POINTS if p[1] == name]
    assert pts
    moved = [gen.key(p) for p in pts if gen.route_of(p) != GOLDEN[gen.key(p)]]
    assert not moved, f"{len(moved)} of {len(pts)} routes of {name} moved: {moved[:5]}"


def test_only_level_1_of_the_ops_that_rescale_is_refused():
    for p in POINTS:
        _, name, _, _, _, _, ell = p
        r = GOLDEN[gen.key(p)]
        if gen.row_of(name).rescales and ell == 1:
            assert REFUSAL in r["rejected"], gen.key(p)
        else:
            assert "rejected" not in r, gen.key(p)
            if name != "hrotate_hoisted":
                assert r["level"] == ell - gen.row_of(name).rescales, gen.key(p)


def test_the_recorded_routes_switch_where_the_sweep_expects():
    seen = set()
    for p in POINTS:
        grid, name, _, logN, _, alpha, ell = p
        r = GOLDEN[gen.key(p)]
        if grid == "E" or "rejected" in r:
            continue
        row, kinds, b = gen.ROWS[name], r["kinds"], gen.beta(ell, alpha)
        merged = {k: kinds.get(k, 0) for k in gen.MERGED_KINDS if kinds.get(k, 0)}
        seen.add((name in OWN_MODUP, min(b, 5)))
        if b <= 4:
            assert merged == row.merged, gen.key(p)
            assert "AUTO" not in kinds and "EWE" not in kinds, gen.key(p)
        else:     # the fallback route: element-wise key products, an automorphism launch per rotation; the tensor launch and hreim's split stay
            assert merged == {k: v for k, v in row.merged.items() if k.startswith("TENSOR") or k == "REIM"}, gen.key(p)
            assert kinds.get("EWE", 0) >= b - 1 and ("AUTO" in kinds) == (row.rotates or name == "hreim"), gen.key(p)
        if name in OWN_MODUP:
            wide16 = logN == 16 and min(ell, alpha) > 15
            assert r["modup_bconv"] == (1 if b > 4 or wide16 else 0), gen.key(p)
            assert r["second_pass_only"] == (1 if b <= 4 else 0), gen.key(p)
            assert kinds.get("NTT_IP", 0) == (1 if b <= 4 else 0) and kinds.get("IP", 0) == (1 if b == 1 else 0), gen.key(p)
        else:
            shared_modups = 2 if row.op == "hbsgs" else 1
            assert r["modup_bconv"] == shared_modups and kinds["NTT"] == shared_modups and r["second_pass_only"] == 0, gen.key(p)
    assert seen == {(own, b) for own in (True, False) for b in range(1, 6)}     # every digit count up to the switch, and the fallback, on both families


def test_where_the_unfused_plan_runs():
    assert [gen.unfused_levels(a) for a in gen.A_ALPHAS] == [[2, 3, 13], [2, 3, 4, 13], [2, 5, 6, 13], [2, 13]]


def test_the_unfused_plan_has_none_of_the_merged_launches():
    for name in gen.ROWS:
        for ell in gen.unfused_levels(3):
            op = gen.make_op(("A", name, gen.CFG15, 15, gen.A_L, 3, ell), fuse=False)
            kinds = {ln.split()[0] for ln in op.plan()}
            op.close()
            assert not kinds & set(gen.MERGED_KINDS) and "NTT_IP" not in kinds, (name, ell, kinds)
