#!/usr/bin/env python3
"""Generate tests/golden/plans_before_plincomb.json: plan() and the SHA-256 of plan(full=True) joined by newlines (count backend, no GPU) of pmult
(with and without rescale), hlincomb (terms 4, with the constant, with and without rescale), hlintrans (rotations = 3), hmult and hrescale as the
host layer printed them BEFORE hplincomb existed (tests/test_host_plincomb_plan.py asserts equality), so that the level-l plaintexts of makeInputs,
the new record fields, the part key, the launch kind, the planner pass and the exception in pass (4p) cannot move a launch of an existing op; and
hrescale's plan, which hplincomb's plan with rescale = 1 is held to.
Run it on a build of the commit before the op, on purpose only: copied into tests/golden/ of a built checkout of that commit (it loads that
checkout's Python package and host library), then copy the JSON back:
    python tests/golden/make_plincomb_parent_plans.py
"""
import hashlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

from homulator_amd import host  # noqa: E402

# (config, L, l, alpha, fuse): the headline shape as it runs, fused, and the small one both fused and launch by launch
POINTS = [("config_4.cfg", 45, 35, 15, True), ("config_4_N15.cfg", 16, 10, 4, True), ("config_4_N15.cfg", 16, 10, 4, False)]
OPS = ([("pmult", {"rescale": r}) for r in (0, 1)] + [("hlincomb", {"terms": 4, "lc_const": 1, "rescale": r}) for r in (0, 1)] +
       [("hlintrans", {"rotations": 3}), ("hmult", {}), ("hrescale", {})])


def record(cfg, op, ov, L, ell, alpha, fuse):
    o = host.Op(cfg, op, L, ell, alpha, backend=host.BACKEND_COUNT, fuse=fuse, overrides=ov or None)
    try:
        return {"cfg": cfg, "op": op, "overrides": ov, "L": L, "l": ell, "alpha": alpha, "fuse": int(fuse), "plan": o.plan(),
                "full_sha256": hashlib.sha256("\n".join(o.plan(full=True)).encode()).hexdigest(), "launches": o.launch_count(),
                "instructions": o.total_instructions()}
    finally:
        o.close()


def main():
    out = {"generated_by": "tests/golden/make_plincomb_parent_plans.py", "points": []}
    for cfg, L, ell, alpha, fuse in POINTS:
        for op, ov in OPS:
            out["points"].append(record(cfg, op, ov, L, ell, alpha, fuse))
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "plans_before_plincomb.json")
    with open(path, "w") as f:
        f.write('{"generated_by": %s, "points": [\n' % json.dumps(out["generated_by"]))   # one point per line
        f.write(",\n".join(json.dumps(p) for p in out["points"]) + "\n]}\n")


if __name__ == "__main__":
    main()
