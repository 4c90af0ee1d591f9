#!/usr/bin/env python3
"""Generate tests/golden/plans_before_mlincomb.json: plan() and the SHA-256 of plan(full=True) joined by newlines (count backend, no GPU) of hmult,
hlincomb (terms 1, 4 and 16, with and without the constant, with and without rescale), hclincomb, hplincomb and hdotadd as the host layer printed
them BEFORE hmlincomb existed (tests/test_host_mlincomb_plan.py asserts equality), so that the new record fields, the part key, the launch kind and
the planner pass behind (5l) cannot move a launch of an existing op.  Run it on a build of the commit before the op, on purpose only:
copied into tests/golden/ of a built checkout of that commit (it loads that checkout's Python package and host library), then copy the JSON back:
    python tests/golden/make_mlincomb_parent_plans.py
"""
import hashlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

from homulator_amd import host  # noqa: E402

# (config, L, l, alpha, fuse): the headline shape as it runs, fused, and the small one launch by launch, unfused; the other combinations of the grid
# are pinned by hash in plan_fingerprints.json
POINTS = [("config_4.cfg", 45, 35, 15, True), ("config_4_N15.cfg", 16, 10, 4, False)]
OPS = ([("hmult", {})] + [("hlincomb", {"terms": t, "lc_const": k, "rescale": r}) for t in (1, 4, 16) for k in (0, 1) for r in (0, 1)] +
       [("hclincomb", {"terms": 4, "cl_const": k}) for k in (0, 1)] + [("hplincomb", {"terms": 4})] +
       [("hdotadd", {"terms": 2, "addends": 1, "da_scale": v, "da_const": v}) for v in (0, 1)])


def record(cfg, op, ov, L, ell, alpha, fuse):
    o = host.Op(cfg, op, L, ell, alpha, backend=host.BACKEND_COUNT, fuse=fuse, overrides=ov or None)
    try:
        return {"cfg": cfg, "op": op, "overrides": ov, "L": L, "l": ell, "alpha": alpha, "fuse": int(fuse), "plan": o.plan(),
                "full_sha256": hashlib.sha256("\n".join(o.plan(full=True)).encode()).hexdigest()}
    finally:
        o.close()


def main():
    out = {"generated_by": "tests/golden/make_mlincomb_parent_plans.py", "points": []}
    for cfg, L, ell, alpha, fuse in POINTS:
        for op, ov in OPS:
            out["points"].append(record(cfg, op, ov, L, ell, alpha, fuse))
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "plans_before_mlincomb.json")
    with open(path, "w") as f:
        f.write('{"generated_by": %s, "points": [\n' % json.dumps(out["generated_by"]))   # one point per line
        f.write(",\n".join(json.dumps(p) for p in out["points"]) + "\n]}\n")


if __name__ == "__main__":
    main()
