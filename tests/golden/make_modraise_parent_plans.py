#!/usr/bin/env python3
"""Generate tests/golden/plans_before_modraise.json: plan() and plan(full=True) (count backend, no GPU) of hmult, hrotate, pmult and hrescale as the
host layer printed them BEFORE hmodraise existed (tests/test_host_modraise_plan.py asserts equality), so that the lifted transform's record field, its
role, its part key and its plan fields cannot move a launch of an existing op.  Run it on a build of the commit before the op, on purpose only:
    python tests/golden/make_modraise_parent_plans.py [path of that build's libhomulator_host.so]
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

from homulator_amd import host  # noqa: E402

POINTS = [("config_4.cfg", 45, 35, 15), ("config_4_N15.cfg", 16, 10, 4)]
OPS = [("hmult", {}), ("hrotate", {}), ("pmult", {}), ("pmult", {"rescale": 1}), ("hrescale", {}), ("hrescale", {"batch": 3})]


def record(cfg, op, ov, L, ell, alpha, fuse):
    o = host.Op(cfg, op, L, ell, alpha, backend=host.BACKEND_COUNT, fuse=fuse, overrides=ov or None)
    try:
        return {"cfg": cfg, "op": op, "overrides": ov, "L": L, "l": ell, "alpha": alpha, "fuse": int(fuse), "plan": o.plan(), "full": o.plan(full=True)}
    finally:
        o.close()


def main():
    if len(sys.argv) > 1:
        host.LIB_PATH = os.path.abspath(sys.argv[1])
    out = {"generated_by": "tests/golden/make_modraise_parent_plans.py", "points": []}
    for cfg, L, ell, alpha in POINTS:
        for op, ov in OPS:
            for fuse in (True, False):
                out["points"].append(record(cfg, op, ov, L, ell, alpha, fuse))
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "plans_before_modraise.json")
    with open(path, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
