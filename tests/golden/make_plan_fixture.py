#!/usr/bin/env python3
"""Generate tests/golden/plans_existing_ops.json: the launch plans (count backend, no GPU) of the five original operations.

The fixture pins the plans as they were before hrotate_hoisted existed (tests/test_host_hoisted_plan.py asserts equality), so that adding
an operation and its fusion pass cannot move a launch of hmult / hrotate / hadd / pmult / padd.  Regenerate only on purpose:
    python tests/golden/make_plan_fixture.py
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

from homulator_amd import host  # noqa: E402

POINTS = [("config_4.cfg", 45, 35, 15), ("config_4_N15.cfg", 16, 10, 4)]
OPS = ["hmult", "hrotate", "hadd", "pmult", "padd"]


def record(cfg, op, L, ell, alpha, fuse):
    o = host.Op(cfg, op, L, ell, alpha, backend=host.BACKEND_COUNT, fuse=fuse)
    try:
        return {"cfg": cfg, "op": op, "L": L, "l": ell, "alpha": alpha, "fuse": int(fuse), "plan": o.plan(),
                "total_instructions": o.total_instructions(), "stage_bytes": o.stage_bytes()}
    finally:
        o.close()


def main():
    out = {"generated_by": "tests/golden/make_plan_fixture.py", "points": []}
    for cfg, L, ell, alpha in POINTS:
        for op in OPS:
            for fuse in (True, False):
                out["points"].append(record(cfg, op, L, ell, alpha, fuse))
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "plans_existing_ops.json")
    with open(path, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
