#!/usr/bin/env python3
"""Generate tests/golden/level_sweep_routes.json: the route every point of the level sweep takes today, on the count backend (no GPU).

The sweep (tests/test_gpu_level_sweep.py) runs every op that switches keys at every level of a 13-limb chain at N = 2^15, where the capability
table (homulator_amd/csrc/hm_caps.h) gives the fused forms, and with digits of 15 to 28 limbs.  This file is the sweep's one table: ROWS names
the op variants, points() lists the grids, and route() reduces a launch plan to what the sweep holds the HIP backend's plan to:
    kinds              the multiset of launch kinds (the first word of every plan line)
    modup_bconv        the launches that are a ModUp base conversion of their own (BCONV ... ModUp_BCONV ...)
    second_pass_only   the inverse transforms whose first pass ran inside the key product
    level              the output level (Op.output_level())
or, where the code rejects the point, the message.  tests/test_host_level_sweep_plan.py holds the planner to the file, so a planner change that
moves a boundary between routes (beta = 4 to 5, 15 to 16 input limbs, l <= alpha) shows up there and in the sweep at once.
Regenerate only on purpose:
    python tests/golden/make_level_sweep_routes.py
"""
import collections
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

from homulator_amd import host  # noqa: E402

PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "level_sweep_routes.json")

Row = collections.namedtuple("Row", "op overrides rescales merged rotates outputs")
R_HOIST = 3
# name: the op, the overrides that select the variant, whether the output is one level down (then l = 1 is refused), the launch kinds of the
# merged route ({kind: launches}), whether the fallback route rotates with AUTO launches, and the output names
ROWS = {
    "hrotate_hoisted": Row("hrotate_hoisted", {"rotations": R_HOIST}, False, {"IP_HOISTED": 1}, True, [f"out{r}" for r in range(1, R_HOIST + 1)]),
    "hlintrans": Row("hlintrans", {"rotations": 3}, False, {"IP_LINTRANS": 1}, True, ["out"]),
    "hlintrans_id": Row("hlintrans", {"rotations": 3, "identity": 1}, False, {"IP_LINTRANS": 1}, True, ["out"]),
    "hdot": Row("hdot", {"terms": 3}, True, {"TENSOR_DOT": 1}, False, ["out"]),
    "hrotsum": Row("hrotsum", {"rotations": 3}, False, {"IP_ROTSUM": 1}, True, ["out"]),
    "hbsgs": Row("hbsgs", {"rotations": 2, "giants": 2}, False, {"IP_LINTRANS_MULTI": 1, "IP_ROTSUM": 1}, True, ["out"]),
    "hbsgs_id": Row("hbsgs", {"rotations": 2, "giants": 2, "identity": 1}, False, {"IP_LINTRANS_MULTI": 1, "IP_ROTSUM": 1}, True, ["out"]),
    "hsquare": Row("hsquare", {"sq_scale": 1, "sq_const": 1}, True, {"TENSOR_SQUARE": 1}, False, ["out"]),
    "hmuladd": Row("hmuladd", {"addends": 2, "ma_scale": 1, "ma_const": 1}, True, {"TENSOR_MULADD": 1}, False, ["out"]),
    "hdotadd": Row("hdotadd", {"terms": 3, "addends": 2, "da_scale": 1, "da_const": 1}, True, {"TENSOR_DOTADD": 1}, False, ["out"]),
    "hreim": Row("hreim", {}, False, {"REIM": 1}, False, ["out", "out_im"]),
    "hlintrans_rescale": Row("hlintrans", {"rotations": 3, "rescale": 1}, True, {"IP_LINTRANS": 1}, True, ["out"]),
    "hrotsum_rescale": Row("hrotsum", {"rotations": 3, "rescale": 1}, True, {"IP_ROTSUM": 1}, True, ["out"]),
    "hbsgs_rescale": Row("hbsgs", {"rotations": 2, "giants": 2, "rescale": 1}, True, {"IP_LINTRANS_MULTI": 1, "IP_ROTSUM": 1}, True, ["out"]),
}
OWN_MODUP = ("hdot", "hsquare", "hmuladd", "hdotadd", "hreim")     # one key switch of their own, hmult's or hrotate's; the others share a stored ModUp
MERGED_KINDS = sorted({k for row in ROWS.values() for k in row.merged})
# the element-wise ops and the level changes, with their constant key on: one launch or two, no key switch
ELEMENTWISE = {
    "hlincomb": Row("hlincomb", {"terms": 3, "lc_const": 1, "rescale": 1}, True, {}, False, ["out"]),
    "hclincomb": Row("hclincomb", {"terms": 3, "cl_const": 1, "rescale": 1}, True, {}, False, ["out"]),
    "hplincomb": Row("hplincomb", {"terms": 3, "pl_addend": 1, "rescale": 1}, True, {}, False, ["out"]),
    "hmlincomb": Row("hmlincomb", {"terms": 3, "outputs": 5, "ml_const": 1, "rescale": 1}, True, {}, False, [f"out{m}" for m in range(1, 6)]),
    "pmult": Row("pmult", {"rescale": 1, "fuse_pmul_rescale": 1}, True, {}, False, ["out"]),
    "hrescale": Row("hrescale", {}, True, {}, False, ["out"]),
}
MODRAISE = Row("hmodraise", {}, False, {}, False, ["out"])     # from level 1 with raise_to = 2 .. L

CFG15, CFG16 = "config_4_N15.cfg", "config_4.cfg"
A_L, A_ALPHAS = 13, (2, 3, 5, 13)
# grid A: (alpha, chain_bits) of every run; chain_bits 0 is the default chain, 60 and 36 run on the generic arithmetic back-end
A_RUNS = [(a, 0) for a in A_ALPHAS] + [(3, 60), (13, 60), (5, 36)]
B_L, B_ALPHA, B_LEVELS, B_CHAINS = 28, 28, (15, 16, 17, 28), (0, 60)
B16_ROWS, B16_LEVEL = ("hdotadd", "hlintrans_id", "hreim"), 17
BATCH, BATCH_ALPHA, BATCH_LEVELS = 3, 3, (2, 4, 7, 13)


def beta(ell, alpha):
    return -(-ell // alpha)


def unfused_levels(alpha):
    """where grid A runs fuse = False as well: the lowest level, both sides of l = alpha, the top"""
    return sorted({2, alpha, min(alpha + 1, A_L), A_L})


def points():
    """[(grid, row, cfg, logN, L, alpha, l)] of everything the sweep runs; the plan does not depend on the chain (the count backend has none)"""
    pts = []
    for name in ROWS:
        for alpha in A_ALPHAS:
            pts += [("A", name, CFG15, 15, A_L, alpha, ell) for ell in range(1, A_L + 1)]
        pts += [("B", name, CFG15, 15, B_L, B_ALPHA, ell) for ell in B_LEVELS]
    pts += [("B16", name, CFG16, 16, B_L, B_ALPHA, B16_LEVEL) for name in B16_ROWS]
    for name in ELEMENTWISE:
        pts += [("E", name, CFG15, 15, A_L, 3, ell) for ell in range(1, A_L + 1)]
    pts += [("E", "hmodraise", CFG15, 15, A_L, 3, T) for T in range(2, A_L + 1)]       # l here is raise_to; the op runs at level 1
    return pts


def row_of(name):
    return MODRAISE if name == "hmodraise" else ROWS.get(name) or ELEMENTWISE[name]


def key(pt):
    _, name, _, logN, L, alpha, ell = pt
    return f"{name} N=2^{logN} L={L} alpha={alpha} l={ell}"


def make_op(pt, backend=host.BACKEND_COUNT, fuse=True, **extra):
    """the op of one point; extra: further overrides (chain_bits, batch)"""
    _, name, cfg, logN, L, alpha, ell = pt
    row = row_of(name)
    ov = dict(row.overrides, N=1 << logN, **extra)
    if name == "hmodraise":
        return host.Op(cfg, row.op, L, 1, alpha, backend=backend, fuse=fuse, overrides=dict(ov, raise_to=ell))
    return host.Op(cfg, row.op, L, ell, alpha, backend=backend, fuse=fuse, overrides=ov)


def route(op, name):
    plan = op.plan()
    kinds = collections.Counter(ln.split()[0] for ln in plan)
    r = {"kinds": dict(sorted(kinds.items())),
         "modup_bconv": sum(ln.startswith("BCONV") and "ModUp_BCONV" in ln for ln in plan),
         "second_pass_only": sum("second_pass_only" in ln for ln in plan)}
    if name != "hrotate_hoisted":      # (its outputs are out1 .. out<R>: output_level() reads out.c0)
        r["level"] = op.output_level()
    return r


def route_of(pt):
    try:
        op = make_op(pt)
    except host.HostError as e:
        return {"rejected": str(e)}
    try:
        return route(op, pt[1])
    finally:
        op.close()


def routes():
    return {key(pt): route_of(pt) for pt in points()}


def main():
    with open(PATH, "w") as f:   # one line per point
        f.write('{"generated_by": "tests/golden/make_level_sweep_routes.py", "routes": {\n')
        f.write(",\n".join(f" {json.dumps(k)}: {json.dumps(v)}" for k, v in routes().items()))
        f.write("}}\n")


if __name__ == "__main__":
    main()
