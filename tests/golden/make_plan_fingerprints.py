#!/usr/bin/env python3
"""Generate tests/golden/plan_fingerprints.json from the launch plans of every point of GRID, on the count backend (no GPU).

A point's fingerprint is the SHA-256 of its FULL launch plan (host.Op.plan(full=True): every operand of every launch, plus the
instruction / launch / byte totals), or, where the code rejects the combination, the exception's message.  The file keeps one SHA-256 per
BUCKET of points (an op at one parameter point under every switch and batch size; one rank of a sharded plan under every plan switch) over
the lines "<point> <fingerprint>", and beside it the messages of the bucket's rejections, so that it stays small enough to read.

tests/test_host_plan_fingerprint.py imports GRID and digests() from here and asserts equality, so that a change of the planner
(Arch::fusePasses, Arch::buildLaunches) that moves one operand of one launch anywhere on the grid, or turns a rejection into a plan, fails
and names the bucket.  To find the points that moved, print them on both sides and compare:
    python tests/golden/make_plan_fingerprints.py --points GROUP
Regenerate only on purpose:
    python tests/golden/make_plan_fingerprints.py
"""
import hashlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

from homulator_amd import host  # noqa: E402
from script.sweep import SETS, min_level  # noqa: E402

PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "plan_fingerprints.json")
HEADLINE = ("config_4.cfg", 45, 35, 15)
MAX_ROT = 16   # HM_IP_HOISTED_MAX_ROT (include/homulator_hip.h): the rotations one hoisted key-product launch takes

# (op, overrides that select the op's variant)
OPS = [("hmult", {}), ("hrotate", {}), ("hrotate", {"galois": 25}), ("pmult", {}), ("hadd", {}), ("padd", {})] + \
      [("hrotate_hoisted", {"rotations": r}) for r in (2, MAX_ROT, MAX_ROT + 1)]
FUSE_KEYS_OFF = {"fuse_hpip": 0, "fuse_bconv": 0, "fuse_ip_inv": 0, "pack_bconv_in": 0, "fuse_auto": 0, "fuse_hoist": 0}
# one switch at a time against the default, and all of them off ("fuse" is the constructor's argument, not an override)
SWITCHES = [{}, {"fuse": 0}] + [{k: 0} for k in FUSE_KEYS_OFF] + [{"fuse_moddown": 1}, {"fuse_bconv_max_in": 15}, {"fuse_bconv_max_in": 32},
                                                                   dict(FUSE_KEYS_OFF)]
CHAINS = [{"chain_bits": b} for b in (0, 60, 36)]   # headline point only: pass 4b does modulus arithmetic
BATCHES = [1, 4]
SET_C = ("config_4.cfg", SETS["C"]["L"], SETS["C"]["L"] // 2, SETS["C"]["alpha"])
# the ops that sum on the extended basis: (op, variants, the op's own planner switch).  Each runs fused, unfused and with its own switch off;
# hbsgs, whose halves are hlintrans's and hrotsum's passes, also with those off
SUM_OPS = [("hlintrans", [{"rotations": r} for r in (1, 4, 16)], "fuse_lintrans"),
           ("hdot", [{"terms": t} for t in (1, 4, 16)], "fuse_dot"),
           ("hrotsum", [{"rotations": g} for g in (1, 2, 16)], "fuse_rotsum"),
           ("hbsgs", [{"rotations": r, "giants": g} for r, g in ((1, 2), (4, 4), (16, 2), (3, 16))], "fuse_bsgs")]
BSGS_SWITCHES = [{"fuse_rotsum": 0}, {"fuse_lintrans": 0, "fuse_bsgs": 0}, {"fuse_hoist": 0, "fuse_lintrans": 0, "fuse_bsgs": 0}]
BSGS_TOP_BATCH = 5   # headline point only: the largest batch of hbsgs's bench shape (limb-polys are addressed by 16-bit indices)
# the fused element-wise ops (passes 5q, 5l, 5L, 5m, 5r, 5c, 5p, 5a): (op, variants, the op's own planner switch).  Each runs fused, unfused and
# with its own switch off, at EW_POINTS
_01 = (0, 1)
EW_OPS = [("hsquare", [{"sq_scale": s, "sq_const": c} for s in _01 for c in _01], "fuse_square"),
          ("hlincomb", [{"terms": t, "lc_const": c, "rescale": r} for t in (1, 4, 16) for c in _01 for r in _01], "fuse_lincomb"),
          ("hmlincomb", [{"terms": t, "outputs": m, "ml_const": c, "rescale": r}
                         for t, m in ((1, 1), (4, 4), (16, 16), (3, 5)) for c in _01 for r in _01], "fuse_mlincomb"),
          ("hmuladd", [{"addends": a, "ma_scale": s, "ma_const": c} for a in (0, 1, 8) for s in _01 for c in _01], "fuse_muladd"),
          ("hreim", [{}], "fuse_reim"),
          ("hclincomb", [{"terms": t, "cl_const": c, "rescale": r} for t in (1, 4, 16) for c in _01 for r in _01], "fuse_clincomb"),
          ("hplincomb", [{"terms": t, "pl_addend": a, "rescale": r} for t in (1, 4, 16) for a in _01 for r in _01], "fuse_plincomb"),
          ("hdotadd", [{"terms": t, "addends": a, "da_scale": s, "da_const": c}
                       for t, a in ((1, 0), (2, 1), (4, 2), (16, 8)) for s in _01 for c in _01], "fuse_dotadd")]
EW_POINTS = [HEADLINE, ("config_4_N15.cfg", 16, 10, 4), ("config_4.cfg", 8, 8, 8)]


def param_points(op):
    pts = []
    for s in SETS.values():
        for ell in (s["L"], s["L"] // 2, min_level(op)):
            pts.append((s["cfg"], s["L"], ell, s["alpha"]))
    return pts + [HEADLINE, ("config_4.cfg", 45, 20, 16), ("config_4_N15.cfg", 16, 10, 4), ("config_4.cfg", 8, 8, 8)]


def sum_points(op):
    return param_points("hmult" if op == "hdot" else "hrotate")   # hdot rescales, as hmult does


def key(pt):
    cfg, L, ell, alpha, op, ov = pt
    return " ".join([cfg, f"{L}/{ell}/{alpha}", op] + [f"{k}={v}" for k, v in ov.items()])


def grid():
    """{group name: [(cfg, L, l, alpha, op, overrides)]}: one group per test case.  Sharded plans: ranks 0, 1 and world - 1 (every rank of
    every world made the grid slower than the rest of the CPU suite together)"""
    g = {}
    for op, variant in OPS:
        name = " ".join([op] + [f"{k}={v}" for k, v in variant.items()])
        pts = []
        for cfg, L, ell, alpha in param_points(op.replace("hrotate_hoisted", "hrotate")):
            for sw in SWITCHES + (CHAINS if (cfg, L, ell, alpha) == HEADLINE else []):
                for b in BATCHES:
                    pts.append((cfg, L, ell, alpha, op, dict(variant, **sw, batch=b)))
        g[name] = pts
    for op, variants, own in SUM_OPS:
        for variant in variants:
            pts = []
            for cfg, L, ell, alpha in sum_points(op):
                for sw in [{}, {"fuse": 0}, {own: 0}] + (BSGS_SWITCHES if op == "hbsgs" else []):
                    for b in BATCHES + ([BSGS_TOP_BATCH] if op == "hbsgs" and (cfg, L, ell, alpha) == HEADLINE else []):
                        pts.append((cfg, L, ell, alpha, op, dict(variant, **sw, batch=b)))
            g[" ".join([op] + [f"{k}={v}" for k, v in variant.items()])] = pts
    for op, variants, own in EW_OPS:
        for variant in variants:
            g[" ".join([op] + [f"{k}={v}" for k, v in variant.items()])] = [
                (cfg, L, ell, alpha, op, dict(variant, **sw, batch=b))
                for cfg, L, ell, alpha in EW_POINTS for sw in ({}, {"fuse": 0}, {own: 0}) for b in BATCHES]
    for cfg, L, ell, alpha in (HEADLINE, SET_C):
        for op in ("hmult", "hrotate"):
            for world in (2, 4, 8, 16):
                g[f"sharded {cfg} {L}/{ell}/{alpha} {op} world={world}"] = [
                    (cfg, L, ell, alpha, op, {"world": world, "rank": r, "shard_plan": sp, "pipeline_digits": pd, "shard_fused": sf, "batch": b})
                    for r in sorted({0, 1, world - 1}) for sp in (1, 2) for pd in (0, 1) for sf in (0, 1) for b in BATCHES]
    return g


GRID = grid()


def fingerprint(pt):
    cfg, L, ell, alpha, op, ov = pt
    ov = dict(ov)
    fuse = bool(ov.pop("fuse", 1))
    try:
        o = host.Op(cfg, op, L, ell, alpha, backend=host.BACKEND_COUNT, fuse=fuse, overrides=ov)
    except host.HostError as e:
        return "rejected: " + str(e)
    try:
        text = "\n".join(o.plan(full=True))
        text += f"\ntotal_instructions={o.total_instructions()} launch_count={o.launch_count()} stage_bytes={o.stage_bytes()}\n"
        return hashlib.sha256(text.encode()).hexdigest()
    except host.HostError as e:
        return "rejected: " + str(e)
    finally:
        o.close()


def bucket(pt):
    cfg, L, ell, alpha, op, ov = pt
    return f"rank={ov['rank']}" if "rank" in ov else f"{cfg} {L}/{ell}/{alpha}"


def digests(group):
    """{bucket: {"points": n, "sha256": of the bucket's "<point> <fingerprint>" lines[, "rejected": the distinct messages]}} of one group"""
    lines = {}
    for p in GRID[group]:
        lines.setdefault(bucket(p), []).append((key(p), fingerprint(p)))
    out = {}
    for b, kv in lines.items():
        out[b] = {"points": len(kv), "sha256": hashlib.sha256("".join(f"{k} {v}\n" for k, v in kv).encode()).hexdigest()}
        rejected = sorted({v for _, v in kv if v.startswith("rejected: ")})
        if rejected:
            out[b]["rejected"] = rejected
    return out


def main():
    if len(sys.argv) > 2 and sys.argv[1] == "--points":
        for p in GRID[sys.argv[2]]:
            print(key(p), fingerprint(p))
        return
    with open(PATH, "w") as f:   # one line per bucket
        f.write('{"generated_by": "tests/golden/make_plan_fingerprints.py", "groups": {\n')
        f.write(",\n".join(json.dumps(name) + ": {\n" + ",\n".join(f" {json.dumps(b)}: {json.dumps(d)}" for b, d in digests(name).items()) + "}"
                           for name in GRID))
        f.write("}}\n")


if __name__ == "__main__":
    main()
