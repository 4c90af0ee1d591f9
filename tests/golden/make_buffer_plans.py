#!/usr/bin/env python3
"""Generate tests/golden/buffer_plans.json: the buffer plan of every op, on the count backend (no GPU).

Per point the fixture keeps, in order, the CLI's `Malloc <name> from <first> to <last>` lines (the address plan: AddrManage, host/include/Addr.h)
and the lines "<name> <limbs>" of Op.buffer_names() (inputs, outputs and temporaries, with each buffer's limb count).  Both are kept as one SHA-256
per point; the points of FULL (one per op) keep the lines themselves as well, so that a failure there can be read.  To read any other point, print it
on both sides of a change and compare:
    python tests/golden/make_buffer_plans.py --point "hrotate_hoisted 16/10/3 rotations=16"

The points: config_4_N15.cfg, L = 16, l = 10 at alpha = 10, 5, 4, 3 and 1 (beta = 1, 2, 3, 4 and 10: the three branches of the key product, a short
last digit at alpha = 4 and 3, and alpha = 1) for hmult, hrotate and hrotate_hoisted with 1, 2 and 16 rotations; hadd, pmult and padd at alpha = 4;
at the same five alphas hlintrans and hrotsum with 1, 2 and 16 rotations, hdot with 1 and 4 terms, hbsgs with 2 x 2 and 4 x 3 steps.
structural.json pins the Malloc lines of the five original ops against the reference at other points; this file is this project's own record and
also covers what the reference does not have (hrotate_hoisted, hlintrans, hdot, hrotsum, hbsgs).

tests/test_host_buffer_plan.py imports POINTS and record() from here and asserts equality.  Regenerate only on purpose:
    python tests/golden/make_buffer_plans.py
"""
import ctypes as C
import hashlib
import json
import os
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

from homulator_amd import host  # noqa: E402

PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "buffer_plans.json")
CLI = os.path.join(ROOT, "host", "Homulator.run")
CFG, L, ELL = "config_4_N15.cfg", 16, 10
KEY_SWITCH_OPS = [("hmult", {}), ("hrotate", {})] + [("hrotate_hoisted", {"rotations": r}) for r in (1, 2, 16)]
# the ops that sum on the extended basis (their buffers are what the GPU tests and OpChain address by name)
SUM_OPS = [("hlintrans", {"rotations": r}) for r in (1, 2, 16)] + [("hdot", {"terms": t}) for t in (1, 4)] + \
          [("hrotsum", {"rotations": g}) for g in (1, 2, 16)] + [("hbsgs", {"rotations": r, "giants": g}) for r, g in ((2, 2), (4, 3))]
ALPHAS = (10, 5, 4, 3, 1)
# (op, alpha, overrides)
POINTS = [(op, alpha, ov) for alpha in ALPHAS for op, ov in KEY_SWITCH_OPS] + [(op, 4, {}) for op in ("hadd", "pmult", "padd")] + \
         [(op, alpha, ov) for alpha in ALPHAS for op, ov in SUM_OPS]
FULL = {("hmult", 4), ("hrotate", 4), ("hrotate_hoisted", 4, 2), ("hadd", 4), ("pmult", 4), ("padd", 4),
        ("hlintrans", 4, 2), ("hdot", 4, 4), ("hrotsum", 4, 2), ("hbsgs", 4, 2, 2)}


def key(pt):
    op, alpha, ov = pt
    return " ".join([op, f"{L}/{ELL}/{alpha}"] + [f"{k}={v}" for k, v in ov.items()])


def malloc_lines(pt):
    """the CLI's Malloc lines; config keys the argv has no place for (rotations) go into a copy of the config file"""
    op, alpha, ov = pt
    with tempfile.TemporaryDirectory() as d:
        cfg = os.path.join(d, CFG)
        with open(os.path.join(ROOT, "config", CFG)) as src, open(cfg, "w") as dst:
            dst.write(src.read() + "".join(f"{k} = {v}\n" for k, v in ov.items()))
        r = subprocess.run([CLI, cfg, op, str(L), str(ELL), str(alpha)], capture_output=True, text=True, env=dict(os.environ, HOMULATOR_BACKEND="count"))
    assert r.returncode == 0 and "Completed Simulate!" in r.stdout, r.stderr[-500:]
    return [ln for ln in r.stdout.split("\n") if ln.startswith("Malloc ")]


def buffer_lines(pt):
    """"<name> <limbs>" per entry of Op.buffer_names(), in its order"""
    op, alpha, ov = pt
    o = host.Op(CFG, op, L, ELL, alpha, backend=host.BACKEND_COUNT, overrides=ov or None)
    try:
        buf = C.create_string_buffer(1 << 20)   # (Op.buffer_names() itself stops at 64 KiB: 16 rotations at beta = 10 have more)
        o._ck(o.L.hh_op_buffer_names(o.h, buf, len(buf)))
        out = []
        for name in buf.value.decode().split("\n"):
            if name:
                n = C.c_uint32()
                o._ck(o.L.hh_op_buffer_limbs(o.h, name.encode(), C.byref(n)))
                out.append(f"{name} {n.value}")
        return out
    finally:
        o.close()


def sha(lines):
    return hashlib.sha256("".join(ln + "\n" for ln in lines).encode()).hexdigest()


def record(pt, full=None):
    op, alpha, ov = pt
    m, b = malloc_lines(pt), buffer_lines(pt)
    rec = {"malloc_lines": len(m), "malloc_sha256": sha(m), "buffers": len(b), "buffers_sha256": sha(b)}
    if full is None:
        full = (op, alpha, *ov.values()) in FULL
    if full:
        rec["malloc"], rec["buffer_limbs"] = m, b
    return rec


def main():
    if len(sys.argv) > 2 and sys.argv[1] == "--point":
        pt = [p for p in POINTS if key(p) == sys.argv[2]][0]
        rec = record(pt, full=True)
        print("\n".join(rec["malloc"] + rec["buffer_limbs"]))
        return
    with open(PATH, "w") as f:
        json.dump({"generated_by": "tests/golden/make_buffer_plans.py", "points": {key(p): record(p) for p in POINTS}}, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
