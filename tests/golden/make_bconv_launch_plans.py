#!/usr/bin/env python3
"""Generate tests/golden/bconv_launch_plans.json: the launches of the base conversion's two entry points — which descriptors a launch holds and in what
order, its kernel, grid and chunk / output groups, the outputs per workgroup and every descriptor's kernel width — computed by the loops of the
commit BEFORE this arithmetic moved into homulator_amd/csrc/hm_bconv_plan.h.  Those loops are kept verbatim in parent_bconv_plans.cpp, which this
script compiles (g++, into a temporary directory) and runs over cases().

The file keeps one SHA-256 per FAMILY of cases, over the lines "<case> <plan>", and the plans of the headline calls in full.
tests/test_emu_bconv_plan.py imports cases() and digest() from here, asks the emulator build of hm_bconv_plan.h for the same plans and asserts
equality.  To find the cases of a family that moved, print the parent's lines and compare them with lines() of the emulator's plans:
    python tests/golden/make_bconv_launch_plans.py --lines FAMILY
Regenerate only on purpose:
    python tests/golden/make_bconv_launch_plans.py
"""
import ctypes as C
import hashlib
import json
import os
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
PATH = os.path.join(HERE, "bconv_launch_plans.json")
PARENT = "e00f8c34375caf07d0846f6b5e49940735c6a3a9"
MAX_LAUNCH = 64
FULL_FAMILY = "headline"   # the family whose plans the file keeps in full
MERGE_WIDTHS = ((15, 5), (9, 3), (4, 4, 2), (28, 17), (20, 6))   # test_digits_of_a_small_call_merged_into_one_launch (tests/test_gpu_kernels.py)


def digits_to_descs(widths, special, packed=1):
    """one conversion per digit, to every limb of the extended basis outside the digit: (n_in, n_out, packed)"""
    ext = sum(widths) + special
    return [(w, ext - w, packed) for w in widths]


def cases():
    """name -> inputs.  kind "fused": descs (n_in, n_out, packed), n_tiles, and the options outs (bconv_col_outs), merge (bconv_col_merge), mix (the call
    has the mix prologue); kind "alone": descs (n_in, n_out), log_len and blocks (the option bconv_blocks)"""
    out = {}

    def fused(family, name, descs, n_tiles=16, outs=0, merge=1, mix=0):
        out[name] = {"kind": "fused", "family": family, "descs": [list(d) for d in descs], "n_tiles": n_tiles, "outs": outs, "merge": merge, "mix": mix}

    def alone(family, name, descs, log_len=16, blocks=3072):
        out[name] = {"kind": "alone", "family": family, "descs": [list(d) for d in descs], "log_len": log_len, "blocks": blocks}

    hmult = digits_to_descs((15, 15, 5), 15)              # hmult 45/35/15 at level 35: digits 15 / 15 / 5 into the 50-limb extended basis
    moddown = [(15, 35, 1), (15, 35, 1)]                  # the ModDown pair: 15 special limbs into the 35 of the level, once per key
    for batch, label in ((1, "one op"), (10, "batch 10")):
        fused("headline", f"hmult 45/35/15, {label}", hmult * batch)
        fused("headline", f"hmult 45/35/15, {label}, plain inputs", [(a, b, 0) for a, b, _ in hmult] * batch)
        alone("headline", f"hmult 45/35/15 ModUp, {label}, stand-alone", [d[:2] for d in hmult] * batch)
        alone("headline", f"ModDown pair, {label}, stand-alone", [d[:2] for d in moddown] * batch)
        for mix in (0, 1):
            fused("headline", f"ModDown pair, {label}, mix {mix}", [(a, b, 0) for a, b, _ in moddown] * batch, mix=mix)
    fused("headline", "hmult 45/35/15, one op, N = 2^15", hmult, n_tiles=8)
    # every option value on the small calls whose digits differ in width, whole limb-polys and column slices, both ring sizes (16 / 8 tiles)
    for widths in MERGE_WIDTHS + ((15, 15, 5), (15,), (16, 15), (15, 16), (16, 16, 15)):
        for packed, plabel in ((1, "packed"), (0, "plain"), (None, "packed and plain")):
            descs = digits_to_descs(widths, 3)
            if packed is None:
                descs = [(a, b, j % 2) for j, (a, b, _) in enumerate(descs)] + [(a, b, 1 - j % 2) for j, (a, b, _) in enumerate(descs)]
            else:
                descs = [(a, b, packed) for a, b, _ in descs]
            for n_tiles in (1, 2, 4, 8, 16):
                for outs in (0, 1, 2):
                    for merge in (0, 1):
                        for mix in ((0, 1) if max(widths) <= 15 and packed == 0 else (0,)):
                            fused("options", f"digits {widths} {plabel}, {n_tiles} tiles, outs {outs}, merge {merge}, mix {mix}", descs, n_tiles, outs, merge, mix)
    # both sides of the thresholds.  wgsAll = sum of n_out x tiles at 4096 | 4097 ...
    for n_tiles, unit in ((16, [(15, 64, 1), (5, 64, 1)] * 2), (1, [(15, 64, 1), (5, 64, 1)] * 32), (4, [(12, 64, 0), (6, 64, 0)] * 8)):
        for extra in (0, 1):   # (at 1 tile: 4096 | 4097)
            descs = unit + [(5, 1, unit[0][2])] * extra
            for outs in (0, 1, 2):
                for merge in (0, 1):
                    fused("thresholds", f"wgsAll {sum(d[1] for d in descs) * n_tiles} on {n_tiles} tiles, outs {outs}, merge {merge}", descs, n_tiles, outs, merge)
    # ... the widest digit at 4 x the narrowest and one above; the one-group family's edge (15 | 16) against narrower and wider digits
    for wide, narrow in ((12, 3), (13, 3), (8, 2), (9, 2), (4, 1), (5, 1), (32, 8), (32, 16), (28, 7), (29, 7), (15, 4), (16, 4), (15, 14), (16, 15), (17, 16), (32, 15)):
        for order in (0, 1):
            w = (wide, narrow) if order == 0 else (narrow, wide)
            for packed in (0, 1):
                fused("thresholds", f"widths {w} packed {packed}", [(a, b, packed) for a, b, _ in digits_to_descs(w, 2)])
    for a in range(1, 33):          # every pair of widths: which merge, which do not
        for b in range(1, a):
            fused("width pairs", f"widths ({a}, {b})", digits_to_descs((a, b), 1, packed=0), n_tiles=2)
    # the stand-alone form
    for n_prob in (1, 2, 255, 256, 257, 513):
        for max_out in (1, 4, 7, 8, 64):
            for log_len in (8, 12, 16):
                for blocks in (1, 3072, 100000):
                    alone("stand-alone", f"{n_prob} of width 15, {max_out} outputs, log_len {log_len}, blocks {blocks}", [(15, max_out)] * n_prob, log_len, blocks)
                    alone("stand-alone", f"{n_prob} of widths 15 | 5 | 28, up to {max_out} outputs, log_len {log_len}, blocks {blocks}",
                          [((15, 5, 28)[i % 3], 1 + (i * 7) % max_out) for i in range(n_prob)], log_len, blocks)
    return out


def run(lib, prefix, case):
    """the plan of a case from the library's <prefix>bconv_plan / <prefix>bcol_plan (the parent's loops, or the emulator build of hm_bconv_plan.h)"""
    u32 = C.c_uint32
    d = case["descs"]
    n = len(d)
    arr = lambda k, t=u32: (t * n)(*[x[k] for x in d])   # noqa: E731
    launch_of, place_of = (u32 * n)(*[0xFFFFFFFF] * n), (u32 * n)(*[0xFFFFFFFF] * n)
    if case["kind"] == "alone":
        info = (u32 * (5 * MAX_LAUNCH))()
        fn = getattr(lib, prefix + "bconv_plan")
        fn.restype = u32
        k = fn(arr(0), arr(1), u32(n), u32(case["log_len"]), u32(case["blocks"]), launch_of, place_of, info, u32(MAX_LAUNCH))
        plan, width = {}, 5
    else:
        info, nout, kn = (u32 * (4 * MAX_LAUNCH))(), u32(0), (u32 * n)()
        fn = getattr(lib, prefix + "bcol_plan")
        fn.restype = u32
        k = fn(arr(0), arr(1), arr(2, C.c_uint8), u32(n), u32(case["n_tiles"]), u32(case["outs"]), C.c_int(case["merge"]), C.c_int(case["mix"]),
               C.byref(nout), kn, launch_of, place_of, info, u32(MAX_LAUNCH))
        plan, width = {"NOUT": nout.value, "kn": list(kn)}, 4
    assert k <= MAX_LAUNCH
    plan["launches"] = [list(info[width * i:width * (i + 1)]) for i in range(k)]   # alone: n_in, chunk, grid x y z; fused: kernel key, groups, grid, logTiles
    plan["launch"], plan["place"] = list(launch_of), list(place_of)
    return plan


def lines(plans, family):
    return [f"{name} {json.dumps(plans[name], separators=(',', ':'))}" for name, c in cases().items() if c["family"] == family]


def digest(plans, family):
    return hashlib.sha256("\n".join(lines(plans, family)).encode()).hexdigest()


def families():
    fams = {}
    for c in cases().values():
        fams[c["family"]] = fams.get(c["family"], 0) + 1
    return fams


def parent_plans():
    with tempfile.TemporaryDirectory() as tmp:
        so = os.path.join(tmp, "parent_bconv_plans.so")
        subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-fPIC", "-shared", "-o", so, os.path.join(HERE, "parent_bconv_plans.cpp")])
        lib = C.CDLL(so)
        return {name: run(lib, "parent_", c) for name, c in cases().items()}


if __name__ == "__main__":
    plans = parent_plans()
    if len(sys.argv) == 3 and sys.argv[1] == "--lines":
        print("\n".join(lines(plans, sys.argv[2])))
    else:
        one = lambda v: json.dumps(v, separators=(",", ":"))   # noqa: E731
        with open(PATH, "w") as f:   # one line per family and per plan
            f.write(f'{{"parent":"{PARENT}",\n"families":{{\n')
            f.write(",\n".join(f'{one(fam)}:{{"cases":{k},"digest":"{digest(plans, fam)}"}}' for fam, k in families().items()))
            f.write('},\n"full":{\n')
            f.write(",\n".join(f"{one(name)}:{one(plans[name])}" for name, c in cases().items() if c["family"] == FULL_FAMILY))
            f.write("}}\n")
        print(f"{len(plans)} cases -> {PATH} ({os.path.getsize(PATH)} bytes)", file=sys.stderr)
