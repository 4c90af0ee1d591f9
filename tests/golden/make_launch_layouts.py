#!/usr/bin/env python3
"""Generate tests/golden/launch_layouts.json: where every limb-poly of a call lands (launch, slot), the group size and every launch's entry
count, for the transforms (ntt_common) and the last pass x key product (hm_ntt_inner_product), computed by the loops of the commit BEFORE this
arithmetic moved into homulator_amd/csrc/hm_launch.h.  Those loops are kept verbatim in parent_launch_layouts.cpp, which this script compiles
(g++, into a temporary directory) and runs over cases().

The file keeps one SHA-256 per FAMILY of cases and policy, over the lines "<case> <layout>", so that it stays small enough to read, and the
layouts of the headline launches of one op in full.  tests/test_emu_launch_layout.py imports cases() and digest() from here, asks the
emulator build of hm_launch.h for the same layouts and asserts equality.  To find the cases of a family that moved, print the parent's lines
and compare them with lines() of the emulator's layouts:
    python tests/golden/make_launch_layouts.py --lines FAMILY POLICY
Regenerate only on purpose:
    python tests/golden/make_launch_layouts.py
"""
import ctypes as C
import hashlib
import json
import os
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
PATH = os.path.join(HERE, "launch_layouts.json")
NTT_MAX_ENTRIES = 448    # HM_NTT_MAX_ENTRIES (hm_ntt_core.h)
NIP_MAX_LIMBS = 4096     # HM_NIP_MAX_LIMBS (hm_backend.hip)
MAX_LAUNCH = 64
FULL_FAMILY = "one op"  # the family whose layouts the file keeps place by place


def cases():
    """name -> inputs.  family: the group of cases it is digested with; mods: the modulus id of every limb-poly; fused_small: the one-launch transform's limit in entries (0 = off);
    entries: the option ntt_launch_entries; coeff / inv: hm_ntt_inner_product's x_is_coeff / out_inverse per limb-poly (they decide its
    heaviest-first order)"""
    out = {}

    def add(family, name, mods, fused_small=0, entries=NTT_MAX_ENTRIES, coeff=None, inv=None):
        mods = list(mods)
        out[name] = {"family": family, "mods": mods, "fused_small": fused_small, "entries": entries,
                     "coeff": coeff if coeff is not None else [0] * len(mods), "inv": inv if inv is not None else [0] * len(mods)}

    # the headline launches, 45 / 35 / 15: one op (the limbs of the extended basis, of a level, of a digit) and a batch of 10 ops x 2 keys
    for limbs in (50, 45, 35, 15, 3):
        add("one op", f"one op, {limbs} limbs", range(limbs))
        add("one op", f"one op, {limbs} limbs, one-launch form", range(limbs), fused_small=64)
        add("batch", f"batch 10 x 2 keys, {limbs} limbs, op-major", [m for _ in range(20) for m in range(limbs)])
        add("batch", f"batch 10 x 2 keys, {limbs} limbs, limb-major", [m for m in range(limbs) for _ in range(20)])
        # the key product of one op and of a batch: the special limbs' digits all go through the transform, the others have one of their own
        heavy = [1 if m >= limbs - 15 else 0 for m in range(limbs)]
        add("one op", f"one op, {limbs} limbs, weighted", range(limbs), coeff=heavy, inv=[m % 2 for m in range(limbs)])
        add("batch", f"batch 10, {limbs} limbs, weighted", [m for _ in range(10) for m in range(limbs)], coeff=heavy * 10,
            inv=[(m + b) % 3 == 0 for b in range(10) for m in range(limbs)])
    for n in range(1, 131):
        add("one modulus", f"{n} on one modulus", [7] * n)
        add("distinct moduli", f"{n} on distinct moduli", range(n))
        add("distinct moduli", f"{n} on distinct moduli, weighted", range(n), coeff=[(i * 7) % 5 < 2 for i in range(n)], inv=[(i * 3) % 4 == 0 for i in range(n)])
    # leftovers on every modulus: G k + 1 limb-polys each
    for G in (2, 4, 8):
        for k in (1, 2, 5, 16):
            for nmod in (3, 8, 50):
                add("leftovers", f"leftovers: {nmod} moduli x ({G} x {k} + 1)", [m for m in range(nmod) for _ in range(G * k + 1)])
    # the one-launch override at and around its limit (entries rounded up to 8), also where a large G would qualify without it
    for fs in (8, 56, 64, 256, 448):
        for n in (fs - 8, fs - 7, fs - 1, fs, fs + 1):
            if n > 0:
                add("one-launch limit", f"one-launch limit {fs}: {n} distinct", range(n), fused_small=fs)
                add("one-launch limit", f"one-launch limit {fs}: {n} in eights", [i // 8 for i in range(n)], fused_small=fs)
    # the option ntt_launch_entries below and at HM_NTT_MAX_ENTRIES (and above: capped), and more groups than one launch holds for both caps
    for entries in (8, 16, 24, 100, 128, 447, NTT_MAX_ENTRIES, 1000):
        for n in (50, 100, 449, 900, 1000):
            add("ntt_launch_entries", f"ntt_launch_entries {entries}: {n} distinct", range(n), entries=entries)
            add("ntt_launch_entries", f"ntt_launch_entries {entries}: {n} in twenties", [i // 20 for i in range(n)], entries=entries)
    for n in (NIP_MAX_LIMBS, NIP_MAX_LIMBS + 1, 3 * NIP_MAX_LIMBS + 17):
        add("many groups", f"many groups: {n} distinct", range(n))
        add("many groups", f"many groups: {n} in twenties", [i // 20 for i in range(n)], coeff=[(i // 20) % 3 == 0 for i in range(n)])
        add("many groups", f"many groups: {n} in nines", [i // 9 for i in range(n)])
    for c in out.values():
        c["coeff"] = [int(bool(x)) for x in c["coeff"]]
        c["inv"] = [int(bool(x)) for x in c["inv"]]
    return out


def one_launch(case):
    """ntt_common's condition for the one-launch form, as the parent states it"""
    n = len(case["mods"])
    return bool(case["fused_small"]) and (n + 7) // 8 * 8 <= case["fused_small"]


def weights(case):
    """hm_ntt_inner_product's cost of a limb-poly with one digit and one key: 3 if its digit goes through the transform, else 1; + 2 K with out_inverse"""
    return [(3 if c else 1) + (2 if i else 0) for c, i in zip(case["coeff"], case["inv"])]


def run(fn, n, *args):
    """call a layout function that ends with (logG*, launch_of*, slot_of*, entries_of*, max_launch) -> launches"""
    u32 = C.c_uint32
    logG, launch_of, slot_of, entries_of = u32(0), (u32 * max(n, 1))(), (u32 * max(n, 1))(), (u32 * MAX_LAUNCH)()
    for i in range(n):
        launch_of[i] = slot_of[i] = 0xFFFFFFFF
    fn.restype = u32
    launches = fn(*args, C.byref(logG), launch_of, slot_of, entries_of, MAX_LAUNCH)
    assert launches <= MAX_LAUNCH
    return {"logG": logG.value, "entries": list(entries_of[:launches]), "launch": list(launch_of[:n]), "slot": list(slot_of[:n])}


def lines(layouts, family, policy):
    """one line per case of a family: its name and its layout under a policy ("ntt" / "nip")"""
    return [f"{name} {json.dumps(layouts[name][policy], separators=(',', ':'))}" for name, c in cases().items() if c["family"] == family]


def digest(layouts, family, policy):
    return hashlib.sha256("\n".join(lines(layouts, family, policy)).encode()).hexdigest()


def fixture(layouts):
    """what the file keeps of the layouts of every case: per family the number of cases and a digest per policy; the headline family in full"""
    fams = {}
    for c in cases().values():
        fams[c["family"]] = fams.get(c["family"], 0) + 1
    return {"families": {f: {"cases": k, "ntt": digest(layouts, f, "ntt"), "nip": digest(layouts, f, "nip")} for f, k in fams.items()},
            "full": {name: layouts[name] for name, c in cases().items() if c["family"] == FULL_FAMILY}}


def parent_layouts():
    with tempfile.TemporaryDirectory() as tmp:
        so = os.path.join(tmp, "parent_launch_layouts.so")
        subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-fPIC", "-shared", "-o", so, os.path.join(HERE, "parent_launch_layouts.cpp")])
        lib = C.CDLL(so)
        out = {}
        for name, c in cases().items():
            n = len(c["mods"])
            mods = (C.c_uint32 * max(n, 1))(*c["mods"])
            coeff, inv = (C.c_uint8 * max(n, 1))(*c["coeff"]), (C.c_uint8 * max(n, 1))(*c["inv"])
            out[name] = {"ntt": run(lib.parent_ntt_layout, n, C.c_uint32(c["fused_small"]), C.c_uint32(c["entries"]), mods, C.c_uint32(n)),
                         "nip": run(lib.parent_nip_layout, n, mods, C.c_uint32(n), coeff, inv)}
        return out


if __name__ == "__main__":
    layouts = parent_layouts()
    if len(sys.argv) == 4 and sys.argv[1] == "--lines":
        print("\n".join(lines(layouts, sys.argv[2], sys.argv[3])))
    else:
        fx, one = fixture(layouts), lambda v: json.dumps(v, separators=(",", ":"))
        with open(PATH, "w") as f:   # one line per family and per layout
            f.write('{"parent":"9ac0d5eb11dc9ca3493f7cd963a7eb1a923b80a5",\n"families":{\n')
            f.write(",\n".join(f"{one(k)}:{one(v)}" for k, v in fx["families"].items()))
            f.write('},\n"full":{\n')
            f.write(",\n".join(f'{one(k)}:{{"ntt":{one(v["ntt"])},\n  "nip":{one(v["nip"])}}}' for k, v in fx["full"].items()))
            f.write("}}\n")
        print(f"{len(layouts)} cases -> {PATH} ({os.path.getsize(PATH)} bytes)", file=sys.stderr)
