"""The base conversion's launch plans, input windows, block map and device table (homulator_amd/csrc/hm_bconv_plan.h, hm_bcol_block in
hm_elem_core.h), compiled into the CPU emulator (no GPU): the plans are the ones recorded in tests/golden/bconv_launch_plans.json (a digest per
family of cases, the headline calls in full) from the loops of the commit before the header existed (tests/golden/make_bconv_launch_plans.py,
parent_bconv_plans.cpp); every block of a fused launch's grid maps to its work exactly once; and a narrow digit converted through the widest
digit's kernel (zero table columns, padded inputs) gives the conversion of its own kernel and of the oracle."""
import ctypes as C
import importlib.util
import json
import os

import numpy as np
import pytest

from test_emu_kernels import Emu, p

HERE = os.path.dirname(os.path.abspath(__file__))
_spec = importlib.util.spec_from_file_location("make_bconv_launch_plans", os.path.join(HERE, "golden", "make_bconv_launch_plans.py"))
gen = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(gen)

GOLDEN = json.load(open(gen.PATH))
CASES = gen.cases()
FUSED = {n: c for n, c in CASES.items() if c["kind"] == "fused"}
ALONE = {n: c for n, c in CASES.items() if c["kind"] == "alone"}
MAX_IN, MAX_PROB, ONE_GROUP = 32, 256, 15   # HM_BCONV_MAX_IN, HM_BCONV_MAX_PROB, HM_BCOL_ONE_GROUP
u32 = C.c_uint32


@pytest.fixture(scope="module")
def lib():
    return Emu("mont32").lib


@pytest.fixture(scope="module")
def plans(lib):
    return {name: gen.run(lib, "emu_", case) for name, case in CASES.items()}


def test_the_fixture_covers_the_cases_and_nothing_else(plans):
    assert GOLDEN["parent"] == gen.PARENT
    assert {f: d["cases"] for f, d in GOLDEN["families"].items()} == gen.families()
    assert set(GOLDEN["full"]) == {name for name, c in CASES.items() if c["family"] == gen.FULL_FAMILY}
    # what the cases are there for: both output counts by launch size and by option, merged and unmerged calls, one launch and several, mix,
    # both sides of the 4096-workgroup threshold, column slices, and launches cut at HM_BCONV_MAX_PROB
    fused = [(c, plans[n]) for n, c in FUSED.items()]
    assert {(c["outs"], pl["NOUT"]) for c, pl in fused} == {(0, 1), (0, 2), (1, 1), (2, 2)}
    assert any(pl["kn"] != [d[0] for d in c["descs"]] for c, pl in fused) and any(c["merge"] and len(pl["launches"]) > 1 for c, pl in fused)
    assert {c["n_tiles"] for c, _ in fused} == {1, 2, 4, 8, 16} and {c["mix"] for c, _ in fused} == {0, 1}
    wgs = {sum(d[1] for d in c["descs"]) * c["n_tiles"] for c, _ in fused}
    assert {4096, 4097} <= wgs
    assert {len(c["descs"]) for c in ALONE.values()} >= {1, 255, 256, 257}
    assert any(row[4] == MAX_PROB for pl in (plans[n] for n in ALONE) for row in pl["launches"])


def test_plans_are_the_recorded_ones(plans):
    moved = [f for f, d in GOLDEN["families"].items() if gen.digest(plans, f) != d["digest"]]
    assert not moved, f"plans moved in the families {moved} (make_bconv_launch_plans.py --lines FAMILY prints the recorded side)"
    for name, want in GOLDEN["full"].items():
        assert plans[name] == want, name


def members_of(plan):
    """per launch, its descriptors in order"""
    out = [{} for _ in plan["launches"]]
    for i, (la, pl) in enumerate(zip(plan["launch"], plan["place"])):
        assert la < len(out) and pl not in out[la]
        out[la][pl] = i
    assert all(sorted(m) == list(range(len(m))) and m for m in out)   # every descriptor in exactly one place, no launch empty
    return [[m[k] for k in range(len(m))] for m in out]


def test_membership(plans):
    for name, case in FUSED.items():
        plan, d = plans[name], case["descs"]
        assert all(kn >= x[0] for kn, x in zip(plan["kn"], d)), name
        keys = [row[0] for row in plan["launches"]]
        assert keys == sorted(set(keys)), name   # one launch per kernel, in key order
        for mem, (key, groups, grid, log_tiles) in zip(members_of(plan), plan["launches"]):
            assert {plan["kn"][i] + 256 * d[i][2] for i in mem} == {key}, name   # one kernel width and one input form per launch
            assert mem == sorted(mem), name
            assert 1 << log_tiles == case["n_tiles"], name
            # a launch's kernel belongs to one family: no digit of up to 15 limbs in a two-group kernel
            assert all((d[i][0] <= ONE_GROUP) == (key % 256 <= ONE_GROUP) for i in mem), name
    for name, case in ALONE.items():
        plan, d = plans[name], case["descs"]
        for mem, (n_in, chunk, gx, gy, gz) in zip(members_of(plan), plan["launches"]):
            assert {d[i][0] for i in mem} == {n_in} and mem == sorted(mem) and gz == len(mem) <= MAX_PROB, name
        first = [mem[0] for mem in members_of(plan)]
        assert first == sorted(first), name   # first-appearance order


def test_every_block_of_a_fused_launch_maps_to_its_work_once(lib, plans):
    """the host's grid against the kernel's own block map (hm_bcol_block): each (conversion, tile of the range, output group with a first output below
    n_out) is reached by exactly one block; every other block takes one of the kernel's two early returns"""
    seen = set()
    for name, case in FUSED.items():
        plan, d = plans[name], case["descs"]
        for tile0 in (0, 3 * case["n_tiles"]):
            for mem, (key, groups, grid, log_tiles) in zip(members_of(plan), plan["launches"]):
                shape = (tuple(d[i][1] for i in mem), groups, grid, log_tiles, plan["NOUT"], tile0)
                if shape in seen:
                    continue
                seen.add(shape)
                assert grid >= groups * 8 * -(-len(mem) * case["n_tiles"] // 8), name
                blocks = np.zeros((grid, 3), dtype=np.uint32)
                lib.emu_bcol_blocks(u32(grid), u32(groups), u32(tile0), u32(log_tiles), p(blocks))
                pi, tile, og = blocks[:, 0].astype(np.int64), blocks[:, 1].astype(np.int64), blocks[:, 2].astype(np.int64)
                n_out = np.array([d[i][1] for i in mem] + [0], dtype=np.int64)
                returns_1 = pi >= len(mem)                                              # `if (pi >= a.n_prob) return;`
                returns_2 = ~returns_1 & (og * plan["NOUT"] >= n_out[np.minimum(pi, len(mem))])   # `if (o0 >= p.n_out) return;`
                work = ~returns_1 & ~returns_2
                assert np.all((tile[work] >= tile0) & (tile[work] < tile0 + case["n_tiles"])) and np.all(og < groups), name
                got = sorted(zip(pi[work].tolist(), tile[work].tolist(), og[work].tolist()))
                want = sorted((k, t, g) for k, i in enumerate(mem) for t in range(tile0, tile0 + case["n_tiles"]) for g in range(-(-d[i][1] // plan["NOUT"])))
                assert got == want, name
    assert len(seen) > 200


def test_the_chunks_of_a_stand_alone_launch_cover_every_output_once(plans):
    for name, case in ALONE.items():
        plan, d = plans[name], case["descs"]
        for mem, (n_in, chunk, gx, gy, gz) in zip(members_of(plan), plan["launches"]):
            max_out = max(d[i][1] for i in mem)
            assert gx == max(1, (1 << case["log_len"]) // 512) and chunk >= 1, name      # a block: 256 threads x 2 coefficients
            assert (gy - 1) * chunk < max_out <= gy * chunk, name   # block y converts outputs [y chunk, min((y + 1) chunk, n_out)): a partition of [0, n_out)
            assert gy == 1 or chunk >= 4, name                      # chunks of at least 4 outputs


def window(lib, limbs, kn, logN):
    base, limb, off = u32(0), (u32 * kn)(), (u32 * kn)()
    fits = lib.emu_bcol_window((u32 * len(limbs))(*limbs), u32(len(limbs)), u32(kn), u32(logN), C.byref(base), limb, off)
    return bool(fits), base.value, list(limb), list(off)


def test_input_window(lib):
    for logN in (15, 16):
        for limbs, kn in (([7, 3, 9, 4], 4), ([7, 3, 9, 4], 9), ([0], 1), ([0], 4), ([5, 6, 7], 15), (list(range(40, 12, -1)), 28), (list(range(17)), 28)):
            fits, base, limb, off = window(lib, limbs, kn, logN)
            assert fits and base == min(limbs)
            assert limb == limbs + [limbs[0]] * (kn - len(limbs))          # padded inputs repeat input 0
            assert off == [(x - base) << (logN + 3) for x in limb]
    # 4 GiB of limb-polys at N = 2^16: 8192 fit one descriptor, 8193 do not (at N = 2^15: 16384 | 16385)
    for logN, span in ((16, 8192), (15, 16384)):
        for lo in (0, 100):
            fits, base, limb, off = window(lib, [lo + span - 1, lo], 2, logN)
            assert fits and base == lo and off == [(span - 1) << (logN + 3), 0] and off[0] < 1 << 32
            assert not window(lib, [lo, lo + span], 2, logN)[0]
            assert not window(lib, [lo + span, lo + 1, lo], 3, logN)[0]
    assert window(lib, [3], 1, 16) == (True, 3, [3], [0])


def test_tile_range(lib):
    """a power of two of tiles, aligned, inside the limb-poly"""
    for all_tiles in (8, 16):
        ok = {(t0, n) for t0 in range(all_tiles + 2) for n in range(1, all_tiles + 2) if lib.emu_tile_range_ok(u32(t0), u32(n), u32(all_tiles))}
        assert ok == {(t0, n) for n in (1, 2, 4, 8, 16) if n <= all_tiles for t0 in range(0, all_tiles, n)}


@pytest.mark.parametrize("chain", ["mont32", "survey"])
@pytest.mark.parametrize("widths", [(15, 5), (9, 3), (28, 17)])
def test_padded_table_computes_the_same_conversion(chain, widths):
    """what the merged launch relies on: a narrow digit through the WIDEST digit's kernel width (kn > n_in: the table of hm_bconv_table_words with zero
    columns, the padded inputs re-reading input 0) gives what its own kernel width gives, and what the oracle's conversion gives.  Operands at q - 1 on
    the first coefficients; plain and packed inputs; both arithmetic builds.  Limb-polys of 2^12 coefficients (log_len) in the smallest ring the
    parameter object takes, 2^13: a conversion does not read the ring size"""
    emu = Emu(chain)
    emu.lib.emu_bconv_kn.restype = C.c_int
    emu.lib.emu_bconv_kn.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_int, C.c_uint32]
    logN, log_len, ell, K = 13, 12, sum(widths), 3
    o = emu.oracle(logN, ell, K)
    mods = np.array(o.moduli, dtype=np.uint64)
    h = emu.lib.emu_create_mods(logN, ell, K, p(mods[:ell]), p(mods[ell:]))
    assert h
    try:
        wide, narrow = max(widths), min(widths)
        in_ids = list(range(wide, wide + narrow))            # the narrow digit: the limbs behind the widest one
        out_ids = [t for t in range(ell + K) if t not in in_ids]
        full = o.fill_uniform(in_ids, 6)
        for r, m in enumerate(in_ids):
            full[r, :8] = o.moduli[m] - 1
        x = np.ascontiguousarray(full[:, :1 << log_len])
        want = o.bconv_matmul(in_ids, out_ids, full)[:, :1 << log_len]   # (coefficient by coefficient)
        ii, oi = np.array(in_ids, dtype=np.uint32), np.array(out_ids, dtype=np.uint32)
        for packed in (0, 1):
            got = {}
            for kn in (narrow, wide):
                got[kn] = np.zeros((len(out_ids), 1 << log_len), dtype=np.uint64)
                assert emu.lib.emu_bconv_kn(h, p(ii), narrow, p(oi), len(oi), kn, p(x), p(got[kn]), packed, log_len) == 0
            assert np.array_equal(got[narrow], got[wide])
            assert np.array_equal(got[wide], want)
    finally:
        emu.lib.emu_destroy(h)
