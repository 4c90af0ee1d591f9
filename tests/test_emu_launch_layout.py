"""The launch-layout arithmetic of the back-end's entry points (homulator_amd/csrc/hm_launch.h), compiled into the CPU emulator (no GPU):
the same-modulus grouping, the split over launches and the slot of every limb-poly are the ones recorded in tests/golden/launch_layouts.json
(a digest per family of cases and policy, the headline launches in full) from the loops of the commit before the header existed
(tests/golden/make_launch_layouts.py, parent_launch_layouts.cpp), and the alias test compares limb-polys by address."""
import ctypes as C
import importlib.util
import json
import os
import random
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
_spec = importlib.util.spec_from_file_location("make_launch_layouts", os.path.join(HERE, "golden", "make_launch_layouts.py"))
gen = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(gen)

GOLDEN = json.load(open(gen.PATH))
CASES = gen.cases()
POLICIES = ("ntt", "nip")
NONE = 0xFFFFFFFF


@pytest.fixture(scope="module")
def emu():
    subprocess.check_call(["make", "-C", os.path.join(HERE, "emu")], stdout=subprocess.DEVNULL)
    lib = C.CDLL(os.path.join(HERE, "emu", "libhm_emu.so"))
    lib.emu_first_overlap.restype = C.c_int64
    lib.emu_first_overlap.argtypes = [C.c_uint64, C.c_void_p, C.c_uint32, C.c_uint64, C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p]
    return lib


def layout(emu, policy, case):
    """the emulator's layout of a case, in the generator's form"""
    n = len(case["mods"])
    mods = (C.c_uint32 * max(n, 1))(*case["mods"])
    if policy == "ntt":
        args = (C.c_int(0), C.c_int(gen.one_launch(case)), C.c_uint32(min(gen.NTT_MAX_ENTRIES, case["entries"])), mods, C.c_uint32(n), None)
    else:
        args = (C.c_int(1), C.c_int(0), C.c_uint32(gen.NIP_MAX_LIMBS), mods, C.c_uint32(n), (C.c_uint32 * max(n, 1))(*gen.weights(case)))
    return gen.run(emu.emu_launch_layout, n, *args)


@pytest.fixture(scope="module")
def layouts(emu):
    return {name: {p: layout(emu, p, case) for p in POLICIES} for name, case in CASES.items()}


def test_the_fixture_covers_the_cases_and_nothing_else(layouts):
    fams = {}
    for c in CASES.values():
        fams[c["family"]] = fams.get(c["family"], 0) + 1
    assert {f: d["cases"] for f, d in GOLDEN["families"].items()} == fams
    assert set(GOLDEN["full"]) == {name for name, c in CASES.items() if c["family"] == gen.FULL_FAMILY}
    # what the cases are there for: every group size of both policies, one launch and several, the one-launch form, the option's range
    for p in POLICIES:
        assert {la[p]["logG"] for la in layouts.values()} == {0, 1, 2, 3}
        assert any(len(la[p]["entries"]) > 1 for la in layouts.values())
    assert any(gen.one_launch(c) for c in CASES.values()) and any(c["fused_small"] and not gen.one_launch(c) for c in CASES.values())
    assert any(c["entries"] < gen.NTT_MAX_ENTRIES for c in CASES.values()) and any(c["entries"] == gen.NTT_MAX_ENTRIES for c in CASES.values())


@pytest.mark.parametrize("policy", POLICIES)
def test_layouts_are_the_recorded_ones(layouts, policy):
    moved = [f for f, d in GOLDEN["families"].items() if gen.digest(layouts, f, policy) != d[policy]]
    assert not moved, f"layouts moved in the families {moved} (make_launch_layouts.py --lines FAMILY {policy} prints the recorded side)"
    for name, want in GOLDEN["full"].items():
        assert layouts[name][policy] == want[policy], name


@pytest.mark.parametrize("policy", POLICIES)
def test_layout_properties(layouts, policy):
    """what hm_block_map needs of a layout, whatever the recorded ones say: every limb-poly in exactly one slot, a launch's entry count a multiple
    of 8 G, the members of a full group on one modulus, empty slots only in groups of leftovers (groups that mix moduli or come after one)"""
    for name, case in CASES.items():
        got = layouts[name][policy]
        G, mods, n = 1 << got["logG"], case["mods"], len(case["mods"])
        assert all(e % (8 * G) == 0 and e > 0 for e in got["entries"]), name
        if policy == "ntt":
            assert all(e <= max(8 * G, min(gen.NTT_MAX_ENTRIES, case["entries"])) for e in got["entries"]), name
        else:
            assert all(e <= gen.NIP_MAX_LIMBS for e in got["entries"]), name
        places = list(zip(got["launch"], got["slot"]))
        assert NONE not in got["launch"] and len(set(places)) == n, name
        assert all(la < len(got["entries"]) and s < got["entries"][la] for la, s in places), name
        # groups: slot = block * 8 G + which * 8 + column
        groups = {}
        for i, (la, s) in enumerate(places):
            groups.setdefault((la, s // (8 * G), s % 8), {})[s % (8 * G) // 8] = i
        assert all(sorted(g) == list(range(len(g))) for g in groups.values()), name   # members fill a group from its first place
        per_mod = {}
        for m in mods:
            per_mod[m] = per_mod.get(m, 0) + 1
        rest = sum(c % G for c in per_mod.values())
        full = [g for g in groups.values() if len(g) == G and len({mods[i] for i in g.values()}) == 1]
        leftover = [g for g in groups.values() if not (len(g) == G and len({mods[i] for i in g.values()}) == 1)]
        assert len(full) == sum(c // G for c in per_mod.values()), name          # every modulus fills as many groups as it can
        assert sum(len(g) for g in leftover) == rest and len(leftover) == -(-rest // G), name
        assert sum(1 for g in leftover if len(g) < G) <= 1, name                 # empty slots: in the last group of leftovers only


# ---- the alias test -------------------------------------------------------------------------------------------------------------------
N = 1 << 12
LB = N * 8   # bytes of a limb-poly
BASE = 1 << 40


def overlap(emu, ob, ol, ib, il, pick=None, no=None, ni=None):
    no = len(ol) if ol is not None else no
    ni = len(il) if il is not None else ni
    arr = lambda l, t=C.c_uint32: None if l is None else (t * max(len(l), 1))(*l)   # noqa: E731
    return emu.emu_first_overlap(ob, arr(ol), no, ib, arr(il), ni, N, arr(pick, C.c_uint8))


def test_overlap_equal_bases(emu):
    assert overlap(emu, BASE, [0, 1, 2], BASE, [3, 4, 5]) == -1
    assert overlap(emu, BASE, [0, 1, 2], BASE, [3, 2, 1]) == 1          # the FIRST entry that overlaps
    assert overlap(emu, BASE, [7], BASE, [7]) == 0
    assert overlap(emu, BASE, [0, 1, 2], BASE, [3, 2, 1], pick=[1, 0, 1]) == 2   # entries the filter leaves out do not count
    assert overlap(emu, BASE, [0, 1, 2], BASE, [0, 1, 2], pick=[0, 0, 0]) == -1
    assert overlap(emu, BASE, [], BASE, [0]) == -1 and overlap(emu, BASE, [0], BASE, []) == -1
    assert overlap(emu, BASE, [0xFFFF, 0], BASE, [0xFFFE, 0xFFFF]) == 1


def test_overlap_bases_offset_by_whole_limb_polys(emu):
    # in = out + 3 limb-polys: input limb l is output limb l + 3
    assert overlap(emu, BASE, [0, 1, 2], BASE + 3 * LB, [0, 1]) == -1
    assert overlap(emu, BASE, [0, 1, 5], BASE + 3 * LB, [0, 1, 2]) == 2
    assert overlap(emu, BASE, [3], BASE + 3 * LB, [0]) == 0
    # negative offsets: in = out - 2 limb-polys
    assert overlap(emu, BASE, [0, 1], BASE - 2 * LB, [0, 1]) == -1
    assert overlap(emu, BASE, [0, 1], BASE - 2 * LB, [0, 1, 2]) == 2
    assert overlap(emu, BASE, [4], BASE - 2 * LB, [6]) == 0


def test_overlap_bases_offset_by_a_fraction_touch_two(emu):
    for frac in (8, LB // 2, LB - 8):
        # input limb 0 covers bytes [frac, frac + LB): output limb-polys 0 and 1
        assert overlap(emu, BASE, [0], BASE + frac, [0]) == 0
        assert overlap(emu, BASE, [1], BASE + frac, [0]) == 0
        assert overlap(emu, BASE, [2], BASE + frac, [0]) == -1
        # negative: bytes [-frac, LB - frac): output limb-polys -1 (none) and 0
        assert overlap(emu, BASE, [0], BASE - frac, [0]) == 0
        assert overlap(emu, BASE, [1], BASE - frac, [0]) == -1
        assert overlap(emu, BASE, [0], BASE - frac, [1]) == 0
        assert overlap(emu, BASE, [1], BASE - frac, [1]) == 0
        assert overlap(emu, BASE, [2], BASE - frac, [1]) == -1
        assert overlap(emu, BASE, [5], BASE - LB - frac, [5]) == -1 and overlap(emu, BASE, [4], BASE - LB - frac, [5]) == 0


def test_overlap_disjoint_allocations(emu):
    far = BASE + (1 << 36)
    assert overlap(emu, BASE, [0, 1, 2, 0xFFFF], far, [0, 1, 2, 0xFFFF]) == -1
    assert overlap(emu, far, [0, 1, 2, 0xFFFF], BASE, [0, 1, 2, 0xFFFF]) == -1
    assert overlap(emu, BASE, [0, 1], BASE + 2 * LB, [0, 1]) == -1      # neighbours in one allocation


def test_overlap_null_limb_lists_are_the_identity(emu):
    assert overlap(emu, BASE, None, BASE, [4], no=4) == -1
    assert overlap(emu, BASE, None, BASE, [4, 3], no=4) == 1
    assert overlap(emu, BASE, [2], BASE, None, ni=4) == 2
    assert overlap(emu, BASE, None, BASE + 4 * LB, None, no=4, ni=4) == -1
    assert overlap(emu, BASE, None, BASE + 3 * LB, None, no=4, ni=4) == 0
    assert overlap(emu, BASE, None, BASE, None, no=3, ni=3, pick=[0, 0, 1]) == 2


def test_overlap_is_the_base_pointer_rule_on_equal_bases(emu):
    """what the guards did before they compared addresses: with in == out, the first picked entry whose limb number is one the call writes"""
    rnd = random.Random(20250607)
    for _ in range(2000):
        top = rnd.choice((4, 20, 300, 0xFFFF))
        ol = [rnd.randint(0, top) for _ in range(rnd.randint(0, 40))]
        il = [rnd.randint(0, top) for _ in range(rnd.randint(0, 40))]
        pick = [rnd.randint(0, 1) for _ in il] if rnd.randint(0, 1) else None
        written = set(ol)
        want = next((i for i, l in enumerate(il) if (pick is None or pick[i]) and l in written), -1)
        assert overlap(emu, BASE, ol, BASE, il, pick=pick) == want
