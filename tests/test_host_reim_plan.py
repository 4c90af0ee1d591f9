"""hreim on the count backend (no GPU): the real and the imaginary part of the slots with one key switch.  The fused plan is
hrotate's plan of the conjugation (galois = 2N - 1), field for field, followed by ONE REIM launch of 2 l records per copy; its instruction total is
the unfused plan's and hrotate's plus the six element-wise stages; fuse_reim = 0 keeps hrotate's launches in front of element-wise ones; the
refusals begin with the op's name, the op chains, its second output binds by name, and no plan of hrotate, hlincomb, hmult or hmuladd moved
(tests/golden/plans_before_reim.json)."""
import hashlib
import json
import os
import re

import pytest

from homulator_amd import host

HERE = os.path.dirname(os.path.abspath(__file__))
POINTS = [("config_4.cfg", 45, 35, 15, 16), ("config_4_N15.cfg", 16, 10, 4, 15)]
# hrotate with galois = 2N - 1 on the commit before this op, counted there (tests/golden/plans_before_reim.json holds the same): launches, instructions
PARENT_HROTATE = {"config_4.cfg": (5, 7328000), "config_4_N15.cfg": (5, 308736)}
HROTATE_KINDS = ["INTT", "NTT_IP", "INTT", "BCONV", "NTT_SUBSCALE"]


def build(cfg, op, L, ell, alpha, fuse=True, **ov):
    o = host.Op(cfg, op, L, ell, alpha, backend=host.BACKEND_COUNT, fuse=fuse, overrides=ov or None)
    try:
        return o.plan(), o.total_instructions(), o.launch_count(), o.plan(full=True)
    finally:
        o.close()


def n_of(line):
    return int(re.search(r" n=(\d+)", line).group(1))


def ref_of(plan):
    return sum(int(re.search(r" ref=(\d+)", ln).group(1)) for ln in plan)


LIMB_FIELDS = {"mulB", "idPt", "d1", "a", "b", "c", "d", "out", "out1", "out2", "x0", "x1", "in", "epA", "epB"}


def by_copy(full, batch):
    """plan(full=True) with every limb index of a batch copy c >= 1 written as <index in the op's own plan>+<c>.  A copy's limbs lie one op's
    limb count further on, and that count is hreim's own (it has more buffers than hrotate): read from the first launch, whose input list holds
    copy 0's limbs, then copy 1's"""
    if batch == 1:
        return full
    a = [int(v) for v in re.search(r" a=([0-9,]+)", full[0]).group(1).split(",")]
    per = a[len(a) // batch] - a[0]
    assert per > max(a[:len(a) // batch])

    def field(m):
        name, vals = m.group(1), m.group(2)
        if name not in LIMB_FIELDS:
            return m.group(0)
        return " " + name + "=" + ",".join(v if int(v) < per or int(v) >= 0xFFFFFF00 else f"{int(v) % per}+{int(v) // per}" for v in vals.split(","))
    return [re.sub(r"[ {]([A-Za-z0-9]+)=([0-9,]+)", lambda m: (m.group(0)[0] if m.group(0)[0] == "{" else "") + field(m), ln) for ln in full]


def kinds_of(plan):
    return [ln.split()[0] for ln in plan]


@pytest.mark.parametrize("cfg,L,ell,alpha,logN", POINTS)
@pytest.mark.parametrize("batch", [1, 10])
def test_the_fused_plan_is_hrotates_plus_one_launch(cfg, L, ell, alpha, logN, batch):
    g = 2 * (1 << logN) - 1
    hr, hr_total, hr_n, hr_full = build(cfg, "hrotate", L, ell, alpha, galois=g, batch=batch)
    assert (hr_n, hr_total) == PARENT_HROTATE[cfg] and kinds_of(hr) == HROTATE_KINDS
    for tag in ("auto_in=", "auto_x=", "auto_addend="):       # the conjugation rides inside hrotate's launches
        assert sum(tag in ln and f"g{g}" in ln for ln in hr) == 1, tag
    p, total, n, full = build(cfg, "hreim", L, ell, alpha, batch=batch)
    assert kinds_of(p) == HROTATE_KINDS + ["REIM"] and n == 6
    assert p[:5] == hr and by_copy(full, batch)[:5] == by_copy(hr_full, batch)    # field for field
    assert n_of(p[5]) == 2 * ell * batch
    assert int(re.search(r" bytes=(\d+)", full[5]).group(1)) == 4 * 2 * ell * batch * 8 * (1 << logN)     # two polynomials read, two written
    # the six element-wise stages, one instruction group per limb each: the same count as six stages of hrotate's final add
    hr0, hr_total0, hr_n0, _ = build(cfg, "hrotate", L, ell, alpha, fuse=False, galois=g, batch=batch)
    p0, total0, n0, _ = build(cfg, "hreim", L, ell, alpha, fuse=False, batch=batch)
    assert n0 == hr_n0 + 6 and kinds_of(p0) == kinds_of(hr0) + ["EWE"] * 6 and all(n_of(ln) == ell * batch for ln in p0[-6:])
    stage = (total0 - hr_total0) // 6
    assert total0 == hr_total0 + 6 * stage and stage > 0
    assert total == total0 and ref_of(p) == ref_of(p0) == total * batch      # fusion moves instructions, never drops them
    assert ref_of(p[5:]) == 6 * stage * batch and hr_total0 == hr_total
    # the config key galois is not read
    assert build(cfg, "hreim", L, ell, alpha, batch=batch, galois=5)[3] == full
    if batch > 1:     # the launch is replicated copy by copy: the records of copy 0, then the same limbs of every further copy
        one = build(cfg, "hreim", L, ell, alpha)[3][5]
        for name in ("a", "c", "out", "out1"):
            v0 = re.search(rf" {name}=([0-9,]+)", one).group(1).split(",")
            vb = re.search(rf" {name}=([0-9+,]+)", by_copy(full, batch)[5]).group(1).split(",")
            assert vb == v0 + [f"{x}+{c}" for c in range(1, batch) for x in v0], name


@pytest.mark.parametrize("cfg,L,ell,alpha,logN", POINTS)
@pytest.mark.parametrize("batch", [1, 10])
def test_without_the_pass_the_tail_is_elementwise(cfg, L, ell, alpha, logN, batch):
    p, total, n, full = build(cfg, "hreim", L, ell, alpha, batch=batch)
    p1, total1, n1, full1 = build(cfg, "hreim", L, ell, alpha, fuse_reim=0, batch=batch)
    assert kinds_of(p1)[:5] == HROTATE_KINDS and set(kinds_of(p1)[5:]) == {"EWE"} and n1 > n and total1 == total
    assert full1[:5] == full[:5]
    assert sum(n_of(ln) for ln in p1[5:]) == 6 * ell * batch
    assert "REIM" not in "".join(p1)


def test_the_fused_launch_does_not_read_the_stored_unit():
    o = host.Op("config_4_N15.cfg", "hreim", 16, 10, 4, backend=host.BACKEND_COUNT)
    try:
        names = set(o.buffer_names())
        line = o.plan(full=True)[5]
    finally:
        o.close()
    assert {"ct1.c0", "ct1.c1", "out.c0", "out.c1", "out_im.c0", "out_im.c1", "conj.c0", "conj.c1", "unit", "ReImOutput(0)", "ReImOutput(1)",
            "ReImDiff(0)", "ReImDiff(1)", "ReImOutputIm(0)", "ReImOutputIm(1)"} <= names and "ct2.c0" not in names
    fields = dict(f.split("=", 1) for f in line.split() if "=" in f)
    assert {k for k in ("a", "b", "c", "d", "out", "out1", "out2") if k in fields} == {"a", "c", "out", "out1"}      # no third operand
    assert all(len(fields[k].split(",")) == 20 for k in ("a", "c", "out", "out1", "mods"))
    assert fields["mods"].split(",") == [str(j) for j in range(10)] * 2


def test_unserved_modes_are_clear_errors():
    with pytest.raises(host.HostError, match="^hreim:.*world"):
        host.Op("config_4_N15.cfg", "hreim", 16, 10, 4, backend=host.BACKEND_COUNT, world=2)
    with pytest.raises(host.HostError, match="^hreim:.*sim"):
        host.Op("config_4_N15.cfg", "hreim", 16, 10, 4, backend=host.BACKEND_SIM)
    # level 1 is served: hrotate's plan at that level and the one launch
    assert build("config_4_N15.cfg", "hreim", 16, 1, 4)[2] == build("config_4_N15.cfg", "hrotate", 16, 1, 4, galois=65535)[2] + 1


def test_chains_keep_the_level_and_continue_with_the_real_part():
    ov = {"backend": host.BACKEND_COUNT, "rotations": 2, "giants": 2}
    for ops, levels in (("hbsgs,hreim", [10, 10]), ("hreim,hsquare", [10, 9]), ("hreim,hreim,hmult,hreim", [10, 10, 9, 9])):
        c = host.Chain("config_4_N15.cfg", ops, 16, 10, 4, overrides=ov)
        assert [c[i].output_level() for i in range(len(levels))] == levels, ops
        for i, name in enumerate(ops.split(",")):
            if name == "hreim":
                assert kinds_of(c[i].plan())[-1] == "REIM"
        c.close()
    c = host.Chain("config_4_N15.cfg", "hmodraise,hreim,hsquare", 16, 1, 4, overrides={"backend": host.BACKEND_COUNT})
    assert [c[i].output_level() for i in range(3)] == [16, 16, 15] and n_of(c[1].plan()[-1]) == 32
    c.close()


def test_the_second_output_binds_by_name():
    mk = lambda op, ell: host.Op("config_4_N15.cfg", op, 16, ell, 4, backend=host.BACKEND_COUNT)
    src, sq, sq2, low, plain = mk("hreim", 10), mk("hsquare", 10), mk("hsquare", 10), mk("hsquare", 9), mk("hrotate", 10)
    try:
        sq.bind_input("ct1", src, output="out_im")
        sq2.bind_input("ct1", src)                                          # the default is "out"
        with pytest.raises(host.HostError, match="HREIM has no output ciphertext out_re"):
            mk("hsquare", 10).bind_input("ct1", src, output="out_re")
        with pytest.raises(host.HostError, match="HROTATE has no output ciphertext out_im"):     # the producer's op name
            mk("hsquare", 10).bind_input("ct1", plain, output="out_im")
        with pytest.raises(host.HostError, match="levels differ"):
            low.bind_input("ct1", src, output="out_im")
        with pytest.raises(host.HostError, match="HSQUARE has no input ciphertext ct2"):
            mk("hsquare", 10).bind_input("ct2", src, output="out_im")
    finally:
        for o in (src, sq, sq2, low, plain):
            o.close()


def test_the_other_ops_keep_their_plans():
    """plan() and plan(full=True) of hrotate (galois = 5 and 2N - 1), hlincomb, hmult and hmuladd, at the headline shape fused and at a small one
    fused and unfused, are the text a build of the commit before this op printed"""
    d = json.load(open(os.path.join(HERE, "golden", "plans_before_reim.json")))
    assert {p["op"] for p in d["points"]} == {"hrotate", "hlincomb", "hmult", "hmuladd"} and len(d["points"]) == 18
    assert {p["overrides"]["galois"] for p in d["points"] if p["op"] == "hrotate"} == {5, 65535, 131071}
    for p in d["points"]:
        o = host.Op(p["cfg"], p["op"], p["L"], p["l"], p["alpha"], backend=host.BACKEND_COUNT, fuse=bool(p["fuse"]), overrides=p["overrides"] or None)
        try:
            what = (p["op"], p["overrides"], p["cfg"], p["fuse"])
            assert o.plan() == p["plan"], what
            assert hashlib.sha256("\n".join(o.plan(full=True)).encode()).hexdigest() == p["full_sha256"], what
            assert (o.launch_count(), o.total_instructions()) == (p["launches"], p["instructions"]), what
            assert "REIM" not in "".join(o.plan())
            if p["op"] == "hrotate" and p["fuse"] and p["overrides"]["galois"] != 5:
                assert (p["launches"], p["instructions"]) == PARENT_HROTATE[p["cfg"]]
        finally:
            o.close()
