"""hclincomb on the count backend (no GPU): out = sum_t (a_t + b_t X^(N/2)) ct<t> + k.  The fused plan is ONE CLINCOMB launch
for both components of all copies whatever T and cl_const say, followed with rescale = 1 by hrescale's two launches; its instruction total is the
unfused plan's, whose launches follow the stage list; the fused launch reads the inputs only, not the stored monomial; the refusals name op and key,
the constants go through set_constants ("scale_im<t>" is stored negated for the stages and handed to the launch as given), the op chains and binds
to both outputs of hreim, and no plan of hlincomb, hreim, hrotate or hmult moved (tests/golden/plans_before_clincomb.json)."""
import hashlib
import json
import os
import re

import pytest

from homulator_amd import host

HERE = os.path.dirname(os.path.abspath(__file__))
POINTS = [("config_4.cfg", 45, 35, 15, 16), ("config_4_N15.cfg", 16, 10, 4, 15)]
RE_STREAM, IM_STREAM, CONST_STREAM = 6450, 8150, 9850


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


def kinds_of(plan):
    return [ln.split()[0] for ln in plan]


def shape_of(plan):
    return [(ln.split()[0], n_of(ln)) for ln in plan]


def fields_of(line):
    return dict(f.split("=", 1) for f in line.split() if "=" in f)


@pytest.mark.parametrize("cfg,L,ell,alpha,logN", POINTS)
@pytest.mark.parametrize("T", [1, 2, 4, 16])
@pytest.mark.parametrize("cl", [0, 1])
def test_the_fused_plan_is_one_launch(cfg, L, ell, alpha, logN, T, cl):
    ov = {"terms": T, "cl_const": cl}
    p, total, n, full = build(cfg, "hclincomb", L, ell, alpha, **ov)
    assert kinds_of(p) == ["CLINCOMB"] and n == 1 and n_of(p[0]) == 2 * ell and f" terms={T} const={cl}" in p[0] + " ", p
    # (T + 1) limb-polys per record: every input read once, the sum written once; the constants ride in the records
    assert int(re.search(r" bytes=(\d+)", full[0]).group(1)) == (T + 1) * 2 * ell * 8 * (1 << logN)
    p0, total0, n0, _ = build(cfg, "hclincomb", L, ell, alpha, fuse=False, **ov)
    assert total0 == total == ref_of(p) == ref_of(p0)                       # fusion moves instructions, never drops them
    # unfused: one launch per stage: per component and term Re, Rot, Im and Term, T - 1 Add stages, and the Const stage of c0
    assert kinds_of(p0) == ["EWE"] * (2 * (5 * T - 1) + cl) and n0 == len(p0) and all(n_of(ln) == ell for ln in p0)
    # fuse_clincomb = 0: the stages of one kind share a launch (no term waits for another), every Add level is one (both components), then the constant
    p1, total1, n1, _ = build(cfg, "hclincomb", L, ell, alpha, fuse_clincomb=0, **ov)
    assert shape_of(p1) == [("EWE", 2 * T * ell)] * 4 + [("EWE", 2 * ell)] * (T - 1) + [("EWE", ell)] * cl and total1 == total
    assert "CLINCOMB" not in "".join(p0 + p1)
    # a batch of ten: the same one launch, ten times the records, the copies under the same constants
    pb, _, nb, fb = build(cfg, "hclincomb", L, ell, alpha, batch=10, **ov)
    assert kinds_of(pb) == ["CLINCOMB"] and nb == 1 and n_of(pb[0]) == 20 * ell and f" terms={T} const={cl}" in pb[0] + " "
    for name in ("k", "maK"):
        k = re.search(rf" {name}=([0-9,]+)", fb[0]).group(1).split(",")
        assert len(k) == 20 * ell * T and k == k[:2 * ell * T] * 10, name
    m = re.search(r" addK=([0-9,]+)", fb[0])
    assert bool(m) == bool(cl)
    if m:
        v = m.group(1).split(",")
        assert len(v) == 20 * ell and v == v[:2 * ell] * 10 and v[ell:2 * ell] == ["0"] * ell      # c1 adds nothing


@pytest.mark.parametrize("cfg,L,ell,alpha,logN", POINTS)
@pytest.mark.parametrize("T,cl,batch", [(1, 0, 1), (4, 1, 1), (16, 1, 10), (2, 0, 10)])
def test_with_rescale_the_launch_is_followed_by_hrescales_launches(cfg, L, ell, alpha, logN, T, cl, batch):
    rs = build(cfg, "hrescale", L, ell, alpha, batch=batch)[0]
    p, total, n, _ = build(cfg, "hclincomb", L, ell, alpha, terms=T, cl_const=cl, rescale=1, batch=batch)
    assert len(rs) == 2 and kinds_of(p) == ["CLINCOMB"] + kinds_of(rs) and n == 3
    assert n_of(p[0]) == 2 * ell * batch and shape_of(p[1:]) == shape_of(rs)
    p0, total0, _, _ = build(cfg, "hclincomb", L, ell, alpha, fuse=False, terms=T, cl_const=cl, rescale=1, batch=batch)
    rs0 = build(cfg, "hrescale", L, ell, alpha, fuse=False, batch=batch)[0]
    assert total0 == total and ref_of(p) == ref_of(p0) == total * batch     # (the total is one op's, the launches carry the batch's)
    assert kinds_of(p0) == ["EWE"] * (2 * (5 * T - 1) + cl) + kinds_of(rs0)


@pytest.mark.parametrize("T,cl", [(1, 0), (3, 1), (16, 1)])
def test_the_fused_launch_reads_the_inputs_only(T, cl):
    ell = 10
    o = host.Op("config_4_N15.cfg", "hclincomb", 16, ell, 4, backend=host.BACKEND_COUNT, overrides={"terms": T, "cl_const": cl})
    try:
        names = set(o.buffer_names())
        line = o.plan(full=True)[0]
    finally:
        o.close()
    assert {f"ct{t}.c{k}" for t in range(1, T + 1) for k in (0, 1)} | {"out.c0", "out.c1", "unit", "CLinCombOutput(0)", "CLinCombOutput(1)"} <= names
    assert f"ct{T + 1}.c0" not in names
    f = fields_of(line)
    assert {k for k in ("a", "b", "c", "d", "out", "out1", "out2", "x0", "x1") if k in f} == {"a", "out"}      # one operand list: no factor is read
    a = [int(v) for v in f["a"].split(",")]
    # the inputs are the op's first buffers, ct<t>.c<k> at limbs ((t - 1) * 2 + k) * l + j; `unit` and every intermediate lie behind them
    assert a == [((t * 2 + k) * ell + j) for k in (0, 1) for j in range(ell) for t in range(T)]
    assert len(f["out"].split(",")) == 2 * ell and f["mods"].split(",") == [str(j) for j in range(ell)] * 2


def test_the_synthetic_constants_are_the_streams_first_words():
    from oracle.homoracle import Oracle
    ell, T = 10, 3
    orc = Oracle(15, 16, 4)
    full = build("config_4_N15.cfg", "hclincomb", 16, ell, 4, terms=T, cl_const=1)[3]
    word0 = lambda s: [int(orc.fill_uniform(range(ell), host.SEED + s)[j][0]) for j in range(ell)]
    a = [word0(RE_STREAM + 100 * t) for t in range(1, T + 1)]
    b = [word0(IM_STREAM + 100 * t) for t in range(1, T + 1)]
    for name, s in (("k", a), ("maK", b)):                                    # [n][T] row-major, c0's records then c1's; b as given, not negated
        assert f" {name}=" + ",".join([str(s[t][j]) for j in range(ell) for t in range(T)] * 2) + " " in full[0] + " ", name
    assert " addK=" + ",".join([str(v) for v in word0(CONST_STREAM)] + ["0"] * ell) + " " in full[0] + " "
    # the stages carry q - b: the stored factor is -X^(N/2)
    q = [int(x) for x in orc.moduli]
    un = build("config_4_N15.cfg", "hclincomb", 16, ell, 4, fuse=False, terms=T, cl_const=1)[3]
    im1 = [ln for ln in un if "CLinComb_Im_(1)_C0" in ln]
    assert len(im1) == 1 and " k=" + ",".join(str((q[j] - b[0][j]) % q[j]) for j in range(ell)) + " " in im1[0] + " "


def test_the_streams_meet_no_other_stream_of_the_op():
    """word 0 of stream s + j is what limb j draws: the 2 T + 1 constant streams of the largest op (T = 16, 45 limbs) are 45 apart from each other and
    from every input stream ct<t>.c<k> = seed + 2000 (t - 1) + 1000 k"""
    used = sorted([RE_STREAM + 100 * t for t in range(1, 17)] + [IM_STREAM + 100 * t for t in range(1, 17)] + [CONST_STREAM] +
                  [2000 * t + 1000 * k for t in range(16) for k in (0, 1)])
    assert all(y - x >= 45 for x, y in zip(used, used[1:]))
    assert used[-1] + 45 <= 100000          # ... and stay below the next copy of a batch


@pytest.mark.parametrize("terms", [0, 17, 100])
def test_terms_outside_1_16_are_refused_as_hlincomb_refuses_them(terms):
    with pytest.raises(host.HostError, match=rf"hclincomb: terms = {terms}, must be in \[1, 16\]"):
        build("config_4_N15.cfg", "hclincomb", 16, 10, 4, terms=terms)
    with pytest.raises(host.HostError, match=rf"hlincomb: terms = {terms}, must be in \[1, 16\]"):
        build("config_4_N15.cfg", "hlincomb", 16, 10, 4, terms=terms)


@pytest.mark.parametrize("key", ["cl_const", "rescale"])
def test_a_key_outside_0_1_is_refused_by_op_and_key(key):
    with pytest.raises(host.HostError, match=rf"hclincomb: {key} = 2, must be 0 or 1"):
        build("config_4_N15.cfg", "hclincomb", 16, 10, 4, **{key: 2})


def test_unserved_modes_are_clear_errors():
    with pytest.raises(host.HostError, match="^hclincomb:.*world"):
        host.Op("config_4_N15.cfg", "hclincomb", 16, 10, 4, backend=host.BACKEND_COUNT, world=2)
    with pytest.raises(host.HostError, match="^hclincomb:.*sim"):
        host.Op("config_4_N15.cfg", "hclincomb", 16, 10, 4, backend=host.BACKEND_SIM)
    for op in ("hclincomb", "hrescale"):     # level 1 with rescale = 1 is refused as hrescale refuses it
        with pytest.raises(host.HostError, match="Rescale needs at least two limbs"):
            host.Op("config_4_N15.cfg", op, 16, 1, 4, backend=host.BACKEND_COUNT, overrides={"rescale": 1})
    assert build("config_4_N15.cfg", "hclincomb", 16, 1, 4)[2] == 1       # without rescale, level 1 is served


def test_set_constants_round_trip_and_refusals():
    from oracle.homoracle import Oracle
    ell, T = 10, 3
    q = [int(x) for x in Oracle(15, 16, 4).moduli]
    mk = lambda **ov: host.Op("config_4_N15.cfg", "hclincomb", 16, ell, 4, backend=host.BACKEND_COUNT, overrides=dict({"terms": T}, **ov))
    o = mk(cl_const=1)
    vals = {"scale1": [2] * ell, "scale2": [0] * ell, "scale3": [q[j] - 1 for j in range(ell)],
            "scale_im1": [0] * ell, "scale_im2": [1] * ell, "scale_im3": [q[j] - 1 - j for j in range(ell)], "const": [q[j] - 1 - j for j in range(ell)]}
    for name, v in vals.items():                                          # accepted: reduced, one per limb; zero is a scalar in both parts
        o.set_constants(name, v)
    for name in ("scale2", "scale_im2"):
        for n in (ell - 1, ell + 1, 0):
            with pytest.raises(host.HostError, match=rf'hclincomb: set_constants\("{name}"\): n = {n} values, the level is {ell}'):
                o.set_constants(name, [1] * n)
    for name in ("scale1", "scale_im1"):
        with pytest.raises(host.HostError, match=rf'hclincomb: set_constants\("{name}"\): values\[3\] is not reduced'):
            o.set_constants(name, [1, 1, 1, q[3]] + [1] * (ell - 4))
    with pytest.raises(host.HostError, match=r'hclincomb: set_constants\("const"\): values\[0\] is not reduced'):
        o.set_constants("const", [q[0]] + [0] * (ell - 1))
    for name in ("scale", "scale0", "scale4", "scale_im", "scale_im0", "scale_im4", "const_im", "offset"):
        with pytest.raises(host.HostError, match=rf'hclincomb: set_constants\("{name}"\): the op has no constants of that name'):
            o.set_constants(name, [0] * ell)
    line = o.plan(full=True)[0] + " "      # builds the plan: the accepted values are in the launch, for both components, b as it was given
    for field, stem in (("k", "scale"), ("maK", "scale_im")):
        rows = [str(vals[f"{stem}{t}"][j]) for j in range(ell) for t in (1, 2, 3)] * 2
        assert f" {field}=" + ",".join(rows) + " " in line, field
    assert " addK=" + ",".join([str(v) for v in vals["const"]] + ["0"] * ell) + " " in line
    for name in vals:
        with pytest.raises(host.HostError, match=rf'hclincomb: set_constants\("{name}"\) after prepare'):
            o.set_constants(name, [1] * ell)
    o.close()
    o = mk()
    with pytest.raises(host.HostError, match=r'hclincomb: set_constants\("const"\): cl_const = 0'):
        o.set_constants("const", [1] * ell)
    o.close()
    # unfused, the monomial stage carries the negation of what was given, and 0 stays 0
    o = host.Op("config_4_N15.cfg", "hclincomb", 16, ell, 4, backend=host.BACKEND_COUNT, fuse=False, overrides={"terms": T})
    for name in ("scale_im1", "scale_im3"):
        o.set_constants(name, vals[name])
    un = o.plan(full=True)
    o.close()
    for t, name in ((1, "scale_im1"), (3, "scale_im3")):
        ln = [x for x in un if f"CLinComb_Im_({t})_C1" in x]
        assert len(ln) == 1 and " k=" + ",".join(str((q[j] - vals[name][j]) % q[j]) for j in range(ell)) + " " in ln[0] + " ", name


def test_chains_keep_the_level_bookkeeping():
    """hclincomb as first, middle and last link: the level is kept, or drops by one with rescale = 1"""
    ov = {"backend": host.BACKEND_COUNT, "terms": 3, "cl_const": 1, "rotations": 2, "giants": 2}
    for ops, levels in (("hreim,hclincomb", [10, 10]), ("hclincomb,hbsgs", [10, 10]), ("hclincomb,hmult,hclincomb,hadd,hclincomb", [10, 9, 9, 9, 9])):
        c = host.Chain("config_4_N15.cfg", ops, 16, 10, 4, overrides=ov)
        assert [c[i].output_level() for i in range(len(levels))] == levels, ops
        for i, name in enumerate(ops.split(",")):
            if name == "hclincomb":
                p = c[i].plan()
                assert kinds_of(p) == ["CLINCOMB"] and n_of(p[0]) == 2 * levels[i] and " terms=3 const=1" in p[0] + " "
        c.close()
    c = host.Chain("config_4_N15.cfg", "hclincomb,hclincomb,hmult,hclincomb", 16, 10, 4, overrides=dict(ov, rescale=1))
    assert [c[i].output_level() for i in range(4)] == [9, 8, 7, 6]
    assert kinds_of(c[3].plan())[0] == "CLINCOMB" and n_of(c[3].plan()[0]) == 2 * 7
    ks = [re.search(r" maK=([0-9,]+)", c[i].plan(full=True)[0]).group(1).split(",") for i in (0, 1, 3)]
    assert ks[0][:6] != ks[1][:6] != ks[2][:6]                            # every link draws its own, from its own seed
    c.close()


def test_it_binds_to_both_outputs_of_hreim_and_to_both_branches_behind_it():
    """the step between EvalMod and SlotToCoeff: hmodraise -> hreim -> hsquare on the real branch, a second hsquare on the imaginary one, and
    hclincomb (T = 2) takes the two back together; bound straight to hreim's two outputs it is the inverse of the split"""
    cnt = {"backend": host.BACKEND_COUNT}
    c = host.Chain("config_4_N15.cfg", "hmodraise,hreim,hsquare", 16, 1, 4, overrides=cnt)
    assert [c[i].output_level() for i in range(3)] == [16, 16, 15]
    mk = lambda op, ell, **ov: host.Op("config_4_N15.cfg", op, 16, ell, 4, backend=host.BACKEND_COUNT, overrides=ov or None)
    sq_im, join, back, low = mk("hsquare", 16), mk("hclincomb", 15, terms=2), mk("hclincomb", 16, terms=2), mk("hclincomb", 15, terms=2)
    try:
        sq_im.bind_input("ct1", c[1], output="out_im")
        join.bind_input("ct1", c[2])
        join.bind_input("ct2", sq_im)
        back.bind_input("ct1", c[1])                                      # the default is "out"
        back.bind_input("ct2", c[1], output="out_im")
        for o, lvl in ((join, 15), (back, 16)):
            p = o.plan()
            assert kinds_of(p) == ["CLINCOMB"] and n_of(p[0]) == 2 * lvl and " terms=2 const=0" in p[0] + " "
        with pytest.raises(host.HostError, match="levels differ"):
            low.bind_input("ct2", c[1], output="out_im")
        with pytest.raises(host.HostError, match="HCLINCOMB has no input ciphertext ct3"):
            mk("hclincomb", 16, terms=2).bind_input("ct3", c[1])
        for t in range(1, 17):                                            # every input of the largest op binds
            o = mk("hclincomb", 16, terms=16)
            o.bind_input(f"ct{t}", c[1], output="out_im" if t % 2 else "out")
            o.close()
    finally:
        for o in (sq_im, join, back, low):
            o.close()
        c.close()


def test_the_other_ops_keep_their_plans():
    """plan() and plan(full=True) of hlincomb (with and without the constant and the rescale), hreim, hrotate, hmult and hrescale, at the headline
    shape fused and at a small one fused and unfused, are the text a build of the commit before this op printed"""
    d = json.load(open(os.path.join(HERE, "golden", "plans_before_clincomb.json")))
    assert {p["op"] for p in d["points"]} == {"hlincomb", "hreim", "hrotate", "hmult", "hrescale"} and len(d["points"]) == 21
    assert {(p["overrides"]["lc_const"], p["overrides"]["rescale"]) for p in d["points"] if p["op"] == "hlincomb"} == {(0, 0), (1, 0), (1, 1)}
    for p in d["points"]:
        o = host.Op(p["cfg"], p["op"], p["L"], p["l"], p["alpha"], backend=host.BACKEND_COUNT, fuse=bool(p["fuse"]), overrides=p["overrides"] or None)
        try:
            what = (p["op"], p["overrides"], p["cfg"], p["fuse"])
            assert o.plan() == p["plan"], what
            assert hashlib.sha256("\n".join(o.plan(full=True)).encode()).hexdigest() == p["full_sha256"], what
            assert (o.launch_count(), o.total_instructions()) == (p["launches"], p["instructions"]), what
            assert "CLINCOMB" not in "".join(o.plan())
        finally:
            o.close()
