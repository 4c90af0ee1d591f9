"""hlincomb on the count backend (no GPU): out = sum_t s_t ct<t> + k.  The fused plan is ONE LINCOMB launch for both components
of all copies whatever T and lc_const say, followed with rescale = 1 by hrescale's two launches; its instruction total is the unfused plan's, whose
launches follow the stage list; the refusals name op and key, the constants go through set_constants, the op chains, and no plan of hmult, hadd,
hsquare or hdot moved (tests/golden/plans_before_lincomb.json)."""
import json
import os
import re

import pytest

from homulator_amd import host

HERE = os.path.dirname(os.path.abspath(__file__))
POINTS = [("config_4.cfg", 45, 35, 15, 16), ("config_4_N15.cfg", 16, 10, 4, 15)]


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


@pytest.mark.parametrize("cfg,L,ell,alpha,logN", POINTS)
@pytest.mark.parametrize("T", [1, 2, 4, 16])
@pytest.mark.parametrize("lc", [0, 1])
def test_the_fused_plan_is_one_launch(cfg, L, ell, alpha, logN, T, lc):
    ov = {"terms": T, "lc_const": lc}
    p, total, n, full = build(cfg, "hlincomb", L, ell, alpha, **ov)
    assert kinds_of(p) == ["LINCOMB"] and n == 1 and n_of(p[0]) == 2 * ell and f" terms={T} const={lc}" in p[0] + " ", p
    # (T + 1) limb-polys per record: every input read once, the sum written once; the constants ride in the records
    assert int(re.search(r" bytes=(\d+)", full[0]).group(1)) == (T + 1) * 2 * ell * 8 * (1 << logN)
    p0, total0, n0, _ = build(cfg, "hlincomb", L, ell, alpha, fuse=False, **ov)
    assert total0 == total == ref_of(p) == ref_of(p0)                       # fusion moves instructions, never drops them
    # unfused: one launch per stage: per component T Scale and T - 1 Add stages, and the Const stage of c0
    assert kinds_of(p0) == ["EWE"] * (2 * (2 * T - 1) + lc) and n0 == len(p0) and all(n_of(ln) == ell for ln in p0)
    # fuse_lincomb = 0: the Scale stages share a launch (no one waits for another), every Add level is one (both components), then the constant
    p1, total1, n1, _ = build(cfg, "hlincomb", L, ell, alpha, fuse_lincomb=0, **ov)
    assert shape_of(p1) == [("EWE", 2 * T * ell)] + [("EWE", 2 * ell)] * (T - 1) + [("EWE", ell)] * lc and total1 == total
    # a batch of ten: the same one launch, ten times the records, the copies under the same constants
    pb, _, nb, fb = build(cfg, "hlincomb", L, ell, alpha, batch=10, **ov)
    assert kinds_of(pb) == ["LINCOMB"] and nb == 1 and n_of(pb[0]) == 20 * ell and f" terms={T} const={lc}" in pb[0] + " "
    k = re.search(r" k=([0-9,]+)", fb[0]).group(1).split(",")
    assert len(k) == 20 * ell * T and k == k[:2 * ell * T] * 10
    m = re.search(r" addK=([0-9,]+)", fb[0])
    assert bool(m) == bool(lc)
    if m:
        v = m.group(1).split(",")
        assert len(v) == 20 * ell and v == v[:2 * ell] * 10 and v[ell:2 * ell] == ["0"] * ell      # c1 adds nothing


@pytest.mark.parametrize("cfg,L,ell,alpha,logN", POINTS)
@pytest.mark.parametrize("T,lc,batch", [(1, 0, 1), (4, 1, 1), (16, 1, 10), (2, 0, 10)])
def test_with_rescale_the_launch_is_followed_by_hrescales_launches(cfg, L, ell, alpha, logN, T, lc, batch):
    rs = build(cfg, "hrescale", L, ell, alpha, batch=batch)[0]
    p, total, n, _ = build(cfg, "hlincomb", L, ell, alpha, terms=T, lc_const=lc, rescale=1, batch=batch)
    assert len(rs) == 2 and kinds_of(p) == ["LINCOMB"] + kinds_of(rs) and n == 3
    assert n_of(p[0]) == 2 * ell * batch and shape_of(p[1:]) == shape_of(rs)
    p0, total0, _, _ = build(cfg, "hlincomb", L, ell, alpha, fuse=False, terms=T, lc_const=lc, rescale=1, batch=batch)
    rs0 = build(cfg, "hrescale", L, ell, alpha, fuse=False, batch=batch)[0]
    assert total0 == total and ref_of(p) == ref_of(p0) == total * batch     # (the total is one op's, the launches carry the batch's)
    assert kinds_of(p0) == ["EWE"] * (2 * (2 * T - 1) + lc) + kinds_of(rs0)


def test_the_synthetic_constants_are_the_streams_first_words():
    from oracle.homoracle import Oracle
    ell, T = 10, 3
    orc = Oracle(15, 16, 4)
    full = build("config_4_N15.cfg", "hlincomb", 16, ell, 4, terms=T, lc_const=1)[3]
    s = [[int(orc.fill_uniform(range(ell), host.SEED + 6200 + 100 * t)[j][0]) for j in range(ell)] for t in range(1, T + 1)]
    k = [int(orc.fill_uniform(range(ell), host.SEED + 6290)[j][0]) for j in range(ell)]
    rows = [str(s[t][j]) for j in range(ell) for t in range(T)] * 2           # [n][T] row-major, c0's records then c1's
    assert " k=" + ",".join(rows) + " " in full[0] + " "
    assert " addK=" + ",".join([str(v) for v in k] + ["0"] * ell) + " " in full[0] + " "


@pytest.mark.parametrize("terms", [0, 17, 100])
def test_terms_outside_1_16_are_refused_as_hdot_refuses_them(terms):
    with pytest.raises(host.HostError, match=rf"hlincomb: terms = {terms}, must be in \[1, 16\]"):
        build("config_4_N15.cfg", "hlincomb", 16, 10, 4, terms=terms)
    with pytest.raises(host.HostError, match=rf"hdot: terms = {terms}, must be in \[1, 16\]"):
        build("config_4_N15.cfg", "hdot", 16, 10, 4, terms=terms)


@pytest.mark.parametrize("key", ["lc_const", "rescale"])
def test_a_key_outside_0_1_is_refused_by_op_and_key(key):
    with pytest.raises(host.HostError, match=rf"hlincomb: {key} = 2, must be 0 or 1"):
        build("config_4_N15.cfg", "hlincomb", 16, 10, 4, **{key: 2})


def test_unserved_modes_are_clear_errors():
    with pytest.raises(host.HostError, match="^hlincomb:.*world"):
        host.Op("config_4_N15.cfg", "hlincomb", 16, 10, 4, backend=host.BACKEND_COUNT, world=2)
    with pytest.raises(host.HostError, match="^hlincomb:.*sim"):
        host.Op("config_4_N15.cfg", "hlincomb", 16, 10, 4, backend=host.BACKEND_SIM)
    for op in ("hlincomb", "hrescale"):     # level 1 with rescale = 1 is refused as hrescale refuses it
        with pytest.raises(host.HostError, match="Rescale needs at least two limbs"):
            host.Op("config_4_N15.cfg", op, 16, 1, 4, backend=host.BACKEND_COUNT, overrides={"rescale": 1})
    assert build("config_4_N15.cfg", "hlincomb", 16, 1, 4)[2] == 1       # without rescale, level 1 is served


def test_set_constants_round_trip_and_refusals():
    from oracle.homoracle import Oracle
    ell, T = 10, 3
    q = [int(x) for x in Oracle(15, 16, 4).moduli]
    mk = lambda **ov: host.Op("config_4_N15.cfg", "hlincomb", 16, ell, 4, backend=host.BACKEND_COUNT, overrides=dict({"terms": T}, **ov))
    o = mk(lc_const=1)
    vals = {"scale1": [2] * ell, "scale2": [0] * ell, "scale3": [q[j] - 1 for j in range(ell)], "const": [q[j] - 1 - j for j in range(ell)]}
    for name, v in vals.items():                                          # accepted: reduced, one per limb; zero is a scalar
        o.set_constants(name, v)
    for n in (ell - 1, ell + 1, 0):
        with pytest.raises(host.HostError, match=rf'hlincomb: set_constants\("scale2"\): n = {n} values, the level is {ell}'):
            o.set_constants("scale2", [1] * n)
    with pytest.raises(host.HostError, match=r'hlincomb: set_constants\("scale1"\): values\[3\] is not reduced'):
        o.set_constants("scale1", [1, 1, 1, q[3]] + [1] * (ell - 4))
    with pytest.raises(host.HostError, match=r'hlincomb: set_constants\("const"\): values\[0\] is not reduced'):
        o.set_constants("const", [q[0]] + [0] * (ell - 1))
    for name in ("scale", "scale0", "scale4", "offset"):
        with pytest.raises(host.HostError, match=rf'hlincomb: set_constants\("{name}"\): the op has no constants of that name'):
            o.set_constants(name, [0] * ell)
    line = o.plan(full=True)[0] + " "      # builds the plan: the accepted values are in the launch, for both components
    rows = [str(vals[f"scale{t}"][j]) for j in range(ell) for t in (1, 2, 3)] * 2
    assert " k=" + ",".join(rows) + " " in line
    assert " addK=" + ",".join([str(v) for v in vals["const"]] + ["0"] * ell) + " " in line
    for name in vals:
        with pytest.raises(host.HostError, match=rf'hlincomb: set_constants\("{name}"\) after prepare'):
            o.set_constants(name, [1] * ell)
    o.close()
    o = mk()
    with pytest.raises(host.HostError, match=r'hlincomb: set_constants\("const"\): lc_const = 0'):
        o.set_constants("const", [1] * ell)
    o.close()


def test_chains_keep_the_level_bookkeeping():
    """hlincomb as first, middle and last link: the level is kept, or drops by one with rescale = 1"""
    ov = {"backend": host.BACKEND_COUNT, "terms": 3, "lc_const": 1}
    c = host.Chain("config_4_N15.cfg", "hlincomb,hmult,hlincomb,hadd,hlincomb", 16, 10, 4, overrides=ov)
    assert [c[i].output_level() for i in range(5)] == [10, 9, 9, 9, 9]
    for i, lvl in ((0, 10), (2, 9), (4, 9)):
        p = c[i].plan()
        assert kinds_of(p) == ["LINCOMB"] and n_of(p[0]) == 2 * lvl and " terms=3 const=1" in p[0] + " "
    ks = [re.search(r" k=([0-9,]+)", c[i].plan(full=True)[0]).group(1).split(",") for i in (0, 2, 4)]
    assert ks[0][:6] != ks[1][:6] != ks[2][:6]                            # every link draws its own, from its own seed
    c.close()
    c = host.Chain("config_4_N15.cfg", "hlincomb,hlincomb,hmult,hlincomb", 16, 10, 4, overrides=dict(ov, rescale=1))
    assert [c[i].output_level() for i in range(4)] == [9, 8, 7, 6]
    assert kinds_of(c[3].plan())[0] == "LINCOMB" and n_of(c[3].plan()[0]) == 2 * 7
    c.close()


def test_buffer_names():
    o = host.Op("config_4_N15.cfg", "hlincomb", 16, 10, 4, backend=host.BACKEND_COUNT, overrides={"terms": 3, "lc_const": 1})
    names = set(o.buffer_names())
    o.close()
    assert {f"ct{t}.c{k}" for t in (1, 2, 3) for k in (0, 1)} | {"out.c0", "out.c1", "LinCombOutput(0)", "LinCombOutput(1)"} <= names
    assert "ct4.c0" not in names


def test_the_other_ops_keep_their_plans():
    """plan() and plan(full=True) of hmult, hadd, hsquare (four key combinations) and hdot, at the headline shape fused and at a small one unfused,
    are the text a build of the commit before this op printed"""
    d = json.load(open(os.path.join(HERE, "golden", "plans_before_lincomb.json")))
    assert {p["op"] for p in d["points"]} == {"hmult", "hadd", "hsquare", "hdot"} and len(d["points"]) == 14
    assert {(p["overrides"]["sq_scale"], p["overrides"]["sq_const"]) for p in d["points"] if p["op"] == "hsquare"} == {(0, 0), (0, 1), (1, 0), (1, 1)}
    for p in d["points"]:
        o = host.Op(p["cfg"], p["op"], p["L"], p["l"], p["alpha"], backend=host.BACKEND_COUNT, fuse=bool(p["fuse"]), overrides=p["overrides"] or None)
        try:
            assert o.plan() == p["plan"] and o.plan(full=True) == p["full"], (p["op"], p["overrides"], p["cfg"], p["fuse"])
            assert "LINCOMB" not in "".join(o.plan())
        finally:
            o.close()
