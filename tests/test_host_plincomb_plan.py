"""hplincomb on the count backend (no GPU): out = (sum_t pt<t> (.) ct<t>.c0 + pt0, sum_t pt<t> (.) ct<t>.c1).  The fused plan
is ONE PLINCOMB launch of l records per copy (a record is one output limb, both components) whatever T and pl_addend say, followed with
rescale = 1 by hrescale's two launches; its instruction total is the unfused plan's, whose launches follow the stage list; the fused launch's
operand limbs are the inputs' own; the refusals name op and key; the streams of the op meet no other; the op chains, binds to hoisted rotations and
to both outputs of hreim; and no plan of pmult, hlincomb, hlintrans, hmult or hrescale moved (tests/golden/plans_before_plincomb.json)."""
import hashlib
import json
import os
import re

import pytest

from homulator_amd import hip, host

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


def fields_of(line):
    return dict(f.split("=", 1) for f in line.split() if "=" in f)


@pytest.mark.parametrize("cfg,L,ell,alpha,logN", POINTS)
@pytest.mark.parametrize("T", [1, 2, 4, 16])
@pytest.mark.parametrize("pa", [0, 1])
def test_the_fused_plan_is_one_launch(cfg, L, ell, alpha, logN, T, pa):
    ov = {"terms": T, "pl_addend": pa}
    p, total, n, full = build(cfg, "hplincomb", L, ell, alpha, **ov)
    assert kinds_of(p) == ["PLINCOMB"] and n == 1 and n_of(p[0]) == ell and f" terms={T} addend={pa}" in p[0] + " ", p
    # (3T + 2 + addend) limb-polys per record: plaintext and both components of every term read once, the addend once, two sums written
    assert int(re.search(r" bytes=(\d+)", full[0]).group(1)) == (3 * T + 2 + pa) * ell * 8 * (1 << logN)
    p0, total0, n0, _ = build(cfg, "hplincomb", L, ell, alpha, fuse=False, **ov)
    assert total0 == total == ref_of(p) == ref_of(p0)                       # fusion moves instructions, never drops them
    # unfused: one launch per stage: per component the Mul and T - 1 Mac stages, and the Addend stage of c0
    assert kinds_of(p0) == ["EWE"] * (2 * T + pa) and n0 == len(p0) and all(n_of(ln) == ell for ln in p0)
    # fuse_plincomb = 0: the two components of a term share a launch (neither waits for the other), term after term, then the addend on c0
    p1, total1, n1, _ = build(cfg, "hplincomb", L, ell, alpha, fuse_plincomb=0, **ov)
    assert shape_of(p1) == [("EWE", 2 * ell)] * T + [("EWE", ell)] * pa and total1 == total and n1 == T + pa
    assert "PLINCOMB" not in "".join(p0 + p1)
    # a batch of ten: the same one launch, ten times the records
    pb, _, nb, fb = build(cfg, "hplincomb", L, ell, alpha, batch=10, **ov)
    assert kinds_of(pb) == ["PLINCOMB"] and nb == 1 and n_of(pb[0]) == 10 * ell and f" terms={T} addend={pa}" in pb[0] + " "
    assert int(re.search(r" bytes=(\d+)", fb[0]).group(1)) == (3 * T + 2 + pa) * 10 * ell * 8 * (1 << logN)
    f = fields_of(fb[0])
    assert len(f["b"].split(",")) == len(f["x0"].split(",")) == len(f["x1"].split(",")) == 10 * ell * T
    assert len(f["out"].split(",")) == len(f["out1"].split(",")) == 10 * ell and ("d" in f) == bool(pa)
    assert len(set(f["out"].split(",") + f["out1"].split(","))) == 20 * ell      # every copy its own outputs


@pytest.mark.parametrize("cfg,L,ell,alpha,logN", POINTS)
@pytest.mark.parametrize("T,pa,batch", [(1, 0, 1), (4, 1, 1), (16, 1, 10), (2, 0, 10)])
def test_with_rescale_the_launch_is_followed_by_hrescales_launches(cfg, L, ell, alpha, logN, T, pa, batch):
    """T = 1 without the addend included: pass (4p), which folds pmult's product into the rescale's transforms, leaves this op's launch alone"""
    rs = build(cfg, "hrescale", L, ell, alpha, batch=batch)[0]
    p, total, n, _ = build(cfg, "hplincomb", L, ell, alpha, terms=T, pl_addend=pa, rescale=1, batch=batch)
    assert len(rs) == 2 and kinds_of(p) == ["PLINCOMB"] + kinds_of(rs) and n == 3
    assert n_of(p[0]) == ell * batch and shape_of(p[1:]) == shape_of(rs)
    p0, total0, _, _ = build(cfg, "hplincomb", L, ell, alpha, fuse=False, terms=T, pl_addend=pa, rescale=1, batch=batch)
    rs0 = build(cfg, "hrescale", L, ell, alpha, fuse=False, batch=batch)[0]
    assert total0 == total and ref_of(p) == ref_of(p0) == total * batch     # (the total is one op's, the launches carry the batch's)
    assert kinds_of(p0) == ["EWE"] * (2 * T + pa) + kinds_of(rs0)


@pytest.mark.parametrize("T,pa", [(1, 0), (3, 1), (16, 1)])
def test_the_fused_launch_reads_the_inputs_own_limbs(T, pa):
    ell = 10
    o = host.Op("config_4_N15.cfg", "hplincomb", 16, ell, 4, backend=host.BACKEND_COUNT, overrides={"terms": T, "pl_addend": pa})
    try:
        names = o.buffer_names()
        line = o.plan(full=True)[0]
    finally:
        o.close()
    want = [f"ct{t}.c{k}" for t in range(1, T + 1) for k in (0, 1)] + [f"pt{t}" for t in range(1, T + 1)] + (["pt0"] if pa else [])
    assert set(want) | {"out.c0", "out.c1", "PLinCombOutput(0)", "PLinCombOutput(1)"} <= set(names)
    assert f"ct{T + 1}.c0" not in names and f"pt{T + 1}" not in names and ("pt0" in names) == bool(pa) and "pt" not in names
    f = fields_of(line)
    assert {k for k in ("a", "b", "c", "d", "out", "out1", "out2", "x0", "x1") if k in f} == {"b", "x0", "x1", "out", "out1"} | ({"d"} if pa else set())
    ints = lambda k: [int(v) for v in f[k].split(",")]
    # the inputs are the op's first buffers: ct<t>.c<k> at limbs ((t - 1) * 2 + k) * l + j, then pt<t> at (2 T + t - 1) * l + j, then pt0; every
    # intermediate lies behind them
    assert ints("x0") == [(t * 2) * ell + j for j in range(ell) for t in range(T)]
    assert ints("x1") == [(t * 2 + 1) * ell + j for j in range(ell) for t in range(T)]
    assert ints("b") == [(2 * T + t) * ell + j for j in range(ell) for t in range(T)]
    if pa:
        assert ints("d") == [3 * T * ell + j for j in range(ell)]
    assert min(ints("out") + ints("out1")) >= (3 * T + pa) * ell and len(set(ints("out") + ints("out1"))) == 2 * ell
    assert f["mods"].split(",") == [str(j) for j in range(ell)]


def test_the_streams_meet_no_other_stream_of_the_op():
    """limb j of a buffer draws stream s + j: the plaintext streams 4000 + 100000 t (t = 1 .. 16, and 17 for pt0) of the largest op (T = 16, 45
    limbs) and the input streams ct<t>.c<k> = 2000 (t - 1) + 1000 k are 45 apart from each other.  (Copy c of a batch draws + 100000 c, so pt<t>
    of copy c is pt<t + c> of copy 0, as with hlintrans's plaintexts, which are numbered the same way: within ONE op no stream meets another.)"""
    used = sorted([4000 + 100000 * t for t in range(1, 18)] + [2000 * t + 1000 * k for t in range(16) for k in (0, 1)])
    assert len(used) == 17 + 32 and all(y - x >= 45 for x, y in zip(used, used[1:]))
    assert used[-1] + 45 < 1 << 32
    # ... and they are the streams the reference draws (tests/plincomb_ref.py; tests/test_gpu_plincomb.py holds the op to them bit for bit)
    from plincomb_ref import pt_stream
    assert [pt_stream(t) for t in (1, 2, 16, 0)] == [104000, 204000, 1604000, 1704000]


@pytest.mark.parametrize("terms", [0, 17, 100])
def test_terms_outside_1_16_are_refused_as_hlincomb_refuses_them(terms):
    with pytest.raises(host.HostError, match=rf"hplincomb: terms = {terms}, must be in \[1, 16\]"):
        build("config_4_N15.cfg", "hplincomb", 16, 10, 4, terms=terms)
    with pytest.raises(host.HostError, match=rf"hlincomb: terms = {terms}, must be in \[1, 16\]"):
        build("config_4_N15.cfg", "hlincomb", 16, 10, 4, terms=terms)


@pytest.mark.parametrize("key", ["pl_addend", "rescale"])
def test_a_key_outside_0_1_is_refused_by_op_and_key(key):
    with pytest.raises(host.HostError, match=rf"hplincomb: {key} = 2, must be 0 or 1"):
        build("config_4_N15.cfg", "hplincomb", 16, 10, 4, **{key: 2})


def test_unserved_modes_are_clear_errors():
    with pytest.raises(host.HostError, match="^hplincomb:.*world"):
        host.Op("config_4_N15.cfg", "hplincomb", 16, 10, 4, backend=host.BACKEND_COUNT, world=2)
    with pytest.raises(host.HostError, match="^hplincomb:.*sim"):
        host.Op("config_4_N15.cfg", "hplincomb", 16, 10, 4, backend=host.BACKEND_SIM)
    for op in ("hplincomb", "hrescale"):     # level 1 with rescale = 1 is refused as hrescale refuses it
        with pytest.raises(host.HostError, match="Rescale needs at least two limbs"):
            host.Op("config_4_N15.cfg", op, 16, 1, 4, backend=host.BACKEND_COUNT, overrides={"rescale": 1})
    assert build("config_4_N15.cfg", "hplincomb", 16, 1, 4)[2] == 1       # without rescale, level 1 is served


def test_a_plaintext_is_no_ciphertext_to_bind():
    src = host.Op("config_4_N15.cfg", "hadd", 16, 10, 4, backend=host.BACKEND_COUNT)
    o = host.Op("config_4_N15.cfg", "hplincomb", 16, 10, 4, backend=host.BACKEND_COUNT, overrides={"terms": 2, "pl_addend": 1})
    try:
        for name in ("pt1", "pt2", "pt0", "ct3"):
            with pytest.raises(host.HostError, match=f"HPLINCOMB has no input ciphertext {name}"):
                o.bind_input(name, src)
    finally:
        o.close()
        src.close()


def test_the_largest_op_fits_a_batch_of_ten():
    """limb-polys are addressed by 16-bit indices over the whole batch.  A copy of hplincomb takes 2 T l (ciphertexts) + (T + a) l (plaintexts)
    + (2 T + a) l (a buffer per stage, used or not): (5 T + 2 a) l = 2 870 at T = 16, a = 1, l = 35, so ten copies take 28 700 of 65 535; with
    rescale = 1 the two Rescale stages add their buffers and ten copies still fit"""
    def top(**ov):
        m = 0
        for ln in build("config_4.cfg", "hplincomb", 45, 35, 15, terms=16, pl_addend=1, batch=10, **ov)[3]:
            for f in re.findall(r"[ {](?:a|b|c|d|out|out1|x0|x1|in)=([\d,]+)", ln):
                m = max(m, max(int(x) for x in f.split(",") if int(x) != hip.NO_LIMB))
        return m
    assert top() == 10 * (5 * 16 + 2) * 35 - 1 == 28699
    assert top() < top(rescale=1) <= 65535


def test_chains_keep_the_level_bookkeeping():
    """hplincomb as first, middle and last link: the level is kept, or drops by one with rescale = 1"""
    ov = {"backend": host.BACKEND_COUNT, "terms": 3, "pl_addend": 1, "rotations": 2, "giants": 2}
    for ops, levels in (("hreim,hplincomb", [10, 10]), ("hplincomb,hbsgs", [10, 10]), ("hplincomb,hmult,hplincomb,hadd,hplincomb", [10, 9, 9, 9, 9])):
        c = host.Chain("config_4_N15.cfg", ops, 16, 10, 4, overrides=ov)
        assert [c[i].output_level() for i in range(len(levels))] == levels, ops
        for i, name in enumerate(ops.split(",")):
            if name == "hplincomb":
                p = c[i].plan()
                assert kinds_of(p) == ["PLINCOMB"] and n_of(p[0]) == levels[i] and " terms=3 addend=1" in p[0] + " "
        c.close()
    c = host.Chain("config_4_N15.cfg", "hplincomb,hplincomb,hmult", 16, 10, 4, overrides=dict(ov, rescale=1))
    assert [c[i].output_level() for i in range(3)] == [9, 8, 7]
    for i, lvl in ((0, 10), (1, 9)):
        assert kinds_of(c[i].plan())[0] == "PLINCOMB" and n_of(c[i].plan()[0]) == lvl and len(c[i].plan()) == 3
    c.close()


def test_it_binds_to_hoisted_rotations_and_to_both_outputs_of_hreim():
    """the inner sum of a baby-step/giant-step transform over rotations that already exist: every ct<t> bound to output t of ONE hrotate_hoisted;
    and both outputs of hreim"""
    mk = lambda op, ell, **ov: host.Op("config_4_N15.cfg", op, 16, ell, 4, backend=host.BACKEND_COUNT, overrides=ov or None)
    R = 3
    rot, reim = mk("hrotate_hoisted", 10, rotations=R), mk("hreim", 10)
    inner, both, low = mk("hplincomb", 10, terms=R, pl_addend=1), mk("hplincomb", 10, terms=2), mk("hplincomb", 9, terms=2)
    try:
        for t in range(1, R + 1):
            inner.bind_input(f"ct{t}", rot, output=f"out{t}")
        p = inner.plan()
        assert kinds_of(p) == ["PLINCOMB"] and n_of(p[0]) == 10 and f" terms={R} addend=1" in p[0] + " "
        both.bind_input("ct1", reim)                                      # the default is "out"
        both.bind_input("ct2", reim, output="out_im")
        p = both.plan()
        assert kinds_of(p) == ["PLINCOMB"] and n_of(p[0]) == 10 and " terms=2 addend=0" in p[0] + " "
        with pytest.raises(host.HostError, match="levels differ"):
            low.bind_input("ct2", reim, output="out_im")
        for t in range(1, 17):                                            # every input of the largest op binds
            o = mk("hplincomb", 10, terms=16)
            o.bind_input(f"ct{t}", reim, output="out_im" if t % 2 else "out")
            o.close()
    finally:
        for o in (inner, both, low, rot, reim):
            o.close()


def test_the_other_ops_keep_their_plans():
    """plan() and plan(full=True) of pmult (with and without rescale), hlincomb, hlintrans, hmult and hrescale, at the headline shape fused and
    at a small one fused and unfused, are the text a build of the commit before this op printed"""
    d = json.load(open(os.path.join(HERE, "golden", "plans_before_plincomb.json")))
    assert {p["op"] for p in d["points"]} == {"pmult", "hlincomb", "hlintrans", "hmult", "hrescale"} and len(d["points"]) == 21
    assert {p["overrides"]["rescale"] for p in d["points"] if p["op"] == "pmult"} == {0, 1}
    for p in d["points"]:
        o = host.Op(p["cfg"], p["op"], p["L"], p["l"], p["alpha"], backend=host.BACKEND_COUNT, fuse=bool(p["fuse"]), overrides=p["overrides"] or None)
        try:
            what = (p["op"], p["overrides"], p["cfg"], p["fuse"])
            assert o.plan() == p["plan"], what
            assert hashlib.sha256("\n".join(o.plan(full=True)).encode()).hexdigest() == p["full_sha256"], what
            assert (o.launch_count(), o.total_instructions()) == (p["launches"], p["instructions"]), what
            assert "PLINCOMB" not in "".join(o.plan())
        finally:
            o.close()
