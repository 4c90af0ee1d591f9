"""hmuladd on the count backend (no GPU): out = Rescale(Relin(s ct1 ct2 + sum_t u_t ct<2+t>) + k).  The fused plan is hmult's
with the first launch swapped for ONE TENSOR_MULADD launch whatever the addend count and the two keys say, its instruction total is the unfused
plan's, fuse_muladd = 0 puts a TENSOR launch and element-wise launches in front of and between hmult's last five, the refusals name op and key, the
op chains and binds, and no plan of hmult, hsquare, hdot or hlincomb moved (tests/golden/plans_before_muladd.json)."""
import hashlib
import itertools
import json
import os
import re

import pytest

from homulator_amd import host

HERE = os.path.dirname(os.path.abspath(__file__))
FUSED = ["TENSOR_MULADD", "INTT", "NTT_IP", "INTT", "BCONV", "NTT_SUBSCALE"]
KEYS = [(0, 0), (0, 1), (1, 0), (1, 1)]
ADDENDS = [0, 1, 8]
SHAPES = [("config_4.cfg", 45, 35, 15), ("config_4_N15.cfg", 16, 10, 4)]


def build(cfg, op, L, ell, alpha, fuse=True, **ov):
    o = host.Op(cfg, op, L, ell, alpha, backend=host.BACKEND_COUNT, fuse=fuse, overrides=ov or None)
    try:
        return o.plan(), o.total_instructions(), o.launch_count(), o.stage_bytes()
    finally:
        o.close()


def n_of(line):
    return int(re.search(r" n=(\d+)", line).group(1))


def ref_of(plan):
    return sum(int(re.search(r" ref=(\d+)", ln).group(1)) for ln in plan)


def kinds_of(plan):
    return [ln.split()[0] for ln in plan]


def ov_of(A, keys):
    return {"addends": A, "ma_scale": keys[0], "ma_const": keys[1]}


def tag(A, keys):
    return f" addends={A} scale={keys[0]} const={keys[1]} "


def tail(plan):
    return [(ln.split()[0], n_of(ln)) for ln in plan[1:]]


@pytest.mark.parametrize("shape", SHAPES, ids=["45-35-15", "16-10-4"])
@pytest.mark.parametrize("A,keys", list(itertools.product(ADDENDS, KEYS)))
def test_launch_list(shape, A, keys):
    cfg, L, ell, alpha = shape
    ov = ov_of(A, keys)
    hm, hm_total, _, _ = build(cfg, "hmult", L, ell, alpha)
    p, total, n, _ = build(cfg, "hmuladd", L, ell, alpha, **ov)
    assert kinds_of(p) == FUSED and n == 6, (A, keys, p)
    assert kinds_of(hm)[0] == "TENSOR" and n_of(p[0]) == ell == n_of(hm[0]) and tag(A, keys) in p[0] + " ", p[0]
    assert tail(p) == tail(hm)                                       # every launch behind the first has hmult's kind and entry count
    p0, total0, n0, _ = build(cfg, "hmuladd", L, ell, alpha, fuse=False, **ov)
    assert total0 == total == ref_of(p) == ref_of(p0)                # fusion moves instructions, never drops them
    assert "TENSOR_MULADD" not in kinds_of(p0) and "TENSOR" not in kinds_of(p0)
    # unfused, every stage is a launch: hmult's, three for the scalar, two MUL_CONST and two ADD per addend, one for the constant
    assert n0 == build(cfg, "hmult", L, ell, alpha, fuse=False)[2] + 3 * keys[0] + 4 * A + keys[1]
    # every constant stage is one element-wise instruction group per limb
    one = (build(cfg, "hmuladd", L, ell, alpha, addends=0, ma_const=1)[1] - hm_total)
    assert one > 0 and total == hm_total + one * (3 * keys[0] + 4 * A + keys[1])
    pb = build(cfg, "hmuladd", L, ell, alpha, batch=10, **ov)[0]
    assert kinds_of(pb) == FUSED and n_of(pb[0]) == 10 * ell and tag(A, keys) in pb[0] + " "
    assert tail(pb) == tail(build(cfg, "hmult", L, ell, alpha, batch=10)[0])


@pytest.mark.parametrize("shape", SHAPES, ids=["45-35-15", "16-10-4"])
@pytest.mark.parametrize("A", range(0, 9))
def test_fuse_muladd_off_gives_a_tensor_launch_and_element_wise_launches(shape, A):
    """without addends the scalar's three stages share one launch and the constant has its own, in front of hmult's last five
    (hsquare's plan); with addends the MUL_CONST stages of scalar and addends share one launch, every addend's two ADDs one, the constant its own,
    and the rescale's work on d0 and d1 leaves hmult's merged launches as the sums arrive later than the key switch needs them: its inverse
    transforms from two links on (A + k >= 2), its conversions from three addends on"""
    cfg, L, ell, alpha = shape
    for keys in KEYS:
        s, k = keys
        p, total, n, _ = build(cfg, "hmuladd", L, ell, alpha, fuse_muladd=0, **ov_of(A, keys))
        kinds = kinds_of(p)
        assert "TENSOR_MULADD" not in kinds and kinds.count("TENSOR") == 1 and kinds[0] == "TENSOR", kinds
        assert total == ref_of(p) == build(cfg, "hmuladd", L, ell, alpha, **ov_of(A, keys))[1]
        expect = 6 + s + k if A == 0 else 6 + 1 + A + k + (A + k >= 2) + (A >= 3)
        assert n == len(p) == expect, (A, keys, kinds)
        assert kinds.count("EWE") == (s + k if A == 0 else 1 + A + k)
        assert [x for x in kinds if x != "EWE"][1:3] == ["INTT", "NTT_IP"] and kinds[-1] == "NTT_SUBSCALE"


def test_byte_model_and_constants_of_the_launch():
    """7 + 2A limb-polys per record: the four operands and both components of every addend read once, the three results written once; the
    constants ride in the records, the same for every copy of a batch"""
    ell = 35
    for A, keys, batch in ((0, (0, 0), 1), (1, (1, 1), 1), (8, (1, 1), 10), (3, (1, 0), 3), (2, (0, 1), 2)):
        o = host.Op("config_4.cfg", "hmuladd", 45, ell, 15, backend=host.BACKEND_COUNT, overrides=dict(ov_of(A, keys), batch=batch))
        line = [ln for ln in o.plan(full=True) if ln.startswith("TENSOR_MULADD")][0]
        o.close()
        assert int(re.search(r" bytes=(\d+)", line).group(1)) == (7 + 2 * A) * ell * batch * 8 * (1 << 16), (A, keys, batch)
        assert f" addends={A}" in line
        for name, on, per in (("k", keys[0], 1), ("addK", keys[1], 1), ("maK", A > 0, A), ("x0", A > 0, A), ("x1", A > 0, A)):
            m = re.search(rf" {name}=([0-9,]+)", line)
            assert bool(m) == bool(on), (name, A, keys)
            if m:
                v = m.group(1).split(",")
                assert len(v) == ell * per * batch
                if name in ("k", "addK", "maK"):
                    assert v == v[:ell * per] * batch
                else:
                    assert len(set(v)) == len(v)           # every copy its own addend limb-polys


@pytest.mark.parametrize("alpha", [2, 5])
def test_every_level_of_a_13_limb_chain(alpha):
    """whatever plan hmult has at a point, hmuladd's is that plan with the first launch swapped, and the fused total is the unfused one"""
    L = 13
    for ell in range(2, L + 1):
        hm = build("config_4_N15.cfg", "hmult", L, ell, alpha, N=1 << 13)[0]
        for A, keys in ((0, (0, 0)), (3, (1, 1))):
            p, total, n, _ = build("config_4_N15.cfg", "hmuladd", L, ell, alpha, N=1 << 13, **ov_of(A, keys))
            assert n == len(p) == len(hm) and kinds_of(p)[0] == "TENSOR_MULADD" and tag(A, keys) in p[0] + " " and tail(p) == tail(hm), (alpha, ell, A)
            p0, total0, _, _ = build("config_4_N15.cfg", "hmuladd", L, ell, alpha, fuse=False, N=1 << 13, **ov_of(A, keys))
            assert total0 == total == ref_of(p) == ref_of(p0), (alpha, ell, A)


def test_keys_outside_their_range_are_refused_by_op_and_key():
    for key in ("ma_scale", "ma_const"):
        with pytest.raises(host.HostError, match=rf"^hmuladd: {key} = 2, must be 0 or 1"):
            build("config_4_N15.cfg", "hmuladd", 16, 10, 4, **{key: 2})
    with pytest.raises(host.HostError, match=r"^hmuladd: addends = 9, must be in \[0, 8\]"):
        build("config_4_N15.cfg", "hmuladd", 16, 10, 4, addends=9)
    assert build("config_4_N15.cfg", "hmuladd", 16, 10, 4)[0][0].split()[0] == "TENSOR_MULADD"
    assert " addends=1 scale=0 const=0" in build("config_4_N15.cfg", "hmuladd", 16, 10, 4)[0][0]      # the defaults


def test_unserved_modes_are_clear_errors():
    with pytest.raises(host.HostError, match="^hmuladd:.*world"):
        host.Op("config_4_N15.cfg", "hmuladd", 16, 10, 4, backend=host.BACKEND_COUNT, world=2)
    with pytest.raises(host.HostError, match="^hmuladd:.*sim"):
        host.Op("config_4_N15.cfg", "hmuladd", 16, 10, 4, backend=host.BACKEND_SIM)
    with pytest.raises(host.HostError, match="^hmuladd: Rescale needs at least two limbs"):
        host.Op("config_4_N15.cfg", "hmuladd", 16, 1, 4, backend=host.BACKEND_COUNT)


def test_set_constants_refusals():
    from oracle.homoracle import Oracle
    ell = 10
    q = [int(x) for x in Oracle(15, 16, 4).moduli]
    mk = lambda **ov: host.Op("config_4_N15.cfg", "hmuladd", 16, ell, 4, backend=host.BACKEND_COUNT, overrides=ov or None)
    o = mk(ma_scale=1, ma_const=1, addends=2)
    o.set_constants("scale", [2] * ell)                                  # accepted: reduced, non-zero, one per limb
    o.set_constants("const", [q[j] - 1 for j in range(ell)])
    o.set_constants("const", [0] * ell)                                  # a zero constant is a constant
    o.set_constants("addscale1", [q[j] - 3 for j in range(ell)])
    o.set_constants("addscale2", [0] * ell)                              # a zero addend scalar is an addend that contributes nothing
    for name in ("scale", "addscale1", "const"):
        for n in (ell - 1, ell + 1, 0):
            with pytest.raises(host.HostError, match=rf'hmuladd: set_constants\("{name}"\): n = {n} values, the level is {ell}'):
                o.set_constants(name, [1] * n)
        with pytest.raises(host.HostError, match=rf'hmuladd: set_constants\("{name}"\): values\[3\] is not reduced'):
            o.set_constants(name, [1, 1, 1, q[3]] + [1] * (ell - 4))
    with pytest.raises(host.HostError, match=r'hmuladd: set_constants\("scale"\): values\[9\] is zero'):
        o.set_constants("scale", [1] * (ell - 1) + [0])
    for name in ("addscale3", "addscale0", "scale1", "offset"):
        with pytest.raises(host.HostError, match=rf'hmuladd: set_constants\("{name}"\): the op has no constants of that name'):
            o.set_constants(name, [0] * ell)
    line = [ln for ln in o.plan(full=True) if ln.startswith("TENSOR_MULADD")][0] + " "     # builds the plan: the accepted values are in the launch
    assert " k=" + ",".join(["2"] * ell) + " " in line and " addK=" + ",".join(["0"] * ell) + " " in line
    assert " maK=" + ",".join(f"{q[j] - 3},0" for j in range(ell)) + " " in line
    for name in ("scale", "addscale1", "const"):
        with pytest.raises(host.HostError, match=rf'hmuladd: set_constants\("{name}"\) after prepare'):
            o.set_constants(name, [1] * ell)
    o.close()
    for ov, name, key in (({"ma_scale": 1}, "const", "ma_const"), ({"ma_const": 1}, "scale", "ma_scale"), ({}, "scale", "ma_scale")):
        o = mk(**ov)
        with pytest.raises(host.HostError, match=rf'hmuladd: set_constants\("{name}"\): {key} = 0'):
            o.set_constants(name, [1] * ell)
        o.close()
    o = mk(addends=0)
    with pytest.raises(host.HostError, match=r'hmuladd: set_constants\("addscale1"\): the op has no constants of that name'):
        o.set_constants("addscale1", [1] * ell)
    o.close()


def test_the_synthetic_constants_are_the_streams_first_words():
    from oracle.homoracle import Oracle
    ell, A = 10, 3
    orc = Oracle(15, 16, 4)
    o = host.Op("config_4_N15.cfg", "hmuladd", 16, ell, 4, backend=host.BACKEND_COUNT, overrides={"ma_scale": 1, "ma_const": 1, "addends": A})
    line = [ln for ln in o.plan(full=True) if ln.startswith("TENSOR_MULADD")][0] + " "
    o.close()
    word0 = lambda stream: [int(orc.fill_uniform(range(ell), host.SEED + stream)[j][0]) for j in range(ell)]
    s, k = [v or 1 for v in word0(6400)], word0(6490)
    u = [word0(6400 + 10 * t) for t in range(1, A + 1)]
    assert " k=" + ",".join(map(str, s)) + " " in line and " addK=" + ",".join(map(str, k)) + " " in line
    assert " maK=" + ",".join(str(u[t][j]) for j in range(ell) for t in range(A)) + " " in line


def test_chains_keep_the_level_bookkeeping():
    c = host.Chain("config_4_N15.cfg", "hmuladd,hmuladd,hmult", 16, 10, 4, overrides={"backend": host.BACKEND_COUNT, "ma_scale": 1, "ma_const": 1, "addends": 2})
    assert [c[i].output_level() for i in range(3)] == [9, 8, 7]
    lines = []
    for i in range(2):
        ma = [ln for ln in c[i].plan(full=True) if ln.startswith("TENSOR_MULADD")]
        assert len(ma) == 1 and kinds_of(c[i].plan()) == FUSED
        lines.append(ma[0])
    for name, per in (("k", 1), ("maK", 2), ("addK", 1)):
        ks = [re.search(rf" {name}=([0-9,]+)", ln).group(1).split(",") for ln in lines]
        assert [len(k) for k in ks] == [10 * per, 9 * per] and ks[0][:9 * per] != ks[1]      # every link draws its own, from its own seed
    assert kinds_of(c[2].plan())[0] == "TENSOR" and n_of(c[2].plan()[0]) == 8
    c.close()
    c = host.Chain("config_4_N15.cfg", "hsquare,hmuladd,hadd", 16, 10, 4, overrides={"backend": host.BACKEND_COUNT})
    assert kinds_of(c[1].plan())[0] == "TENSOR_MULADD" and n_of(c[1].plan()[0]) == 9 and n_of(c[2].plan()[0]) == 2 * 8
    c.close()


def test_bind_input_works_for_every_input_and_refuses_a_wrong_level():
    mk = lambda op, ell, **ov: host.Op("config_4_N15.cfg", op, 16, ell, 4, backend=host.BACKEND_COUNT, overrides=ov or None)
    prods = [mk("hsquare", 10) for _ in range(4)]
    cons = mk("hmuladd", 9, addends=2)
    for i, p in enumerate(prods):
        cons.bind_input(f"ct{i + 1}", p)
    assert kinds_of(cons.plan()) == FUSED
    wrong = mk("hsquare", 9)
    other = mk("hmuladd", 9, addends=2)
    for name in ("ct1", "ct2", "ct3", "ct4"):
        with pytest.raises(host.HostError, match="levels differ"):
            other.bind_input(name, wrong)
    with pytest.raises(host.HostError):
        other.bind_input("ct5", prods[0])
    for o in [cons, other, wrong] + prods:
        o.close()


def test_buffer_names():
    o = host.Op("config_4_N15.cfg", "hmuladd", 16, 10, 4, backend=host.BACKEND_COUNT, overrides={"ma_scale": 1, "ma_const": 1, "addends": 2})
    names = set(o.buffer_names())
    o.close()
    assert {"ct1.c0", "ct1.c1", "ct2.c0", "ct2.c1", "ct3.c0", "ct4.c1", "out.c0", "out.c1", "MaD0Out", "MaD1Out", "MaD2Out", "MaD0Scale", "MaD1Scale",
            "MaD2Scale", "MaD0Const", "HMULTHaddOutput(0)", "HMULTHaddOutput(1)"} <= names
    assert "ct5.c0" not in names and "TensorD0Out" not in names
    assert {f"IP_Key{k}_{j}" for k in range(2) for j in range(3)} <= names


def test_the_other_ops_keep_their_plans():
    """plan() and plan(full=True) of hmult, hsquare (four key combinations), hdot and hlincomb, at the headline shape fused and at a small one
    unfused, are what a build of the commit before this op printed: plan() as text, plan(full=True), every field of every launch, by its SHA-256"""
    d = json.load(open(os.path.join(HERE, "golden", "plans_before_muladd.json")))
    assert {p["op"] for p in d["points"]} == {"hmult", "hsquare", "hdot", "hlincomb"} and len(d["points"]) == 16
    for p in d["points"]:
        o = host.Op(p["cfg"], p["op"], p["L"], p["l"], p["alpha"], backend=host.BACKEND_COUNT, fuse=bool(p["fuse"]), overrides=p["overrides"] or None)
        try:
            assert o.plan() == p["plan"], (p["op"], p["overrides"], p["cfg"], p["fuse"])
            assert hashlib.sha256("\n".join(o.plan(full=True)).encode()).hexdigest() == p["full_sha256"], (p["op"], p["overrides"], p["cfg"], p["fuse"])
            assert "TENSOR_MULADD" not in "".join(o.plan())
        finally:
            o.close()
