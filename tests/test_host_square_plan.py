"""hsquare on the count backend (no GPU): out = Rescale(Relin(s ct1^2) + k).  The fused plan is hmult's with the first launch
swapped for ONE TENSOR_SQUARE launch whatever the two keys say, its instruction total is the unfused plan's, fuse_square = 0 puts a TENSOR launch and
element-wise launches in front of hmult's last five, the refusals name op and key, the op chains, and no plan of hmult or hdot moved
(tests/golden/plans_before_square.json)."""
import json
import os
import re

import pytest

from homulator_amd import host

HERE = os.path.dirname(os.path.abspath(__file__))
FUSED = ["TENSOR_SQUARE", "INTT", "NTT_IP", "INTT", "BCONV", "NTT_SUBSCALE"]
KEYS = [(0, 0), (0, 1), (1, 0), (1, 1)]


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


def assert_hmult_with_the_first_launch_swapped(p, hm, n_sq, keys, what):
    """every launch behind the first has hmult's kind and entry count at the same point; the first is the one TENSOR_SQUARE"""
    assert len(p) == len(hm), (what, kinds_of(p), kinds_of(hm))
    assert kinds_of(hm)[0] == "TENSOR" and kinds_of(p)[0] == "TENSOR_SQUARE", (what, kinds_of(p))
    assert n_of(p[0]) == n_sq == n_of(hm[0]) and f" scale={keys[0]} const={keys[1]}" in p[0] + " ", (what, p[0])
    assert [(ln.split()[0], n_of(ln)) for ln in p[1:]] == [(ln.split()[0], n_of(ln)) for ln in hm[1:]], what
    assert "TENSOR" not in kinds_of(p), (what, kinds_of(p))


@pytest.mark.parametrize("keys", KEYS)
def test_launch_list_at_45_35_15(keys):
    ell = 35
    ov = {"sq_scale": keys[0], "sq_const": keys[1]}
    hm = build("config_4.cfg", "hmult", 45, ell, 15)[0]
    p, total, n, _ = build("config_4.cfg", "hsquare", 45, ell, 15, **ov)
    assert kinds_of(p) == FUSED and n == 6, (keys, p)
    assert_hmult_with_the_first_launch_swapped(p, hm, ell, keys, keys)
    p0, total0, n0, _ = build("config_4.cfg", "hsquare", 45, ell, 15, fuse=False, **ov)
    assert total0 == total == ref_of(p) == ref_of(p0) and n0 > n      # fusion moves instructions, never drops them
    assert "TENSOR_SQUARE" not in kinds_of(p0) and "TENSOR" not in kinds_of(p0)
    pb = build("config_4.cfg", "hsquare", 45, ell, 15, batch=10, **ov)[0]
    assert kinds_of(pb) == FUSED and n_of(pb[0]) == 10 * ell and f" scale={keys[0]} const={keys[1]}" in pb[0] + " "
    assert [(ln.split()[0], n_of(ln)) for ln in pb[1:]] == [(ln.split()[0], n_of(ln)) for ln in build("config_4.cfg", "hmult", 45, ell, 15, batch=10)[0][1:]]


def test_the_constants_cost_what_their_stages_cost():
    """every constant stage is one element-wise instruction group per limb: the totals of the four key combinations differ by exactly those"""
    t = {k: build("config_4.cfg", "hsquare", 45, 35, 15, sq_scale=k[0], sq_const=k[1])[1] for k in KEYS}
    one = t[(0, 1)] - t[(0, 0)]
    assert one > 0 and t[(1, 0)] - t[(0, 0)] == 3 * one and t[(1, 1)] - t[(0, 0)] == 4 * one
    assert t[(0, 0)] == build("config_4.cfg", "hmult", 45, 35, 15)[1]


def test_byte_model_of_the_launch():
    """5 limb-polys per record: the two polynomials read once, the three results written once; the constants ride in the records"""
    for keys, batch in (((0, 0), 1), ((1, 1), 1), ((1, 1), 10), ((1, 0), 3)):
        o = host.Op("config_4.cfg", "hsquare", 45, 35, 15, backend=host.BACKEND_COUNT, overrides={"sq_scale": keys[0], "sq_const": keys[1], "batch": batch})
        line = [ln for ln in o.plan(full=True) if ln.startswith("TENSOR_SQUARE")][0]
        o.close()
        assert int(re.search(r" bytes=(\d+)", line).group(1)) == 5 * 35 * batch * 8 * (1 << 16), (keys, batch)
        # one scalar and one constant per entry, the same for every copy of the batch
        for name, on in (("k", keys[0]), ("addK", keys[1])):
            m = re.search(rf" {name}=([0-9,]+)", line)
            assert bool(m) == bool(on), (name, keys)
            if m:
                v = m.group(1).split(",")
                assert len(v) == 35 * batch and v == v[:35] * batch


@pytest.mark.parametrize("keys", KEYS)
def test_fuse_square_off_gives_a_tensor_launch_and_element_wise_launches(keys):
    ov = {"sq_scale": keys[0], "sq_const": keys[1]}
    hm = build("config_4.cfg", "hmult", 45, 35, 15)[0]
    p, total, n, _ = build("config_4.cfg", "hsquare", 45, 35, 15, fuse_square=0, **ov)
    kinds = kinds_of(p)
    assert "TENSOR_SQUARE" not in kinds and kinds.count("TENSOR") == 1 and kinds[0] == "TENSOR", kinds
    assert kinds[1:-5] == ["EWE"] * (keys[0] + keys[1]), kinds                   # the three scalar stages share a launch, the constant has its own
    assert [(ln.split()[0], n_of(ln)) for ln in p[-5:]] == [(ln.split()[0], n_of(ln)) for ln in hm[-5:]]
    assert total == ref_of(p) == build("config_4.cfg", "hsquare", 45, 35, 15, **ov)[1]
    if keys[0]:
        assert n_of(p[1]) == 3 * 35


@pytest.mark.parametrize("alpha", [1, 2, 3, 5, 13])
def test_every_level_of_a_13_limb_chain(alpha):
    """the grid of tests/test_host_dot_plan.py (N = 2^13, every level a rescale can start from): whatever plan hmult has at a point, hsquare's is
    that plan with the first launch swapped, and the fused total is the unfused one"""
    L = 13
    for ell in range(2, L + 1):
        hm = build("config_4_N15.cfg", "hmult", L, ell, alpha, N=1 << 13)[0]
        for keys in ((0, 0), (1, 1)):
            ov = {"sq_scale": keys[0], "sq_const": keys[1]}
            p, total, n, _ = build("config_4_N15.cfg", "hsquare", L, ell, alpha, N=1 << 13, **ov)
            assert n == len(p)
            assert_hmult_with_the_first_launch_swapped(p, hm, ell, keys, (alpha, ell, keys))
            p0, total0, _, _ = build("config_4_N15.cfg", "hsquare", L, ell, alpha, fuse=False, N=1 << 13, **ov)
            assert total0 == total == ref_of(p) == ref_of(p0), (alpha, ell, keys)


@pytest.mark.parametrize("key", ["sq_scale", "sq_const"])
def test_a_key_outside_0_1_is_refused_by_op_and_key(key):
    with pytest.raises(host.HostError, match=rf"hsquare: {key} = 2, must be 0 or 1"):
        build("config_4_N15.cfg", "hsquare", 16, 10, 4, **{key: 2})


def test_unserved_modes_are_clear_errors():
    with pytest.raises(host.HostError, match="^hsquare:.*world"):
        host.Op("config_4_N15.cfg", "hsquare", 16, 10, 4, backend=host.BACKEND_COUNT, world=2)
    with pytest.raises(host.HostError, match="^hsquare:.*sim"):
        host.Op("config_4_N15.cfg", "hsquare", 16, 10, 4, backend=host.BACKEND_SIM)
    with pytest.raises(host.HostError, match="Rescale needs at least two limbs"):
        host.Op("config_4_N15.cfg", "hsquare", 16, 1, 4, backend=host.BACKEND_COUNT)


def test_set_constants_refusals():
    from oracle.homoracle import Oracle
    ell = 10
    q = [int(x) for x in Oracle(15, 16, 4).moduli]
    mk = lambda **ov: host.Op("config_4_N15.cfg", "hsquare", 16, ell, 4, backend=host.BACKEND_COUNT, overrides=ov or None)
    o = mk(sq_scale=1, sq_const=1)
    o.set_constants("scale", [2] * ell)                                  # accepted: reduced, non-zero, one per limb
    o.set_constants("const", [q[j] - 1 for j in range(ell)])
    o.set_constants("const", [0] * ell)                                  # a zero constant is a constant
    for n in (ell - 1, ell + 1, 0):
        with pytest.raises(host.HostError, match=rf'hsquare: set_constants\("scale"\): n = {n} values, the level is {ell}'):
            o.set_constants("scale", [1] * n)
    with pytest.raises(host.HostError, match=r'hsquare: set_constants\("scale"\): values\[3\] is not reduced'):
        o.set_constants("scale", [1, 1, 1, q[3]] + [1] * (ell - 4))
    with pytest.raises(host.HostError, match=r'hsquare: set_constants\("scale"\): values\[9\] is zero'):
        o.set_constants("scale", [1] * (ell - 1) + [0])
    with pytest.raises(host.HostError, match=r'hsquare: set_constants\("const"\): values\[0\] is not reduced'):
        o.set_constants("const", [q[0]] + [0] * (ell - 1))
    with pytest.raises(host.HostError, match=r'hsquare: set_constants\("offset"\)'):
        o.set_constants("offset", [0] * ell)
    line = [ln for ln in o.plan(full=True) if ln.startswith("TENSOR_SQUARE")][0] + " "     # builds the plan: the accepted values are in the launch
    assert " k=" + ",".join(["2"] * ell) + " " in line and " addK=" + ",".join(["0"] * ell) + " " in line
    for name in ("scale", "const"):
        with pytest.raises(host.HostError, match=rf'hsquare: set_constants\("{name}"\) after prepare'):
            o.set_constants(name, [1] * ell)
    o.close()
    for ov, name, key in (({"sq_scale": 1}, "const", "sq_const"), ({"sq_const": 1}, "scale", "sq_scale"), ({}, "scale", "sq_scale")):
        o = mk(**ov)
        with pytest.raises(host.HostError, match=rf'hsquare: set_constants\("{name}"\): {key} = 0'):
            o.set_constants(name, [1] * ell)
        o.close()
    o = host.Op("config_4_N15.cfg", "hmult", 16, ell, 4, backend=host.BACKEND_COUNT)
    with pytest.raises(host.HostError, match=r'hmult: set_constants\("scale"\)'):
        o.set_constants("scale", [1] * ell)
    o.close()


def test_the_synthetic_constants_are_the_streams_first_words():
    from oracle.homoracle import Oracle
    ell = 10
    orc = Oracle(15, 16, 4)
    o = host.Op("config_4_N15.cfg", "hsquare", 16, ell, 4, backend=host.BACKEND_COUNT, overrides={"sq_scale": 1, "sq_const": 1})
    line = [ln for ln in o.plan(full=True) if ln.startswith("TENSOR_SQUARE")][0] + " "
    o.close()
    s = [int(orc.fill_uniform(range(ell), host.SEED + 6000)[j][0]) or 1 for j in range(ell)]
    k = [int(orc.fill_uniform(range(ell), host.SEED + 6100)[j][0]) for j in range(ell)]
    assert " k=" + ",".join(map(str, s)) + " " in line and " addK=" + ",".join(map(str, k)) + " " in line


def test_chains_keep_the_level_bookkeeping():
    c = host.Chain("config_4_N15.cfg", "hmodraise,hsquare", 16, 1, 4, overrides={"backend": host.BACKEND_COUNT, "raise_to": 9, "sq_scale": 1})
    assert len(c) == 2 and c[0].output_level() == 9 and c[1].output_level() == 8
    p = c[1].plan()
    assert kinds_of(p)[0] == "TENSOR_SQUARE" and n_of(p[0]) == 9 and " scale=1 const=0" in p[0]
    c.close()
    c = host.Chain("config_4_N15.cfg", "hsquare,hsquare,hsquare", 16, 10, 4, overrides={"backend": host.BACKEND_COUNT, "sq_scale": 1, "sq_const": 1})
    assert [c[i].output_level() for i in range(3)] == [9, 8, 7]
    lines = []
    for i in range(3):
        p = c[i].plan(full=True)
        sq = [ln for ln in p if ln.startswith("TENSOR_SQUARE")]
        assert len(sq) == 1 and kinds_of(c[i].plan()) == FUSED
        lines.append(sq[0])
    ks = [re.search(r" k=([0-9,]+)", ln).group(1).split(",") for ln in lines]
    assert [len(k) for k in ks] == [10, 9, 8] and ks[0][:8] != ks[1][:8] != ks[2][:8]      # every link draws its own, from its own seed
    c.close()
    c = host.Chain("config_4_N15.cfg", "hmult,hsquare,hadd", 16, 10, 4, overrides={"backend": host.BACKEND_COUNT})
    assert kinds_of(c[1].plan())[0] == "TENSOR_SQUARE" and n_of(c[1].plan()[0]) == 9 and n_of(c[2].plan()[0]) == 2 * 8
    c.close()


def test_buffer_names():
    o = host.Op("config_4_N15.cfg", "hsquare", 16, 10, 4, backend=host.BACKEND_COUNT, overrides={"sq_scale": 1, "sq_const": 1})
    names = set(o.buffer_names())
    o.close()
    assert {"ct1.c0", "ct1.c1", "out.c0", "out.c1", "SqD0Out", "SqD1Out", "SqD2Out", "SqD0Scale", "SqD1Scale", "SqD2Scale", "SqD0Const",
            "HMULTHaddOutput(0)", "HMULTHaddOutput(1)"} <= names
    assert "ct2.c0" not in names and "TensorD0Out" not in names
    assert {f"IP_Key{k}_{j}" for k in range(2) for j in range(3)} <= names


def test_the_other_ops_keep_their_plans():
    """plan() and plan(full=True) of hmult and hdot (terms 1 and 4), at the headline shape fused and at a small one unfused, are the text a build of the commit before this op printed"""
    d = json.load(open(os.path.join(HERE, "golden", "plans_before_square.json")))
    assert {(p["op"], p["overrides"].get("terms")) for p in d["points"]} == {("hmult", None), ("hdot", 1), ("hdot", 4)}
    for p in d["points"]:
        o = host.Op(p["cfg"], p["op"], p["L"], p["l"], p["alpha"], backend=host.BACKEND_COUNT, fuse=bool(p["fuse"]), overrides=p["overrides"] or None)
        try:
            assert o.plan() == p["plan"] and o.plan(full=True) == p["full"], (p["op"], p["overrides"], p["cfg"], p["fuse"])
            assert "TENSOR_SQUARE" not in "".join(o.plan())
        finally:
            o.close()
