"""hrotate_hoisted on the count backend (no GPU): R rotations of one ciphertext with one ModUp.  The fused plan has one hoisted key-product
launch and no automorphism launch whatever R is, its instruction total is the unfused plan's, the plans of the other ops do not move, and the
CPU reference the GPU tests compare against reproduces the oracle's key switch."""
import json
import os
import re

import numpy as np
import pytest

from homulator_amd import host

HERE = os.path.dirname(os.path.abspath(__file__))
SETS = [("config_4.cfg", 45, 35, 15), ("config_4_N15.cfg", 16, 10, 4), ("config_4.cfg", 28, 28, 28)]


def build(cfg, L, ell, alpha, fuse=True, **ov):
    o = host.Op(cfg, "hrotate_hoisted", L, ell, alpha, backend=host.BACKEND_COUNT, fuse=fuse, overrides=ov or None)
    try:
        return o.plan(), o.total_instructions(), o.launch_count(), o.stage_bytes()
    finally:
        o.close()


def n_of(line):
    return int(re.search(r" n=(\d+)", line).group(1))


@pytest.mark.parametrize("cfg,L,ell,alpha", SETS)
def test_one_hoisted_key_product_whatever_the_rotation_count(cfg, L, ell, alpha):
    counts = set()
    for R in (1, 2, 4, 8):
        p, total, n, _ = build(cfg, L, ell, alpha, rotations=R)
        kinds = [ln.split()[0] for ln in p]
        assert kinds == ["INTT", "BCONV", "NTT", "IP_HOISTED", "INTT", "BCONV", "NTT_SUBSCALE"], (R, kinds)
        assert kinds.count("IP_HOISTED") == 1 and "AUTO" not in kinds and "IP" not in kinds
        hoisted = p[3]
        assert f" rot={R} " in hoisted + " " and n_of(hoisted) == ell + alpha
        # the R ModDowns coalesce: 2R x the entries of one key
        assert n_of(p[4]) == 2 * R * alpha and n_of(p[5]) == 2 * R * ell and n_of(p[6]) == 2 * R * ell
        assert f"auto_addend={R * ell}/" in p[6]                 # sigma_r(c0) is gathered by every rotation's final transform
        _, total0, n0, _ = build(cfg, L, ell, alpha, fuse=False, rotations=R)
        assert total0 == total and n0 > n                         # the invariant of every op: fusion moves instructions, never drops them
        counts.add(n)
    assert counts == {7}


@pytest.mark.parametrize("alpha", [1, 2, 3, 5, 13])
def test_route_by_digit_count_at_every_level(alpha):
    """every level of a 13-limb chain (N = 2^13 override; the grid tests/test_gpu_hoisted_shapes.py executes): pass 6 builds key-product records
    of at most 4 terms, so beta = ceil(l / alpha) <= 4 takes the hoisted route (7 launches, no automorphism launch) and beta >= 5 the fallback
    route (an automorphism launch per rotation, element-wise key products, no hoisted launch); both keep the unfused plan's instruction total"""
    L = 13
    for ell in range(1, L + 1):
        beta = -(-ell // alpha)
        for R in (1, 4):
            p, total, n, _ = build("config_4_N15.cfg", L, ell, alpha, N=1 << 13, rotations=R)
            kinds = [ln.split()[0] for ln in p]
            assert n == len(kinds)
            if beta <= 4:
                assert kinds == ["INTT", "BCONV", "NTT", "IP_HOISTED", "INTT", "BCONV", "NTT_SUBSCALE"] and n == 7, (ell, R, kinds)
                assert f" rot={R} " in p[3] + " "
            else:
                assert "IP_HOISTED" not in kinds and kinds.count("AUTO") >= 1 and "EWE" in kinds, (ell, R, kinds)
            assert build("config_4_N15.cfg", L, ell, alpha, fuse=False, N=1 << 13, rotations=R)[1] == total, (ell, R)


def test_batched_hoisted_launch_carries_every_op():
    """batch = B: ONE hoisted launch of B (l + alpha) entries, the launch count of the single op, B times its stage bytes"""
    one = build("config_4.cfg", 45, 35, 15, rotations=4)
    p, _, n, nbytes = build("config_4.cfg", 45, 35, 15, rotations=4, batch=10)
    assert n == one[2] == 7 and nbytes == 10 * one[3]
    assert n_of(p[3]) == 10 * (35 + 15) and p[3].split()[0] == "IP_HOISTED"


def test_fuse_hoist_off_keeps_a_key_product_per_rotation():
    p, total, _, _ = build("config_4.cfg", 45, 35, 15, rotations=4, fuse_hoist=0)
    kinds = [ln.split()[0] for ln in p]
    assert "IP_HOISTED" not in kinds and kinds.count("AUTO") >= 1
    assert total == build("config_4.cfg", 45, 35, 15, rotations=4)[1]


def test_hoisting_moves_fewer_bytes_than_separate_rotations():
    h = host.Op("config_4.cfg", "hrotate", 45, 35, 15, backend=host.BACKEND_COUNT)
    one = h.stage_bytes()
    h.close()
    assert build("config_4.cfg", 45, 35, 15, rotations=4)[3] < 4 * one


def test_galois_elements_of_the_plan():
    p = build("config_4_N15.cfg", 16, 10, 4, rotations=3, galois=3)[0]
    assert p[3].rstrip().endswith("rot=3 g=3,9,27")


@pytest.mark.parametrize("ov,what", [
    ({"galois": 4}, "odd"), ({"galois": 2 * 32768}, "odd"), ({"galois": 1}, "distinct"), ({"galois": 2 * 32768 - 1, "rotations": 2}, "distinct"),
    ({"rotations": 0}, r"\[1, 16\]"), ({"rotations": 17}, r"\[1, 16\]"),
])
def test_bad_parameters_are_clear_errors(ov, what):
    with pytest.raises(host.HostError, match=what):
        build("config_4_N15.cfg", 16, 10, 4, **ov)


def test_unserved_modes_are_clear_errors():
    with pytest.raises(host.HostError, match="world"):
        host.Op("config_4_N15.cfg", "hrotate_hoisted", 16, 10, 4, backend=host.BACKEND_COUNT, world=2)
    with pytest.raises(host.HostError, match="sim"):
        host.Op("config_4_N15.cfg", "hrotate_hoisted", 16, 10, 4, backend=host.BACKEND_SIM)
    with pytest.raises(host.HostError, match="last op"):
        host.Chain("config_4_N15.cfg", "hrotate_hoisted,hadd", 16, 10, 4, overrides={"backend": host.BACKEND_COUNT})
    c = host.Chain("config_4_N15.cfg", "hadd,hrotate_hoisted", 16, 10, 4, overrides={"backend": host.BACKEND_COUNT, "rotations": 2})
    assert len(c) == 2
    c.close()


def test_buffer_names():
    o = host.Op("config_4_N15.cfg", "hrotate_hoisted", 16, 10, 4, backend=host.BACKEND_COUNT, overrides={"rotations": 2})
    names = set(o.buffer_names())
    o.close()
    for r in (1, 2):
        assert {f"out{r}.c0", f"out{r}.c1"} <= names
        assert {f"IP_Rot{r}_Key{k}_{j}" for k in range(2) for j in range(3)} <= names
    assert "out.c0" not in names and "IP_Key0_0" not in names


def test_existing_plans_are_unchanged():
    """the plans of the five original ops as they were before hrotate_hoisted (tests/golden/make_plan_fixture.py)"""
    d = json.load(open(os.path.join(HERE, "golden", "plans_existing_ops.json")))
    assert len(d["points"]) == 20
    for p in d["points"]:
        o = host.Op(p["cfg"], p["op"], p["L"], p["l"], p["alpha"], backend=host.BACKEND_COUNT, fuse=bool(p["fuse"]))
        try:
            assert o.plan() == p["plan"], (p["cfg"], p["op"], p["fuse"])
            assert o.total_instructions() == p["total_instructions"] and o.stage_bytes() == p["stage_bytes"]
        finally:
            o.close()


def test_reference_helper_reproduces_the_oracle_key_switch():
    """fed the ModUp digits of sigma(c1), the helper's key product + ModDown is Oracle.keyswitch(ell, sigma(c1), evk)"""
    from oracle.homoracle import Oracle
    from hoisted_ref import key_product_moddown, modup_digits
    o = Oracle(13, 6, 2)
    ell = 5
    c1 = o.fill_uniform(list(range(ell)), 77)
    evk = o.synth_evk(ell, 5000)
    rc1 = o.automorph_eval(c1, 5)
    exp0, exp1 = o.keyswitch(ell, rc1, evk)
    got0, got1 = key_product_moddown(o, ell, modup_digits(o, ell, rc1), evk)
    assert np.array_equal(got0, exp0) and np.array_equal(got1, exp1)
