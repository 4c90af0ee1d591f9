"""hlintrans with identity = 1 on the count backend (no GPU), DESIGN.md section 16: the unrotated term pt0 * ct joins the weighted sum of the
rotations without a launch of its own.  The fused plan keeps its 7 launches whatever R is — the head link of U, the lone MUL W and the c1 add all
go into launches that exist already — its instruction total is the unfused plan's, identity = 0 is the op as it was, and every refusal names the
key.  hbsgs with identity = 1 (giant groups 0..G, baby steps 0..R) keeps its 14 launches for every R and G: the baby step forms G + 1 sums,
the inner ModDowns cover G groups, and group 0's sums are the initial sums of the giant step's launch."""
import re

import pytest

from homulator_amd import host

FUSED = ["INTT", "BCONV", "NTT", "IP_LINTRANS", "INTT", "BCONV", "NTT_SUBSCALE"]


def build(cfg, L, ell, alpha, fuse=True, op="hlintrans", full=False, **ov):
    o = host.Op(cfg, op, L, ell, alpha, backend=host.BACKEND_COUNT, fuse=fuse, overrides=ov or None)
    try:
        return o.plan(full=full), o.total_instructions(), o.launch_count(), o.stage_bytes()
    finally:
        o.close()


def n_of(line):
    return int(re.search(r" n=(\d+)", line).group(1))


def kinds_of(plan):
    return [ln.split()[0] for ln in plan]


def identity_is_read(cfg="config_4_N15.cfg", L=16, ell=10, alpha=4, **ov):
    """hlintrans reads the key: its merged launch carries the identity step (what the tests below take for granted)"""
    p = build(cfg, L, ell, alpha, identity=1, **ov)[0]
    return kinds_of(p) == FUSED and p[3].rstrip().endswith("id=1")


@pytest.mark.parametrize("R", [1, 4, 15])
def test_launch_list_at_45_35_15(R):
    """still 7 launches: ModUp (3), ONE launch for the sums with id=1, ONE ModDown whose last transform adds U to c0 AND W to c1"""
    ell, alpha, beta = 35, 15, 3
    p, total, n, _ = build("config_4.cfg", 45, ell, alpha, rotations=R, identity=1)
    assert kinds_of(p) == FUSED and n == 7, (R, p)
    g = ",".join(str(pow(5, r, 1 << 17)) for r in range(1, R + 1))
    assert n_of(p[3]) == ell + alpha and p[3].rstrip().endswith(f" rot={R} g={g} addend={ell} id=1"), p[3]
    assert n_of(p[4]) == 2 * alpha and n_of(p[5]) == 2 * ell and n_of(p[6]) == 2 * ell
    p0, total0, n0, _ = build("config_4.cfg", 45, ell, alpha, fuse=False, rotations=R, identity=1)
    assert total0 == total and "IP_LINTRANS" not in kinds_of(p0)
    # against identity = 0: unfused, three more stages of l limbs each (U's head MUL, W's MUL, c1's ADD); fused, none
    q, totalq, nq, _ = build("config_4.cfg", 45, ell, alpha, rotations=R)
    q0, _, nq0, _ = build("config_4.cfg", 45, ell, alpha, fuse=False, rotations=R)
    assert kinds_of(q) == FUSED and nq == 7 and " id=1" not in q[3] and n0 == nq0 + 3
    assert kinds_of(p0).count("EWE") == kinds_of(q0).count("EWE") + 3 and kinds_of(p0).count("AUTO") == kinds_of(q0).count("AUTO")
    assert total > totalq


def test_identity_0_is_the_op_as_it_was():
    """the key left out and identity = 0: the same plan, field for field"""
    a = build("config_4.cfg", 45, 35, 15, full=True, rotations=4)
    b = build("config_4.cfg", 45, 35, 15, full=True, rotations=4, identity=0)
    assert a == b
    assert a[0] != build("config_4.cfg", 45, 35, 15, full=True, rotations=4, identity=1)[0]


def test_byte_model_of_the_launch():
    """limb-polys of the merged launch at batch 1 (one sum: one tile): n beta digits + 2 R n beta keys + R n plaintexts + n_Q c0 read and 2 n + n_Q
    written, as without the identity step, plus n_Q c1 and n_Q identity plaintext limbs read and n_Q limbs of W written"""
    n, beta, R, nq = 50, 3, 4, 35
    lines = {}
    for identity in (0, 1):
        p = build("config_4.cfg", 45, 35, 15, full=True, rotations=R, identity=identity)[0]
        lines[identity] = [ln for ln in p if ln.startswith("IP_LINTRANS")][0]
    b = {k: int(re.search(r" bytes=(\d+)", v).group(1)) for k, v in lines.items()}
    base = n * beta + 2 * R * n * beta + R * n + nq + 2 * n + nq
    assert b[0] == base * 8 * (1 << 16) and b[1] == (base + 3 * nq) * 8 * (1 << 16)
    # the launch's own lists: identity plaintexts and second addend outputs per entry, the c1 source; none of them without the identity step
    assert " idPt=" in lines[1] and " d1=" in lines[1] and " out2=" in lines[1]
    assert " idPt=" not in lines[0] and " d1=" not in lines[0] and " out2=" not in lines[0]


def test_batched_launch_gives_every_op_its_own_identity_plaintext_and_outputs():
    one = build("config_4.cfg", 45, 35, 15, full=True, rotations=2, identity=1)
    p, _, n, nbytes = build("config_4.cfg", 45, 35, 15, full=True, rotations=2, identity=1, batch=3)
    assert n == one[2] == 7 and nbytes == 3 * one[3]
    line = [ln for ln in p if ln.startswith("IP_LINTRANS")][0]
    for field in ("idPt", "d1", "out2"):
        v = [int(x) for x in re.search(rf" {field}=([\d,]+)", line).group(1).split(",")]
        own = [x for x in v if x != 0xFFFFFFFF]
        assert len(v) == 3 * (35 + 15) and len(own) == 3 * 35 and len(set(own)) == len(own), field


@pytest.mark.parametrize("alpha", [1, 2, 3, 5, 13])
def test_fused_total_is_the_unfused_total_at_every_level(alpha):
    """every level of a 13-limb chain at N = 2^13: beta <= 4 merges everything between the ModUp and the ModDown into one launch with id=1;
    beta >= 5 (no key-product record to merge) keeps separate launches.  Both keep the unfused plan's instruction total."""
    L = 13
    for ell in range(1, L + 1):
        beta = -(-ell // alpha)
        p, total, n, _ = build("config_4_N15.cfg", L, ell, alpha, N=1 << 13, rotations=2, identity=1)
        kinds = kinds_of(p)
        if beta <= 4:
            assert kinds == FUSED and p[3].rstrip().endswith(f"addend={ell} id=1"), (ell, kinds)
            assert n_of(p[4]) == 2 * alpha and n_of(p[6]) == 2 * ell
        else:
            assert "IP_LINTRANS" not in kinds and "AUTO" in kinds and "EWE" in kinds, (ell, kinds)
        assert build("config_4_N15.cfg", L, ell, alpha, fuse=False, N=1 << 13, rotations=2, identity=1)[1] == total, ell


def test_fuse_lintrans_off_gives_a_plan_without_the_launch():
    p, total, n, _ = build("config_4.cfg", 45, 35, 15, rotations=4, identity=1, fuse_lintrans=0)
    kinds = kinds_of(p)
    assert "IP_LINTRANS" not in kinds and kinds.count("IP_HOISTED") == 1 and "EWE" in kinds
    assert total == build("config_4.cfg", 45, 35, 15, rotations=4, identity=1)[1] and n > 7
    assert " id=1" not in "".join(p)


@pytest.mark.parametrize("op,ov,what", [
    ("hlintrans", {"identity": 2}, "identity = 2"), ("hlintrans", {"identity": 7}, "identity = 7"),
    ("hlintrans", {"identity": 1, "rotations": 16}, r"rotations = 16 with identity = 1"),
    ("hbsgs", {"identity": 2}, "identity = 2"), ("hbsgs", {"identity": 1, "rotations": 16}, r"rotations = 16 with identity = 1"),
    ("hbsgs", {"identity": 1, "giants": 16}, r"giants = 16 with identity = 1"),
])
def test_refusals_name_the_key(op, ov, what):
    with pytest.raises(host.HostError, match=what) as e:
        build("config_4_N15.cfg", 16, 10, 4, op=op, **ov)
    assert op in str(e.value)


def test_rotations_16_stays_served_without_the_identity_step():
    assert build("config_4_N15.cfg", 16, 10, 4, rotations=16)[2] == 7
    assert build("config_4_N15.cfg", 16, 10, 4, rotations=15, identity=1)[2] == 7 and identity_is_read(rotations=15)


def test_unserved_modes_stay_refused():
    assert identity_is_read()
    with pytest.raises(host.HostError, match="hlintrans.*world"):
        host.Op("config_4_N15.cfg", "hlintrans", 16, 10, 4, backend=host.BACKEND_COUNT, world=2, overrides={"identity": 1})
    with pytest.raises(host.HostError, match="hlintrans.*sim"):
        host.Op("config_4_N15.cfg", "hlintrans", 16, 10, 4, backend=host.BACKEND_SIM, overrides={"identity": 1})


def test_other_ops_do_not_read_the_key():
    assert identity_is_read()
    assert build("config_4_N15.cfg", 16, 10, 4, op="hmult", identity=1) == build("config_4_N15.cfg", 16, 10, 4, op="hmult")


def test_middle_link_of_a_chain():
    c = host.Chain("config_4_N15.cfg", "hmult,hlintrans,hadd", 16, 10, 4, overrides={"backend": host.BACKEND_COUNT, "rotations": 2, "identity": 1})
    assert kinds_of(c[1].plan()) == FUSED and c[1].plan()[3].rstrip().endswith("id=1") and n_of(c[1].plan()[3]) == 9 + 4
    assert n_of(c[2].plan()[0]) == 2 * 9
    c.close()


def test_buffer_names():
    o = host.Op("config_4_N15.cfg", "hlintrans", 16, 10, 4, backend=host.BACKEND_COUNT, overrides={"rotations": 2, "identity": 1})
    names = set(o.buffer_names())
    o.close()
    assert {"ct1.c0", "ct1.c1", "out.c0", "out.c1", "pt0", "pt1", "pt2", "LinTransOut_C0", "LinTransOut_C1", "HLINTRANSOutput(1)"} <= names
    o = host.Op("config_4_N15.cfg", "hlintrans", 16, 10, 4, backend=host.BACKEND_COUNT, overrides={"rotations": 2})
    names0 = set(o.buffer_names())
    o.close()
    assert not {"pt0", "LinTransOut_C1", "HLINTRANSOutput(1)"} & names0


# ---- hbsgs
BSGS = ["INTT", "BCONV", "NTT", "IP_LINTRANS_MULTI", "INTT", "BCONV", "NTT_SUBSCALE", "INTT", "BCONV", "NTT", "IP_ROTSUM", "INTT", "BCONV", "NTT_SUBSCALE"]


def bsgs(cfg, L, ell, alpha, **kw):
    return build(cfg, L, ell, alpha, op="hbsgs", **kw)


@pytest.mark.parametrize("R,G", [(1, 1), (4, 4), (15, 2)])
def test_bsgs_launch_list_at_45_35_15(R, G):
    ell, alpha, beta = 35, 15, 3
    p, total, n, _ = bsgs("config_4.cfg", 45, ell, alpha, rotations=R, giants=G, identity=1)
    assert kinds_of(p) == BSGS and n == 14, (R, G, p)
    h = pow(5, R + 1, 1 << 17)                                          # the default galois_giant with the identity step: g^(R+1)
    hs = ",".join(str(pow(h, i, 1 << 17)) for i in range(1, G + 1))
    assert n_of(p[3]) == ell + alpha and f" rot={R} " in p[3] and p[3].rstrip().endswith(f" out={G + 1} addend={ell} id=1"), p[3]
    # the coalesced inner ModDowns cover G groups, not G + 1: group 0 is never brought down on its own
    assert n_of(p[4]) == G * 2 * alpha and n_of(p[5]) == G * 2 * ell and n_of(p[6]) == G * 2 * ell
    assert n_of(p[7]) == G * ell and n_of(p[8]) == n_of(p[9]) == G * (beta * (ell + alpha) - ell)
    assert n_of(p[10]) == ell + alpha and p[10].rstrip().endswith(f" rot={G} g={hs} addend={ell} init=1"), p[10]
    assert n_of(p[11]) == 2 * alpha and n_of(p[13]) == 2 * ell          # ONE final ModDown; c1's add in its last transform
    p0, total0, n0, _ = bsgs("config_4.cfg", 45, ell, alpha, fuse=False, rotations=R, giants=G, identity=1)
    assert total0 == total and n0 > n and "IP_ROTSUM" not in kinds_of(p0)
    q, totalq, nq, _ = bsgs("config_4.cfg", 45, ell, alpha, rotations=R, giants=G)
    assert nq == 14 and " init=1" not in "".join(q) and " id=1" not in "".join(q) and total > totalq   # (G = 1 without it: IP_LINTRANS, IP_HOISTED)


def test_bsgs_identity_0_is_the_op_as_it_was():
    a = bsgs("config_4.cfg", 45, 35, 15, full=True, rotations=2, giants=2)
    assert a == bsgs("config_4.cfg", 45, 35, 15, full=True, rotations=2, giants=2, identity=0)
    assert a[0] != bsgs("config_4.cfg", 45, 35, 15, full=True, rotations=2, giants=2, identity=1)[0]


@pytest.mark.parametrize("G", [1, 2, 4, 5])
def test_bsgs_byte_model_of_the_two_changed_launches(G):
    """batch 1.  The baby step with M = G + 1 sums in t = ceil(M / TILE) tiles: t (n beta + 2 R n beta + 2 n_Q) + M R n + M n_Q read and
    M (2 n + 2 n_Q) written.  The giant step: as without initial sums, plus 2 n + n_Q initial limb-polys read"""
    from homulator_amd import hip
    n, beta, R, nq, M = 50, 3, 4, 35, G + 1
    t = -(-M // hip.LINTRANS_MULTI_TILE)
    p = bsgs("config_4.cfg", 45, 35, 15, full=True, rotations=R, giants=G, identity=1)[0]
    q = bsgs("config_4.cfg", 45, 35, 15, full=True, rotations=R, giants=G)[0]   # (G = 1 without the identity step: no IP_ROTSUM launch)
    nbytes = lambda plan, kind: int(re.search(r" bytes=(\d+)", [ln for ln in plan if ln.startswith(kind + " ")][0]).group(1))
    LP = 8 * (1 << 16)
    assert nbytes(p, "IP_LINTRANS_MULTI") == (t * (n * beta + 2 * R * n * beta + 2 * nq) + M * R * n + M * nq + M * (2 * n + 2 * nq)) * LP
    plain = n * (G * 3 * beta + 2) + nq * (G + 1)   # every ciphertext's digits, keys and addend source once, two outputs and the addend output
    assert nbytes(p, "IP_ROTSUM") == (plain + 2 * n + nq) * LP
    if G > 1:
        assert nbytes(q, "IP_ROTSUM") == plain * LP


def test_bsgs_fused_total_is_the_unfused_total_on_the_13_limb_grid():
    """(R, G) = (2, 2) at every level and digit size of a 13-limb chain at N = 2^13: beta <= 4 merges both steps (14 launches); beta >= 5 keeps
    separate launches.  Both keep the unfused plan's instruction total"""
    L = 13
    for alpha in (1, 2, 3, 5, 13):
        for ell in range(1, L + 1):
            beta = -(-ell // alpha)
            p, total, n, _ = bsgs("config_4_N15.cfg", L, ell, alpha, N=1 << 13, rotations=2, giants=2, identity=1)
            kinds = kinds_of(p)
            if beta <= 4:
                assert kinds == BSGS and p[3].rstrip().endswith("id=1") and p[10].rstrip().endswith("init=1"), (alpha, ell, kinds)
            else:
                assert "IP_LINTRANS_MULTI" not in kinds and "IP_ROTSUM" not in kinds and "EWE" in kinds, (alpha, ell, kinds)
            assert bsgs("config_4_N15.cfg", L, ell, alpha, fuse=False, N=1 << 13, rotations=2, giants=2, identity=1)[1] == total, (alpha, ell)


@pytest.mark.parametrize("ov,has,lacks", [({"fuse_bsgs": 0}, "IP_ROTSUM", "IP_LINTRANS_MULTI"), ({"fuse_rotsum": 0}, "IP_LINTRANS_MULTI", "IP_ROTSUM")])
def test_bsgs_with_one_merge_off(ov, has, lacks):
    p, total, n, _ = bsgs("config_4.cfg", 45, 35, 15, rotations=2, giants=2, identity=1, **ov)
    kinds = kinds_of(p)
    assert kinds.count(has) == 1 and lacks not in kinds and "EWE" in kinds and n > 14
    assert total == bsgs("config_4.cfg", 45, 35, 15, rotations=2, giants=2, identity=1)[1]
    line = [ln for ln in p if ln.startswith(has + " ")][0].rstrip()
    assert line.endswith("init=1" if has == "IP_ROTSUM" else "id=1")


def test_bsgs_batched_launches_give_every_op_its_own_operands():
    one = bsgs("config_4.cfg", 45, 35, 15, full=True, rotations=2, giants=2, identity=1)
    p, _, n, nbytes = bsgs("config_4.cfg", 45, 35, 15, full=True, rotations=2, giants=2, identity=1, batch=3)
    assert n == one[2] == 14 and nbytes == 3 * one[3]
    rs = [ln for ln in p if ln.startswith("IP_ROTSUM ")][0]
    for field, width, own_count in (("c", 2 * 50, 2 * 50), ("d1", 50, 35)):
        v = [int(x) for x in re.search(rf" {field}=([\d,]+)", rs).group(1).split(",")]
        own = [x for x in v if x != 0xFFFFFFFF]
        assert len(v) == 3 * width and len(own) == 3 * own_count and len(set(own)) == len(own), field


def test_bsgs_buffer_names_and_default_giant_element():
    o = host.Op("config_4_N15.cfg", "hbsgs", 16, 10, 4, backend=host.BACKEND_COUNT, overrides={"rotations": 2, "giants": 2, "identity": 1})
    names, plan = set(o.buffer_names()), o.plan()
    o.close()
    assert {"pt1", "pt4", "pt0_0", "pt0_1", "pt0_2", "ptg1", "ptg2", "out.c0", "out.c1", "HBSGSOutput(1)"} <= names
    assert "pt0_3" not in names and "ptg3" not in names and "pt5" not in names
    assert f" g={pow(5, 3, 1 << 16)},{pow(5, 6, 1 << 16)} " in [ln for ln in plan if ln.startswith("IP_ROTSUM")][0]
    o = host.Op("config_4_N15.cfg", "hbsgs", 16, 10, 4, backend=host.BACKEND_COUNT, overrides={"rotations": 2, "giants": 2})
    assert not {"pt0_0", "ptg1", "HBSGSOutput(1)"} & set(o.buffer_names())
    o.close()
