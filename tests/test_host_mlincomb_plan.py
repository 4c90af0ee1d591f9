"""hmlincomb on the count backend (no GPU): out<m> = sum_t s_{m,t} ct<t> + k_m for m = 1 .. M.  The fused plan is ONE
LINCOMB_MULTI launch for both components of all copies whatever T, M and ml_const say (M = 1: hlincomb's LINCOMB launch), followed with rescale = 1 by
the coalesced launches of the M rescales; its instruction total is the unfused plan's, whose launches follow the stage list; fuse_mlincomb = 0 leaves
the M sums to ONE LINCOMB launch; the refusals name op and key, the constants go through set_constants, their streams meet no other stream, the op
chains and binds by output, the pool statement holds, and no plan of hmult, hlincomb, hclincomb, hplincomb or hdotadd moved
(tests/golden/plans_before_mlincomb.json)."""
import hashlib
import json
import os
import re

import pytest

from homulator_amd import hip, host

HERE = os.path.dirname(os.path.abspath(__file__))
POINTS = [("config_4.cfg", 45, 35, 15, 16), ("config_4_N15.cfg", 16, 10, 4, 15)]
TM = [(1, 1), (4, 4), (8, 8), (16, 16), (8, 2)]
TILE = hip.LINCOMB_MULTI_TILE
POOL = 65535        # limb-polys are addressed by 16-bit indices over the whole batch


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


def top(full):
    """the highest limb-poly index a launch of the plan names"""
    m = 0
    for ln in full:
        for f in re.findall(r"[ {](?:a|b|c|d|out|out1|out2|x0|x1|in)=([\d,]+)", ln):
            m = max(m, max(int(x) for x in f.split(",") if int(x) != hip.NO_LIMB))
    return m


def limb_polys(T, M, mc, ell, rescale=0):
    """what a copy takes (a buffer per stage, used by the fused plan or not): the inputs 2 T l; per output and component T scaled terms and T - 1
    sums, (2T - 1) l, the last of them the output; with ml_const one more on c0, l; with rescale per output and component two single limb-polys
    and three buffers of l - 1"""
    return 2 * T * ell + M * (2 * (2 * T - 1) + mc) * ell + rescale * M * 2 * (3 * ell - 1)


def largest_batch(T, M, mc, ell):
    return min(10, POOL // limb_polys(T, M, mc, ell))


def model_bytes(T, M, ell, batch, logN):
    """(ceil(M / TILE) T + M) limb-polys per entry: the inputs once per tile of outputs, every output once"""
    return (-(-M // TILE) * T + M) * 2 * ell * batch * 8 * (1 << logN)


@pytest.mark.parametrize("cfg,L,ell,alpha,logN", POINTS)
@pytest.mark.parametrize("T,M", TM)
@pytest.mark.parametrize("mc", [0, 1])
def test_the_fused_plan_is_one_launch(cfg, L, ell, alpha, logN, T, M, mc):
    ov = {"terms": T, "outputs": M, "ml_const": mc}
    for batch in sorted({1, largest_batch(T, M, mc, ell)}):
        p, total, n, full = build(cfg, "hmlincomb", L, ell, alpha, batch=batch, **ov)
        assert n == 1 and len(p) == 1, p
        if M == 1:      # one sum: (5l)'s record and launch, hlincomb's plan
            assert kinds_of(p) == ["LINCOMB"] and n_of(p[0]) == 2 * ell * batch and f" terms={T} const={mc} " in p[0] + " "
            assert int(re.search(r" bytes=(\d+)", full[0]).group(1)) == (T + 1) * 2 * ell * batch * 8 * (1 << logN)
            continue
        assert kinds_of(p) == ["LINCOMB_MULTI"] and n_of(p[0]) == 2 * ell * M * batch and f" terms={T} out={M} const={mc} " in p[0] + " ", p
        assert int(re.search(r" bytes=(\d+)", full[0]).group(1)) == model_bytes(T, M, ell, batch, logN)
        assert f" multiOuts={M} " in full[0] and top(full) == batch * limb_polys(T, M, mc, ell) - 1 <= POOL
        # the copies run under the same constants: [n][M][T] scalars and [n][M] constants, c0's entries then c1's, copy after copy
        k = re.search(r" k=([0-9,]+)", full[0]).group(1).split(",")
        assert len(k) == 2 * ell * M * T * batch and k == k[:2 * ell * M * T] * batch and k[:ell * M * T] == k[ell * M * T:2 * ell * M * T]
        a = re.search(r" addK=([0-9,]+)", full[0])
        assert bool(a) == bool(mc)
        if a:
            v = a.group(1).split(",")
            assert len(v) == 2 * ell * M * batch and v == v[:2 * ell * M] * batch and v[ell * M:2 * ell * M] == ["0"] * (ell * M)      # c1 adds nothing


@pytest.mark.parametrize("cfg,L,ell,alpha,logN", POINTS)
@pytest.mark.parametrize("T,M", TM)
@pytest.mark.parametrize("mc", [0, 1])
def test_instruction_totals_and_the_other_routes(cfg, L, ell, alpha, logN, T, M, mc):
    ov = {"terms": T, "outputs": M, "ml_const": mc}
    p, total, n, _ = build(cfg, "hmlincomb", L, ell, alpha, **ov)
    p0, total0, n0, _ = build(cfg, "hmlincomb", L, ell, alpha, fuse=False, **ov)
    assert total0 == total == ref_of(p) == ref_of(p0)                       # fusion moves instructions, never drops them
    # M hlincomb ops have the same instructions
    assert total == M * build(cfg, "hlincomb", L, ell, alpha, terms=T, lc_const=mc)[1]
    # unfused: one launch per stage: per output and component T Scale and T - 1 Add stages, and the Const stage of c0
    assert kinds_of(p0) == ["EWE"] * (M * (2 * (2 * T - 1) + mc)) and n0 == len(p0) and all(n_of(ln) == ell for ln in p0)
    # fuse_mlincomb = 0: the M 2 l records of (5l) share ONE LINCOMB launch (no sum waits for another)
    p1, total1, n1, _ = build(cfg, "hmlincomb", L, ell, alpha, fuse_mlincomb=0, **ov)
    assert shape_of(p1) == [("LINCOMB", 2 * ell * M)] and n1 == 1 and total1 == total and f" terms={T} const={mc} " in p1[0] + " "
    # fuse_lincomb = 0 leaves nothing for the new pass to merge: hlincomb's element-wise plan over all outputs
    p2, total2, _, _ = build(cfg, "hmlincomb", L, ell, alpha, fuse_lincomb=0, **ov)
    assert set(kinds_of(p2)) == {"EWE"} and total2 == total
    assert shape_of(p2) == [("EWE", 2 * T * M * ell)] + [("EWE", 2 * M * ell)] * (T - 1) + [("EWE", M * ell)] * mc


@pytest.mark.parametrize("cfg,L,ell,alpha,logN", POINTS)
@pytest.mark.parametrize("T,M,mc,batch", [(1, 1, 0, 1), (4, 4, 1, 1), (8, 2, 1, 3), (3, 5, 0, 2), (16, 16, 1, 1)])
def test_with_rescale_the_rescales_of_all_outputs_coalesce(cfg, L, ell, alpha, logN, T, M, mc, batch):
    """every output goes through Rescale; the M rescales are of equal depth and share hrescale's two launches: 3 launches, within 1 + 2 M"""
    rs = build(cfg, "hrescale", L, ell, alpha, batch=batch)[0]
    p, total, n, full = build(cfg, "hmlincomb", L, ell, alpha, terms=T, outputs=M, ml_const=mc, rescale=1, batch=batch)
    assert len(rs) == 2 and n == len(p) == 3 <= 1 + 2 * M
    assert kinds_of(p) == ["LINCOMB_MULTI" if M > 1 else "LINCOMB"] + kinds_of(rs)
    assert n_of(p[0]) == 2 * ell * M * batch and [n_of(ln) for ln in p[1:]] == [M * n_of(ln) for ln in rs]
    p0, total0, _, full0 = build(cfg, "hmlincomb", L, ell, alpha, fuse=False, terms=T, outputs=M, ml_const=mc, rescale=1, batch=batch)
    assert total0 == total and ref_of(p) == ref_of(p0) == total * batch     # (the total is one op's, the launches carry the batch's)
    assert kinds_of(p0)[:M * (2 * (2 * T - 1) + mc)] == ["EWE"] * (M * (2 * (2 * T - 1) + mc))
    # the pool use per copy, by the unfused plan, which names every buffer (the fused one never touches the last rescale's last buffer)
    assert top(full) < top(full0) == batch * limb_polys(T, M, mc, ell, rescale=1) - 1
    o = host.Op(cfg, "hmlincomb", L, ell, alpha, backend=host.BACKEND_COUNT, overrides={"terms": T, "outputs": M, "rescale": 1})
    assert o.output_level() == ell - 1
    o.close()


def test_the_pool_statement():
    """limb-polys per copy at 45/35/15 with ml_const = 1 against the pool of 65 535: T = M = 16 takes 36 400 (one copy), T = M = 8 takes 9 240
    (seven), (4, 4) 2 380 and (8, 2) 2 730 (ten and more); a batch beyond the pool is planned and refused when it executes"""
    cfg, L, ell, alpha, _ = POINTS[0]
    assert [limb_polys(T, M, 1, ell) for T, M in ((16, 16), (8, 8), (4, 4), (8, 2))] == [36400, 9240, 2380, 2730]
    assert [largest_batch(T, M, 1, ell) for T, M in ((16, 16), (8, 8), (4, 4), (8, 2))] == [1, 7, 10, 10]
    over = build(cfg, "hmlincomb", L, ell, alpha, terms=8, outputs=8, ml_const=1, batch=8)[3]
    assert top(over) == 8 * 9240 - 1 > POOL


def test_the_synthetic_constants_are_the_streams_first_words():
    from oracle.homoracle import Oracle
    from mlincomb_ref import const_stream, scale_stream
    ell, T, M = 10, 3, 2
    orc = Oracle(15, 16, 4)
    full = build("config_4_N15.cfg", "hmlincomb", 16, ell, 4, terms=T, outputs=M, ml_const=1)[3]
    word0 = lambda stream: [int(orc.fill_uniform(range(ell), stream)[j][0]) for j in range(ell)]
    s = [[word0(scale_stream(host.SEED, m, t)) for t in range(1, T + 1)] for m in range(1, M + 1)]
    k = [word0(const_stream(host.SEED, m)) for m in range(1, M + 1)]
    rows = [str(s[m][t][j]) for j in range(ell) for m in range(M) for t in range(T)] * 2           # [n][M][T] row-major, c0's records then c1's
    assert " k=" + ",".join(rows) + " " in full[0] + " "
    assert " addK=" + ",".join([str(k[m][j]) for j in range(ell) for m in range(M)] + ["0"] * (ell * M)) + " " in full[0] + " "


def test_no_constant_stream_meets_an_input_stream_or_another_constant_stream():
    """T = M = 16 at l = 45: a value is word 0 of limb j of its stream, stream + j; an input is stream seed + 2000 i + 1000 k + j"""
    from mlincomb_ref import const_stream, scale_stream
    T = M = 16
    ell = 45
    inputs = {2000 * i + 1000 * k + j for i in range(T) for k in range(2) for j in range(ell)}
    consts = [scale_stream(0, m, t) + j for m in range(1, M + 1) for t in range(1, T + 1) for j in range(ell)]
    consts += [const_stream(0, m) + j for m in range(1, M + 1) for j in range(ell)]
    assert len(consts) == len(set(consts)) == (T + 1) * M * ell and not inputs & set(consts)
    assert all(150 <= c % 1000 < 995 for c in consts) and all(x % 1000 < 45 for x in inputs)


@pytest.mark.parametrize("key,lo,hi", [("terms", 0, 17), ("outputs", 0, 17)])
def test_counts_outside_1_16_are_refused_by_op_and_key(key, lo, hi):
    for v in (lo, hi, 100):
        with pytest.raises(host.HostError, match=rf"^hmlincomb: {key} = {v}, must be in \[1, 16\]"):
            build("config_4_N15.cfg", "hmlincomb", 16, 10, 4, **{key: v})


@pytest.mark.parametrize("key", ["ml_const", "rescale", "fuse_mlincomb"])
def test_a_key_outside_0_1_is_refused_by_op_and_key(key):
    with pytest.raises(host.HostError, match=rf"^hmlincomb: {key} = 2, must be 0 or 1"):
        build("config_4_N15.cfg", "hmlincomb", 16, 10, 4, **{key: 2})


def test_the_defaults_are_four_terms_four_outputs_no_constant():
    p = build("config_4_N15.cfg", "hmlincomb", 16, 10, 4)[0]
    assert kinds_of(p) == ["LINCOMB_MULTI"] and " terms=4 out=4 const=0 " in p[0] + " "


def test_unserved_modes_are_clear_errors():
    with pytest.raises(host.HostError, match="^hmlincomb:.*world"):
        host.Op("config_4_N15.cfg", "hmlincomb", 16, 10, 4, backend=host.BACKEND_COUNT, world=2)
    with pytest.raises(host.HostError, match="^hmlincomb:.*sim"):
        host.Op("config_4_N15.cfg", "hmlincomb", 16, 10, 4, backend=host.BACKEND_SIM)
    with pytest.raises(host.HostError, match="^hmlincomb: Rescale needs at least two limbs"):     # hrescale's text
        host.Op("config_4_N15.cfg", "hmlincomb", 16, 1, 4, backend=host.BACKEND_COUNT, overrides={"rescale": 1})
    with pytest.raises(host.HostError, match="Rescale needs at least two limbs"):
        host.Op("config_4_N15.cfg", "hrescale", 16, 1, 4, backend=host.BACKEND_COUNT)
    assert build("config_4_N15.cfg", "hmlincomb", 16, 1, 4)[2] == 1       # without rescale, level 1 is served


def test_set_constants_round_trip_and_refusals():
    from oracle.homoracle import Oracle
    ell, T, M = 10, 3, 2
    q = [int(x) for x in Oracle(15, 16, 4).moduli]
    mk = lambda **ov: host.Op("config_4_N15.cfg", "hmlincomb", 16, ell, 4, backend=host.BACKEND_COUNT, overrides=dict({"terms": T, "outputs": M}, **ov))
    o = mk(ml_const=1)
    vals = {"scale1_1": [2] * ell, "scale1_2": [0] * ell, "scale1_3": [q[j] - 1 for j in range(ell)], "scale2_1": [5] * ell, "scale2_2": [j for j in range(ell)],
            "scale2_3": [0] * ell, "const1": [q[j] - 1 - j for j in range(ell)], "const2": [0] * ell}
    for name, v in vals.items():                                          # accepted: reduced, one per limb; zero is a scalar and a constant
        o.set_constants(name, v)
    for n in (ell - 1, ell + 1, 0):
        with pytest.raises(host.HostError, match=rf'hmlincomb: set_constants\("scale2_2"\): n = {n} values, the level is {ell}'):
            o.set_constants("scale2_2", [1] * n)
    with pytest.raises(host.HostError, match=r'hmlincomb: set_constants\("scale1_1"\): values\[3\] is not reduced'):
        o.set_constants("scale1_1", [1, 1, 1, q[3]] + [1] * (ell - 4))
    with pytest.raises(host.HostError, match=r'hmlincomb: set_constants\("const2"\): values\[0\] is not reduced'):
        o.set_constants("const2", [q[0]] + [0] * (ell - 1))
    for name in ("scale", "scale1", "scale0_1", "scale3_1", "scale1_4", "const", "const3", "offset"):
        with pytest.raises(host.HostError, match=rf'hmlincomb: set_constants\("{name}"\): the op has no constants of that name'):
            o.set_constants(name, [0] * ell)
    line = o.plan(full=True)[0] + " "      # builds the plan: the accepted values are in the launch, for both components
    rows = [str(vals[f"scale{m}_{t}"][j]) for j in range(ell) for m in (1, 2) for t in (1, 2, 3)] * 2
    assert " k=" + ",".join(rows) + " " in line
    assert " addK=" + ",".join([str(vals[f"const{m}"][j]) for j in range(ell) for m in (1, 2)] + ["0"] * (ell * M)) + " " in line
    for name in vals:
        with pytest.raises(host.HostError, match=rf'hmlincomb: set_constants\("{name}"\) after prepare'):
            o.set_constants(name, [1] * ell)
    o.close()
    o = mk()
    with pytest.raises(host.HostError, match=r'hmlincomb: set_constants\("const2"\): ml_const = 0'):
        o.set_constants("const2", [1] * ell)
    o.close()


def test_chains_keep_the_level_bookkeeping():
    """hmlincomb as first, middle and last link ("out" names out1): the level is kept, or drops by one with rescale = 1; every link draws its own
    constants"""
    ov = {"backend": host.BACKEND_COUNT, "terms": 3, "outputs": 2, "ml_const": 1}
    c = host.Chain("config_4_N15.cfg", "hmlincomb,hmult", 16, 10, 4, overrides=ov)
    assert [c[i].output_level() for i in range(2)] == [10, 9]
    c.close()
    c = host.Chain("config_4_N15.cfg", "hmult,hmlincomb,hadd", 16, 10, 4, overrides=ov)
    assert [c[i].output_level() for i in range(3)] == [9, 9, 9]
    p = c[1].plan()
    assert kinds_of(p) == ["LINCOMB_MULTI"] and n_of(p[0]) == 2 * 9 * 2 and " terms=3 out=2 const=1 " in p[0] + " "
    c.close()
    c = host.Chain("config_4_N15.cfg", "hmlincomb,hmlincomb,hmlincomb", 16, 10, 4, overrides=dict(ov, rescale=1))
    assert [c[i].output_level() for i in range(3)] == [9, 8, 7]
    ks = [re.search(r" k=([0-9,]+)", c[i].plan(full=True)[0]).group(1).split(",") for i in range(3)]
    assert ks[0][:6] != ks[1][:6] != ks[2][:6]                            # every link draws its own, from its own seed
    c.close()


def test_bind_input_for_every_input_and_from_every_output():
    T, M, ell = 3, 3, 10
    mk = lambda op, lvl, **ov: host.Op("config_4_N15.cfg", op, 16, lvl, 4, backend=host.BACKEND_COUNT, overrides=ov or None)
    src = mk("hmlincomb", ell, terms=T, outputs=M)
    prod = mk("hadd", ell)
    dst = mk("hmlincomb", ell, terms=T, outputs=M, seed=host.SEED + 31)
    for t in range(1, T + 1):                 # every input takes a producer's "out" ...
        dst.bind_input(f"ct{t}", prod)
    dst.close()
    for m in range(1, M + 1):                 # ... and every output feeds a consumer
        use = mk("hlincomb", ell, terms=2, seed=host.SEED + 62)
        use.bind_input("ct2", src, output=f"out{m}")
        use.close()
    use = mk("hlincomb", ell, terms=2)
    use.bind_input("ct1", src)                # "out" is out1
    with pytest.raises(host.HostError, match="has no output ciphertext out4"):
        use.bind_input("ct2", src, output="out4")
    use.close()
    wrong = mk("hlincomb", ell - 1, terms=2)
    with pytest.raises(host.HostError, match="levels differ"):
        wrong.bind_input("ct1", src, output="out2")
    wrong.close()
    down = mk("hmlincomb", ell, terms=T, outputs=M, rescale=1)
    ok = mk("hlincomb", ell - 1, terms=2)
    ok.bind_input("ct2", down, output="out3")  # rescaled outputs are at level l - 1
    for x in (ok, down, prod, src):
        x.close()


def test_buffer_names():
    o = host.Op("config_4_N15.cfg", "hmlincomb", 16, 10, 4, backend=host.BACKEND_COUNT, overrides={"terms": 3, "outputs": 2, "ml_const": 1})
    names = set(o.buffer_names())
    o.close()
    want = {f"ct{t}.c{k}" for t in (1, 2, 3) for k in (0, 1)} | {f"out{m}.c{k}" for m in (1, 2) for k in (0, 1)} | {"out.c0", "out.c1"}
    want |= {f"MLinCombOutput({m},{k})" for m in (1, 2) for k in (0, 1)} | {"MLinCombScaled(2,3)_C1", "MLinCombSum(1,2)_C0"}
    assert want <= names and "ct4.c0" not in names and "out3.c0" not in names


def test_the_other_ops_keep_their_plans():
    """plan() and plan(full=True) of hmult, hlincomb, hclincomb, hplincomb and hdotadd, at the headline shape fused and at a small one unfused, are
    the text a build of the commit before this op printed"""
    d = json.load(open(os.path.join(HERE, "golden", "plans_before_mlincomb.json")))
    assert {p["op"] for p in d["points"]} == {"hmult", "hlincomb", "hclincomb", "hplincomb", "hdotadd"} and len(d["points"]) == 36
    for p in d["points"]:
        o = host.Op(p["cfg"], p["op"], p["L"], p["l"], p["alpha"], backend=host.BACKEND_COUNT, fuse=bool(p["fuse"]), overrides=p["overrides"] or None)
        try:
            assert o.plan() == p["plan"], (p["op"], p["overrides"], p["cfg"], p["fuse"])
            assert hashlib.sha256("\n".join(o.plan(full=True)).encode()).hexdigest() == p["full_sha256"], (p["op"], p["overrides"], p["cfg"], p["fuse"])
            assert "LINCOMB_MULTI" not in "".join(o.plan())
        finally:
            o.close()
