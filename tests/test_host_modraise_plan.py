"""hmodraise on the count backend (no GPU): two launches at any batch (the INTT of the two input limb-polys, then ONE lifted
forward transform launch of 2 T limb-polys per op, plan field lift=1), the output level T by default and with raise_to, every refusal names the op,
the op is a legal link of a chain with the next op at level T, and the plans of the ops that existed before it are the text their parent printed
(tests/golden/plans_before_modraise.json)."""
import json
import os
import re

import pytest

from homulator_amd import host

HERE = os.path.dirname(os.path.abspath(__file__))
POINTS = [("config_4.cfg", 16, (45, 1, 15)), ("config_4_N15.cfg", 15, (16, 1, 4))]


def build(cfg, lv, fuse=True, op="hmodraise", backend=host.BACKEND_COUNT, **ov):
    o = host.Op(cfg, op, *lv, backend=backend, fuse=fuse, overrides=ov or None)
    try:
        return {"plan": o.plan(), "full": o.plan(full=True), "n": o.launch_count(), "level": o.output_level(), "bytes": o.stage_bytes(),
                "total": o.total_instructions()}
    finally:
        o.close()


def n_of(line):
    return int(re.search(r" n=(\d+)", line).group(1))


def field(line, name):
    m = re.search(r" %s=([0-9,]+)" % name, line)
    return [int(x) for x in m.group(1).split(",")] if m else None


@pytest.mark.parametrize("cfg,logN,lv", POINTS)
@pytest.mark.parametrize("batch", [1, 3])
def test_two_launches_at_any_batch(cfg, logN, lv, batch):
    T, LP = lv[0], 8 << logN
    for fuse in (True, False):
        r = build(cfg, lv, fuse=fuse, batch=batch)
        assert r["n"] == 2 and [ln.split()[0] for ln in r["plan"]] == ["INTT", "NTT"], r["plan"]
        assert n_of(r["plan"][0]) == 2 * batch and n_of(r["plan"][1]) == 2 * batch * T
        assert "lift=1" in r["plan"][1] and "lift=1" not in r["plan"][0]
        assert r["level"] == T
        intt, ntt = r["full"]
        # every record of the second launch is lifted from q_0; component k of copy c reads ONE source, the INTT's output, for all T moduli
        assert field(ntt, "liftMods") == [0] * (2 * batch * T) and field(intt, "liftMods") is None
        assert field(ntt, "mods") == list(range(T)) * (2 * batch) and field(intt, "mods") == [0] * (2 * batch)
        src = field(ntt, "a")
        assert [src[i * T:(i + 1) * T] for i in range(2 * batch)] == [[a] * T for a in field(intt, "out")]
        assert len(set(field(ntt, "out"))) == 2 * batch * T and not set(field(ntt, "out")) & set(src)
        # byte model: the INTT reads and writes 2 limb-polys per op, the lifted launch reads 2 and writes 2 T
        assert [int(re.search(r" bytes=(\d+)", ln).group(1)) for ln in r["full"]] == [4 * batch * LP, (2 + 2 * T) * batch * LP]
    assert build(cfg, lv, fuse=False, batch=batch)["total"] == build(cfg, lv, batch=batch)["total"]


@pytest.mark.parametrize("cfg,logN,lv", POINTS)
def test_raise_to_sets_the_output_level(cfg, logN, lv):
    L = lv[0]
    for T in (2, 7, L):
        r = build(cfg, lv, raise_to=T)
        assert r["level"] == T and r["n"] == 2 and n_of(r["plan"][1]) == 2 * T and field(r["full"][1], "mods") == list(range(T)) * 2
    assert build(cfg, lv)["level"] == L


def test_both_arithmetic_back_ends_take_the_same_plan():
    cfg, _, lv = POINTS[0]
    assert build(cfg, lv, chain_bits=60)["full"] == build(cfg, lv)["full"] and build(cfg, lv, chain_bits=36)["plan"] == build(cfg, lv)["plan"]


def test_every_refusal_names_the_op():
    cfg, _, lv = POINTS[0]
    L, _, alpha = lv
    with pytest.raises(host.HostError, match=r"hmodraise: level 2 "):
        build(cfg, (L, 2, alpha))
    with pytest.raises(host.HostError, match=r"hmodraise: level 35 "):
        build(cfg, (L, 35, alpha))
    for T in (0, 1, L + 1):
        with pytest.raises(host.HostError, match=r"hmodraise: raise_to = %d" % T):
            build(cfg, lv, raise_to=T)
    with pytest.raises(host.HostError, match=r"hmodraise: backend = sim"):
        build(cfg, lv, backend=host.BACKEND_SIM)
    with pytest.raises(host.HostError, match=r"hmodraise: world > 1"):
        build(cfg, lv, world=2)


@pytest.mark.parametrize("second", ["hrotate", "hmult"])
def test_chain_continues_at_the_raised_level(second):
    """hmodraise is a link like any other: the next op is built at level T (its first launch carries T limb-polys of the ModUp's input)"""
    L, alpha, T = 16, 4, 8
    chain = host.Chain("config_4_N15.cfg", "hmodraise," + second, L, 1, alpha, overrides={"raise_to": T, "backend": host.BACKEND_COUNT})
    try:
        assert chain[0].output_level() == T
        assert chain[1].output_level() == (T - 1 if second == "hmult" else T)
        alone = host.Op("config_4_N15.cfg", second, L, T, alpha, backend=host.BACKEND_COUNT)
        assert [re.sub(r" ref=\d+", "", ln) for ln in chain[1].plan()] == [re.sub(r" ref=\d+", "", ln) for ln in alone.plan()]
        alone.close()
    finally:
        chain.close()
    with pytest.raises(host.HostError, match="hmodraise: level 5"):
        host.Chain("config_4_N15.cfg", "hrotate,hmodraise", L, 5, alpha, overrides={"backend": host.BACKEND_COUNT})


def test_existing_ops_keep_the_plans_their_parent_printed():
    d = json.load(open(os.path.join(HERE, "golden", "plans_before_modraise.json")))
    assert {p["op"] for p in d["points"]} == {"hmult", "hrotate", "pmult", "hrescale"}
    for p in d["points"]:
        r = build(p["cfg"], (p["L"], p["l"], p["alpha"]), fuse=bool(p["fuse"]), op=p["op"], **p["overrides"])
        assert r["plan"] == p["plan"] and r["full"] == p["full"], (p["op"], p["overrides"], p["cfg"], p["fuse"])
        assert "lift" not in "".join(r["full"])
