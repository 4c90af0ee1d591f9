"""hbsgs on the GPU, on both arithmetic back-ends (mont32 and chain_bits = 60), bit for bit:
 A. hm_inner_product_lintrans_multi against the oracle's automorphism and MUL / MAC_ADD chains AND against n_out calls of
    hm_inner_product_lintrans on the same buffers, on permuted limb lists with guard limb-polys, and its refusals;
 B. the op, fused (one IP_LINTRANS_MULTI and one IP_ROTSUM launch) and unfused (one launch per stage), against tests/bsgs_ref.py, and against G
    hlintrans ops + one hrotsum op run on the GPU;
 C. the op as the middle link of a chain;
 D. on real data (tests/toy_ckks.py) out decrypts to sum_i sigma_{h_i}(sum_r p_{i,r} * sigma_{g_r}(m))."""
import types

import numpy as np
import pytest

from homulator_amd import host
from oracle.homoracle import EWE_MAC_ADD, EWE_MUL, Oracle, chain_below

pytestmark = pytest.mark.gpu
CHAINS = ["mont32", "survey"]
SEED = host.SEED
BATCH_SEED_STRIDE = 100000   # host/src/Arch.cpp kBatchSeedStride
NQ, NP = 6, 3
GUARD = 0x5A5A5A5A5A5A5A5A
_oracles = {}


def oracle(logN, L, K, chain="mont32", threads=8):
    key = (logN, L, K, chain)
    if key not in _oracles:
        _oracles[key] = Oracle(logN, L, K, chain=chain)
    _oracles[key].set_threads(threads)
    return _oracles[key]


def chain_ov(chain, base):
    return dict(base, chain_bits=60) if chain != "mont32" else dict(base)


def tile():
    from homulator_amd import hip
    return hip.LINTRANS_MULTI_TILE


# ============================================================================================================================
# A. the kernel
# ============================================================================================================================
@pytest.fixture(scope="module")
def envs():
    """(hip context, oracle on the same moduli) per (logN, chain), made on first use"""
    from homulator_amd import hip
    made = {}

    def get(logN, chain):
        if (logN, chain) not in made:
            if chain == "mont32":
                ctx = hip.Context(logN, NQ, NP)
            else:
                mods = chain_below(logN, 60, NQ + NP)
                ctx = hip.Context(logN, NQ, NP, q=mods[:NQ], p=mods[NQ:])
            o = oracle(logN, NQ, NP, chain)
            assert ctx.moduli == o.moduli
            made[(logN, chain)] = (ctx, o)
        return made[(logN, chain)]
    yield get
    for ctx, _ in made.values():
        ctx.close()


def run_kernel_case(ctx, o, mods, T, galois, G, seed, add_mask, fill="uniform", y_rot_cap=None, tile_opt=0):
    """one hm_inner_product_lintrans_multi call of G outputs; every limb list is a random permutation of its buffer, the two output buffers keep one
    guard limb-poly each.  add_mask[i]: entry i carries an addend.  fill: "uniform" (device fill), "q-1" or "zero" (every operand).  y_rot_cap
    bounds the key pool: rotation r reads the keys of rotation r mod cap.  Checks every output against the oracle, against G calls of
    hm_inner_product_lintrans into a second pair of output buffers (whole buffers, guards included), and the guards."""
    from homulator_amd import hip
    from lintrans_ref import weighted_sum
    n, R, N = len(mods), len(galois), ctx.N
    rng = np.random.default_rng(seed)
    Ry = min(R, y_rot_cap or R)
    adds = [i for i in range(n) if add_mask[i]]
    nx, ny, npt, nc, no, na = n * T, Ry * n * 2 * T, G * R * n, max(1, len(adds)), G * 2 * n + 1, G * len(adds) + 1
    xb, yb, pb, cb, ob, ab, ob2, ab2 = (ctx.alloc(k) for k in (nx, ny, npt, nc, no, na, no, na))
    xl, ypool, pl, cperm, operm, aperm = ([int(v) for v in rng.permutation(k)] for k in (nx, ny, npt, nc, no, na))
    yl = [ypool[e % ny] for e in range(R * n * 2 * T)]
    ol = operm[:G * 2 * n]                                    # [m][n][2]
    cl = [hip.NO_LIMB] * n
    al = [hip.NO_LIMB] * (G * n)                              # [m][n]
    for t, i in enumerate(adds):
        cl[i] = cperm[t]
        for m in range(G):
            al[m * n + i] = aperm[m * len(adds) + t]
    xm = {xl[i * T + j]: mods[i] for i in range(n) for j in range(T)}
    ym = {yl[((r * n + i) * 2 + k) * T + j]: mods[i] for r in range(R) for i in range(n) for k in range(2) for j in range(T)}
    pm = {pl[(m * R + r) * n + i]: mods[i] for m in range(G) for r in range(R) for i in range(n)}
    cm = {cl[i]: mods[i] for i in adds} or {0: 0}
    for buf, mm in ((xb, xm), (yb, ym), (pb, pm), (cb, cm)):
        if fill == "uniform":
            ctx.fill_uniform(buf, [mm[k] for k in sorted(mm)], seed * 11 + len(mm), out_limbs=sorted(mm))
        else:
            buf.upload(np.stack([np.full(N, ctx.moduli[mm[k]] - 1 if fill == "q-1" else 0, dtype=np.uint64) for k in sorted(mm)]))
    for b in (ob, ob2):
        b.upload(np.full((no, N), GUARD, dtype=np.uint64))
    for b in (ab, ab2):
        b.upload(np.full((na, N), GUARD, dtype=np.uint64))
    opt = lambda v: v if adds else None
    ctx.set_option("ip_multi_tile", tile_opt)
    try:
        ctx.inner_product_lintrans_multi(xb, xl, yb, yl, pb, pl, ob, ol, mods, T, galois, G,
                                         addend=opt(cb), addend_limbs=opt(cl), addend_out=opt(ab), addend_out_limbs=opt(al))
    finally:
        ctx.set_option("ip_multi_tile", 0)
    for m in range(G):
        ctx.inner_product_lintrans(xb, xl, yb, yl, pb, pl[m * R * n:(m + 1) * R * n], ob2, ol[m * 2 * n:(m + 1) * 2 * n], mods, T, galois,
                                   addend=opt(cb), addend_limbs=opt(cl), addend_out=opt(ab2), addend_out_limbs=opt(al[m * n:(m + 1) * n]))
    X, Y, P, Cs, got, gotA, got2, gotA2 = (b.download() for b in (xb, yb, pb, cb, ob, ab, ob2, ab2))
    for b in (xb, yb, pb, cb, ob, ab, ob2, ab2):
        b.free()
    what = (T, R, G, n, fill, tile_opt)
    assert np.array_equal(got, got2) and np.array_equal(gotA, gotA2), (what, "differs from n_out calls of hm_inner_product_lintrans")
    # reference: per rotation the key product of the rotated digits (MUL, MAC_ADD), ONCE, then every output's weighted sums over the rotations
    terms = [[], []]
    for r, g in enumerate(galois):
        rx = [o.automorph_eval(np.stack([X[xl[i * T + j]] for i in range(n)]), g) for j in range(T)]
        for k in range(2):
            key = lambda j: np.stack([Y[yl[((r * n + i) * 2 + k) * T + j]] for i in range(n)])
            acc = o.ewe(EWE_MUL, mods, rx[0], key(0))
            for j in range(1, T):
                acc = o.ewe(EWE_MAC_ADD, mods, rx[j], key(j), acc)
            terms[k].append(acc)
    if adds:
        amods = [mods[i] for i in adds]
        c0 = np.stack([Cs[cl[i]] for i in adds])
        rc0 = [o.automorph_eval(c0, g) for g in galois]
    for m in range(G):
        pts = [np.stack([P[pl[(m * R + r) * n + i]] for i in range(n)]) for r in range(R)]
        for k in range(2):
            exp = weighted_sum(o, mods, terms[k], pts)
            assert np.array_equal(got[[ol[(m * n + i) * 2 + k] for i in range(n)]], exp), (what, "output", m, "key", k)
        if adds:
            exp = weighted_sum(o, amods, rc0, [p[adds] for p in pts])
            assert np.array_equal(gotA[[al[m * n + i] for i in adds]], exp), (what, "output", m, "addend")
    assert np.all(got[operm[G * 2 * n]] == GUARD) and np.all(gotA[aperm[G * len(adds)]] == GUARD), "a guard limb-poly was written"
    if fill == "zero":
        assert not got[ol].any()


def elements(logN, R):
    twoN = 2 << logN
    return {1: [3], 3: [5, twoN - 1, twoN - 3]}.get(R) or [pow(5, r, twoN) for r in range(1, R + 1)]


@pytest.mark.parametrize("chain", CHAINS)
@pytest.mark.parametrize("T", [1, 2, 3, 4])
def test_kernel_against_the_oracle_and_the_single_sum_kernel(envs, chain, T):
    """digits 1..4 x rotations 1 / 3 / 16 (elements 3; 5, 2N - 1, 2N - 3; 5^r) x outputs 1 / TILE + 1 / 16, 7 entries with repeated moduli, with
    the addend on every second entry"""
    ctx, o = envs(13, chain)
    rng = np.random.default_rng(T)
    for R in (1, 3, 16):
        for G in (1, tile() + 1, 16):
            mods = [int(x) for x in rng.integers(0, NQ + NP, 7)]
            run_kernel_case(ctx, o, mods, T, elements(13, R), G, 100 * T + R + 1000 * G, add_mask=[i % 2 == 0 for i in range(7)])


@pytest.mark.parametrize("chain", CHAINS)
@pytest.mark.parametrize("tile_opt", [2, 4])
def test_kernel_both_tile_sizes_at_their_boundaries(envs, chain, tile_opt):
    """the two built tile sizes (hm_set_option ip_multi_tile) at a full tile, one more and one fewer"""
    ctx, o = envs(13, chain)
    for G in (tile_opt - 1, tile_opt, tile_opt + 1, 2 * tile_opt + 1):
        run_kernel_case(ctx, o, [0, NQ, 3, NQ + NP - 1], 3, elements(13, 3), G, 50 + G, add_mask=[True, False, True, False], tile_opt=tile_opt)


@pytest.mark.parametrize("chain", CHAINS)
@pytest.mark.parametrize("fill", ["q-1", "zero"])
def test_kernel_worst_case_operands(envs, chain, fill):
    """16 outputs over 16 rotations of 4 digits with every operand q - 1: the largest value the 128-bit accumulators and the wide reduction ever
    see; and all zeros"""
    ctx, o = envs(13, chain)
    run_kernel_case(ctx, o, [0, NQ + NP - 1, 3], 4, elements(13, 16), 16, 7, add_mask=[True, False, True], fill=fill)


@pytest.mark.parametrize("chain", CHAINS)
@pytest.mark.parametrize("n", [1, 65, 130])
def test_kernel_entry_counts(envs, chain, n):
    ctx, o = envs(13, chain)
    mods = [i % (NQ + NP) for i in range(n)]
    run_kernel_case(ctx, o, mods, 2, elements(13, 3), tile() + 1, 40 + n, add_mask=[m < NQ for m in mods], y_rot_cap=2)


def test_kernel_without_any_addend(envs):
    ctx, o = envs(13, "mont32")
    run_kernel_case(ctx, o, [NQ, NQ + 1, NQ + 2], 3, elements(13, 3), tile() + 1, 9, add_mask=[False] * 3)


@pytest.mark.parametrize("chain", CHAINS)
def test_kernel_at_n_2_16(envs, chain):
    ctx, o = envs(16, chain)
    run_kernel_case(ctx, o, [0, 5, NQ, 5, 2], 3, elements(16, 4), tile() + 1, 16, add_mask=[True, True, False, True, True])


def _alias_call(ctx, big, out=60, addend_out=80):
    """n = 4 entries of 2 digits, one rotation, 2 outputs, in ONE allocation, each operand through a base pointer of its own: digits limbs 0..7,
    keys 16..31, plaintexts 32..39, addend sources 40..43; outputs from limb `out` (16 limb-polys) and `addend_out` (8)"""
    at = lambda limb: types.SimpleNamespace(ptr=big.limb_ptr(limb))
    n, T, G = 4, 2, 2
    ctx.inner_product_lintrans_multi(big, list(range(n * T)), at(16), list(range(n * 2 * T)), at(32), list(range(G * n)), at(out),
                                     list(range(G * 2 * n)), [0] * n, T, [5], G, addend=at(40), addend_limbs=list(range(n)),
                                     addend_out=at(addend_out), addend_out_limbs=list(range(G * n)))


@pytest.mark.parametrize("where,what", [({"out": 5}, "digit"), ({"out": 30}, "key"), ({"out": 37}, "plaintext"), ({"out": 42}, "addend source"),
                                        ({"addend_out": 6}, "addend output.*digit"), ({"addend_out": 38}, "addend output.*plaintext"),
                                        ({"addend_out": 70}, "two output"), ({"out": 75}, "two output")])
def test_refuses_an_output_over_an_input_or_another_output_through_another_base_pointer(where, what):
    from homulator_amd import hip
    ctx = hip.Context(13, NQ, NP)
    big = ctx.alloc(96)
    ctx.fill_uniform(big, [0] * 96, 5)
    _alias_call(ctx, big)                                   # disjoint: accepted
    with pytest.raises(hip.HmError, match=what):
        _alias_call(ctx, big, **where)
    ctx.close()


def test_refuses_bad_arguments():
    from homulator_amd import hip
    ctx = hip.Context(13, NQ, NP)
    b = ctx.alloc(128)

    def call(T, g, G=1, xl=None, mods=None, ol=None, **kw):
        R = len(g)
        ctx.inner_product_lintrans_multi(b, xl or list(range(T)), b, list(range(8, 8 + 2 * T * R)), b, list(range(50, 50 + G * R)), b,
                                         ol or list(range(90, 90 + 2 * G)), mods or [0], T, g, G, **kw)
    call(1, [5], 2)                                          # accepted
    with pytest.raises(hip.HmError, match="n_terms"):
        call(5, [5])
    with pytest.raises(hip.HmError, match="n_rot"):
        ctx.inner_product_lintrans_multi(b, [0], b, list(range(8, 42)), b, list(range(50, 67)), b, [90, 91], [0], 1,
                                         [pow(5, r, 1 << 14) for r in range(1, 18)], 1)
    with pytest.raises(hip.HmError, match="n_out"):
        call(1, [5], 0)
    with pytest.raises(hip.HmError, match="n_out"):
        call(1, [5], 17, ol=list(range(90, 124)))
    with pytest.raises(hip.HmError, match="odd"):
        call(1, [4])
    with pytest.raises(hip.HmError, match="odd"):
        call(1, [(2 << 13) + 1])
    with pytest.raises(hip.HmError, match="65535"):
        call(1, [5], xl=[70000])
    with pytest.raises(hip.HmError, match="mod id"):
        call(1, [5], mods=[NQ + NP])
    with pytest.raises(hip.HmError, match="null"):
        call(1, [5], addend_limbs=[60])                      # an addend list without its buffers
    with pytest.raises(hip.HmError, match="null"):
        call(1, [5], addend=b)                               # an addend source without addend outputs
    with pytest.raises(hip.HmError, match="two output"):
        call(1, [5], 2, ol=[90, 91, 92, 90])                 # two outputs share a limb-poly
    ctx.close()


# ============================================================================================================================
# B. the op
# ============================================================================================================================
def read_out(op, copy=0):
    return op.read("out.c0", copy=copy), op.read("out.c1", copy=copy)


def assert_ct(got, exp, what):
    assert np.array_equal(got[0], exp[0]), (what, "c0")
    assert np.array_equal(got[1], exp[1]), (what, "c1")


def kind_counts(op):
    kinds = [ln.split()[0] for ln in op.plan()]
    return {k: kinds.count(k) for k in ("IP_LINTRANS_MULTI", "IP_ROTSUM", "IP_LINTRANS", "IP_HOISTED", "AUTO")}


def reference(o, ell, R, G, g=5, h=None, seed=SEED, copy=0):
    from bsgs_ref import bsgs, synthetic_inputs
    ct, baby, giant, pts = synthetic_inputs(o, ell, R, G, seed, copy=copy)
    return bsgs(o, ell, ct, g, h or pow(g, R, 2 * o.N), baby, giant, pts)


def check_op(chain, cfg, logN, L, ell, alpha, R, G, batch, merged, extra=None, counts=None):
    o = oracle(logN, L, alpha, chain, threads=16)
    ov = chain_ov(chain, dict({"rotations": R, "giants": G, "galois": 5, "batch": batch, "N": 1 << logN}, **(extra or {})))
    got = {}
    for fuse in (True, False):
        op = host.Op(cfg, "hbsgs", L, ell, alpha, fuse=fuse, overrides=ov)
        op.execute(1)
        got[fuse] = [read_out(op, c) for c in range(batch)]
        c = kind_counts(op)
        if not fuse:
            assert c["IP_LINTRANS_MULTI"] == c["IP_ROTSUM"] == c["IP_LINTRANS"] == c["IP_HOISTED"] == 0 and c["AUTO"] > 0, c
        elif counts is not None:
            assert c == counts, c
        elif merged:
            assert c == {"IP_LINTRANS_MULTI": 1, "IP_ROTSUM": 1, "IP_LINTRANS": 0, "IP_HOISTED": 0, "AUTO": 0}, c
        else:
            assert c["IP_LINTRANS_MULTI"] == c["IP_ROTSUM"] == 0, c
        op.close()
    for c in range(batch):
        exp = reference(o, ell, R, G, copy=c)
        assert_ct(got[True][c], exp, ("fused", c))
        assert_ct(got[False][c], exp, ("unfused", c))


@pytest.mark.parametrize("chain", CHAINS)
@pytest.mark.parametrize("R,G", [(2, 2), (3, 4)])
@pytest.mark.parametrize("ell,alpha,merged", [(13, 13, True), (10, 5, True), (7, 3, True), (12, 3, True), (11, 2, False)],
                         ids=["beta1", "beta2", "beta3-one-limb-last", "beta4", "beta6-fallback"])
def test_op_fused_unfused_and_reference_agree(chain, ell, alpha, merged, R, G):
    """points of the 13-limb grid at N = 2^13: every digit count the merged launches take, a one-limb last digit, and the route without them"""
    check_op(chain, "config_4_N15.cfg", 13, 13, ell, alpha, R, G, 1, merged)


@pytest.mark.parametrize("chain", CHAINS)
def test_op_config_1_batch_3(chain):
    check_op(chain, "config_4_N15.cfg", 15, 16, 10, 4, 2, 3, 3, True)


def test_op_with_fuse_bsgs_off():
    """the baby key products as one hoisted launch, element-wise weighted sums, the giant step still merged: the same ciphertext"""
    check_op("mont32", "config_4_N15.cfg", 13, 13, 7, 3, 3, 2, 1, False, extra={"fuse_bsgs": 0},
             counts={"IP_LINTRANS_MULTI": 0, "IP_ROTSUM": 1, "IP_LINTRANS": 0, "IP_HOISTED": 1, "AUTO": 3})


@pytest.mark.parametrize("chain", CHAINS)
def test_one_giant_step_equals_hlintrans_then_a_hoisted_rotation(chain):
    """G = 1: hlintrans, then hrotate_hoisted with rotations = 1, galois = h, under the giant key"""
    R, h = 3, 125
    ov = chain_ov(chain, {"galois": 5, "N": 1 << 13})
    a = host.Op("config_4_N15.cfg", "hbsgs", 13, 7, 3, overrides=dict(ov, rotations=R, giants=1))
    assert kind_counts(a) == {"IP_LINTRANS_MULTI": 0, "IP_ROTSUM": 0, "IP_LINTRANS": 1, "IP_HOISTED": 1, "AUTO": 0}
    a.execute(1)
    lin = host.Op("config_4_N15.cfg", "hlintrans", 13, 7, 3, overrides=dict(ov, rotations=R))
    lin.execute(1)
    rot = host.Op("config_4_N15.cfg", "hrotate_hoisted", 13, 7, 3, overrides=dict(ov, rotations=1, galois=h))
    rot.write("ct1.c0", lin.read("out.c0"))
    rot.write("ct1.c1", lin.read("out.c1"))
    for j in range(3):
        for k in range(2):
            rot.write(f"IP_Rot1_Key{k}_{j}", a.read(f"IP_Giant1_Key{k}_{j}"))
    rot.execute(1)
    assert_ct(read_out(a), (rot.read("out1.c0"), rot.read("out1.c1")), "G = 1")
    for op in (a, lin, rot):
        op.close()


@pytest.mark.parametrize("chain", CHAINS)
def test_equals_g_hlintrans_ops_and_one_hrotsum_op(chain):
    """the composition the op replaces, run on the GPU: op i = hlintrans on ct1 with the plaintexts pt_{i,.} (same baby keys under the same seed),
    then one hrotsum of the G outputs with galois = h under the giant keys.  Bit for bit."""
    R, G, ell, alpha, beta = 3, 4, 7, 3, 3
    h = pow(5, R, 2 << 13)
    ov = chain_ov(chain, {"galois": 5, "N": 1 << 13})
    a = host.Op("config_4_N15.cfg", "hbsgs", 13, ell, alpha, overrides=dict(ov, rotations=R, giants=G))
    a.execute(1)
    lin = host.Op("config_4_N15.cfg", "hlintrans", 13, ell, alpha, overrides=dict(ov, rotations=R))
    rs = host.Op("config_4_N15.cfg", "hrotsum", 13, ell, alpha, overrides=dict(ov, rotations=G, galois=h))
    for i in range(1, G + 1):
        for r in range(1, R + 1):
            lin.write(f"pt{r}", a.read(f"pt{(i - 1) * R + r}"))
        lin.execute(1)
        rs.write(f"ct{i}.c0", lin.read("out.c0"))
        rs.write(f"ct{i}.c1", lin.read("out.c1"))
        for j in range(beta):
            for k in range(2):
                rs.write(f"IP_Rot{i}_Key{k}_{j}", a.read(f"IP_Giant{i}_Key{k}_{j}"))
    rs.execute(1)
    assert_ct(read_out(a), read_out(rs), "hbsgs against G hlintrans + hrotsum")
    for op in (a, lin, rs):
        op.close()


def test_bench_shape_largest_batch_graph_replay():
    """config_4.cfg 45/35/15, R = G = 4 at the largest batch the 16-bit limb index allows (12 950 limb-polys per op: 5 ops), the plan captured into
    a HIP graph (run 1 direct, run 2 captures, run 3 replays): the first and the last copy of the batch after the replay"""
    cfg, logN, L, ell, alpha, R, G, B = "config_4.cfg", 16, 45, 35, 15, 4, 4, 5
    o = oracle(logN, L, alpha, threads=16)
    op = host.Op(cfg, "hbsgs", L, ell, alpha, overrides={"rotations": R, "giants": G, "batch": B, "graph": 1})
    merged = [ln for ln in op.plan() if ln.startswith("IP_LINTRANS_MULTI")]
    assert len(merged) == 1 and f" n={B * (ell + alpha)} " in merged[0] and f" out={G} addend={B * ell}" in merged[0] and op.launch_count() == 14
    for _ in range(3):
        op.execute(1)
    for c in (0, B - 1):
        assert_ct(read_out(op, c), reference(o, ell, R, G, copy=c), f"copy {c}")
    op.close()


# ============================================================================================================================
# C. in a chain
# ============================================================================================================================
def test_middle_link_of_a_chain():
    """hmult,hbsgs,hadd at N = 2^15 against the same sequence of reference calls.  Link k runs under seed + 31 k (OpChain): its keys, plaintexts
    and second operand are drawn from there, its first operand is the link before's output."""
    from bsgs_ref import bsgs, synthetic_inputs
    L, ell, alpha, R, G = 6, 5, 2, 2, 2
    o = oracle(15, L, alpha)
    chain = host.Chain("config_4_N15.cfg", "hmult,hbsgs,hadd", L, ell, alpha, overrides={"rotations": R, "giants": G})
    chain.execute(1)
    a = o.hmult(ell, o.synth_ct(ell, SEED), o.synth_ct(ell, SEED + 2000), o.synth_evk(ell, SEED + 10000))
    _, baby, giant, pts = synthetic_inputs(o, ell - 1, R, G, SEED + 31)
    b = bsgs(o, ell - 1, np.stack(a), 5, pow(5, R, 2 * o.N), baby, giant, pts)
    c = o.hadd(ell - 1, np.stack(b), o.synth_ct(ell - 1, SEED + 62 + 2000))
    assert kind_counts(chain[1]) == {"IP_LINTRANS_MULTI": 1, "IP_ROTSUM": 1, "IP_LINTRANS": 0, "IP_HOISTED": 0, "AUTO": 0}
    assert_ct(read_out(chain[0]), a, "hmult")
    assert_ct(read_out(chain[1]), b, "hbsgs")
    assert_ct(read_out(chain[2]), c, "hadd")
    chain.close()


# ============================================================================================================================
# D. real data
# ============================================================================================================================
def test_real_data_decrypts_to_the_baby_step_giant_step_transform():
    """m encrypted as in tests/test_gpu_lintrans.py; plaintexts: integer polynomials of 8 non-zero coefficients of magnitude <= 2^10, reduced
    modulo each of the E moduli and transformed.  dec(out) = sum_i sigma_{h_i}(sum_r p_{i,r} * sigma_{g_r}(m)) in Z[X] / (X^N + 1) within
    G * (R * 8 * 2^10 * 2^16 + 2^16): hlintrans's bound per inner sum (tests/test_gpu_lintrans.py), which a rotation preserves, plus hrotate's
    2^16 per giant step (tests/test_gpu_real_data.py).  The reference's own output is held to that bound on the CPU before the GPU runs."""
    from bsgs_ref import bsgs
    from toy_ckks import Toy
    LOGN, L, ELL, ALPHA, R, G, g = 13, 6, 5, 2, 3, 2, 5
    BOUND = G * (R * 8 * (1 << 10) * (1 << 16) + (1 << 16))
    o = oracle(LOGN, L, ALPHA)
    twoN = 2 * o.N
    h = pow(g, R, twoN)
    toy = Toy(o, seed=4243)
    m = toy.rng.integers(-1000, 1000, o.N).astype(object) * (1 << 30)
    ct = toy.encrypt(m, ELL)
    ids = o.ext_ids(ELL)
    baby = [toy.evk_at_level(toy.gen_evk(toy.automorph(toy.s, pow(g, r, twoN))), ELL) for r in range(1, R + 1)]
    giant = [toy.evk_at_level(toy.gen_evk(toy.automorph(toy.s, pow(h, i, twoN))), ELL) for i in range(1, G + 1)]
    pts = []
    exp = np.zeros(o.N, dtype=object)
    for i in range(1, G + 1):
        inner = np.zeros(o.N, dtype=object)
        row = []
        for r in range(1, R + 1):
            p = np.zeros(o.N, dtype=object)
            for x in toy.rng.choice(o.N, 8, replace=False):
                p[int(x)] = int(toy.rng.integers(-(1 << 10), (1 << 10) + 1))
            row.append(toy.to_rns_eval(p, ids))
            inner = inner + toy.negacyclic_mul(p, toy.automorph(m, pow(g, r, twoN)))
        pts.append(row)
        exp = exp + toy.automorph(inner, pow(h, i, twoN))
    err = lambda out: max(abs(int(a) - int(b)) for a, b in zip(toy.decrypt(np.stack(out), ELL)[0], exp))
    ref = bsgs(o, ELL, ct, g, h, baby, giant, pts)
    ref_err = err(ref)
    print(f"reference: max |dec - exact| = {ref_err} (bound {BOUND})")
    assert ref_err < BOUND
    op = host.Op("config_4_N15.cfg", "hbsgs", L, ELL, ALPHA, overrides={"N": 1 << LOGN, "rotations": R, "giants": G, "galois": g})
    op.write("ct1.c0", ct[0])
    op.write("ct1.c1", ct[1])
    for i in range(G):
        for r in range(R):
            op.write(f"pt{i * R + r + 1}", pts[i][r])
    for name, keys in (("Rot", baby), ("Giant", giant)):
        for x, key in enumerate(keys, 1):
            for j in range(key.shape[0]):
                for k in range(2):
                    op.write(f"IP_{name}{x}_Key{k}_{j}", key[j][k])
    op.execute(1)
    out = read_out(op)
    op.close()
    gpu_err = err(out)
    print(f"GPU: max |dec - exact| = {gpu_err} (bound {BOUND})")
    assert gpu_err < BOUND
    assert_ct(out, ref, "real data")
