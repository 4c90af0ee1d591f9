"""hrotsum on the GPU, on both arithmetic back-ends (mont32 and chain_bits = 60), bit for bit:
 A. hm_inner_product_rotsum against the oracle's automorphism, MUL / MAC_ADD per ciphertext and ADD chains, on permuted limb lists with guard
    limb-polys, and its refusals, of outputs that overlap an input through another base pointer among them;
 B. the op, fused (one IP_ROTSUM launch) and unfused (one launch per stage), against tests/rotsum_ref.py;
 C. the op as the middle link of a chain;
 D. on real data (tests/toy_ckks.py) out decrypts to sum_i sigma_i(m_i)."""
import types

import numpy as np
import pytest

from homulator_amd import host
from oracle.homoracle import EWE_MAC_ADD, EWE_MUL, Oracle, chain_below

pytestmark = pytest.mark.gpu
CHAINS = ["mont32", "survey"]
SEED = host.SEED
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


def run_kernel_case(ctx, o, mods, T, galois, seed, add_mask, fill="uniform", pool_cap=None):
    """one hm_inner_product_rotsum call; every limb list is a random permutation of its buffer, the two output buffers keep one guard limb-poly
    each.  add_mask[i]: entry i carries addend sources.  fill: "uniform" (device fill), "q-1" or "zero" (every operand).  pool_cap bounds the
    digit, key and addend pools: ciphertext c reads the limbs of ciphertext c mod cap.  Checks every output against the oracle and the guards."""
    from homulator_amd import hip
    from rotsum_ref import add_chain
    n, G, N = len(mods), len(galois), ctx.N
    rng = np.random.default_rng(seed)
    Gp = min(G, pool_cap or G)
    adds = [i for i in range(n) if add_mask[i]]
    nx, ny, nc, no, na = Gp * n * T, Gp * n * 2 * T, max(1, Gp * len(adds)), 2 * n + 1, len(adds) + 1
    xb, yb, cb, ob, ab = (ctx.alloc(k) for k in (nx, ny, nc, no, na))
    xpool, ypool, cperm, operm, aperm = ([int(v) for v in rng.permutation(k)] for k in (nx, ny, nc, no, na))
    xl = [xpool[e % nx] for e in range(G * n * T)]
    yl = [ypool[e % ny] for e in range(G * n * 2 * T)]
    ol = operm[:2 * n]
    cl = [hip.NO_LIMB] * (G * n)
    al = [hip.NO_LIMB] * n
    for t, i in enumerate(adds):
        al[i] = aperm[t]
        for c in range(G):
            cl[c * n + i] = cperm[(c % Gp) * len(adds) + t]
    xm = {xl[(c * n + i) * T + j]: mods[i] for c in range(G) for i in range(n) for j in range(T)}
    ym = {yl[((c * n + i) * 2 + k) * T + j]: mods[i] for c in range(G) for i in range(n) for k in range(2) for j in range(T)}
    cm = {cl[c * n + i]: mods[i] for c in range(G) for i in adds} or {0: 0}
    for buf, m in ((xb, xm), (yb, ym), (cb, cm)):
        if fill == "uniform":
            ctx.fill_uniform(buf, [m[k] for k in sorted(m)], seed * 11 + len(m), out_limbs=sorted(m))
        else:
            buf.upload(np.stack([np.full(N, ctx.moduli[m[k]] - 1 if fill == "q-1" else 0, dtype=np.uint64) for k in sorted(m)]))
    ob.upload(np.full((no, N), GUARD, dtype=np.uint64))
    ab.upload(np.full((na, N), GUARD, dtype=np.uint64))
    ctx.inner_product_rotsum(xb, xl, yb, yl, ob, ol, mods, T, galois,
                             addend=cb if adds else None, addend_limbs=cl if adds else None, addend_out=ab if adds else None,
                             addend_out_limbs=al if adds else None)
    X, Y, Cs, got, gotA = (b.download() for b in (xb, yb, cb, ob, ab))
    for b in (xb, yb, cb, ob, ab):
        b.free()
    # reference: per ciphertext the key product of its rotated digits (MUL, MAC_ADD), then the ADD chains over the ciphertexts
    terms = [[], []]
    for c, g in enumerate(galois):
        rx = [o.automorph_eval(np.stack([X[xl[(c * n + i) * T + j]] for i in range(n)]), g) for j in range(T)]
        for k in range(2):
            key = lambda j: np.stack([Y[yl[((c * n + i) * 2 + k) * T + j]] for i in range(n)])
            acc = o.ewe(EWE_MUL, mods, rx[0], key(0))
            for j in range(1, T):
                acc = o.ewe(EWE_MAC_ADD, mods, rx[j], key(j), acc)
            terms[k].append(acc)
    for k in range(2):
        exp = add_chain(o, mods, terms[k])
        assert np.array_equal(got[[ol[i * 2 + k] for i in range(n)]], exp), (T, G, n, fill, "key", k)
    if adds:
        amods = [mods[i] for i in adds]
        exp = add_chain(o, amods, [o.automorph_eval(np.stack([Cs[cl[c * n + i]] for i in adds]), g) for c, g in enumerate(galois)])
        assert np.array_equal(gotA[[al[i] for i in adds]], exp), (T, G, n, fill, "addend")
    assert np.all(got[operm[2 * n]] == GUARD) and np.all(gotA[aperm[len(adds)]] == GUARD), "a guard limb-poly was written"
    if fill == "zero":
        assert not got[ol].any()


def elements(logN, G):
    twoN = 2 << logN
    return {1: [3], 3: [5, twoN - 1, twoN - 3]}.get(G) or [pow(5, c, twoN) for c in range(1, G + 1)]


@pytest.mark.parametrize("chain", CHAINS)
@pytest.mark.parametrize("T", [1, 2, 3, 4])
def test_kernel_against_the_oracle(envs, chain, T):
    """digits 1..4 x ciphertexts 1 / 3 / 16 (elements 3; 5, 2N - 1, 2N - 3; 5^c), 7 entries with repeated moduli, an addend on some entries"""
    ctx, o = envs(13, chain)
    rng = np.random.default_rng(T)
    for G in (1, 3, 16):
        mods = [int(x) for x in rng.integers(0, NQ + NP, 7)]
        run_kernel_case(ctx, o, mods, T, elements(13, G), 100 * T + G, add_mask=[i % 2 == 0 for i in range(7)])


@pytest.mark.parametrize("chain", CHAINS)
@pytest.mark.parametrize("fill", ["q-1", "zero"])
def test_kernel_worst_case_operands(envs, chain, fill):
    """16 ciphertexts of 4 digits with every operand q - 1: 64 (q - 1)^2 in every 128-bit accumulator, 16 (q - 1) in the addend's; and all zeros"""
    ctx, o = envs(13, chain)
    run_kernel_case(ctx, o, [0, NQ + NP - 1, 3], 4, elements(13, 16), 7, add_mask=[True, False, True], fill=fill)


@pytest.mark.parametrize("chain", CHAINS)
@pytest.mark.parametrize("n", [1, 65, 130])
def test_kernel_entry_counts(envs, chain, n):
    """one grid and one record table whatever the entry count"""
    ctx, o = envs(13, chain)
    mods = [i % (NQ + NP) for i in range(n)]
    run_kernel_case(ctx, o, mods, 2, elements(13, 3), 40 + n, add_mask=[m < NQ for m in mods], pool_cap=2)


@pytest.mark.parametrize("add", [False, True])
def test_kernel_with_and_without_addend(envs, add):
    ctx, o = envs(13, "mont32")
    run_kernel_case(ctx, o, [NQ, NQ + 1, 2], 3, elements(13, 3), 9, add_mask=[add] * 3)


def test_kernel_two_ciphertexts_under_the_same_element(envs):
    ctx, o = envs(13, "mont32")
    run_kernel_case(ctx, o, [1, 4, NQ], 2, [25, 5, 25], 10, add_mask=[True, True, False])


@pytest.mark.parametrize("chain", CHAINS)
def test_kernel_at_n_2_16(envs, chain):
    ctx, o = envs(16, chain)
    run_kernel_case(ctx, o, [0, 5, NQ, 5, 2], 3, elements(16, 4), 16, add_mask=[True, True, False, True, True])


def _alias_call(ctx, big, out=44, addend_out=52, out_limbs=None, addend_out_limbs=None):
    """n = 4 entries of 2 digits, one ciphertext, in ONE allocation, each operand through a base pointer of its own: digits limbs 0..7, keys
    16..31, addend sources 36..39; outputs from limb `out` (8 limb-polys) and `addend_out` (4)"""
    at = lambda limb: types.SimpleNamespace(ptr=big.limb_ptr(limb))
    n, T = 4, 2
    ctx.inner_product_rotsum(big, list(range(n * T)), at(16), list(range(n * 2 * T)), at(out), out_limbs or list(range(2 * n)),
                             [0] * n, T, [5], addend=at(36), addend_limbs=list(range(n)), addend_out=at(addend_out),
                             addend_out_limbs=addend_out_limbs or list(range(n)))


@pytest.mark.parametrize("where,what", [({"out": 5}, "digit"), ({"out": 30}, "key"), ({"out": 38}, "addend source"),
                                        ({"addend_out": 6}, "addend output.*digit"), ({"addend_out": 30}, "addend output.*key"),
                                        ({"addend_out": 50}, "overlaps an addend output"), ({"out_limbs": [0, 1, 2, 3, 4, 5, 6, 0]}, "the same"),
                                        ({"addend_out_limbs": [0, 1, 1, 2]}, "the same")])
def test_refuses_an_output_over_an_input_or_another_output(where, what):
    """by address range, through another base pointer too"""
    from homulator_amd import hip
    ctx = hip.Context(13, NQ, NP)
    big = ctx.alloc(64)
    ctx.fill_uniform(big, [0] * 64, 5)
    _alias_call(ctx, big)                                   # disjoint: accepted
    with pytest.raises(hip.HmError, match=what):
        _alias_call(ctx, big, **where)
    ctx.close()


def test_refuses_bad_arguments():
    from homulator_amd import hip
    ctx = hip.Context(13, NQ, NP)
    b = ctx.alloc(80)
    call = lambda T, g, xl=None, mods=None, **kw: ctx.inner_product_rotsum(b, xl or list(range(T * len(g))), b, list(range(8, 8 + 2 * T * len(g))), b,
                                                                          [70, 71], mods or [0], T, g, **kw)
    with pytest.raises(hip.HmError, match="n_terms"):
        call(5, [5])
    with pytest.raises(hip.HmError, match="n_ct"):
        call(1, [pow(5, c, 1 << 14) for c in range(1, 18)])
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
    with pytest.raises(hip.HmError, match="some ciphertexts only"):
        call(1, [5, 25], addend=b, addend_limbs=[60, hip.NO_LIMB], addend_out=b, addend_out_limbs=[72])
    call(1, [5, 5])                                          # two ciphertexts under one element: accepted
    ctx.close()


# ============================================================================================================================
# B. the op
# ============================================================================================================================
def read_out(op, copy=0):
    return op.read("out.c0", copy=copy), op.read("out.c1", copy=copy)


def assert_ct(got, exp, what):
    assert np.array_equal(got[0], exp[0]), (what, "c0")
    assert np.array_equal(got[1], exp[1]), (what, "c1")


def check_op(chain, cfg, logN, L, ell, alpha, G, batch, merged, extra=None):
    from rotsum_ref import rotsum, synthetic_inputs
    o = oracle(logN, L, alpha, chain, threads=16)
    ov = chain_ov(chain, dict({"rotations": G, "galois": 5, "batch": batch, "N": 1 << logN}, **(extra or {})))
    got = {}
    for fuse in (True, False):
        op = host.Op(cfg, "hrotsum", L, ell, alpha, fuse=fuse, overrides=ov)
        op.execute(1)
        got[fuse] = [read_out(op, c) for c in range(batch)]
        assert [ln.split()[0] for ln in op.plan()].count("IP_ROTSUM") == (1 if fuse and merged else 0)
        op.close()
    for c in range(batch):
        cts, keys = synthetic_inputs(o, ell, G, SEED, copy=c)
        exp = rotsum(o, ell, cts, 5, keys)
        assert_ct(got[True][c], exp, ("fused", c))
        assert_ct(got[False][c], exp, ("unfused", c))


@pytest.mark.parametrize("chain", CHAINS)
@pytest.mark.parametrize("G", [2, 4])
@pytest.mark.parametrize("ell,alpha,merged", [(13, 13, True), (10, 5, True), (7, 3, True), (12, 3, True), (11, 2, False)],
                         ids=["beta1", "beta2", "beta3-one-limb-last", "beta4", "beta6-fallback"])
def test_op_fused_unfused_and_reference_agree(chain, ell, alpha, merged, G):
    """points of the 13-limb grid at N = 2^13: every digit count the merged launch takes, a one-limb last digit, and the route without it"""
    check_op(chain, "config_4_N15.cfg", 13, 13, ell, alpha, G, 1, merged)


@pytest.mark.parametrize("chain", CHAINS)
def test_op_config_1_batch_3(chain):
    check_op(chain, "config_4_N15.cfg", 15, 16, 10, 4, 3, 3, True)


def test_op_with_fuse_rotsum_off():
    """single-rotation hoisted key products and element-wise sums: the same ciphertext"""
    check_op("mont32", "config_4_N15.cfg", 13, 13, 7, 3, 3, 1, False, extra={"fuse_rotsum": 0})


@pytest.mark.parametrize("chain", CHAINS)
def test_one_ciphertext_equals_the_hoisted_rotation(chain):
    ov = chain_ov(chain, {"rotations": 1, "galois": 5, "N": 1 << 13})
    outs = {}
    for name, out in (("hrotsum", "out"), ("hrotate_hoisted", "out1")):
        op = host.Op("config_4_N15.cfg", name, 13, 7, 3, overrides=ov)
        op.execute(1)
        outs[name] = (op.read(out + ".c0"), op.read(out + ".c1"))
        op.close()
    assert_ct(outs["hrotsum"], outs["hrotate_hoisted"], "G = 1")


def test_bench_shape_batch_10_graph_replay():
    """config_4.cfg 45/35/15, 10 ops per launch, 4 ciphertexts, the plan captured into a HIP graph (run 1 direct, run 2 captures, run 3 replays):
    copies 0 and 9 of the batch after the replay"""
    from rotsum_ref import rotsum, synthetic_inputs
    cfg, logN, L, ell, alpha, G, B = "config_4.cfg", 16, 45, 35, 15, 4, 10
    o = oracle(logN, L, alpha, threads=16)
    op = host.Op(cfg, "hrotsum", L, ell, alpha, overrides={"rotations": G, "batch": B, "graph": 1})
    merged = [ln for ln in op.plan() if ln.startswith("IP_ROTSUM")]
    assert len(merged) == 1 and f" n={B * (ell + alpha)} " in merged[0] and op.launch_count() == 7
    for _ in range(3):
        op.execute(1)
    for c in (0, 9):
        cts, keys = synthetic_inputs(o, ell, G, SEED, copy=c)
        assert_ct(read_out(op, c), rotsum(o, ell, cts, 5, keys), f"copy {c}")
    op.close()


# ============================================================================================================================
# C. in a chain
# ============================================================================================================================
def test_middle_link_of_a_chain():
    """hmult,hrotsum,hadd at N = 2^15 against the same sequence of reference calls.  Link k runs under seed + 31 k (OpChain): its keys and its
    further ciphertexts are drawn from there, its first ciphertext is the link before's output."""
    from rotsum_ref import rotsum, synthetic_inputs
    L, ell, alpha, G = 6, 5, 2, 3
    o = oracle(15, L, alpha)
    chain = host.Chain("config_4_N15.cfg", "hmult,hrotsum,hadd", L, ell, alpha, overrides={"rotations": G})
    chain.execute(1)
    a = o.hmult(ell, o.synth_ct(ell, SEED), o.synth_ct(ell, SEED + 2000), o.synth_evk(ell, SEED + 10000))
    cts, keys = synthetic_inputs(o, ell - 1, G, SEED + 31)
    b = rotsum(o, ell - 1, [np.stack(a)] + cts[1:], 5, keys)
    c = o.hadd(ell - 1, np.stack(b), o.synth_ct(ell - 1, SEED + 62 + 2000))
    assert [ln.split()[0] for ln in chain[1].plan()].count("IP_ROTSUM") == 1
    assert_ct(read_out(chain[0]), a, "hmult")
    assert_ct(read_out(chain[1]), b, "hrotsum")
    assert_ct(read_out(chain[2]), c, "hadd")
    chain.close()


# ============================================================================================================================
# D. real data
# ============================================================================================================================
def test_real_data_decrypts_to_the_sum_of_rotations():
    """G = 3 messages encrypted under one secret as in tests/test_gpu_hoisted.py, rotation keys for g, g^2, g^3.  dec(out) = sum_i sigma_i(m_i)
    within G * 2^16: the single-rotation bound of tests/test_gpu_hoisted.py once per ciphertext (the key-switch errors add; the one ModDown rounds
    once, which that bound already holds per rotation).  The reference's own output is held to the same bound on the CPU before the GPU runs."""
    from rotsum_ref import rotsum
    from toy_ckks import Toy
    LOGN, L, ELL, ALPHA, G, g = 13, 6, 5, 2, 3, 5
    BOUND = G * (1 << 16)
    o = oracle(LOGN, L, ALPHA)
    toy = Toy(o, seed=4243)
    ms, cts, keys = [], [], []
    exp = np.zeros(o.N, dtype=object)
    for i in range(1, G + 1):
        m = toy.rng.integers(-1000, 1000, o.N).astype(object) * (1 << 30)
        ms.append(m)
        cts.append(toy.encrypt(m, ELL))
        keys.append(toy.evk_at_level(toy.gen_evk(toy.automorph(toy.s, pow(g, i, 2 * o.N))), ELL))
        exp = exp + toy.automorph(m, pow(g, i, 2 * o.N))
    err = lambda out: max(abs(int(a) - int(b)) for a, b in zip(toy.decrypt(np.stack(out), ELL)[0], exp))
    ref = rotsum(o, ELL, cts, g, keys)
    ref_err = err(ref)
    print(f"reference: max |dec - exact| = {ref_err} (bound {BOUND})")
    assert ref_err < BOUND
    op = host.Op("config_4_N15.cfg", "hrotsum", L, ELL, ALPHA, overrides={"N": 1 << LOGN, "rotations": G, "galois": g})
    for i in range(1, G + 1):
        op.write(f"ct{i}.c0", cts[i - 1][0])
        op.write(f"ct{i}.c1", cts[i - 1][1])
        for j in range(keys[i - 1].shape[0]):
            for k in range(2):
                op.write(f"IP_Rot{i}_Key{k}_{j}", keys[i - 1][j][k])
    op.execute(1)
    out = read_out(op)
    op.close()
    gpu_err = err(out)
    print(f"GPU: max |dec - exact| = {gpu_err} (bound {BOUND})")
    assert gpu_err < BOUND
    assert_ct(out, ref, "real data")
