"""hlintrans on the GPU, on both arithmetic back-ends (mont32 and chain_bits = 60), bit for bit:
 A. hm_inner_product_lintrans against the oracle's automorphism and MUL / MAC_ADD chains, on permuted limb lists with guard limb-polys, and its
    refusals of outputs that overlap an input through another base pointer;
 B. the op, fused (one IP_LINTRANS launch) and unfused (one launch per stage), against tests/lintrans_ref.py;
 C. the op as the middle link of a chain;
 D. on real data (tests/toy_ckks.py) out decrypts to sum_r pt_r * sigma_r(m)."""
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


def run_kernel_case(ctx, o, mods, T, galois, seed, add_mask, fill="uniform", y_rot_cap=None):
    """one hm_inner_product_lintrans call; every limb list is a random permutation of its buffer, the two output buffers keep one guard limb-poly
    each.  add_mask[i]: entry i carries an addend.  fill: "uniform" (device fill), "q-1" or "zero" (every operand).  y_rot_cap bounds the key pool:
    rotation r reads the keys of rotation r mod cap.  Checks every output against the oracle and the guards."""
    from homulator_amd import hip
    from lintrans_ref import weighted_sum
    n, R, N = len(mods), len(galois), ctx.N
    rng = np.random.default_rng(seed)
    Ry = min(R, y_rot_cap or R)
    adds = [i for i in range(n) if add_mask[i]]
    nx, ny, npt, nc, no, na = n * T, Ry * n * 2 * T, R * n, max(1, len(adds)), 2 * n + 1, len(adds) + 1
    xb, yb, pb, cb, ob, ab = (ctx.alloc(k) for k in (nx, ny, npt, nc, no, na))
    xl, ypool, pl, cperm, operm, aperm = ([int(v) for v in rng.permutation(k)] for k in (nx, ny, npt, nc, no, na))
    yl = [ypool[e % ny] for e in range(R * n * 2 * T)]
    ol = operm[:2 * n]
    cl = [hip.NO_LIMB] * n
    al = [hip.NO_LIMB] * n
    for t, i in enumerate(adds):
        cl[i], al[i] = cperm[t], aperm[t]
    xm = {xl[i * T + j]: mods[i] for i in range(n) for j in range(T)}
    ym = {yl[((r * n + i) * 2 + k) * T + j]: mods[i] for r in range(R) for i in range(n) for k in range(2) for j in range(T)}
    pm = {pl[r * n + i]: mods[i] for r in range(R) for i in range(n)}
    cm = {cl[i]: mods[i] for i in adds} or {0: 0}
    for buf, m in ((xb, xm), (yb, ym), (pb, pm), (cb, cm)):
        if fill == "uniform":
            ctx.fill_uniform(buf, [m[k] for k in sorted(m)], seed * 11 + len(m), out_limbs=sorted(m))
        else:
            buf.upload(np.stack([np.full(N, ctx.moduli[m[k]] - 1 if fill == "q-1" else 0, dtype=np.uint64) for k in sorted(m)]))
    ob.upload(np.full((no, N), GUARD, dtype=np.uint64))
    ab.upload(np.full((na, N), GUARD, dtype=np.uint64))
    ctx.inner_product_lintrans(xb, xl, yb, yl, pb, pl, ob, ol, mods, T, galois,
                               addend=cb if adds else None, addend_limbs=cl if adds else None, addend_out=ab if adds else None,
                               addend_out_limbs=al if adds else None)
    X, Y, P, Cs, got, gotA = (b.download() for b in (xb, yb, pb, cb, ob, ab))
    for b in (xb, yb, pb, cb, ob, ab):
        b.free()
    # reference: per rotation the key product of the rotated digits (MUL, MAC_ADD), then the weighted sums over the rotations
    terms = [[], []]
    for r, g in enumerate(galois):
        rx = [o.automorph_eval(np.stack([X[xl[i * T + j]] for i in range(n)]), g) for j in range(T)]
        for k in range(2):
            key = lambda j: np.stack([Y[yl[((r * n + i) * 2 + k) * T + j]] for i in range(n)])
            acc = o.ewe(EWE_MUL, mods, rx[0], key(0))
            for j in range(1, T):
                acc = o.ewe(EWE_MAC_ADD, mods, rx[j], key(j), acc)
            terms[k].append(acc)
    pts = [np.stack([P[pl[r * n + i]] for i in range(n)]) for r in range(R)]
    for k in range(2):
        exp = weighted_sum(o, mods, terms[k], pts)
        assert np.array_equal(got[[ol[i * 2 + k] for i in range(n)]], exp), (T, R, n, fill, "key", k)
    if adds:
        amods = [mods[i] for i in adds]
        c0 = np.stack([Cs[cl[i]] for i in adds])
        exp = weighted_sum(o, amods, [o.automorph_eval(c0, g) for g in galois], [p[adds] for p in pts])
        assert np.array_equal(gotA[[al[i] for i in adds]], exp), (T, R, n, fill, "addend")
    assert np.all(got[operm[2 * n]] == GUARD) and np.all(gotA[aperm[len(adds)]] == GUARD), "a guard limb-poly was written"
    if fill == "zero":
        assert not got[ol].any()


def elements(logN, R):
    twoN = 2 << logN
    return {1: [3], 3: [5, twoN - 1, twoN - 3]}.get(R) or [pow(5, r, twoN) for r in range(1, R + 1)]


@pytest.mark.parametrize("chain", CHAINS)
@pytest.mark.parametrize("T", [1, 2, 3, 4])
def test_kernel_against_the_oracle(envs, chain, T):
    """digits 1..4 x rotations 1 / 3 / 16 (elements 3; 5, 2N - 1, 2N - 3; 5^r), 7 entries with repeated moduli, with and without the addend"""
    ctx, o = envs(13, chain)
    rng = np.random.default_rng(T)
    for R in (1, 3, 16):
        mods = [int(x) for x in rng.integers(0, NQ + NP, 7)]
        run_kernel_case(ctx, o, mods, T, elements(13, R), 100 * T + R, add_mask=[i % 2 == 0 for i in range(7)])


@pytest.mark.parametrize("chain", CHAINS)
@pytest.mark.parametrize("fill", ["q-1", "zero"])
def test_kernel_worst_case_operands(envs, chain, fill):
    """16 rotations of 4 digits with every operand q - 1: the largest value the 128-bit accumulators and the wide reduction ever see; and all zeros"""
    ctx, o = envs(13, chain)
    run_kernel_case(ctx, o, [0, NQ + NP - 1, 3], 4, elements(13, 16), 7, add_mask=[True, False, True], fill=fill)


@pytest.mark.parametrize("chain", CHAINS)
@pytest.mark.parametrize("n", [1, 65, 130])
def test_kernel_entry_counts(envs, chain, n):
    ctx, o = envs(13, chain)
    mods = [i % (NQ + NP) for i in range(n)]
    run_kernel_case(ctx, o, mods, 2, elements(13, 3), 40 + n, add_mask=[m < NQ for m in mods], y_rot_cap=2)


def test_kernel_without_any_addend(envs):
    ctx, o = envs(13, "mont32")
    run_kernel_case(ctx, o, [NQ, NQ + 1, NQ + 2], 3, elements(13, 3), 9, add_mask=[False] * 3)


@pytest.mark.parametrize("chain", CHAINS)
def test_kernel_at_n_2_16(envs, chain):
    ctx, o = envs(16, chain)
    run_kernel_case(ctx, o, [0, 5, NQ, 5, 2], 3, elements(16, 4), 16, add_mask=[True, True, False, True, True])


def _alias_call(ctx, big, out=44, addend_out=52):
    """n = 4 entries of 2 digits, one rotation, in ONE allocation, each operand through a base pointer of its own: digits limbs 0..7, keys
    16..31, plaintexts 32..35, addend sources 36..39; outputs from limb `out` (8 limb-polys) and `addend_out` (4)"""
    at = lambda limb: types.SimpleNamespace(ptr=big.limb_ptr(limb))
    n, T = 4, 2
    ctx.inner_product_lintrans(big, list(range(n * T)), at(16), list(range(n * 2 * T)), at(32), list(range(n)), at(out), list(range(2 * n)),
                               [0] * n, T, [5], addend=at(36), addend_limbs=list(range(n)), addend_out=at(addend_out),
                               addend_out_limbs=list(range(n)))


@pytest.mark.parametrize("where,what", [({"out": 5}, "digit"), ({"out": 30}, "key"), ({"out": 33}, "plaintext"), ({"out": 38}, "addend source"),
                                        ({"addend_out": 6}, "addend output.*digit"), ({"addend_out": 34}, "addend output.*plaintext")])
def test_refuses_an_output_over_an_input_through_another_base_pointer(where, what):
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
    b = ctx.alloc(32)
    call = lambda T, g, xl=None: ctx.inner_product_lintrans(b, xl or list(range(T)), b, list(range(8, 8 + 2 * T * len(g))), b, [20] * len(g), b,
                                                           [30, 31], [0], T, g)
    with pytest.raises(hip.HmError, match="n_terms"):
        call(5, [5])
    with pytest.raises(hip.HmError, match="n_rot"):
        ctx.inner_product_lintrans(b, [0], b, list(range(34)), b, [20] * 17, b, [30, 31], [0], 1, [pow(5, r, 1 << 14) for r in range(1, 18)])
    with pytest.raises(hip.HmError, match="odd"):
        call(1, [4])
    with pytest.raises(hip.HmError, match="odd"):
        call(1, [(2 << 13) + 1])
    with pytest.raises(hip.HmError, match="65535"):
        call(1, [5], xl=[70000])
    ctx.close()


# ============================================================================================================================
# B. the op
# ============================================================================================================================
def keys_and_plaintexts(o, ell, R, seed=SEED):
    """rotation r's key (one for every op of a batch) and, per op c of the batch, its plaintext: the op's synthetic streams"""
    keys = [o.synth_evk(ell, seed + 10000 + 100000 * r) for r in range(1, R + 1)]
    pts = lambda c: [o.fill_uniform(o.ext_ids(ell), seed + 4000 + 100000 * r + c * BATCH_SEED_STRIDE) for r in range(1, R + 1)]
    return keys, pts


def read_out(op, copy=0):
    return op.read("out.c0", copy=copy), op.read("out.c1", copy=copy)


def assert_ct(got, exp, what):
    assert np.array_equal(got[0], exp[0]), (what, "c0")
    assert np.array_equal(got[1], exp[1]), (what, "c1")


@pytest.mark.parametrize("chain", CHAINS)
@pytest.mark.parametrize("cfg,logN,L,ell,alpha,R,batch,merged", [
    ("config_4_N15.cfg", 15, 16, 10, 4, 3, 2, True),
    ("config_4_N15.cfg", 15, 8, 8, 8, 2, 1, True),       # beta = 1
    ("config_4_N15.cfg", 13, 6, 5, 1, 2, 1, False),      # beta = 5: the fallback route (separate launches)
    ("config_4.cfg", 16, 45, 35, 15, 4, 1, True),        # the headline shape
])
def test_op_fused_unfused_and_reference_agree(chain, cfg, logN, L, ell, alpha, R, batch, merged):
    from lintrans_ref import lintrans
    o = oracle(logN, L, alpha, chain, threads=16)
    ov = chain_ov(chain, {"rotations": R, "galois": 5, "batch": batch, "N": 1 << logN})
    got = {}
    for fuse in (True, False):
        op = host.Op(cfg, "hlintrans", L, ell, alpha, fuse=fuse, overrides=ov)
        op.execute(1)
        got[fuse] = [read_out(op, c) for c in range(batch)]
        assert [ln.split()[0] for ln in op.plan()].count("IP_LINTRANS") == (1 if fuse and merged else 0)
        op.close()
    keys, pts = keys_and_plaintexts(o, ell, R)
    for c in range(batch):
        exp = lintrans(o, ell, o.synth_ct(ell, SEED + c * BATCH_SEED_STRIDE), 5, keys, pts(c))
        assert_ct(got[True][c], exp, ("fused", c))
        assert_ct(got[False][c], exp, ("unfused", c))


def test_bench_shape_batch_10_graph_replay():
    """config_4.cfg 45/35/15, 10 ops per launch, 4 rotations, the plan captured into a HIP graph (run 1 direct, run 2 captures, run 3 replays):
    copies 0 and 9 of the batch after the replay"""
    from lintrans_ref import lintrans
    cfg, logN, L, ell, alpha, R, B = "config_4.cfg", 16, 45, 35, 15, 4, 10
    o = oracle(logN, L, alpha, threads=16)
    op = host.Op(cfg, "hlintrans", L, ell, alpha, overrides={"rotations": R, "batch": B, "graph": 1})
    merged = [ln for ln in op.plan() if ln.startswith("IP_LINTRANS")]
    assert len(merged) == 1 and f" n={B * (ell + alpha)} " in merged[0] and op.launch_count() == 7
    for _ in range(3):
        op.execute(1)
    keys, pts = keys_and_plaintexts(o, ell, R)
    for c in (0, 9):
        assert_ct(read_out(op, c), lintrans(o, ell, o.synth_ct(ell, SEED + c * BATCH_SEED_STRIDE), 5, keys, pts(c)), f"copy {c}")
    op.close()


# ============================================================================================================================
# C. in a chain
# ============================================================================================================================
def test_middle_link_of_a_chain():
    """hmult,hlintrans,hadd at N = 2^15 against the same sequence of reference calls.  Link k runs under seed + 31 k (OpChain): its keys,
    plaintexts and second operand are drawn from there, its first operand is the link before's output."""
    from lintrans_ref import lintrans
    L, ell, alpha, R = 6, 5, 2, 2
    o = oracle(15, L, alpha)
    chain = host.Chain("config_4_N15.cfg", "hmult,hlintrans,hadd", L, ell, alpha, overrides={"rotations": R})
    chain.execute(1)
    a = o.hmult(ell, o.synth_ct(ell, SEED), o.synth_ct(ell, SEED + 2000), o.synth_evk(ell, SEED + 10000))
    keys, pts = keys_and_plaintexts(o, ell - 1, R, SEED + 31)
    b = lintrans(o, ell - 1, a, 5, keys, pts(0))
    c = o.hadd(ell - 1, np.stack(b), o.synth_ct(ell - 1, SEED + 62 + 2000))
    assert [ln.split()[0] for ln in chain[1].plan()].count("IP_LINTRANS") == 1
    assert_ct(read_out(chain[0]), a, "hmult")
    assert_ct(read_out(chain[1]), b, "hlintrans")
    assert_ct(read_out(chain[2]), c, "hadd")
    chain.close()


# ============================================================================================================================
# D. real data
# ============================================================================================================================
def test_real_data_decrypts_to_the_weighted_sum_of_rotations():
    """m encrypted as in test_real_data_decrypts_to_every_rotation; plaintexts: integer polynomials of 8 non-zero coefficients of magnitude
    <= 2^10, reduced modulo each of the E moduli and transformed.  dec(out) = sum_r pt_r * sigma_r(m) in Z[X] / (X^N + 1) within
    R * 8 * 2^10 * 2^16: hrotate's per-rotation bound 2^16 (tests/test_gpu_real_data.py) times the largest plaintext 1-norm times R.
    The reference's own output is held to the same bound on the CPU before the GPU runs."""
    from lintrans_ref import lintrans
    from toy_ckks import Toy
    LOGN, L, ELL, ALPHA, R, g = 13, 6, 5, 2, 3, 5
    BOUND = R * 8 * (1 << 10) * (1 << 16)
    o = oracle(LOGN, L, ALPHA)
    toy = Toy(o, seed=4243)
    m = toy.rng.integers(-1000, 1000, o.N).astype(object) * (1 << 30)
    ct = toy.encrypt(m, ELL)
    ids = o.ext_ids(ELL)
    polys, pts, keys = [], [], []
    exp = np.zeros(o.N, dtype=object)
    for r in range(1, R + 1):
        p = np.zeros(o.N, dtype=object)
        for i in toy.rng.choice(o.N, 8, replace=False):
            p[int(i)] = int(toy.rng.integers(-(1 << 10), (1 << 10) + 1))
        polys.append(p)
        pts.append(toy.to_rns_eval(p, ids))
        keys.append(toy.evk_at_level(toy.gen_evk(toy.automorph(toy.s, pow(g, r, 2 * o.N))), ELL))
        exp = exp + toy.negacyclic_mul(p, toy.automorph(m, pow(g, r, 2 * o.N)))
    err = lambda out: max(abs(int(a) - int(b)) for a, b in zip(toy.decrypt(np.stack(out), ELL)[0], exp))
    ref = lintrans(o, ELL, ct, g, keys, pts)
    ref_err = err(ref)
    print(f"reference: max |dec - exact| = {ref_err} (bound {BOUND})")
    assert ref_err < BOUND
    op = host.Op("config_4_N15.cfg", "hlintrans", L, ELL, ALPHA, overrides={"N": 1 << LOGN, "rotations": R, "galois": g})
    op.write("ct1.c0", ct[0])
    op.write("ct1.c1", ct[1])
    for r in range(1, R + 1):
        op.write(f"pt{r}", pts[r - 1])
        for j in range(keys[r - 1].shape[0]):
            for k in range(2):
                op.write(f"IP_Rot{r}_Key{k}_{j}", keys[r - 1][j][k])
    op.execute(1)
    out = read_out(op)
    op.close()
    gpu_err = err(out)
    print(f"GPU: max |dec - exact| = {gpu_err} (bound {BOUND})")
    assert gpu_err < BOUND
    assert_ct(out, ref, "real data")
