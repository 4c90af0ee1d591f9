"""The identity steps of hlintrans and hbsgs on the GPU, on both arithmetic back-ends (mont32 and chain_bits = 60), bit for bit:
 A. hm_inner_product_lintrans_id against the oracle's element-wise chains AND against hm_inner_product_lintrans_multi followed by hm_ewe
    (MAC_ADD / MUL), on permuted limb lists with guard limb-polys, and its refusals;
 B. the op with identity = 1, fused (one IP_LINTRANS launch with id=1) and unfused (one launch per stage), against tests/identity_ref.py;
 C. batched, replayed from a graph, and as the middle link of a chain;
 D. on real data (tests/toy_ckks.py) out decrypts to pt_0 * m + sum_r pt_r * sigma_r(m);
 E. hm_inner_product_rotsum_init against hm_inner_product_rotsum followed by hm_ewe (ADD), which tests/test_gpu_rotsum.py holds to the oracle;
 F. hbsgs with identity = 1: fused, unfused and by reference, batched, replayed, in a chain and on real data."""
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
    """(hip context, oracle on the same moduli) per chain at N = 2^13, made on first use"""
    from homulator_amd import hip
    made = {}

    def get(chain):
        if chain not in made:
            if chain == "mont32":
                ctx = hip.Context(13, NQ, NP)
            else:
                mods = chain_below(13, 60, NQ + NP)
                ctx = hip.Context(13, NQ, NP, q=mods[:NQ], p=mods[NQ:])
            o = oracle(13, NQ, NP, chain)
            assert ctx.moduli == o.moduli
            made[chain] = (ctx, o)
        return made[chain]
    yield get
    for ctx, _ in made.values():
        ctx.close()


def elements(R):
    twoN = 2 << 13
    return {1: [3], 3: [5, twoN - 1, twoN - 3]}.get(R) or [pow(5, r, twoN) for r in range(1, R + 1)]


def run_kernel_case(ctx, o, mods, T, galois, G, seed, add_mask, fill="uniform"):
    """one hm_inner_product_lintrans_id call with G outputs; every limb list is a random permutation of its buffer, the three output buffers keep
    one guard limb-poly each; the identity plaintexts are limbs of the plaintext buffer.  add_mask[i]: entry i carries the two addend sources.
    Checks every output against the oracle, against hm_inner_product_lintrans_multi + hm_ewe, and the guards."""
    from homulator_amd import hip
    from lintrans_ref import weighted_sum
    n, R, N = len(mods), len(galois), ctx.N
    rng = np.random.default_rng(seed)
    adds = [i for i in range(n) if add_mask[i]]
    A = len(adds)
    assert A, "the entry point needs an addend"
    nx, ny, npt, nc, no, na = n * T, R * n * 2 * T, G * R * n + G * A, A, G * 2 * n + 1, G * A + 1
    xb, yb, pb, cb, c1b, ob, ab, wb, ob2, ab2, wb2 = (ctx.alloc(k) for k in (nx, ny, npt, nc, nc, no, na, na, no, na, na))
    xl, yl, ppool, cperm, c1perm, operm, aperm, wperm = ([int(v) for v in rng.permutation(k)] for k in (nx, ny, npt, nc, nc, no, na, na))
    pl, idpool = ppool[:G * R * n], ppool[G * R * n:]
    ol = operm[:G * 2 * n]
    NOL = hip.NO_LIMB
    cl, c1l = [NOL] * n, [NOL] * n
    idl, al, wl = [NOL] * (G * n), [NOL] * (G * n), [NOL] * (G * n)
    for t, i in enumerate(adds):
        cl[i], c1l[i] = cperm[t], c1perm[t]
        for m in range(G):
            idl[m * n + i], al[m * n + i], wl[m * n + i] = idpool[m * A + t], aperm[m * A + t], wperm[m * A + t]
    xm = {xl[i * T + j]: mods[i] for i in range(n) for j in range(T)}
    ym = {yl[((r * n + i) * 2 + k) * T + j]: mods[i] for r in range(R) for i in range(n) for k in range(2) for j in range(T)}
    pm = {pl[(m * R + r) * n + i]: mods[i] for m in range(G) for r in range(R) for i in range(n)}
    pm.update({idl[m * n + i]: mods[i] for m in range(G) for i in adds})
    cm, c1m = {cl[i]: mods[i] for i in adds}, {c1l[i]: mods[i] for i in adds}
    for which, (buf, mm) in enumerate(((xb, xm), (yb, ym), (pb, pm), (cb, cm), (c1b, c1m))):
        if fill == "uniform":
            ctx.fill_uniform(buf, [mm[k] for k in sorted(mm)], seed * 11 + which, out_limbs=sorted(mm))
        else:
            buf.upload(np.stack([np.full(N, ctx.moduli[mm[k]] - 1 if fill == "q-1" else 0, dtype=np.uint64) for k in sorted(mm)]))
    for b, k in ((ob, no), (ab, na), (wb, na), (ob2, no), (ab2, na), (wb2, na)):
        b.upload(np.full((k, N), GUARD, dtype=np.uint64))
    ctx.inner_product_lintrans_id(xb, xl, yb, yl, pb, pl, ob, ol, mods, T, galois, G, cb, cl, ab, al, idl, c1b, c1l, wb, wl)
    # the composition the header promises: the entry point without the identity step, then MAC_ADD into the addend outputs and MUL
    ctx.inner_product_lintrans_multi(xb, xl, yb, yl, pb, pl, ob2, ol, mods, T, galois, G, addend=cb, addend_limbs=cl, addend_out=ab2, addend_out_limbs=al)
    for m in range(G):
        la, lb, lo, lw = [cl[i] for i in adds], [idl[m * n + i] for i in adds], [al[m * n + i] for i in adds], [wl[m * n + i] for i in adds]
        amods = [mods[i] for i in adds]
        ctx.ewe(hip.OP_MAC_ADD, ab2, amods, a=cb, b=pb, c=ab2, la=la, lb=lb, lc=lo, lo=lo)
        ctx.ewe(hip.OP_MUL, wb2, amods, a=c1b, b=pb, la=[c1l[i] for i in adds], lb=lb, lo=lw)
    X, Y, P, C0, C1, got, gotA, gotW, got2, gotA2, gotW2 = (b.download() for b in (xb, yb, pb, cb, c1b, ob, ab, wb, ob2, ab2, wb2))
    for b in (xb, yb, pb, cb, c1b, ob, ab, wb, ob2, ab2, wb2):
        b.free()
    what = (T, R, n, G, fill)
    assert np.array_equal(got, got2) and np.array_equal(gotA, gotA2) and np.array_equal(gotW, gotW2), (what, "differs from lintrans_multi + hm_ewe")
    # the oracle: per rotation the key product of the rotated digits (MUL, MAC_ADD), then the weighted sums; the unrotated terms in front
    terms = [[], []]
    for r, g in enumerate(galois):
        rx = [o.automorph_eval(np.stack([X[xl[i * T + j]] for i in range(n)]), g) for j in range(T)]
        for k in range(2):
            key = lambda j: np.stack([Y[yl[((r * n + i) * 2 + k) * T + j]] for i in range(n)])
            acc = o.ewe(EWE_MUL, mods, rx[0], key(0))
            for j in range(1, T):
                acc = o.ewe(EWE_MAC_ADD, mods, rx[j], key(j), acc)
            terms[k].append(acc)
    amods = [mods[i] for i in adds]
    c0, c1 = np.stack([C0[cl[i]] for i in adds]), np.stack([C1[c1l[i]] for i in adds])
    rc0 = [o.automorph_eval(c0, g) for g in galois]
    for m in range(G):
        pts = [np.stack([P[pl[(m * R + r) * n + i]] for i in range(n)]) for r in range(R)]
        pt0 = np.stack([P[idl[m * n + i]] for i in adds])
        for k in range(2):
            exp = weighted_sum(o, mods, terms[k], pts)
            assert np.array_equal(got[[ol[(m * n + i) * 2 + k] for i in range(n)]], exp), (what, m, "key", k)
        expU = weighted_sum(o, amods, [c0] + rc0, [pt0] + [p[adds] for p in pts])
        assert np.array_equal(gotA[[al[m * n + i] for i in adds]], expU), (what, m, "addend")
        assert np.array_equal(gotW[[wl[m * n + i] for i in adds]], o.ewe(EWE_MUL, amods, c1, pt0)), (what, m, "second addend")
    assert np.all(got[operm[-1]] == GUARD) and np.all(gotA[aperm[-1]] == GUARD) and np.all(gotW[wperm[-1]] == GUARD), "a guard limb-poly was written"


@pytest.mark.parametrize("chain", CHAINS)
@pytest.mark.parametrize("T", [1, 2, 3, 4])
def test_kernel_against_the_oracle_and_the_composition(envs, chain, T):
    """digits 1..4 x rotations 1 / 3 / 15 x outputs 1 (the single-sum kernel form) / TILE + 1 (the several-sums form), 7 entries with repeated
    moduli, every other entry without the addends"""
    from homulator_amd import hip
    ctx, o = envs(chain)
    rng = np.random.default_rng(T)
    for R, G in ((1, 1), (3, hip.LINTRANS_MULTI_TILE + 1), (15, 1)):
        mods = [int(x) for x in rng.integers(0, NQ + NP, 7)]
        run_kernel_case(ctx, o, mods, T, elements(R), G, 100 * T + R, add_mask=[i % 2 == 0 for i in range(7)])


@pytest.mark.parametrize("chain", CHAINS)
@pytest.mark.parametrize("tile_opt", [2, 4])
def test_kernel_both_tile_sizes_at_their_boundaries(envs, chain, tile_opt):
    """an explicit tile size keeps the several-sums kernel form at one output too"""
    ctx, o = envs(chain)
    ctx.set_option("ip_multi_tile", tile_opt)
    try:
        for G in (tile_opt - 1, tile_opt, tile_opt + 1, 2 * tile_opt + 1):
            run_kernel_case(ctx, o, [0, NQ, 3], 2, elements(3), G, 50 + G, add_mask=[True, False, True])
    finally:
        ctx.set_option("ip_multi_tile", 0)


@pytest.mark.parametrize("chain", CHAINS)
@pytest.mark.parametrize("fill", ["q-1", "zero"])
def test_kernel_worst_case_operands(envs, chain, fill):
    """15 rotations of 4 digits and the identity term with every operand q - 1: 16 (q - 1)^2 in the addend accumulator, the largest value the wide
    reduction is stated for; and all zeros"""
    ctx, o = envs(chain)
    run_kernel_case(ctx, o, [0, NQ + NP - 1, 3], 4, elements(15), 2, 7, add_mask=[True, True, True], fill=fill)


@pytest.mark.parametrize("chain", CHAINS)
@pytest.mark.parametrize("n", [1, 65])
def test_kernel_entry_counts(envs, chain, n):
    ctx, o = envs(chain)
    mods = [i % (NQ + NP) for i in range(n)]
    run_kernel_case(ctx, o, mods, 2, elements(1), 2, 40 + n, add_mask=[m < NQ for m in mods])


def test_kernel_with_an_addend_on_every_entry(envs):
    ctx, o = envs("mont32")
    run_kernel_case(ctx, o, [0, 1, 2], 3, elements(3), 1, 9, add_mask=[True] * 3)


def _alias_call(ctx, big, out=44, addend_out=52, addend1_out=56, id_pt=32, addend1=40):
    """n = 4 entries of 2 digits, one rotation, one output, in ONE allocation, each operand through a base pointer of its own: digits limbs 0..7,
    keys 16..31, plaintexts 32..35 (the identity plaintexts: limbs id_pt .. of them), c0 36..39, c1 40..43; outputs from limb `out` (8 limb-polys),
    `addend_out` (4) and `addend1_out` (4)"""
    at = lambda limb: types.SimpleNamespace(ptr=big.limb_ptr(limb))
    n, T = 4, 2
    ctx.inner_product_lintrans_id(big, list(range(n * T)), at(16), list(range(n * 2 * T)), at(32), list(range(n)), at(out), list(range(2 * n)),
                                  [0] * n, T, [5], 1, at(36), list(range(n)), at(addend_out), list(range(n)),
                                  [id_pt - 32 + i for i in range(n)], at(addend1), list(range(n)), at(addend1_out), list(range(n)))


@pytest.mark.parametrize("where,what", [
    ({"out": 5}, "digit"), ({"out": 30}, "key"), ({"out": 33}, "plaintext"), ({"out": 38}, "addend source"), ({"out": 41}, "second addend source"),
    ({"addend_out": 6}, "addend output.*digit"), ({"addend_out": 42}, "addend output.*second addend source"),
    ({"addend1_out": 6}, "second addend output.*digit"), ({"addend1_out": 34}, "second addend output.*plaintext"),
    ({"addend1_out": 37}, "second addend output.*addend source"), ({"addend1_out": 41}, "second addend output.*second addend source"),
    ({"addend1_out": 46}, "two output"), ({"addend1_out": 53}, "two output"),
    ({"out": 58, "id_pt": 60}, "identity plaintext"),
])
def test_refuses_an_output_over_an_input_or_another_output_through_another_base_pointer(where, what):
    from homulator_amd import hip
    ctx = hip.Context(13, NQ, NP)
    big = ctx.alloc(72)
    ctx.fill_uniform(big, [0] * 72, 5)
    _alias_call(ctx, big)                                   # disjoint: accepted
    with pytest.raises(hip.HmError, match=what):
        _alias_call(ctx, big, **where)
    ctx.close()


def test_refuses_bad_arguments():
    from homulator_amd import hip
    ctx = hip.Context(13, NQ, NP)
    b = ctx.alloc(40)

    def call(T=1, g=(5,), G=1, addend=b, cl=(36,), idl=(21,), addend1=b, c1l=(37,), addend1_out=b, wl=(33,), xl=None):
        ctx.inner_product_lintrans_id(b, xl or list(range(T)), b, list(range(8, 8 + 2 * T * len(g))), b, [20] * (G * len(g)), b, list(range(30, 30 + 2)) * G,
                                      [0], T, list(g), G, addend, list(cl) if cl is not None else None, b if addend is not None else None,
                                      [32] * G if cl is not None else None, list(idl) * G if idl is not None else None, addend1,
                                      list(c1l) if c1l is not None else None, addend1_out, list(wl) * G if wl is not None else None)
    call()                                                  # accepted
    with pytest.raises(hip.HmError, match="n_terms"):
        call(T=5)
    with pytest.raises(hip.HmError, match=r"n_rot in \[1,15\]"):
        ctx.inner_product_lintrans_id(b, [0], b, list(range(32)), b, [20] * 16, b, [30, 31], [0], 1, [pow(5, r, 1 << 14) for r in range(1, 17)], 1,
                                      b, [36], b, [32], [21], b, [37], b, [33])
    with pytest.raises(hip.HmError, match="n_out"):
        call(G=17)
    with pytest.raises(hip.HmError, match="odd"):
        call(g=(4,))
    with pytest.raises(hip.HmError, match="65535"):
        call(xl=[70000])
    with pytest.raises(hip.HmError, match="identity step needs"):
        call(addend=None, cl=None)                          # the addend is required
    for missing in ({"idl": None}, {"addend1": None}, {"c1l": None}, {"addend1_out": None}, {"wl": None}):
        with pytest.raises(hip.HmError, match="identity step needs"):
            call(**missing)
    with pytest.raises(hip.HmError, match="one of the two addend sources"):
        call(c1l=(hip.NO_LIMB,))
    with pytest.raises(hip.HmError, match="two output"):
        call(wl=(32,))                                      # W on top of U
    ctx.close()


# ============================================================================================================================
# B. the op
# ============================================================================================================================
def inputs(o, ell, R, c=0, seed=SEED):
    """the op's synthetic streams for op c of a batch: the ciphertext, rotation r's key (one for every op of the batch), pt<r> and pt0"""
    from identity_ref import lintrans_id_inputs
    return lintrans_id_inputs(o, ell, R, seed, copy=c, batch_seed_stride=BATCH_SEED_STRIDE)


def read_out(op, copy=0):
    return op.read("out.c0", copy=copy), op.read("out.c1", copy=copy)


def assert_ct(got, exp, what):
    assert np.array_equal(got[0], exp[0]), (what, "c0")
    assert np.array_equal(got[1], exp[1]), (what, "c1")


def check_op(chain, cfg, logN, L, ell, alpha, R, batch, merged, extra=None):
    from identity_ref import lintrans_id
    from lintrans_ref import lintrans
    o = oracle(logN, L, alpha, chain, threads=16)
    ov = chain_ov(chain, dict({"rotations": R, "galois": 5, "batch": batch, "N": 1 << logN, "identity": 1}, **(extra or {})))
    got = {}
    for fuse in (True, False):
        op = host.Op(cfg, "hlintrans", L, ell, alpha, fuse=fuse, overrides=ov)
        op.execute(1)
        got[fuse] = [read_out(op, c) for c in range(batch)]
        lines = [ln for ln in op.plan() if ln.startswith("IP_LINTRANS")]
        assert len(lines) == (1 if fuse and merged else 0) and all(ln.rstrip().endswith("id=1") for ln in lines)
        op.close()
    for c in range(batch):
        ct, keys, pts, pt0 = inputs(o, ell, R, c)
        exp = lintrans_id(o, ell, ct, 5, keys, pts, pt0)
        assert_ct(got[True][c], exp, ("fused", c))
        assert_ct(got[False][c], exp, ("unfused", c))
        if c == 0:   # ... and the identity term is there: without it both components differ
            base = lintrans(o, ell, ct, 5, keys, pts)
            assert not np.array_equal(exp[0], base[0]) and not np.array_equal(exp[1], base[1])


@pytest.mark.parametrize("chain", CHAINS)
@pytest.mark.parametrize("ell,alpha,merged", [(13, 13, True), (10, 5, True), (7, 3, True), (12, 3, True), (11, 2, False)],
                         ids=["beta1", "beta2", "beta3", "beta4", "beta6-unmerged"])
def test_op_fused_unfused_and_reference_agree(chain, ell, alpha, merged):
    check_op(chain, "config_4_N15.cfg", 13, 13, ell, alpha, 2, 1, merged)


@pytest.mark.parametrize("chain", CHAINS)
def test_op_config_1_batch_3(chain):
    check_op(chain, "config_4_N15.cfg", 15, 16, 10, 4, 2, 3, True)


def test_op_with_fuse_lintrans_off():
    check_op("mont32", "config_4_N15.cfg", 13, 13, 7, 3, 2, 1, False, extra={"fuse_lintrans": 0})


def test_a_zero_identity_plaintext_gives_identity_0_bit_for_bit():
    """with pt0 = 0 the op's output is the op without the identity step"""
    ov = {"rotations": 3, "N": 1 << 13}
    a = host.Op("config_4_N15.cfg", "hlintrans", 13, 7, 3, overrides=dict(ov, identity=1))
    a.write("pt0", np.zeros((7 + 3, 1 << 13), dtype=np.uint64))
    a.execute(1)
    b = host.Op("config_4_N15.cfg", "hlintrans", 13, 7, 3, overrides=ov)
    b.execute(1)
    assert_ct(read_out(a), read_out(b), "pt0 = 0")
    a.close()
    b.close()


# ============================================================================================================================
# C. graph replay, chain
# ============================================================================================================================
def test_graph_replay():
    """the plan captured into a HIP graph (run 1 direct, run 2 captures, run 3 replays): both copies of a batch of 2 after the replay"""
    from identity_ref import lintrans_id
    logN, L, ell, alpha, R, B = 13, 13, 7, 3, 3, 2
    o = oracle(logN, L, alpha, threads=16)
    op = host.Op("config_4_N15.cfg", "hlintrans", L, ell, alpha, overrides={"rotations": R, "batch": B, "graph": 1, "identity": 1, "N": 1 << logN})
    assert op.launch_count() == 7
    for _ in range(3):
        op.execute(1)
    for c in range(B):
        ct, keys, pts, pt0 = inputs(o, ell, R, c)
        assert_ct(read_out(op, c), lintrans_id(o, ell, ct, 5, keys, pts, pt0), f"copy {c}")
    op.close()


def test_middle_link_of_a_chain():
    """hmult,hlintrans,hadd at N = 2^15 against the same sequence of reference calls.  Link k runs under seed + 31 k (OpChain)"""
    from identity_ref import lintrans_id
    L, ell, alpha, R = 6, 5, 2, 2
    o = oracle(15, L, alpha)
    chain = host.Chain("config_4_N15.cfg", "hmult,hlintrans,hadd", L, ell, alpha, overrides={"rotations": R, "identity": 1})
    chain.execute(1)
    a = o.hmult(ell, o.synth_ct(ell, SEED), o.synth_ct(ell, SEED + 2000), o.synth_evk(ell, SEED + 10000))
    _, keys, pts, pt0 = inputs(o, ell - 1, R, seed=SEED + 31)
    b = lintrans_id(o, ell - 1, a, 5, keys, pts, pt0)
    c = o.hadd(ell - 1, np.stack(b), o.synth_ct(ell - 1, SEED + 62 + 2000))
    assert [ln for ln in chain[1].plan() if ln.startswith("IP_LINTRANS")][0].rstrip().endswith("id=1")
    assert_ct(read_out(chain[0]), a, "hmult")
    assert_ct(read_out(chain[1]), b, "hlintrans")
    assert_ct(read_out(chain[2]), c, "hadd")
    chain.close()


# ============================================================================================================================
# D. real data
# ============================================================================================================================
def test_real_data_decrypts_to_the_weighted_sum_with_the_unrotated_term():
    """m, the keys and the plaintexts as in tests/test_gpu_lintrans.py's real-data test (integer polynomials of 8 non-zero coefficients of magnitude
    <= 2^10), and one more such plaintext pt_0.  dec(out) = pt_0 * m + sum_r pt_r * sigma_r(m) in Z[X] / (X^N + 1) within (R + 1) * 8 * 2^10 * 2^16:
    per rotated term hrotate's bound 2^16 (tests/test_gpu_real_data.py) times the largest plaintext 1-norm, as that test derives it; the
    unrotated term meets no key, so its error is the fresh encryption noise alone, which is part of (so below) that same 2^16, times the same
    1-norm.  The reference's own output is held to the bound on the CPU before the GPU runs."""
    from identity_ref import lintrans_id
    from toy_ckks import Toy
    LOGN, L, ELL, ALPHA, R, g = 13, 6, 5, 2, 3, 5
    BOUND = (R + 1) * 8 * (1 << 10) * (1 << 16)
    o = oracle(LOGN, L, ALPHA)
    toy = Toy(o, seed=4244)
    m = toy.rng.integers(-1000, 1000, o.N).astype(object) * (1 << 30)
    ct = toy.encrypt(m, ELL)
    ids = o.ext_ids(ELL)
    pts, keys = [], []
    exp = np.zeros(o.N, dtype=object)
    for r in range(0, R + 1):
        p = np.zeros(o.N, dtype=object)
        for i in toy.rng.choice(o.N, 8, replace=False):
            p[int(i)] = int(toy.rng.integers(-(1 << 10), (1 << 10) + 1))
        pts.append(toy.to_rns_eval(p, ids))
        if r:
            keys.append(toy.evk_at_level(toy.gen_evk(toy.automorph(toy.s, pow(g, r, 2 * o.N))), ELL))
        exp = exp + toy.negacyclic_mul(p, toy.automorph(m, pow(g, r, 2 * o.N)) if r else m)
    err = lambda out: max(abs(int(a) - int(b)) for a, b in zip(toy.decrypt(np.stack(out), ELL)[0], exp))
    ref = lintrans_id(o, ELL, ct, g, keys, pts[1:], pts[0])
    ref_err = err(ref)
    print(f"reference: max |dec - exact| = {ref_err} (bound {BOUND})")
    assert ref_err < BOUND
    op = host.Op("config_4_N15.cfg", "hlintrans", L, ELL, ALPHA, overrides={"N": 1 << LOGN, "rotations": R, "galois": g, "identity": 1})
    op.write("ct1.c0", ct[0])
    op.write("ct1.c1", ct[1])
    for r in range(0, R + 1):
        op.write(f"pt{r}", pts[r])
    for r in range(1, R + 1):
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


# ============================================================================================================================
# E. the sum over ciphertexts with initial sums
# ============================================================================================================================
def run_init_case(ctx, mods, T, galois, seed, add_mask, fill="uniform"):
    """one hm_inner_product_rotsum_init call against hm_inner_product_rotsum + hm_ewe(ADD) on the same operands; permuted limb lists, one guard
    limb-poly per output buffer; the initial addend sums are limbs of the addend buffer"""
    from homulator_amd import hip
    n, G, N = len(mods), len(galois), ctx.N
    rng = np.random.default_rng(seed)
    adds = [i for i in range(n) if add_mask[i]]
    A = len(adds)
    nx, ny, ni, nc, no, na = G * n * T, G * n * 2 * T, 2 * n, max(1, G * A + A), 2 * n + 1, A + 1
    xb, yb, ib, cb, ob, ab, ob2, ab2 = (ctx.alloc(k) for k in (nx, ny, ni, nc, no, na, no, na))
    xl, yl, il, cperm, operm, aperm = ([int(v) for v in rng.permutation(k)] for k in (nx, ny, ni, nc, no, na))
    ol = operm[:2 * n]
    NOL = hip.NO_LIMB
    cl, al, cil = [NOL] * (G * n), [NOL] * n, [NOL] * n
    for t, i in enumerate(adds):
        al[i], cil[i] = aperm[t], cperm[G * A + t]
        for c in range(G):
            cl[c * n + i] = cperm[c * A + t]
    xm = {xl[(c * n + i) * T + j]: mods[i] for c in range(G) for i in range(n) for j in range(T)}
    ym = {yl[((c * n + i) * 2 + k) * T + j]: mods[i] for c in range(G) for i in range(n) for k in range(2) for j in range(T)}
    im = {il[i * 2 + k]: mods[i] for i in range(n) for k in range(2)}
    cm = {cl[c * n + i]: mods[i] for c in range(G) for i in adds}
    cm.update({cil[i]: mods[i] for i in adds})
    for which, (buf, mm) in enumerate(((xb, xm), (yb, ym), (ib, im), (cb, cm))):
        if not mm:
            continue
        if fill == "uniform":
            ctx.fill_uniform(buf, [mm[k] for k in sorted(mm)], seed * 13 + which, out_limbs=sorted(mm))
        else:
            buf.upload(np.stack([np.full(N, ctx.moduli[mm[k]] - 1, dtype=np.uint64) for k in sorted(mm)]))
    for b, k in ((ob, no), (ab, na), (ob2, no), (ab2, na)):
        b.upload(np.full((k, N), GUARD, dtype=np.uint64))
    kw = lambda out_a: dict(addend=cb, addend_limbs=cl, addend_out=out_a, addend_out_limbs=al) if adds else {}
    ctx.inner_product_rotsum_init(xb, xl, yb, yl, ob, ol, mods, T, galois, ib, il, addend_init_limbs=cil if adds else None, **kw(ab))
    ctx.inner_product_rotsum(xb, xl, yb, yl, ob2, ol, mods, T, galois, **kw(ab2))
    ctx.ewe(hip.OP_ADD, ob2, [mods[i] for i in range(n) for _ in range(2)], a=ob2, c=ib, la=ol, lc=il, lo=ol)
    if adds:
        lo = [al[i] for i in adds]
        ctx.ewe(hip.OP_ADD, ab2, [mods[i] for i in adds], a=ab2, c=cb, la=lo, lc=[cil[i] for i in adds], lo=lo)
    got, gotA, got2, gotA2, I = (b.download() for b in (ob, ab, ob2, ab2, ib))
    for b in (xb, yb, ib, cb, ob, ab, ob2, ab2):
        b.free()
    what = (T, G, n, fill)
    assert np.array_equal(got, got2) and np.array_equal(gotA, gotA2), (what, "differs from rotsum + hm_ewe ADD")
    assert np.all(got[operm[-1]] == GUARD) and np.all(gotA[aperm[-1]] == GUARD), "a guard limb-poly was written"
    assert not np.any(got[ol] == GUARD)
    if fill == "uniform":   # the initial sums matter
        assert not np.array_equal(got[ol], I[il])


@pytest.mark.parametrize("chain", CHAINS)
@pytest.mark.parametrize("T", [1, 2, 3, 4])
def test_rotsum_init_against_the_composition(envs, chain, T):
    """digits 1..4 x ciphertexts 1 / 3 / 15, 7 entries with repeated moduli, every other entry without addends"""
    ctx, _ = envs(chain)
    rng = np.random.default_rng(T)
    for G in (1, 3, 15):
        mods = [int(x) for x in rng.integers(0, NQ + NP, 7)]
        run_init_case(ctx, mods, T, elements(G), 300 * T + G, add_mask=[i % 2 == 0 for i in range(7)])


@pytest.mark.parametrize("chain", CHAINS)
@pytest.mark.parametrize("n", [1, 65])
def test_rotsum_init_entry_counts(envs, chain, n):
    ctx, _ = envs(chain)
    mods = [i % (NQ + NP) for i in range(n)]
    run_init_case(ctx, mods, 2, elements(3), 70 + n, add_mask=[m < NQ for m in mods])


@pytest.mark.parametrize("chain", CHAINS)
def test_rotsum_init_worst_case_and_no_addend(envs, chain):
    """15 ciphertexts of 4 digits with every operand q - 1: 60 (q - 1)^2 + (q - 1) per accumulator, 16 (q - 1) in the addend accumulator"""
    ctx, _ = envs(chain)
    run_init_case(ctx, [0, NQ + NP - 1, 3], 4, elements(15), 8, add_mask=[True, True, True], fill="q-1")
    run_init_case(ctx, [NQ, NQ + 1], 3, elements(3), 9, add_mask=[False, False])


def test_rotsum_init_refuses_bad_arguments():
    from homulator_amd import hip
    ctx = hip.Context(13, NQ, NP)
    b = ctx.alloc(48)

    def call(g=(5,), init=b, il=(20, 21), cil=(37,), out=(30, 31), al=(32,)):
        ctx.inner_product_rotsum_init(b, list(range(len(g))), b, list(range(8, 8 + 2 * len(g))), b, list(out), [0], 1, list(g), init,
                                      list(il) if il is not None else None, addend=b, addend_limbs=[36] * len(g), addend_out=b,
                                      addend_out_limbs=list(al), addend_init_limbs=list(cil) if cil is not None else None)
    call()                                                  # accepted
    with pytest.raises(hip.HmError, match=r"n_ct in \[1,15\]"):
        call(g=[pow(5, r, 1 << 14) for r in range(1, 17)])
    for missing in ({"init": None}, {"il": None}, {"cil": None}):
        with pytest.raises(hip.HmError, match="null argument"):
            call(**missing)
    with pytest.raises(hip.HmError, match="initial addend sum without"):
        call(cil=(hip.NO_LIMB,))
    with pytest.raises(hip.HmError, match="output limb-poly overlaps an initial sum"):
        call(out=(30, 21))
    with pytest.raises(hip.HmError, match="addend output limb-poly overlaps an initial addend sum"):
        call(al=(37,))
    with pytest.raises(hip.HmError, match="output limb-poly overlaps an initial addend sum"):
        call(out=(37, 31))
    ctx.close()


# ============================================================================================================================
# F. hbsgs with the identity steps
# ============================================================================================================================
def bsgs_expected(o, ell, R, G, c=0, seed=SEED, ct=None, h=None):
    from bsgs_ref import synthetic_inputs
    from identity_ref import bsgs_id, bsgs_id_inputs
    ct0, baby, giant, pts = synthetic_inputs(o, ell, R, G, seed, copy=c)
    pt0s, ptgs = bsgs_id_inputs(o, ell, R, G, seed, copy=c)
    return bsgs_id(o, ell, ct0 if ct is None else ct, 5, h or pow(5, R + 1, 2 * o.N), baby, giant, pts, pt0s, ptgs)


def check_bsgs(chain, cfg, logN, L, ell, alpha, R, G, batch, merged, extra=None):
    o = oracle(logN, L, alpha, chain, threads=16)
    ov = chain_ov(chain, dict({"rotations": R, "giants": G, "galois": 5, "batch": batch, "N": 1 << logN, "identity": 1}, **(extra or {})))
    got = {}
    for fuse in (True, False):
        op = host.Op(cfg, "hbsgs", L, ell, alpha, fuse=fuse, overrides=ov)
        op.execute(1)
        got[fuse] = [read_out(op, c) for c in range(batch)]
        if fuse and merged:
            lines = [ln.rstrip() for ln in op.plan() if ln.startswith("IP_")]
            assert len(lines) == 2 and lines[0].startswith("IP_LINTRANS_MULTI") and f" out={G + 1} " in lines[0] and lines[0].endswith("id=1"), lines
            assert lines[1].startswith("IP_ROTSUM") and lines[1].endswith("init=1") and op.launch_count() == 14, lines
        op.close()
    for c in range(batch):
        exp = bsgs_expected(o, ell, R, G, c)
        assert_ct(got[True][c], exp, ("fused", c))
        assert_ct(got[False][c], exp, ("unfused", c))


@pytest.mark.parametrize("chain", CHAINS)
@pytest.mark.parametrize("R,G", [(2, 2), (1, 1)])
@pytest.mark.parametrize("ell,alpha,merged", [(13, 13, True), (10, 5, True), (7, 3, True), (12, 3, True), (11, 2, False)],
                         ids=["beta1", "beta2", "beta3", "beta4", "beta6-unmerged"])
def test_bsgs_fused_unfused_and_reference_agree(chain, ell, alpha, merged, R, G):
    check_bsgs(chain, "config_4_N15.cfg", 13, 13, ell, alpha, R, G, 1, merged)


@pytest.mark.parametrize("chain", CHAINS)
def test_bsgs_config_1_batch_3(chain):
    check_bsgs(chain, "config_4_N15.cfg", 15, 16, 10, 4, 2, 2, 3, True)


@pytest.mark.parametrize("extra", [{"fuse_bsgs": 0}, {"fuse_rotsum": 0}], ids=["fuse_bsgs-0", "fuse_rotsum-0"])
def test_bsgs_with_a_merge_off(extra):
    check_bsgs("mont32", "config_4_N15.cfg", 13, 13, 7, 3, 2, 2, 1, False, extra=extra)


def test_bsgs_with_zeroed_identity_and_group_0_plaintexts_gives_identity_0_bit_for_bit():
    ov = {"rotations": 2, "giants": 2, "N": 1 << 13, "galois_giant": pow(5, 3, 1 << 14)}
    zero = np.zeros((7 + 3, 1 << 13), dtype=np.uint64)
    a = host.Op("config_4_N15.cfg", "hbsgs", 13, 7, 3, overrides=dict(ov, identity=1))
    for name in ("pt0_0", "pt0_1", "pt0_2", "ptg1", "ptg2"):
        a.write(name, zero)
    a.execute(1)
    b = host.Op("config_4_N15.cfg", "hbsgs", 13, 7, 3, overrides=ov)
    b.execute(1)
    assert_ct(read_out(a), read_out(b), "identity and group-0 plaintexts zero")
    a.close()
    b.close()


def test_bsgs_graph_replay():
    logN, L, ell, alpha, R, G, B = 13, 13, 7, 3, 2, 2, 2
    o = oracle(logN, L, alpha, threads=16)
    op = host.Op("config_4_N15.cfg", "hbsgs", L, ell, alpha,
                 overrides={"rotations": R, "giants": G, "batch": B, "graph": 1, "identity": 1, "N": 1 << logN})
    assert op.launch_count() == 14
    for _ in range(3):
        op.execute(1)
    for c in range(B):
        assert_ct(read_out(op, c), bsgs_expected(o, ell, R, G, c), f"copy {c}")
    op.close()


def test_bsgs_middle_link_of_a_chain():
    """hmult,hbsgs,hadd at N = 2^15 against the same sequence of reference calls.  Link k runs under seed + 31 k (OpChain)"""
    L, ell, alpha, R, G = 6, 5, 2, 2, 2
    o = oracle(15, L, alpha)
    chain = host.Chain("config_4_N15.cfg", "hmult,hbsgs,hadd", L, ell, alpha, overrides={"rotations": R, "giants": G, "identity": 1})
    chain.execute(1)
    a = o.hmult(ell, o.synth_ct(ell, SEED), o.synth_ct(ell, SEED + 2000), o.synth_evk(ell, SEED + 10000))
    b = bsgs_expected(o, ell - 1, R, G, seed=SEED + 31, ct=np.stack(a))
    c = o.hadd(ell - 1, np.stack(b), o.synth_ct(ell - 1, SEED + 62 + 2000))
    assert [ln.split()[0] for ln in chain[1].plan()].count("IP_ROTSUM") == 1 and chain[1].launch_count() == 14
    assert_ct(read_out(chain[0]), a, "hmult")
    assert_ct(read_out(chain[1]), b, "hbsgs")
    assert_ct(read_out(chain[2]), c, "hadd")
    chain.close()


def test_bsgs_real_data_decrypts_to_the_transform_with_both_identity_steps():
    """as tests/test_gpu_bsgs.py's real-data test, with giant groups i = 0..G and baby steps r = 0..R: dec(out) =
    sum_{i=0..G} sigma_{h^i}(sum_{r=0..R} p_{i,r} * sigma_{g^r}(m)) within (G + 1) (R + 1) 8 2^10 2^16 + G 2^16: that test's bound per inner sum
    with R + 1 terms (the unrotated term's error is the fresh noise alone, part of the per-term 2^16), G + 1 inner sums, and hrotate's 2^16 for
    each of the G giant steps; group 0 meets no giant key.  The reference's own output is held to the bound on the CPU before the GPU runs."""
    from identity_ref import bsgs_id
    from toy_ckks import Toy
    LOGN, L, ELL, ALPHA, R, G, g = 13, 6, 5, 2, 2, 2, 5
    BOUND = (G + 1) * (R + 1) * 8 * (1 << 10) * (1 << 16) + G * (1 << 16)
    o = oracle(LOGN, L, ALPHA)
    twoN = 2 * o.N
    h = pow(g, R + 1, twoN)
    toy = Toy(o, seed=4245)
    m = toy.rng.integers(-1000, 1000, o.N).astype(object) * (1 << 30)
    ct = toy.encrypt(m, ELL)
    ids = o.ext_ids(ELL)
    baby = [toy.evk_at_level(toy.gen_evk(toy.automorph(toy.s, pow(g, r, twoN))), ELL) for r in range(1, R + 1)]
    giant = [toy.evk_at_level(toy.gen_evk(toy.automorph(toy.s, pow(h, i, twoN))), ELL) for i in range(1, G + 1)]
    rows = []
    exp = np.zeros(o.N, dtype=object)
    for i in range(0, G + 1):
        inner = np.zeros(o.N, dtype=object)
        row = []
        for r in range(0, R + 1):
            p = np.zeros(o.N, dtype=object)
            for x in toy.rng.choice(o.N, 8, replace=False):
                p[int(x)] = int(toy.rng.integers(-(1 << 10), (1 << 10) + 1))
            row.append(toy.to_rns_eval(p, ids))
            inner = inner + toy.negacyclic_mul(p, toy.automorph(m, pow(g, r, twoN)) if r else m)
        rows.append(row)
        exp = exp + (toy.automorph(inner, pow(h, i, twoN)) if i else inner)
    pts, pt0s, ptgs = [rows[i][1:] for i in range(1, G + 1)], [rows[i][0] for i in range(G + 1)], rows[0][1:]
    err = lambda out: max(abs(int(a) - int(b)) for a, b in zip(toy.decrypt(np.stack(out), ELL)[0], exp))
    ref = bsgs_id(o, ELL, ct, g, h, baby, giant, pts, pt0s, ptgs)
    ref_err = err(ref)
    print(f"reference: max |dec - exact| = {ref_err} (bound {BOUND})")
    assert ref_err < BOUND
    op = host.Op("config_4_N15.cfg", "hbsgs", L, ELL, ALPHA, overrides={"N": 1 << LOGN, "rotations": R, "giants": G, "galois": g, "identity": 1})
    op.write("ct1.c0", ct[0])
    op.write("ct1.c1", ct[1])
    for i in range(G):
        for r in range(R):
            op.write(f"pt{i * R + r + 1}", pts[i][r])
    for i in range(G + 1):
        op.write(f"pt0_{i}", pt0s[i])
    for r in range(R):
        op.write(f"ptg{r + 1}", ptgs[r])
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
