"""hlincomb on the GPU, on both arithmetic back-ends (mont32 and chain_bits = 60), bit for bit:
 A. hm_lincomb through the ABI: against the oracle's MUL_CONST / ADD (tests/lincomb_ref.py's primitives) and against MUL_CONST / ADD / ADD_CONST
    through hm_ewe on the same device data, on permuted and repeated input limbs with mixed moduli and a guard limb-poly; the refusals; n = 0; a
    captured call replayed;
 B. the op, fused (one LINCOMB launch), unfused (one launch per stage) and with fuse_lincomb = 0, against the reference; batch 2, graph = 1, caller
    constants, a chain hlincomb,hlincomb,hmult link by link, two hsquare producers bound to ct1 and ct2, and real data (tests/toy_ckks.py)."""
import ctypes as C
import types

import numpy as np
import pytest

from homulator_amd import host
from oracle.homoracle import EWE_ADD, EWE_MUL_CONST, Oracle, chain_below

pytestmark = pytest.mark.gpu
CHAINS = ["mont32", "survey"]
SEED = host.SEED
NQ, NP = 6, 3
PER_MOD = 3            # input limb-polys per modulus in the kernel cases: term lists draw from them with repetition
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
    """(hip context, oracle on the same moduli, the input pool on the device and on the host) per (logN, chain), made on first use.  The pool holds
    PER_MOD limb-polys per modulus, limb m * PER_MOD + r filled for modulus m; it is never written again"""
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
            pool = ctx.alloc((NQ + NP) * PER_MOD)
            ctx.fill_uniform(pool, [m for m in range(NQ + NP) for _ in range(PER_MOD)], 900 + logN)
            made[(logN, chain)] = (ctx, o, pool, pool.download())
        return made[(logN, chain)]
    yield get
    for ctx, _, pool, _ in made.values():
        pool.free()
        ctx.close()


def add_const_rows(x, ks, qs):
    out = np.empty_like(x)
    for i, (k, q) in enumerate(zip(ks, qs)):
        t = x[i] + np.uint64(k)
        out[i] = np.where(t >= np.uint64(q), t - np.uint64(q), t)
    return out


def kernel_lists(mods, T, moduli, rng, scale="random", const="random"):
    """per record T input limbs of its modulus from the pool (repeats allowed), T scalars and a constant of the named kinds (const None: no list)"""
    n = len(mods)
    li = [mods[i] * PER_MOD + int(rng.integers(0, PER_MOD)) for i in range(n) for _ in range(T)]
    val = lambda kind, q: {"0": 0, "1": 1, "q-1": q - 1}[kind] if kind != "random" else int(rng.integers(0, q))
    s = [val(scale, moduli[mods[i]]) for i in range(n) for _ in range(T)]
    k = None if const is None else [val(const, moduli[m]) for m in mods]
    return li, s, k


def expected_rows(o, host_pool, mods, T, li, s, k):
    """the Python-side reference: MUL_CONST per term, ADD between them (the oracle's element-wise primitives), the constant by numpy"""
    n = len(mods)
    acc = None
    for t in range(T):
        rows = np.stack([host_pool[li[i * T + t]] for i in range(n)])
        term = o.ewe(EWE_MUL_CONST, mods, rows, k=[s[i * T + t] for i in range(n)])
        acc = term if acc is None else o.ewe(EWE_ADD, mods, acc, None, term)
    return acc if k is None else add_const_rows(acc, k, [o.moduli[m] for m in mods])


def run_kernel_case(env, mods, T, seed, scale="random", const="random", composed=True):
    """one hm_lincomb call: the output buffer holds n limb-polys and one guard limb-poly, the output list is a random permutation"""
    from homulator_amd import hip
    ctx, o, pool, host_pool = env
    n, N = len(mods), ctx.N
    rng = np.random.default_rng(seed)
    li, s, k = kernel_lists(mods, T, ctx.moduli, rng, scale, const)
    perm = [int(v) for v in rng.permutation(n + 1)]
    lo = perm[:n]
    out = ctx.alloc(n + 1)
    out.upload(np.full((n + 1, N), GUARD, dtype=np.uint64))
    ctx.lincomb(pool, li, out, lo, mods, T, s, k)
    got = out.download()
    exp = expected_rows(o, host_pool, mods, T, li, s, k)
    what = (n, T, scale, const)
    assert np.array_equal(got[lo], exp), what
    assert np.all(got[perm[n]] == GUARD), "the guard limb-poly was written"
    if T <= 3:   # the definition in Python integers on a stretch of some records
        for i in sorted({0, n // 2, n - 1}):
            q = ctx.moduli[mods[i]]
            for x in (0, 1, N - 1):
                e = (sum(s[i * T + t] * int(host_pool[li[i * T + t]][x]) for t in range(T)) + (k[i] if k else 0)) % q
                assert int(got[lo[i]][x]) == e, (what, i, x)
    if composed:   # the same from the calls it replaces, on the same device data
        acc, tmp = ctx.alloc(n), ctx.alloc(n)
        for t in range(T):
            ctx.ewe(hip.OP_MUL_CONST, acc if t == 0 else tmp, mods, a=pool, la=[li[i * T + t] for i in range(n)], k=[s[i * T + t] for i in range(n)])
            if t:
                ctx.ewe(hip.OP_ADD, acc, mods, a=acc, c=tmp)
        if k is not None:
            ctx.ewe(hip.OP_ADD_CONST, acc, mods, a=acc, k=k)
        assert np.array_equal(acc.download(), got[lo]), (what, "composed")
        acc.free(); tmp.free()
    out.free()


@pytest.mark.parametrize("chain", CHAINS)
@pytest.mark.parametrize("T", [1, 2, 3, 16])
@pytest.mark.parametrize("n", [1, 3, 65, 130])
def test_kernel_entry_and_term_counts(envs, chain, n, T):
    """ONE launch for any n (across the 64- and 128-entry cuts of the launches whose records travel as kernel arguments); T = 1 runs no round of
    the two-term loop, 2 the tail behind it, 3 one round, 16 the most; Q and P limbs, mixed moduli"""
    run_kernel_case(envs(13, chain), [(5 * i + 2) % (NQ + NP) for i in range(n)], T, 40 + 17 * n + T)


@pytest.mark.parametrize("chain", CHAINS)
def test_kernel_scalars_and_constants_at_the_ends_of_the_range(envs, chain):
    """every scalar kind (0, 1, q - 1, random) with every constant kind (none, 0, q - 1, random), 5 records, T = 3 and T = 16"""
    mods = [0, NQ + NP - 1, 3, 0, NQ]
    i = 0
    for T in (3, 16):
        for s in ("0", "1", "q-1", "random"):
            for k in (None, "0", "q-1", "random"):
                run_kernel_case(envs(13, chain), mods, T, 7 + i, scale=s, const=k, composed=(i % 5 == 3))
                i += 1


@pytest.mark.parametrize("chain", CHAINS)
@pytest.mark.parametrize("logN", [15, 16])
def test_kernel_at_larger_rings(envs, chain, logN):
    for T in (2, 16):
        run_kernel_case(envs(logN, chain), [0, 5, NQ, 5, 2], T, logN + T)


def _alias_call(ctx, big, out_at=40, n=4, T=2):
    """n = 4 records of 2 terms in ONE allocation: the inputs are limbs 0 .. 7 through the allocation's base, the outputs n limbs from `out_at`
    through a base pointer of their own"""
    at = lambda limb: types.SimpleNamespace(ptr=big.limb_ptr(limb))
    ctx.lincomb(big, list(range(n * T)), at(out_at), None, [0] * n, T, [1] * (n * T))


def test_refuses_an_output_over_an_input_through_another_base_pointer():
    from homulator_amd import hip
    ctx = hip.Context(13, NQ, NP)
    big = ctx.alloc(64)
    ctx.fill_uniform(big, [0] * 64, 5)
    _alias_call(ctx, big)                                   # disjoint: accepted
    for out_at in (7, 4, 0):
        with pytest.raises(hip.HmError, match=r"hm_lincomb: an output limb-poly \(out\) overlaps an input limb-poly \(in\)"):
            _alias_call(ctx, big, out_at=out_at)
    ctx.sync()
    ctx.close()


def test_refuses_bad_arguments_and_accepts_n_0():
    from homulator_amd import hip
    ctx = hip.Context(13, NQ, NP)
    src, out = ctx.alloc(4), ctx.alloc(4)
    ctx.fill_uniform(src, [0] * 4, 5)
    q0 = ctx.moduli[0]
    null = types.SimpleNamespace(ptr=None)
    with pytest.raises(hip.HmError, match="hm_lincomb: null buffer"):
        ctx.lincomb(null, [0], out, [0], [0], 1, [1])
    with pytest.raises(hip.HmError, match="hm_lincomb: null buffer"):
        ctx.lincomb(src, [0], null, [0], [0], 1, [1])
    with pytest.raises(hip.HmError, match="hm_lincomb: scale is null"):
        ctx.lincomb(src, [0], out, [0], [0], 1, None)
    with pytest.raises(hip.HmError, match="hm_lincomb: mod_ids is null"):
        ctx._ck(ctx.L.hm_lincomb(ctx.h, src.ptr, None, out.ptr, None, None, 1, 1, hip._u64([1])[1], None))
    for T in (0, 17):
        with pytest.raises(hip.HmError, match=rf"hm_lincomb: n_terms = {T}, must be in \[1, 16\]"):
            ctx.lincomb(src, [0] * T, out, [0], [0], T, [1] * max(T, 1))
    with pytest.raises(hip.HmError, match="65535"):
        ctx.lincomb(src, [0, 70000], out, [0], [0], 2, [1, 1])
    with pytest.raises(hip.HmError, match="65535"):
        ctx.lincomb(src, [0, 1], out, [70000], [0], 2, [1, 1])
    with pytest.raises(hip.HmError, match="mod id"):
        ctx.lincomb(src, [0], out, [0], [NQ + NP], 1, [1])
    with pytest.raises(hip.HmError, match=r"scale\[1\]\[0\] is not reduced"):
        ctx.lincomb(src, [0, 1, 2, 3], out, [0, 1], [0, 0], 2, [1, 0, q0, 1])
    with pytest.raises(hip.HmError, match=r"addend\[1\] is not reduced"):
        ctx.lincomb(src, [0, 1], out, [0, 1], [0, 0], 1, [1, 1], [0, q0])
    with pytest.raises(hip.HmError, match="two output"):
        ctx.lincomb(src, [0, 1], out, [2, 2], [0, 0], 1, [1, 1])
    with pytest.raises(hip.HmError, match="two output limb-polys overlap"):   # entries 0 and 2, apart in the list; no input touched
        ctx.lincomb(src, [0, 1, 2], out, [2, 0, 2], [0, 0, 0], 1, [1, 1, 1])
    with pytest.raises(hip.HmError, match="overlaps an input"):
        ctx.lincomb(src, [0, 1], src, [3, 1], [0, 0], 1, [1, 1])
    keep = [hip._u32([0]), hip._u64([1, 1, 1])]
    ctx._ck(ctx.L.hm_lincomb(ctx.h, src.ptr, None, out.ptr, None, keep[0][1], 0, 3, keep[1][1], None))   # n = 0: nothing to do
    ctx.lincomb(src, [0, 1, 1, 0], out, [3, 0], [0, 0], 2, [0, q0 - 1, 1, 0], [0, q0 - 1])   # and a call with nothing wrong is accepted
    ctx.sync()
    ctx.close()


@pytest.mark.parametrize("chain", CHAINS)
def test_a_captured_call_replays(envs, chain):
    """the records live in a cached device table: after one warm run the call is captured into a graph and replayed on new input data"""
    ctx, o, _, _ = envs(13, chain)
    ctx.L.hm_graph_launch.argtypes = [C.c_void_p, C.c_void_p]
    ctx.L.hm_graph_destroy.argtypes = [C.c_void_p]
    T = 3
    mods = [(3 * i + 1) % (NQ + NP) for i in range(70)]
    fill_mods = [m for m in range(NQ + NP) for _ in range(PER_MOD)]
    rng = np.random.default_rng(3)
    li, s, k = kernel_lists(mods, T, ctx.moduli, rng)
    src, out = ctx.alloc(len(fill_mods)), ctx.alloc(len(mods))
    run = lambda: ctx.lincomb(src, li, out, None, mods, T, s, k)
    ctx.fill_uniform(src, fill_mods, 1)
    run()
    g = C.c_void_p()
    ctx._ck(ctx.L.hm_capture_begin(ctx.h))
    run()
    ctx._ck(ctx.L.hm_capture_end(ctx.h, C.byref(g)))
    ctx.fill_uniform(src, fill_mods, 2)
    out.upload(np.full((len(mods), ctx.N), GUARD, dtype=np.uint64))
    ctx._ck(ctx.L.hm_graph_launch(ctx.h, g))
    ctx.sync()
    assert np.array_equal(out.download(), expected_rows(o, src.download(), mods, T, li, s, k)), chain
    ctx.L.hm_graph_destroy(g)
    src.free(); out.free()


# ============================================================================================================================
# B. the op
# ============================================================================================================================
def read_out(op, copy=0):
    return op.read("out.c0", copy=copy), op.read("out.c1", copy=copy)


SHAPES = [
    ("config_4_N15.cfg", 15, 16, 10, 4, 2),
    ("config_4_N15.cfg", 13, 6, 5, 2, 1),
    ("config_4.cfg", 16, 6, 3, 2, 1),           # N = 2^16 at a low level
]
KEYS = [(1, 0, 0), (3, 1, 1), (4, 1, 0), (4, 0, 1)]     # (terms, lc_const, rescale): every T, both values of either key
_ref = {}


def reference(chain, logN, L, ell, alpha, keys, copy=0, seed=SEED):
    """the reference output on the op's synthetic inputs, computed once per case"""
    from lincomb_ref import lincomb, synthetic_constants, synthetic_inputs
    key = (chain, logN, L, ell, alpha, keys, copy, seed)
    if key not in _ref:
        T, lc, rs = keys
        o = oracle(logN, L, alpha, chain, threads=16)
        _ref[key] = lincomb(o, ell, synthetic_inputs(o, ell, seed, T, copy=copy), *synthetic_constants(o, ell, seed, T, lc), rescale=bool(rs))
    return _ref[key]


@pytest.mark.parametrize("chain", CHAINS)
@pytest.mark.parametrize("keys", KEYS)
@pytest.mark.parametrize("cfg,logN,L,ell,alpha,batch", SHAPES)
def test_op_fused_unfused_and_reference_agree(chain, keys, cfg, logN, L, ell, alpha, batch):
    """fused, unfused and fuse_lincomb = 0 against the reference; batch 2 (first shape): both copies, under the same constants"""
    from lincomb_ref import assert_ct
    T, lc, rs = keys
    ov = chain_ov(chain, {"terms": T, "lc_const": lc, "rescale": rs, "batch": batch, "N": 1 << logN})
    for mode, fuse, extra in (("fused", True, {}), ("unfused", False, {}), ("fuse_lincomb = 0", True, {"fuse_lincomb": 0})):
        op = host.Op(cfg, "hlincomb", L, ell, alpha, fuse=fuse, overrides=dict(ov, **extra))
        op.execute(1)
        kinds = [ln.split()[0] for ln in op.plan()]
        assert kinds.count("LINCOMB") == (1 if mode == "fused" else 0), (mode, kinds)
        for c in range(batch):
            got = read_out(op, c)
            assert got[0].shape[0] == ell - rs
            assert_ct(got, reference(chain, logN, L, ell, alpha, keys, copy=c), (mode, keys, c))
        op.close()


def test_graph_replay_with_a_batch():
    """graph = 1: run 1 direct, run 2 captures, run 3 replays; both copies after the replay"""
    from lincomb_ref import assert_ct
    cfg, logN, L, ell, alpha, batch = SHAPES[0]
    keys = (3, 1, 1)
    op = host.Op(cfg, "hlincomb", L, ell, alpha, overrides={"terms": 3, "lc_const": 1, "rescale": 1, "batch": batch, "graph": 1})
    lc = [ln for ln in op.plan() if ln.startswith("LINCOMB")]
    assert len(lc) == 1 and f" n={2 * batch * ell} " in lc[0] and " terms=3 const=1" in lc[0]
    for _ in range(3):
        op.execute(1)
    for c in range(batch):
        assert_ct(read_out(op, c), reference("mont32", logN, L, ell, alpha, keys, copy=c), f"copy {c}")
    op.close()


@pytest.mark.parametrize("chain", CHAINS)
@pytest.mark.parametrize("fuse", [True, False])
def test_caller_constants(chain, fuse):
    from lincomb_ref import assert_ct, lincomb, synthetic_inputs
    L, ell, alpha, T = 6, 5, 2, 3
    o = oracle(13, L, alpha, chain)
    scales = [[2, o.moduli[1] - 1, 1, 12345, o.moduli[4] // 2], [0] * ell, [o.moduli[j] - 3 for j in range(ell)]]
    const = [(7 << 40) % o.moduli[j] for j in range(ell)]
    op = host.Op("config_4_N15.cfg", "hlincomb", L, ell, alpha, fuse=fuse, overrides=chain_ov(chain, {"terms": T, "lc_const": 1, "N": 1 << 13}))
    for t in range(T):
        op.set_constants(f"scale{t + 1}", scales[t])
    op.set_constants("const", const)
    op.execute(1)
    assert_ct(read_out(op), lincomb(o, ell, synthetic_inputs(o, ell, SEED, T), scales, const), ("caller constants", chain, fuse))
    with pytest.raises(host.HostError, match=r'hlincomb: set_constants\("scale2"\) after prepare'):
        op.set_constants("scale2", scales[1])
    op.close()


def test_chain_lincomb_lincomb_hmult_link_by_link():
    """hlincomb,hlincomb,hmult at N = 2^13 with rescale = 1: link k runs under seed + 31 k (OpChain): its further inputs and its constants are
    drawn from there, its ct1 is the link before's output, and the levels follow"""
    from lincomb_ref import assert_ct, lincomb, synthetic_constants, synthetic_inputs
    L, ell, alpha, T = 6, 5, 2, 3
    o = oracle(13, L, alpha)
    chain = host.Chain("config_4_N15.cfg", "hlincomb,hlincomb,hmult", L, ell, alpha, overrides={"terms": T, "lc_const": 1, "rescale": 1, "N": 1 << 13})
    chain.execute(1)
    ct = None
    for k in range(2):
        lvl, seed = ell - k, SEED + 31 * k
        cts = synthetic_inputs(o, lvl, seed, T)
        if ct is not None:
            cts[0] = ct
        out = lincomb(o, lvl, cts, *synthetic_constants(o, lvl, seed, T, 1), rescale=True)
        assert [ln.split()[0] for ln in chain[k].plan()].count("LINCOMB") == 1
        assert_ct(read_out(chain[k]), out, f"link {k}")
        ct = np.stack(out)
    lvl, seed = ell - 2, SEED + 62
    assert_ct(read_out(chain[2]), o.hmult(lvl, ct, o.synth_ct(lvl, seed + 2000), o.synth_evk(lvl, seed + 10000)), "link 2 (hmult)")
    chain.close()


def test_two_squares_bound_to_ct1_and_ct2():
    """the Chebyshev recombination the op exists for: two hsquare ops with different seeds produce ct1 and ct2 of an hlincomb with terms = 2, checked
    against the reference on the oracle's hsquare outputs"""
    from lincomb_ref import assert_ct, lincomb, synthetic_constants
    import square_ref
    L, ell, alpha = 6, 5, 2
    o = oracle(13, L, alpha)
    sq_ov = {"sq_scale": 1, "sq_const": 1, "N": 1 << 13}
    seeds = [SEED, SEED + 77]
    prods = [host.Op("config_4_N15.cfg", "hsquare", L, ell, alpha, overrides=dict(sq_ov, seed=s)) for s in seeds]
    for p in prods:
        p.execute(1)
    lseed = SEED + 31
    op = host.Op("config_4_N15.cfg", "hlincomb", L, ell - 1, alpha, overrides={"terms": 2, "lc_const": 1, "rescale": 0, "N": 1 << 13, "seed": lseed})
    op.bind_input("ct1", prods[0])
    op.bind_input("ct2", prods[1])
    op.execute(1)
    squares = [np.stack(square_ref.square(o, ell, *square_ref.synthetic_inputs(o, ell, s), *square_ref.synthetic_constants(o, ell, s, 1, 1))) for s in seeds]
    for p, e in zip(prods, squares):
        assert_ct(read_out(p), e, "producer")
    assert_ct(read_out(op), lincomb(o, ell - 1, squares, *synthetic_constants(o, ell - 1, lseed, 2, 1)), "two producers")
    wrong = host.Op("config_4_N15.cfg", "hlincomb", L, ell, alpha, overrides={"terms": 2, "N": 1 << 13})
    with pytest.raises(host.HostError, match="levels differ"):
        wrong.bind_input("ct2", prods[1])
    for x in (op, wrong, *prods):
        x.close()


def test_real_data_decrypts_to_the_linear_combination():
    """four fresh toy ciphertexts, small signed scalars and the constant c Delta written into the op: the output is the reference's bit for bit and
    decrypts to sum_t s_t m_t Delta + c Delta within sum_t |s_t| times the bound of one fresh error; the reference is held to it first"""
    from lincomb_ref import REAL_SCALARS, assert_ct, decryption_error, lincomb, real_case
    from toy_ckks import Toy
    LOGN, L, ELL, ALPHA = 13, 6, 5, 2
    o = oracle(LOGN, L, ALPHA)
    toy = Toy(o, seed=4247)
    cts, scales, const, exact = real_case(toy, ELL)
    ref = lincomb(o, ELL, cts, scales, const)
    ref_err, bound = decryption_error(toy, ref, ELL, exact)
    print(f"reference: max |dec - exact| = {ref_err} (bound {bound})")
    assert ref_err <= bound
    op = host.Op("config_4_N15.cfg", "hlincomb", L, ELL, ALPHA, overrides={"N": 1 << LOGN, "terms": len(REAL_SCALARS), "lc_const": 1})
    for t, s in enumerate(scales):          # (the constants first: writing a buffer prepares the op)
        op.set_constants(f"scale{t + 1}", s)
    op.set_constants("const", const)
    for t, ct in enumerate(cts):
        op.write(f"ct{t + 1}.c0", ct[0])
        op.write(f"ct{t + 1}.c1", ct[1])
    op.execute(1)
    out = read_out(op)
    op.close()
    gpu_err, _ = decryption_error(toy, out, ELL, exact)
    print(f"GPU: max |dec - exact| = {gpu_err} (bound {bound})")
    assert gpu_err <= bound
    assert_ct(out, ref, "real data")
