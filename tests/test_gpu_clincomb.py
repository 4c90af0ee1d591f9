"""hclincomb on the GPU, on both arithmetic back-ends (mont32 and chain_bits = 60), bit for bit:
 A. hm_clincomb through the ABI: against the reference's primitives (tests/clincomb_ref.py: MUL_CONST, MUL by the oracle's NTT of X^(N/2), ADD) and
    against the element-wise chain through hm_ewe with an uploaded U = -X^(N/2) on the same device data, on permuted and repeated input limbs with
    mixed moduli and a guard limb-poly; with null imaginary parts it is hm_lincomb; the refusals; n = 0; a captured call replayed;
 B. the op, fused (one CLINCOMB launch), unfused (one launch per stage) and with fuse_clincomb = 0, against the reference; batch 2, graph = 1,
    caller constants, the chain hreim -> hclincomb that gives back hreim's input, and real data (tests/toy_ckks.py)."""
import ctypes as C
import types

import numpy as np
import pytest

from homulator_amd import host
from oracle.homoracle import Oracle, chain_below

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


def kernel_lists(mods, T, moduli, rng, re="random", im="random", const="random", im_const=True):
    """per record T input limbs of its modulus from the pool (repeats allowed), T scalars of the named kinds in both parts and a constant in both
    parts (const None: no lists; im_const False: the real one only)"""
    n = len(mods)
    li = [mods[i] * PER_MOD + int(rng.integers(0, PER_MOD)) for i in range(n) for _ in range(T)]
    val = lambda kind, q: {"0": 0, "1": 1, "q-1": q - 1}[kind] if kind != "random" else int(rng.integers(0, q))
    a = [val(re, moduli[mods[i]]) for i in range(n) for _ in range(T)]
    b = [val(im, moduli[mods[i]]) for i in range(n) for _ in range(T)]
    kr = None if const is None else [val(const, moduli[m]) for m in mods]
    ki = None if const is None or not im_const else [val(const, moduli[m]) for m in mods]
    return li, a, b, kr, ki


def expected_rows(o, host_pool, mods, T, li, a, b, kr, ki):
    """the Python-side reference, from the reference's primitives: the terms by clincomb_poly (MUL_CONST, MUL by NTT(X^(N/2)), ADD), the real
    constant by numpy, the monomial constant as one more term k_im X^(N/2) 1 (a limb-poly of ones)"""
    from clincomb_ref import clincomb_poly
    n = len(mods)
    xs = [np.stack([host_pool[li[i * T + t]] for i in range(n)]) for t in range(T)]
    re = [[a[i * T + t] for i in range(n)] for t in range(T)]
    im = [[b[i * T + t] for i in range(n)] for t in range(T)]
    if ki is not None:
        xs, re, im = xs + [np.ones((n, o.N), dtype=np.uint64)], re + [[0] * n], im + [list(ki)]
    return clincomb_poly(o, list(mods), xs, re, im, kr)


def run_kernel_case(env, mods, T, seed, re="random", im="random", const="random", im_const=True, composed=True):
    """one hm_clincomb call: the output buffer holds n limb-polys and one guard limb-poly, the output list is a random permutation"""
    from homulator_amd import hip
    import reim_ref
    ctx, o, pool, host_pool = env
    n, N = len(mods), ctx.N
    rng = np.random.default_rng(seed)
    li, a, b, kr, ki = kernel_lists(mods, T, ctx.moduli, rng, re, im, const, im_const)
    perm = [int(v) for v in rng.permutation(n + 1)]
    lo = perm[:n]
    out = ctx.alloc(n + 1)
    out.upload(np.full((n + 1, N), GUARD, dtype=np.uint64))
    ctx.clincomb(pool, li, out, lo, mods, T, a, b, kr, ki)
    got = out.download()
    exp = expected_rows(o, host_pool, mods, T, li, a, b, kr, ki)
    what = (n, T, re, im, const)
    assert np.array_equal(got[lo], exp), what
    assert np.all(got[perm[n]] == GUARD), "the guard limb-poly was written"
    if T <= 3:   # the definition in Python integers on a stretch of some records: v = psi^(N/2) below N/2, q - v behind
        for i in sorted({0, n // 2, n - 1}):
            q = int(ctx.moduli[mods[i]])
            v = pow(int(o.psis[mods[i]]), N // 2, q)
            for x in (0, 1, N // 2 - 1, N // 2, N - 1):
                m = v if x < N // 2 else q - v
                k = (kr[i] if kr else 0) + (ki[i] * m if ki else 0)
                e = (sum((a[i * T + t] + b[i * T + t] * m) * int(host_pool[li[i * T + t]][x]) for t in range(T)) + k) % q
                assert int(got[lo[i]][x]) == e, (what, i, x)
    if composed and ki is None:   # the same from the calls it replaces, on the same device data, with the stored U = -X^(N/2)
        qs = [int(ctx.moduli[m]) for m in mods]
        unit = ctx.alloc(n)
        unit.upload(reim_ref.unit(o, list(mods)))
        acc, tre, tim = ctx.alloc(n), ctx.alloc(n), ctx.alloc(n)
        for t in range(T):
            la = [li[i * T + t] for i in range(n)]
            ctx.ewe(hip.OP_MUL_CONST, tre, mods, a=pool, la=la, k=[a[i * T + t] for i in range(n)])
            ctx.ewe(hip.OP_MUL, tim, mods, a=pool, la=la, b=unit)
            ctx.ewe(hip.OP_MUL_CONST, tim, mods, a=tim, k=[(qs[i] - b[i * T + t]) % qs[i] for i in range(n)])
            ctx.ewe(hip.OP_ADD, acc if t == 0 else tre, mods, a=tre, c=tim)
            if t:
                ctx.ewe(hip.OP_ADD, acc, mods, a=acc, c=tre)
        if kr is not None:
            ctx.ewe(hip.OP_ADD_CONST, acc, mods, a=acc, k=kr)
        assert np.array_equal(acc.download(), got[lo]), (what, "composed")
        for buf in (unit, acc, tre, tim):
            buf.free()
    out.free()


@pytest.mark.parametrize("chain", CHAINS)
@pytest.mark.parametrize("T", [1, 2, 3, 16])
@pytest.mark.parametrize("n", [1, 3, 65, 130])
def test_kernel_entry_and_term_counts(envs, chain, n, T):
    """ONE launch for any n (across the 64- and 128-entry cuts of the launches whose records travel as kernel arguments); T = 1 runs no round of
    the two-term loop, 2 the tail behind it, 3 one round, 16 the most; Q and P limbs, mixed moduli.  Once with both constants (the monomial one is
    the ABI's alone), once with the real constant only, which the element-wise chain can form: compared with it on the same device data"""
    mods = [(5 * i + 2) % (NQ + NP) for i in range(n)]
    run_kernel_case(envs(13, chain), mods, T, 40 + 17 * n + T)
    run_kernel_case(envs(13, chain), mods, T, 90 + 17 * n + T, im_const=False)


@pytest.mark.parametrize("chain", CHAINS)
def test_kernel_scalars_and_constants_at_the_ends_of_the_range(envs, chain):
    """every scalar kind (0, 1, q - 1, random) in the real part with every kind in the monomial part, the constant kinds (none, 0, q - 1, random)
    in turn, 5 records, T = 3 and T = 16"""
    mods = [0, NQ + NP - 1, 3, 0, NQ]
    kinds = ("0", "1", "q-1", "random")
    consts = (None, "0", "q-1", "random")
    i = 0
    for T in (3, 16):
        for re in kinds:
            for im in kinds:
                run_kernel_case(envs(13, chain), mods, T, 7 + i, re=re, im=im, const=consts[i % 4], im_const=(i % 3 == 0))
                i += 1


@pytest.mark.parametrize("chain", CHAINS)
@pytest.mark.parametrize("logN", [15, 16])
def test_kernel_at_larger_rings(envs, chain, logN):
    run_kernel_case(envs(logN, chain), [0, 5, NQ, 5, 2], 3, logN + 3, im_const=False)
    run_kernel_case(envs(logN, chain), [0, 5, NQ, 5, 2], 16, logN + 16, composed=False)


@pytest.mark.parametrize("chain", CHAINS)
@pytest.mark.parametrize("T", [1, 4, 16])
def test_with_null_imaginary_parts_it_is_hm_lincomb(envs, chain, T):
    ctx, o, pool, _ = envs(13, chain)
    mods = [(7 * i + 1) % (NQ + NP) for i in range(70)]
    li, a, _, kr, _ = kernel_lists(mods, T, ctx.moduli, np.random.default_rng(T))
    lin, cl, cl0 = ctx.alloc(70), ctx.alloc(70), ctx.alloc(70)
    ctx.lincomb(pool, li, lin, None, mods, T, a, kr)
    ctx.clincomb(pool, li, cl, None, mods, T, a, None, kr, None)
    ctx.clincomb(pool, li, cl0, None, mods, T, a, [0] * len(a), kr, [0] * 70)      # explicit zeros are the same call
    ref = lin.download()
    assert ref.any() and np.array_equal(cl.download(), ref) and np.array_equal(cl0.download(), ref)
    for buf in (lin, cl, cl0):
        buf.free()


def _alias_call(ctx, big, out_at=40, n=4, T=2):
    """n = 4 records of 2 terms in ONE allocation: the inputs are limbs 0 .. 7 through the allocation's base, the outputs n limbs from `out_at`
    through a base pointer of their own"""
    at = lambda limb: types.SimpleNamespace(ptr=big.limb_ptr(limb))
    ctx.clincomb(big, list(range(n * T)), at(out_at), None, [0] * n, T, [1] * (n * T), [2] * (n * T))


def test_refuses_an_output_over_an_input_through_another_base_pointer():
    from homulator_amd import hip
    ctx = hip.Context(13, NQ, NP)
    big = ctx.alloc(64)
    ctx.fill_uniform(big, [0] * 64, 5)
    _alias_call(ctx, big)                                   # disjoint: accepted
    for out_at in (7, 4, 0):
        with pytest.raises(hip.HmError, match=r"hm_clincomb: an output limb-poly \(out\) overlaps an input limb-poly \(in\)"):
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
    with pytest.raises(hip.HmError, match="hm_clincomb: null buffer"):
        ctx.clincomb(null, [0], out, [0], [0], 1, [1])
    with pytest.raises(hip.HmError, match="hm_clincomb: null buffer"):
        ctx.clincomb(src, [0], null, [0], [0], 1, [1])
    with pytest.raises(hip.HmError, match="hm_clincomb: scale_re is null"):
        ctx.clincomb(src, [0], out, [0], [0], 1, None, [1])
    with pytest.raises(hip.HmError, match="hm_clincomb: mod_ids is null"):
        ctx._ck(ctx.L.hm_clincomb(ctx.h, src.ptr, None, out.ptr, None, None, 1, 1, hip._u64([1])[1], None, None, None))
    for T in (0, 17):
        with pytest.raises(hip.HmError, match=rf"hm_clincomb: n_terms = {T}, must be in \[1, 16\]"):
            ctx.clincomb(src, [0] * T, out, [0], [0], T, [1] * max(T, 1))
    with pytest.raises(hip.HmError, match="65535"):
        ctx.clincomb(src, [0, 70000], out, [0], [0], 2, [1, 1])
    with pytest.raises(hip.HmError, match="65535"):
        ctx.clincomb(src, [0, 1], out, [70000], [0], 2, [1, 1])
    with pytest.raises(hip.HmError, match="mod id"):
        ctx.clincomb(src, [0], out, [0], [NQ + NP], 1, [1])
    with pytest.raises(hip.HmError, match=r"scale_re\[1\]\[0\] is not reduced"):
        ctx.clincomb(src, [0, 1, 2, 3], out, [0, 1], [0, 0], 2, [1, 0, q0, 1])
    with pytest.raises(hip.HmError, match=r"scale_im\[0\]\[1\] is not reduced"):
        ctx.clincomb(src, [0, 1, 2, 3], out, [0, 1], [0, 0], 2, [1, 0, 1, 1], [0, q0, 0, 0])
    with pytest.raises(hip.HmError, match=r"addend_re\[1\] is not reduced"):
        ctx.clincomb(src, [0, 1], out, [0, 1], [0, 0], 1, [1, 1], None, [0, q0])
    with pytest.raises(hip.HmError, match=r"addend_im\[0\] is not reduced"):
        ctx.clincomb(src, [0, 1], out, [0, 1], [0, 0], 1, [1, 1], None, None, [q0 + 5, 0])
    with pytest.raises(hip.HmError, match="two output"):
        ctx.clincomb(src, [0, 1], out, [2, 2], [0, 0], 1, [1, 1])
    with pytest.raises(hip.HmError, match="two output limb-polys overlap"):   # entries 0 and 2, apart in the list; no input touched
        ctx.clincomb(src, [0, 1, 2], out, [2, 0, 2], [0, 0, 0], 1, [1, 1, 1])
    with pytest.raises(hip.HmError, match="overlaps an input"):
        ctx.clincomb(src, [0, 1], src, [3, 1], [0, 0], 1, [1, 1])
    keep = [hip._u32([0]), hip._u64([1, 1, 1])]
    ctx._ck(ctx.L.hm_clincomb(ctx.h, src.ptr, None, out.ptr, None, keep[0][1], 0, 3, keep[1][1], None, None, None))   # n = 0: nothing to do
    ctx.clincomb(src, [0, 1, 1, 0], out, [3, 0], [0, 0], 2, [0, q0 - 1, 1, 0], [q0 - 1, 0, 0, 1], [0, q0 - 1], [q0 - 1, 0])   # nothing wrong: accepted
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
    li, a, b, kr, ki = kernel_lists(mods, T, ctx.moduli, rng)
    src, out = ctx.alloc(len(fill_mods)), ctx.alloc(len(mods))
    run = lambda: ctx.clincomb(src, li, out, None, mods, T, a, b, kr, ki)
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
    assert np.array_equal(out.download(), expected_rows(o, src.download(), mods, T, li, a, b, kr, ki)), chain
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
KEYS = [(1, 0, 0), (2, 1, 1), (4, 1, 0), (4, 0, 1)]     # (terms, cl_const, rescale): every T, both values of either key
_ref = {}


def reference(chain, logN, L, ell, alpha, keys, copy=0, seed=SEED):
    """the reference output on the op's synthetic inputs, computed once per case"""
    from clincomb_ref import clincomb, synthetic_constants
    from lincomb_ref import synthetic_inputs
    key = (chain, logN, L, ell, alpha, keys, copy, seed)
    if key not in _ref:
        T, cl, rs = keys
        o = oracle(logN, L, alpha, chain, threads=16)
        _ref[key] = clincomb(o, ell, synthetic_inputs(o, ell, seed, T, copy=copy), *synthetic_constants(o, ell, seed, T, cl), rescale=bool(rs))
    return _ref[key]


@pytest.mark.parametrize("chain", CHAINS)
@pytest.mark.parametrize("keys", KEYS)
@pytest.mark.parametrize("cfg,logN,L,ell,alpha,batch", SHAPES)
def test_op_fused_unfused_and_reference_agree(chain, keys, cfg, logN, L, ell, alpha, batch):
    """fused, unfused and fuse_clincomb = 0 against the reference; batch 2 (first shape): both copies, under the same constants"""
    from clincomb_ref import assert_ct
    T, cl, rs = keys
    ov = chain_ov(chain, {"terms": T, "cl_const": cl, "rescale": rs, "batch": batch, "N": 1 << logN})
    for mode, fuse, extra in (("fused", True, {}), ("unfused", False, {}), ("fuse_clincomb = 0", True, {"fuse_clincomb": 0})):
        op = host.Op(cfg, "hclincomb", L, ell, alpha, fuse=fuse, overrides=dict(ov, **extra))
        op.execute(1)
        kinds = [ln.split()[0] for ln in op.plan()]
        assert kinds.count("CLINCOMB") == (1 if mode == "fused" else 0), (mode, kinds)
        for c in range(batch):
            got = read_out(op, c)
            assert got[0].shape[0] == ell - rs
            assert_ct(got, reference(chain, logN, L, ell, alpha, keys, copy=c), (mode, keys, c))
        op.close()


def test_graph_replay_with_a_batch():
    """graph = 1: run 1 direct, run 2 captures, run 3 replays; both copies after the replay"""
    from clincomb_ref import assert_ct
    cfg, logN, L, ell, alpha, batch = SHAPES[0]
    keys = (2, 1, 1)
    op = host.Op(cfg, "hclincomb", L, ell, alpha, overrides={"terms": 2, "cl_const": 1, "rescale": 1, "batch": batch, "graph": 1})
    lc = [ln for ln in op.plan() if ln.startswith("CLINCOMB")]
    assert len(lc) == 1 and f" n={2 * batch * ell} " in lc[0] and " terms=2 const=1" in lc[0]
    for _ in range(3):
        op.execute(1)
    for c in range(batch):
        assert_ct(read_out(op, c), reference("mont32", logN, L, ell, alpha, keys, copy=c), f"copy {c}")
    op.close()


@pytest.mark.parametrize("chain", CHAINS)
@pytest.mark.parametrize("fuse", [True, False])
def test_caller_constants(chain, fuse):
    from clincomb_ref import assert_ct, clincomb
    from lincomb_ref import synthetic_inputs
    L, ell, alpha, T = 6, 5, 2, 3
    o = oracle(13, L, alpha, chain)
    q = [int(v) for v in o.moduli]
    re = [[2, q[1] - 1, 1, 12345, q[4] // 2], [0] * ell, [q[j] - 3 for j in range(ell)]]
    im = [[0] * ell, [1, q[1] - 1, 0, 54321, q[4] // 3], [q[j] - 2 for j in range(ell)]]
    const = [(7 << 40) % q[j] for j in range(ell)]
    op = host.Op("config_4_N15.cfg", "hclincomb", L, ell, alpha, fuse=fuse, overrides=chain_ov(chain, {"terms": T, "cl_const": 1, "N": 1 << 13}))
    for t in range(T):
        op.set_constants(f"scale{t + 1}", re[t])
        op.set_constants(f"scale_im{t + 1}", im[t])
    op.set_constants("const", const)
    op.execute(1)
    assert_ct(read_out(op), clincomb(o, ell, synthetic_inputs(o, ell, SEED, T), re, im, const), ("caller constants", chain, fuse))
    with pytest.raises(host.HostError, match=r'hclincomb: set_constants\("scale_im2"\) after prepare'):
        op.set_constants("scale_im2", im[1])
    op.close()


@pytest.mark.parametrize("chain", CHAINS)
def test_chain_reim_clincomb_gives_back_the_input(chain):
    """hreim -> hclincomb with ct1 = out under (h, 0) and ct2 = out_im under (0, h), h = (q_j + 1) / 2: h (ct + conj) + i h (-i) (ct - conj) = ct, so
    the output is hreim's ct1 bit for bit, on the device"""
    from clincomb_ref import assert_ct
    L, ell, alpha = 6, 5, 2
    o = oracle(13, L, alpha, chain)
    ov = chain_ov(chain, {"N": 1 << 13})
    src = host.Op("config_4_N15.cfg", "hreim", L, ell, alpha, overrides=ov)
    op = host.Op("config_4_N15.cfg", "hclincomb", L, ell, alpha, overrides=dict(ov, terms=2, seed=SEED + 31))
    h, zero = [(int(o.moduli[j]) + 1) // 2 for j in range(ell)], [0] * ell
    for name, v in (("scale1", h), ("scale_im1", zero), ("scale2", zero), ("scale_im2", h)):
        op.set_constants(name, v)
    op.bind_input("ct1", src)
    op.bind_input("ct2", src, output="out_im")
    src.execute(1)
    op.execute(1)
    assert [ln.split()[0] for ln in op.plan()] == ["CLINCOMB"]
    ct = (src.read("ct1.c0"), src.read("ct1.c1"))
    assert ct[0].any() and not np.array_equal(src.read("out.c0"), ct[0])
    assert_ct(read_out(op), ct, ("hreim -> hclincomb", chain))
    op.close()
    src.close()


def test_real_data_decrypts_to_the_complex_combination():
    """two fresh toy ciphertexts, the scalars 3 - 2i and 1 + 5i and the constant 7 Delta written into the op: the output is the reference's bit for
    bit and decrypts to sum_t (a_t + b_t X^(N/2)) m_t Delta + 7 Delta within sum_t (|a_t| + |b_t|) times the bound of one fresh error; the reference
    is held to it first"""
    from clincomb_ref import REAL_BOUND, REAL_SCALARS, assert_ct, decryption_error, real_reference
    LOGN, L, ELL, ALPHA = 13, 6, 5, 2
    _, toy, cts, re, im, const, ref, exact = real_reference(LOGN, L, ELL, ALPHA)
    ref_err = decryption_error(toy, ref, ELL, exact)
    print(f"reference: max |dec - exact| = {ref_err} (bound {REAL_BOUND})")
    assert ref_err <= REAL_BOUND
    op = host.Op("config_4_N15.cfg", "hclincomb", L, ELL, ALPHA, overrides={"N": 1 << LOGN, "terms": len(REAL_SCALARS), "cl_const": 1})
    for t in range(len(REAL_SCALARS)):      # (the constants first: writing a buffer prepares the op)
        op.set_constants(f"scale{t + 1}", re[t])
        op.set_constants(f"scale_im{t + 1}", im[t])
    op.set_constants("const", const)
    for t, ct in enumerate(cts):
        op.write(f"ct{t + 1}.c0", ct[0])
        op.write(f"ct{t + 1}.c1", ct[1])
    op.execute(1)
    out = read_out(op)
    op.close()
    gpu_err = decryption_error(toy, out, ELL, exact)
    print(f"GPU: max |dec - exact| = {gpu_err} (bound {REAL_BOUND})")
    assert gpu_err <= REAL_BOUND
    assert_ct(out, ref, "real data")
