"""hmuladd on the GPU, on both arithmetic back-ends (mont32 and chain_bits = 60), bit for bit:
 A. hm_tensor_muladd through the ABI: against the oracle's MUL / MAC2 / MUL_CONST / ADD (tests/muladd_ref.py's primitives) and against hm_tensor +
    MUL_CONST / ADD / ADD_CONST through hm_ewe on the same device data, on permuted and repeated limbs with mixed moduli and a guard limb-poly; the
    refusals; n = 0; a captured call replayed;
 B. the op, fused (one TENSOR_MULADD launch), unfused (one launch per stage) and with fuse_muladd = 0, against the reference; batch 2, graph = 1,
    caller constants, A = 0 against hmult's output, a chain hmuladd,hmuladd,hmult link by link, hsquare producers bound to ct1 and ct3, and the
    real-data case T_3 = 2 T_2 x - x (tests/toy_ckks.py)."""
import ctypes as C
import types

import numpy as np
import pytest

from homulator_amd import host
from oracle.homoracle import EWE_ADD, EWE_MAC2, EWE_MUL, EWE_MUL_CONST, Oracle, chain_below

pytestmark = pytest.mark.gpu
CHAINS = ["mont32", "survey"]
SEED = host.SEED
NQ, NP = 6, 3
PER_MOD = 4            # input limb-polys per modulus in the kernel cases: operand and addend lists draw from them with repetition
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
            ctx.fill_uniform(pool, [m for m in range(NQ + NP) for _ in range(PER_MOD)], 700 + logN)
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


def kernel_lists(mods, A, moduli, rng, scale="random", add_scale="random", const="random"):
    """per record the four operand limbs and the 2A addend limbs of its modulus from the pool (repeats allowed), a scalar, A addend scalars and a
    constant of the named kinds (scale / const None: no list)"""
    n = len(mods)
    draw = lambda i: mods[i] * PER_MOD + int(rng.integers(0, PER_MOD))
    ops = [[draw(i) for i in range(n)] for _ in range(4)]
    lx0 = [draw(i) for i in range(n) for _ in range(A)]
    lx1 = [draw(i) for i in range(n) for _ in range(A)]
    val = lambda kind, q, lo=0: {"0": 0, "1": 1, "2": 2, "q-1": q - 1}[kind] if kind != "random" else int(rng.integers(lo, q))
    s = None if scale is None else [val(scale, moduli[m], 1) for m in mods]
    u = [val(add_scale, moduli[mods[i]]) for i in range(n) for _ in range(A)]
    k = None if const is None else [val(const, moduli[m]) for m in mods]
    return ops, lx0, lx1, s, u, k


def expected_rows(o, host_pool, mods, A, ops, lx0, lx1, s, u, k):
    """the Python-side reference from the oracle's element-wise primitives, the constant by numpy: (d0, d1, d2), [n][N] each"""
    n = len(mods)
    rows = lambda limbs: np.stack([host_pool[x] for x in limbs])
    a, b, c, d = (rows(l) for l in ops)
    d0, d1, d2 = o.ewe(EWE_MUL, mods, a, b), o.ewe(EWE_MAC2, mods, a, d, c, b), o.ewe(EWE_MUL, mods, c, d)
    if s is not None:
        d0, d1, d2 = (o.ewe(EWE_MUL_CONST, mods, p, k=s) for p in (d0, d1, d2))
    for t in range(A):
        ut = [u[i * A + t] for i in range(n)]
        d0 = o.ewe(EWE_ADD, mods, d0, None, o.ewe(EWE_MUL_CONST, mods, rows([lx0[i * A + t] for i in range(n)]), k=ut))
        d1 = o.ewe(EWE_ADD, mods, d1, None, o.ewe(EWE_MUL_CONST, mods, rows([lx1[i * A + t] for i in range(n)]), k=ut))
    if k is not None:
        d0 = add_const_rows(d0, k, [o.moduli[m] for m in mods])
    return d0, d1, d2


def run_kernel_case(env, mods, A, seed, scale="random", add_scale="random", const="random", composed=True):
    """one hm_tensor_muladd call: the output buffer holds 3 n limb-polys and one guard limb-poly, the output lists are a random permutation"""
    from homulator_amd import hip
    ctx, o, pool, host_pool = env
    n, N = len(mods), ctx.N
    rng = np.random.default_rng(seed)
    ops, lx0, lx1, s, u, k = kernel_lists(mods, A, ctx.moduli, rng, scale, add_scale, const)
    perm = [int(v) for v in rng.permutation(3 * n + 1)]
    lo = [perm[:n], perm[n:2 * n], perm[2 * n:3 * n]]
    out = ctx.alloc(3 * n + 1)
    out.upload(np.full((3 * n + 1, N), GUARD, dtype=np.uint64))
    ctx.tensor_muladd(pool, pool, pool, pool, pool if A else None, out, out, out, mods, A, lx0 if A else None, lx1 if A else None, s, u if A else None, k,
                      limbs=ops + lo)
    got = out.download()
    exp = expected_rows(o, host_pool, mods, A, ops, lx0, lx1, s, u, k)
    what = (n, A, scale, add_scale, const)
    for i in range(3):
        assert np.array_equal(got[lo[i]], exp[i]), (what, f"d{i}")
    assert np.all(got[perm[3 * n]] == GUARD), "the guard limb-poly was written"
    for i in sorted({0, n // 2, n - 1}):   # the definition in Python integers on some entries of some records
        q = ctx.moduli[mods[i]]
        si, ki = (s[i] if s else 1), (k[i] if k else 0)
        for x in (0, 1, N - 1):
            a, b, c, d = (int(host_pool[l[i]][x]) for l in ops)
            e0 = (si * a * b + sum(u[i * A + t] * int(host_pool[lx0[i * A + t]][x]) for t in range(A)) + ki) % q
            e1 = (si * (a * d + c * b) + sum(u[i * A + t] * int(host_pool[lx1[i * A + t]][x]) for t in range(A))) % q
            assert (int(got[lo[0][i]][x]), int(got[lo[1][i]][x]), int(got[lo[2][i]][x])) == (e0, e1, si * c * d % q), (what, i, x)
    if composed:   # the same from the calls it replaces, on the same device data
        d, tmp = [ctx.alloc(n) for _ in range(3)], ctx.alloc(n)
        ctx.tensor(pool, pool, pool, pool, d[0], d[1], d[2], mods, limbs=ops + [None] * 3)
        if s is not None:
            for p in d:
                ctx.ewe(hip.OP_MUL_CONST, p, mods, a=p, k=s)
        for t in range(A):
            ut = [u[i * A + t] for i in range(n)]
            for p, lx in ((d[0], lx0), (d[1], lx1)):
                ctx.ewe(hip.OP_MUL_CONST, tmp, mods, a=pool, la=[lx[i * A + t] for i in range(n)], k=ut)
                ctx.ewe(hip.OP_ADD, p, mods, a=p, c=tmp)
        if k is not None:
            ctx.ewe(hip.OP_ADD_CONST, d[0], mods, a=d[0], k=k)
        for i in range(3):
            assert np.array_equal(d[i].download(), got[lo[i]]), (what, f"composed d{i}")
        for p in d + [tmp]:
            p.free()
    out.free()


@pytest.mark.parametrize("chain", CHAINS)
@pytest.mark.parametrize("A", [0, 1, 2, 3, 8])
@pytest.mark.parametrize("n", [1, 3, 65, 130])
def test_kernel_entry_and_addend_counts(envs, chain, n, A):
    """ONE launch for any n (across the 64- and 128-entry cuts of the launches whose records travel as kernel arguments); A = 0 and 1 run no round
    of the two-addend loop, 2 the tail behind it, 3 one round, 8 the most; Q and P limbs, mixed moduli"""
    run_kernel_case(envs(13, chain), [(5 * i + 2) % (NQ + NP) for i in range(n)], A, 40 + 17 * n + A)


@pytest.mark.parametrize("chain", CHAINS)
def test_kernel_scalars_and_constants_at_the_ends_of_the_range(envs, chain):
    """every scalar kind (none, 2, q - 1, random) with every addend-scalar kind (0, 1, q - 1, random) and constant kind (none, 0, q - 1, random),
    5 records, A = 3 and A = 8"""
    mods = [0, NQ + NP - 1, 3, 0, NQ]
    i = 0
    for A in (3, 8):
        for s, u, k in zip((None, "2", "q-1", "random") * 4, ("0", "1", "q-1", "random", "1", "q-1", "random", "0", "q-1", "random", "0", "1", "random", "0", "1", "q-1"),
                           (None, "0", "q-1", "random", "q-1", "random", None, "0", "0", None, "random", "q-1", "random", "q-1", "0", None)):
            run_kernel_case(envs(13, chain), mods, A, 7 + i, scale=s, add_scale=u, const=k, composed=(i % 5 == 3))
            i += 1
    run_kernel_case(envs(13, chain), mods, 8, 99, scale="q-1", add_scale="q-1", const="q-1")


@pytest.mark.parametrize("chain", CHAINS)
@pytest.mark.parametrize("logN", [15, 16])
def test_kernel_at_larger_rings(envs, chain, logN):
    run_kernel_case(envs(logN, chain), [0, 5, NQ, 5, 2], 3, logN)


def _alias_call(ctx, big, out_at=40, n=2, x_at=8):
    """n = 2 records of 1 addend in ONE allocation: the operands are limbs 0 .. 7, the addend components from limb x_at on, all through the
    allocation's base; the outputs 3 n limbs from `out_at` through a base pointer of their own"""
    at = lambda limb: types.SimpleNamespace(ptr=big.limb_ptr(limb))
    o = at(out_at)
    ctx.tensor_muladd(big, big, big, big, big, o, o, o, [0] * n, 1, [x_at, x_at + 1], [x_at + 2, x_at + 3], None, [1] * n, None,
                      limbs=[[0, 1], [2, 3], [4, 5], [6, 7], [0, 1], [2, 3], [4, 5]])


def test_refuses_an_output_over_an_input_through_another_base_pointer():
    from homulator_amd import hip
    ctx = hip.Context(13, NQ, NP)
    big = ctx.alloc(64)
    ctx.fill_uniform(big, [0] * 64, 5)
    _alias_call(ctx, big)                                   # disjoint: accepted
    for out_at in (7, 4, 0, 2):
        with pytest.raises(hip.HmError, match=r"hm_tensor_muladd: an output limb-poly \(o\d\) overlaps an input limb-poly \(\w\)"):
            _alias_call(ctx, big, out_at=out_at)
    with pytest.raises(hip.HmError, match=r"hm_tensor_muladd: an output limb-poly \(o\d\) overlaps an input limb-poly \(x\)"):
        _alias_call(ctx, big, out_at=40, x_at=43)           # an addend component under an output
    ctx.sync()
    ctx.close()


def test_refuses_bad_arguments_and_accepts_n_0():
    from homulator_amd import hip
    ctx = hip.Context(13, NQ, NP)
    src, out = ctx.alloc(8), ctx.alloc(6)
    ctx.fill_uniform(src, [0] * 8, 5)
    q0 = ctx.moduli[0]
    null = types.SimpleNamespace(ptr=None)
    ok = dict(limbs=[[0], [1], [2], [3], [0], [1], [2]])
    call = lambda a=src, b=src, c=src, d=src, x=src, o0=out, o1=out, o2=out, mods=(0,), A=1, lx0=(4,), lx1=(5,), s=None, u=(1,), k=None, limbs=None: \
        ctx.tensor_muladd(a, b, c, d, x, o0, o1, o2, list(mods), A, None if lx0 is None else list(lx0), None if lx1 is None else list(lx1), s,
                          None if u is None else list(u), k, limbs=limbs or ok["limbs"])
    for kw in ("a", "b", "c", "d", "o0", "o1", "o2"):
        with pytest.raises(hip.HmError, match="hm_tensor_muladd: null buffer"):
            call(**{kw: null})
    with pytest.raises(hip.HmError, match="hm_tensor_muladd: null buffer"):
        call(x=None)
    with pytest.raises(hip.HmError, match="hm_tensor_muladd: x0_limbs or x1_limbs is null"):
        call(lx0=None)
    with pytest.raises(hip.HmError, match="hm_tensor_muladd: x0_limbs or x1_limbs is null"):
        call(lx1=None)
    with pytest.raises(hip.HmError, match="hm_tensor_muladd: add_scale is null"):
        call(u=None)
    with pytest.raises(hip.HmError, match="hm_tensor_muladd: mod_ids is null"):
        ctx._ck(ctx.L.hm_tensor_muladd(ctx.h, src.ptr, None, src.ptr, None, src.ptr, None, src.ptr, None, None, None, None, out.ptr, None, out.ptr, None,
                                       out.ptr, None, None, 1, 0, None, None, None))
    with pytest.raises(hip.HmError, match=r"hm_tensor_muladd: n_addends = 9, must be in \[0, 8\]"):
        call(A=9, lx0=[4] * 9, lx1=[5] * 9, u=[1] * 9)
    with pytest.raises(hip.HmError, match="65535"):
        call(limbs=[[70000], [1], [2], [3], [0], [1], [2]])
    with pytest.raises(hip.HmError, match="65535"):
        call(limbs=[[0], [1], [2], [3], [0], [1], [70000]])
    with pytest.raises(hip.HmError, match="65535"):
        call(lx1=[70000])
    with pytest.raises(hip.HmError, match="mod id"):
        call(mods=[NQ + NP])
    with pytest.raises(hip.HmError, match=r"scale\[0\] is not reduced"):
        call(s=[q0])
    with pytest.raises(hip.HmError, match=r"scale\[0\] is zero"):
        call(s=[0])
    with pytest.raises(hip.HmError, match=r"add_scale\[0\]\[1\] is not reduced"):
        call(A=2, lx0=[4, 6], lx1=[5, 7], u=[0, q0])
    with pytest.raises(hip.HmError, match=r"addend\[0\] is not reduced"):
        call(k=[q0])
    with pytest.raises(hip.HmError, match="two output"):
        call(limbs=[[0], [1], [2], [3], [0], [1], [1]])
    with pytest.raises(hip.HmError, match="two output limb-polys overlap"):   # two entries: entry 0 of o1 and entry 1 of o2, no input touched
        call(mods=(0, 0), lx0=(4, 6), lx1=(5, 7), u=(1, 1), limbs=[[0, 0], [1, 1], [2, 2], [3, 3], [0, 1], [2, 3], [4, 2]])
    with pytest.raises(hip.HmError, match="overlaps an input"):
        call(o1=src, limbs=[[0], [1], [2], [3], [0], [5], [2]])
    keep = [hip._u32([0])]
    ctx._ck(ctx.L.hm_tensor_muladd(ctx.h, src.ptr, None, src.ptr, None, src.ptr, None, src.ptr, None, None, None, None, out.ptr, None, out.ptr, None,
                                   out.ptr, None, keep[0][1], 0, 0, None, None, None))   # n = 0: nothing to do
    call(A=0, x=None, lx0=None, lx1=None, u=None)                    # all four may be null without addends
    call(s=[q0 - 1], u=[0], k=[q0 - 1])                              # and a call with nothing wrong is accepted
    ctx.sync()
    ctx.close()


@pytest.mark.parametrize("chain", CHAINS)
def test_a_captured_call_replays(envs, chain):
    """the records live in a cached device table: after one warm run the call is captured into a graph and replayed on new input data"""
    ctx, o, _, _ = envs(13, chain)
    ctx.L.hm_graph_launch.argtypes = [C.c_void_p, C.c_void_p]
    ctx.L.hm_graph_destroy.argtypes = [C.c_void_p]
    A = 3
    mods = [(3 * i + 1) % (NQ + NP) for i in range(70)]
    n = len(mods)
    fill_mods = [m for m in range(NQ + NP) for _ in range(PER_MOD)]
    rng = np.random.default_rng(3)
    ops, lx0, lx1, s, u, k = kernel_lists(mods, A, ctx.moduli, rng)
    src, out = ctx.alloc(len(fill_mods)), ctx.alloc(3 * n)
    lo = [list(range(n)), list(range(n, 2 * n)), list(range(2 * n, 3 * n))]
    run = lambda: ctx.tensor_muladd(src, src, src, src, src, out, out, out, mods, A, lx0, lx1, s, u, k, limbs=ops + lo)
    ctx.fill_uniform(src, fill_mods, 1)
    run()
    g = C.c_void_p()
    ctx._ck(ctx.L.hm_capture_begin(ctx.h))
    run()
    ctx._ck(ctx.L.hm_capture_end(ctx.h, C.byref(g)))
    ctx.fill_uniform(src, fill_mods, 2)
    out.upload(np.full((3 * n, ctx.N), GUARD, dtype=np.uint64))
    ctx._ck(ctx.L.hm_graph_launch(ctx.h, g))
    ctx.sync()
    got = out.download()
    exp = expected_rows(o, src.download(), mods, A, ops, lx0, lx1, s, u, k)
    for i in range(3):
        assert np.array_equal(got[lo[i]], exp[i]), (chain, i)
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
KEYS = [(0, 0, 0), (1, 1, 1), (3, 1, 0), (3, 0, 1)]     # (addends, ma_scale, ma_const): every A, both values of either key
_ref = {}


def reference(chain, logN, L, ell, alpha, keys, copy=0, seed=SEED):
    """the reference output on the op's synthetic inputs, computed once per case"""
    from muladd_ref import muladd, synthetic_constants, synthetic_inputs
    key = (chain, logN, L, ell, alpha, keys, copy, seed)
    if key not in _ref:
        A, ms, mc = keys
        o = oracle(logN, L, alpha, chain, threads=16)
        ct1, ct2, adds, evk = synthetic_inputs(o, ell, seed, A, copy=copy)
        scale, us, const = synthetic_constants(o, ell, seed, A, ms, mc)
        _ref[key] = muladd(o, ell, ct1, ct2, evk, adds, scale, us, const)
    return _ref[key]


@pytest.mark.parametrize("chain", CHAINS)
@pytest.mark.parametrize("keys", KEYS)
@pytest.mark.parametrize("cfg,logN,L,ell,alpha,batch", SHAPES)
def test_op_fused_unfused_and_reference_agree(chain, keys, cfg, logN, L, ell, alpha, batch):
    """fused, unfused and fuse_muladd = 0 against the reference; batch 2 (first shape): both copies, under the same constants"""
    from muladd_ref import assert_ct
    A, ms, mc = keys
    ov = chain_ov(chain, {"addends": A, "ma_scale": ms, "ma_const": mc, "batch": batch, "N": 1 << logN})
    for mode, fuse, extra in (("fused", True, {}), ("unfused", False, {}), ("fuse_muladd = 0", True, {"fuse_muladd": 0})):
        op = host.Op(cfg, "hmuladd", L, ell, alpha, fuse=fuse, overrides=dict(ov, **extra))
        op.execute(1)
        kinds = [ln.split()[0] for ln in op.plan()]
        assert kinds.count("TENSOR_MULADD") == (1 if mode == "fused" else 0), (mode, kinds)
        for c in range(batch):
            got = read_out(op, c)
            assert got[0].shape[0] == ell - 1
            assert_ct(got, reference(chain, logN, L, ell, alpha, keys, copy=c), (mode, keys, c))
        op.close()


@pytest.mark.parametrize("chain", CHAINS)
def test_without_addends_and_constants_it_is_hmult(chain):
    from muladd_ref import assert_ct
    cfg, logN, L, ell, alpha, _ = SHAPES[1]
    ov = chain_ov(chain, {"N": 1 << logN})
    hm = host.Op(cfg, "hmult", L, ell, alpha, overrides=ov)
    hm.execute(1)
    op = host.Op(cfg, "hmuladd", L, ell, alpha, overrides=dict(ov, addends=0))
    op.execute(1)
    assert_ct(read_out(op), read_out(hm), "A = 0, both keys 0: hmult")
    hm.close(); op.close()


def test_graph_replay_with_a_batch():
    """graph = 1: run 1 direct, run 2 captures, run 3 replays; both copies after the replay"""
    from muladd_ref import assert_ct
    cfg, logN, L, ell, alpha, batch = SHAPES[0]
    keys = (3, 1, 1)
    op = host.Op(cfg, "hmuladd", L, ell, alpha, overrides={"addends": 3, "ma_scale": 1, "ma_const": 1, "batch": batch, "graph": 1})
    ma = [ln for ln in op.plan() if ln.startswith("TENSOR_MULADD")]
    assert len(ma) == 1 and f" n={batch * ell} " in ma[0] and " addends=3 scale=1 const=1" in ma[0]
    for _ in range(3):
        op.execute(1)
    for c in range(batch):
        assert_ct(read_out(op, c), reference("mont32", logN, L, ell, alpha, keys, copy=c), f"copy {c}")
    op.close()


@pytest.mark.parametrize("chain", CHAINS)
@pytest.mark.parametrize("fuse", [True, False])
def test_caller_constants(chain, fuse):
    from muladd_ref import assert_ct, muladd, synthetic_inputs
    L, ell, alpha, A = 6, 5, 2, 3
    o = oracle(13, L, alpha, chain)
    scale = [2, o.moduli[1] - 1, 1, 12345, o.moduli[4] // 2]
    us = [[3, o.moduli[1] - 1, 1, 54321, o.moduli[4] // 3], [0] * ell, [o.moduli[j] - 3 for j in range(ell)]]
    const = [(7 << 40) % o.moduli[j] for j in range(ell)]
    op = host.Op("config_4_N15.cfg", "hmuladd", L, ell, alpha, fuse=fuse, overrides=chain_ov(chain, {"addends": A, "ma_scale": 1, "ma_const": 1, "N": 1 << 13}))
    op.set_constants("scale", scale)
    for t in range(A):
        op.set_constants(f"addscale{t + 1}", us[t])
    op.set_constants("const", const)
    op.execute(1)
    ct1, ct2, adds, evk = synthetic_inputs(o, ell, SEED, A)
    assert_ct(read_out(op), muladd(o, ell, ct1, ct2, evk, adds, scale, us, const), ("caller constants", chain, fuse))
    with pytest.raises(host.HostError, match=r'hmuladd: set_constants\("addscale2"\) after prepare'):
        op.set_constants("addscale2", us[1])
    op.close()


def test_chain_muladd_muladd_hmult_link_by_link():
    """hmuladd,hmuladd,hmult at N = 2^13: link k runs under seed + 31 k (OpChain): its further inputs, its key and its constants are drawn from
    there, its ct1 is the link before's output, and the levels follow"""
    from muladd_ref import assert_ct, muladd, synthetic_constants, synthetic_inputs
    L, ell, alpha, A = 6, 5, 2, 2
    o = oracle(13, L, alpha)
    chain = host.Chain("config_4_N15.cfg", "hmuladd,hmuladd,hmult", L, ell, alpha, overrides={"addends": A, "ma_scale": 1, "ma_const": 1, "N": 1 << 13})
    chain.execute(1)
    ct = None
    for k in range(2):
        lvl, seed = ell - k, SEED + 31 * k
        ct1, ct2, adds, evk = synthetic_inputs(o, lvl, seed, A)
        if ct is not None:
            ct1 = ct
        out = muladd(o, lvl, ct1, ct2, evk, adds, *synthetic_constants(o, lvl, seed, A, 1, 1))
        assert [ln.split()[0] for ln in chain[k].plan()].count("TENSOR_MULADD") == 1
        assert_ct(read_out(chain[k]), out, f"link {k}")
        ct = np.stack(out)
    lvl, seed = ell - 2, SEED + 62
    assert_ct(read_out(chain[2]), o.hmult(lvl, ct, o.synth_ct(lvl, seed + 2000), o.synth_evk(lvl, seed + 10000)), "link 2 (hmult)")
    chain.close()


def test_squares_bound_to_ct1_and_ct3():
    """two hsquare ops with different seeds produce ct1 and ct3 of an hmuladd with one addend, checked against the reference on the oracle's hsquare
    outputs; ct2 stays synthetic"""
    from muladd_ref import assert_ct, muladd, synthetic_constants
    import square_ref
    L, ell, alpha = 6, 5, 2
    o = oracle(13, L, alpha)
    sq_ov = {"sq_scale": 1, "sq_const": 1, "N": 1 << 13}
    seeds = [SEED, SEED + 77]
    prods = [host.Op("config_4_N15.cfg", "hsquare", L, ell, alpha, overrides=dict(sq_ov, seed=s)) for s in seeds]
    for p in prods:
        p.execute(1)
    mseed = SEED + 31
    op = host.Op("config_4_N15.cfg", "hmuladd", L, ell - 1, alpha, overrides={"addends": 1, "ma_scale": 1, "ma_const": 1, "N": 1 << 13, "seed": mseed})
    op.bind_input("ct1", prods[0])
    op.bind_input("ct3", prods[1])
    op.execute(1)
    squares = [np.stack(square_ref.square(o, ell, *square_ref.synthetic_inputs(o, ell, s), *square_ref.synthetic_constants(o, ell, s, 1, 1))) for s in seeds]
    for p, e in zip(prods, squares):
        assert_ct(read_out(p), e, "producer")
    scale, us, const = synthetic_constants(o, ell - 1, mseed, 1, 1, 1)
    exp = muladd(o, ell - 1, squares[0], o.synth_ct(ell - 1, mseed + 2000), o.synth_evk(ell - 1, mseed + 10000), [squares[1]], scale, us, const)
    assert_ct(read_out(op), exp, "two producers")
    wrong = host.Op("config_4_N15.cfg", "hmuladd", L, ell, alpha, overrides={"N": 1 << 13})
    with pytest.raises(host.HostError, match="levels differ"):
        wrong.bind_input("ct3", prods[1])
    for x in (op, wrong, *prods):
        x.close()


def test_ct2_bound_to_ct1s_data_is_hsquare():
    """ct1 and ct2 bound to the same producer, A = 0, with hsquare's constants: hsquare's output bit for bit"""
    from muladd_ref import assert_ct
    L, ell, alpha = 6, 5, 2
    o = oracle(13, L, alpha)
    ov = {"N": 1 << 13}
    prod = host.Op("config_4_N15.cfg", "hsquare", L, ell, alpha, overrides=ov)
    prod.execute(1)
    seed = SEED + 31
    scale = [int(o.moduli[j]) - 2 for j in range(ell - 1)]
    const = [(5 << 40) % o.moduli[j] for j in range(ell - 1)]
    sq = host.Op("config_4_N15.cfg", "hsquare", L, ell - 1, alpha, overrides=dict(ov, sq_scale=1, sq_const=1, seed=seed))
    ma = host.Op("config_4_N15.cfg", "hmuladd", L, ell - 1, alpha, overrides=dict(ov, addends=0, ma_scale=1, ma_const=1, seed=seed))
    for op, names in ((sq, ["ct1"]), (ma, ["ct1", "ct2"])):
        op.set_constants("scale", scale)
        op.set_constants("const", const)
        for nm in names:
            op.bind_input(nm, prod)
        op.execute(1)
    assert_ct(read_out(ma), read_out(sq), "hmuladd(ct, ct) against hsquare(ct)")
    for x in (sq, ma, prod):
        x.close()


def test_real_data_t3():
    """T_3 = 2 T_2 x - x on toy-scheme data: an hsquare op (T_2 = 2 x^2 - 1, level 5) bound to ct1 of an hmuladd at level 4, x written into ct2 and
    ct3, the keys written.  The output is the reference's bit for bit and decrypts within the bound the reference met (tests/muladd_ref.py)"""
    from muladd_ref import assert_ct, decryption_error, muladd, real_case
    from square_ref import square
    from toy_ckks import Toy
    LOGN, L, ELL, ALPHA = 13, 6, 5, 2
    o = oracle(LOGN, L, ALPHA)
    toy = Toy(o, seed=4247)
    x, evk_full, sq_scale, sq_const, scale, u1, D, exact = real_case(toy, ELL)
    evk5, evk4 = toy.evk_at_level(evk_full, ELL), toy.evk_at_level(evk_full, ELL - 1)
    x4 = np.ascontiguousarray(x[:, :ELL - 1])
    t2 = square(o, ELL, x, evk5, sq_scale, sq_const)
    ref = muladd(o, ELL - 1, np.stack(t2), x4, evk4, [x4], scale, [u1], None)
    ref_err, bound = decryption_error(toy, ref, ELL, D, exact)
    print(f"reference: max |dec q_3 q_4 - exact| = 2^{ref_err.bit_length()} (bound 2^{bound.bit_length() - 1})")
    assert ref_err <= bound

    def write_keys(op, evk):
        for j in range(evk.shape[0]):
            for k in range(2):
                op.write(f"IP_Key{k}_{j}", evk[j][k])

    sq = host.Op("config_4_N15.cfg", "hsquare", L, ELL, ALPHA, overrides={"N": 1 << LOGN, "sq_scale": 1, "sq_const": 1})
    sq.set_constants("scale", sq_scale)          # (the constants first: writing a buffer prepares the op)
    sq.set_constants("const", sq_const)
    sq.write("ct1.c0", x[0])
    sq.write("ct1.c1", x[1])
    write_keys(sq, evk5)
    sq.execute(1)
    assert_ct(read_out(sq), t2, "T_2")
    op = host.Op("config_4_N15.cfg", "hmuladd", L, ELL - 1, ALPHA, overrides={"N": 1 << LOGN, "addends": 1, "ma_scale": 1})
    op.set_constants("scale", scale)
    op.set_constants("addscale1", u1)
    op.bind_input("ct1", sq)
    for name in ("ct2", "ct3"):
        op.write(f"{name}.c0", x4[0])
        op.write(f"{name}.c1", x4[1])
    write_keys(op, evk4)
    op.execute(1)
    out = read_out(op)
    op.close(); sq.close()
    gpu_err, _ = decryption_error(toy, out, ELL, D, exact)
    print(f"GPU: max |dec q_3 q_4 - exact| = 2^{gpu_err.bit_length()} (bound 2^{bound.bit_length() - 1})")
    assert gpu_err <= bound
    assert_ct(out, ref, "real data")
