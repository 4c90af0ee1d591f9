"""hdotadd on the GPU, on both arithmetic back-ends (mont32 and chain_bits = 60), bit for bit:
 A. hm_tensor_dotadd through the ABI: against the oracle's MUL / MAC2 / MUL_CONST / ADD (tests/dotadd_ref.py's primitives) and against hm_tensor +
    MUL_CONST / ADD / ADD_CONST through hm_ewe on the same device data, on permuted and repeated limbs with mixed moduli and a guard limb-poly, the
    addends in an allocation of their own and once in the operands'; A = 0 without scalars against hm_tensor_dot and T = 1 against hm_tensor_muladd
    on the same data; the refusals; n = 0; a captured call replayed;
 B. the op, fused (one TENSOR_DOTADD launch), unfused (one launch per stage) and with fuse_dotadd = 0, against the reference; batch 2, graph = 1,
    caller constants, A = 0 without keys against hdot's output, T = 1 against hmuladd's, both outputs of an hreim bound to the pairs of
    re^2 - im^2 link by link, and the real-data case 3 m1 m2 - 2 m3 m4 + 5 m5 + 7 (tests/toy_ckks.py)."""
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
TA = [(1, 0), (1, 1), (2, 1), (2, 2), (3, 3), (16, 8)]
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
    """(hip context, oracle on the same moduli, the operand pool and the addend pool on the device and on the host) per (logN, chain), made on
    first use.  Either pool holds PER_MOD limb-polys per modulus, limb m * PER_MOD + r filled for modulus m; they are never written again"""
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
            fill_mods = [m for m in range(NQ + NP) for _ in range(PER_MOD)]
            pool, xpool = ctx.alloc(len(fill_mods)), ctx.alloc(len(fill_mods))
            ctx.fill_uniform(pool, fill_mods, 700 + logN)
            ctx.fill_uniform(xpool, fill_mods, 900 + logN)
            made[(logN, chain)] = (ctx, o, pool, pool.download(), xpool, xpool.download())
        return made[(logN, chain)]
    yield get
    for ctx, _, pool, _, xpool, _ in made.values():
        pool.free()
        xpool.free()
        ctx.close()


def add_const_rows(x, ks, qs):
    out = np.empty_like(x)
    for i, (k, q) in enumerate(zip(ks, qs)):
        t = x[i] + np.uint64(k)
        out[i] = np.where(t >= np.uint64(q), t - np.uint64(q), t)
    return out


MIXED = ["1", "2", "q-1", "random"]


def kernel_lists(mods, T, A, moduli, rng, scale="random", add_scale="random", const="random"):
    """per record the 4T operand limbs and the 2A addend limbs of its modulus from the pools (repeats allowed), T pair scalars, A addend scalars and
    a constant of the named kinds (scale / const None: no list; scale "mixed": 1, 2, q - 1, random by pair)"""
    n = len(mods)
    draw = lambda i: mods[i] * PER_MOD + int(rng.integers(0, PER_MOD))
    ops = [[draw(i) for i in range(n) for _ in range(T)] for _ in range(4)]
    lx0 = [draw(i) for i in range(n) for _ in range(A)]
    lx1 = [draw(i) for i in range(n) for _ in range(A)]
    val = lambda kind, q, lo=0: {"0": 0, "1": 1, "2": 2, "q-1": q - 1}[kind] if kind != "random" else int(rng.integers(lo, q))
    s = None if scale is None else [val(MIXED[t % 4] if scale == "mixed" else scale, moduli[m], 1) for m in mods for t in range(T)]
    u = [val(add_scale, moduli[mods[i]]) for i in range(n) for _ in range(A)]
    k = None if const is None else [val(const, moduli[m]) for m in mods]
    return ops, lx0, lx1, s, u, k


def expected_rows(o, host_pool, host_x, mods, T, A, ops, lx0, lx1, s, u, k):
    """the Python-side reference from the oracle's element-wise primitives, the constant by numpy: (d0, d1, d2), [n][N] each"""
    n = len(mods)
    rows = lambda pool, limbs: np.stack([pool[x] for x in limbs])
    d = None
    for t in range(T):
        a, b, c, dd = (rows(host_pool, [l[i * T + t] for i in range(n)]) for l in ops)
        p = (o.ewe(EWE_MUL, mods, a, b), o.ewe(EWE_MAC2, mods, a, dd, c, b), o.ewe(EWE_MUL, mods, c, dd))
        if s is not None:
            p = tuple(o.ewe(EWE_MUL_CONST, mods, v, k=[s[i * T + t] for i in range(n)]) for v in p)
        d = p if d is None else tuple(o.ewe(EWE_ADD, mods, v, None, w) for v, w in zip(d, p))
    d0, d1, d2 = d
    for r in range(A):
        ur = [u[i * A + r] for i in range(n)]
        d0 = o.ewe(EWE_ADD, mods, d0, None, o.ewe(EWE_MUL_CONST, mods, rows(host_x, [lx0[i * A + r] for i in range(n)]), k=ur))
        d1 = o.ewe(EWE_ADD, mods, d1, None, o.ewe(EWE_MUL_CONST, mods, rows(host_x, [lx1[i * A + r] for i in range(n)]), k=ur))
    if k is not None:
        d0 = add_const_rows(d0, k, [o.moduli[m] for m in mods])
    return d0, d1, d2


def run_kernel_case(env, mods, T, A, seed, scale="mixed", add_scale="random", const="random", composed=True, addends_in_operand_pool=False):
    """one hm_tensor_dotadd call: the output buffer holds 3 n limb-polys and one guard limb-poly, the output lists are a random permutation"""
    from homulator_amd import hip
    ctx, o, pool, host_pool, xpool, host_x = env
    if addends_in_operand_pool:
        xpool, host_x = pool, host_pool
    n, N = len(mods), ctx.N
    rng = np.random.default_rng(seed)
    ops, lx0, lx1, s, u, k = kernel_lists(mods, T, A, ctx.moduli, rng, scale, add_scale, const)
    perm = [int(v) for v in rng.permutation(3 * n + 1)]
    lo = [perm[:n], perm[n:2 * n], perm[2 * n:3 * n]]
    out = ctx.alloc(3 * n + 1)
    out.upload(np.full((3 * n + 1, N), GUARD, dtype=np.uint64))
    ctx.tensor_dotadd(pool, pool, pool, pool, xpool if A else None, out, out, out, mods, T, A, lx0 if A else None, lx1 if A else None, s, u if A else None,
                      k, limbs=ops + lo)
    got = out.download()
    exp = expected_rows(o, host_pool, host_x, mods, T, A, ops, lx0, lx1, s, u, k)
    what = (n, T, A, scale, add_scale, const)
    for i in range(3):
        assert np.array_equal(got[lo[i]], exp[i]), (what, f"d{i}")
    assert np.all(got[perm[3 * n]] == GUARD), "the guard limb-poly was written"
    for i in sorted({0, n // 2, n - 1}):   # the definition in Python integers on some entries of some records
        q = ctx.moduli[mods[i]]
        ki = k[i] if k else 0
        for x in (0, 1, N - 1):
            e0, e1, e2 = ki, 0, 0
            for t in range(T):
                st = s[i * T + t] if s else 1
                a, b, c, d = (int(host_pool[l[i * T + t]][x]) for l in ops)
                e0, e1, e2 = e0 + st * a * b, e1 + st * (a * d + c * b), e2 + st * c * d
            e0 += sum(u[i * A + r] * int(host_x[lx0[i * A + r]][x]) for r in range(A))
            e1 += sum(u[i * A + r] * int(host_x[lx1[i * A + r]][x]) for r in range(A))
            assert (int(got[lo[0][i]][x]), int(got[lo[1][i]][x]), int(got[lo[2][i]][x])) == (e0 % q, e1 % q, e2 % q), (what, i, x)
    if composed:   # the same from the calls it replaces, on the same device data
        d, p, tmp = [ctx.alloc(n) for _ in range(3)], [ctx.alloc(n) for _ in range(3)], ctx.alloc(n)
        for t in range(T):
            dst = d if t == 0 else p
            ctx.tensor(pool, pool, pool, pool, dst[0], dst[1], dst[2], mods, limbs=[[l[i * T + t] for i in range(n)] for l in ops] + [None] * 3)
            if s is not None:
                for v in dst:
                    ctx.ewe(hip.OP_MUL_CONST, v, mods, a=v, k=[s[i * T + t] for i in range(n)])
            if t:
                for v, w in zip(d, p):
                    ctx.ewe(hip.OP_ADD, v, mods, a=v, c=w)
        for r in range(A):
            ur = [u[i * A + r] for i in range(n)]
            for v, lx in ((d[0], lx0), (d[1], lx1)):
                ctx.ewe(hip.OP_MUL_CONST, tmp, mods, a=xpool, la=[lx[i * A + r] for i in range(n)], k=ur)
                ctx.ewe(hip.OP_ADD, v, mods, a=v, c=tmp)
        if k is not None:
            ctx.ewe(hip.OP_ADD_CONST, d[0], mods, a=d[0], k=k)
        for i in range(3):
            assert np.array_equal(d[i].download(), got[lo[i]]), (what, f"composed d{i}")
        for v in d + p + [tmp]:
            v.free()
    out.free()


@pytest.mark.parametrize("chain", CHAINS)
@pytest.mark.parametrize("T,A", TA)
@pytest.mark.parametrize("n", [1, 3, 65, 130])
def test_kernel_entry_pair_and_addend_counts(envs, chain, n, T, A):
    """ONE launch for any n (across the 64- and 128-entry cuts of the launches whose records travel as kernel arguments); (T, A): no round of either
    term loop, addend 0 under the pairs, one tail, both tails, one round of both, the most; Q and P limbs, mixed moduli, mixed scalars in a record"""
    run_kernel_case(envs(13, chain), [(5 * i + 2) % (NQ + NP) for i in range(n)], T, A, 40 + 17 * n + 5 * T + A, composed=(n <= 65))


@pytest.mark.parametrize("chain", CHAINS)
def test_kernel_scalars_and_constants_at_the_ends_of_the_range(envs, chain):
    """every pair-scalar kind (none, 2, q - 1, random, mixed) with every addend-scalar kind (0, 1, q - 1, random) and constant kind (none, 0, q - 1,
    random), 5 records, (3, 3) and (16, 8); the addends once in the operands' allocation"""
    mods = [0, NQ + NP - 1, 3, 0, NQ]
    i = 0
    for T, A in ((3, 3), (16, 8)):
        for s, u, k in zip((None, "2", "q-1", "random", "mixed") * 4, ("0", "1", "q-1", "random") * 5,
                           (None, "0", "q-1", "random", "q-1", "random", None, "0", "0", None, "random", "q-1", "random", "q-1", "0", None, "0", "random", None, "q-1")):
            run_kernel_case(envs(13, chain), mods, T, A, 7 + i, scale=s, add_scale=u, const=k, composed=(i % 7 == 3))
            i += 1
    run_kernel_case(envs(13, chain), mods, 16, 8, 99, scale="q-1", add_scale="q-1", const="q-1")
    run_kernel_case(envs(13, chain), mods, 2, 2, 98, addends_in_operand_pool=True)


@pytest.mark.parametrize("chain", CHAINS)
@pytest.mark.parametrize("logN", [15, 16])
def test_kernel_at_larger_rings(envs, chain, logN):
    run_kernel_case(envs(logN, chain), [0, 5, NQ, 5, 2], 3, 3, logN)


@pytest.mark.parametrize("chain", CHAINS)
def test_without_addends_and_scalars_it_is_hm_tensor_dot_and_with_one_pair_hm_tensor_muladd(envs, chain):
    ctx, o, pool, _, xpool, _ = envs(13, chain)
    mods = [(5 * i + 2) % (NQ + NP) for i in range(67)]
    n = len(mods)
    lo = [list(range(n)), list(range(n, 2 * n)), list(range(2 * n, 3 * n))]
    a, b = ctx.alloc(3 * n), ctx.alloc(3 * n)
    for T in (1, 4, 16):
        ops = kernel_lists(mods, T, 0, ctx.moduli, np.random.default_rng(T))[0]
        ctx.tensor_dot(pool, pool, pool, pool, a, a, a, mods, T, limbs=ops + lo)
        ctx.tensor_dotadd(pool, pool, pool, pool, None, b, b, b, mods, T, 0, limbs=ops + lo)
        assert np.array_equal(a.download(), b.download()), ("hm_tensor_dot", T)
    for A, scale, const in ((0, None, None), (1, "random", "random"), (8, "q-1", None), (3, None, "q-1")):
        ops, lx0, lx1, s, u, k = kernel_lists(mods, 1, A, ctx.moduli, np.random.default_rng(50 + A), scale, "random", const)
        ctx.tensor_muladd(pool, pool, pool, pool, xpool if A else None, a, a, a, mods, A, lx0 if A else None, lx1 if A else None, s, u if A else None, k,
                          limbs=ops + lo)
        ctx.tensor_dotadd(pool, pool, pool, pool, xpool if A else None, b, b, b, mods, 1, A, lx0 if A else None, lx1 if A else None, s, u if A else None, k,
                          limbs=ops + lo)
        assert np.array_equal(a.download(), b.download()), ("hm_tensor_muladd", A)
    a.free(); b.free()


def _alias_call(ctx, big, out_at=40, n=2, x_at=16):
    """n = 2 records of 2 pairs and 1 addend in ONE allocation: the operands are limbs 0 .. 15, the addend components from limb x_at on, all through
    the allocation's base; the outputs 3 n limbs from `out_at` through a base pointer of their own"""
    at = lambda limb: types.SimpleNamespace(ptr=big.limb_ptr(limb))
    o = at(out_at)
    ctx.tensor_dotadd(big, big, big, big, big, o, o, o, [0] * n, 2, 1, [x_at, x_at + 1], [x_at + 2, x_at + 3], None, [1] * n, None,
                      limbs=[[0, 1, 2, 3], [4, 5, 6, 7], [8, 9, 10, 11], [12, 13, 14, 15], [0, 1], [2, 3], [4, 5]])


def test_refuses_an_output_over_an_input_through_another_base_pointer():
    from homulator_amd import hip
    ctx = hip.Context(13, NQ, NP)
    big = ctx.alloc(64)
    ctx.fill_uniform(big, [0] * 64, 5)
    _alias_call(ctx, big)                                   # disjoint: accepted
    for out_at in (15, 10, 0, 3):
        with pytest.raises(hip.HmError, match=r"hm_tensor_dotadd: an output limb-poly \(o\d\) overlaps an input limb-poly \(\w\)"):
            _alias_call(ctx, big, out_at=out_at)
    with pytest.raises(hip.HmError, match=r"hm_tensor_dotadd: an output limb-poly \(o\d\) overlaps an input limb-poly \(x\)"):
        _alias_call(ctx, big, out_at=40, x_at=43)           # an addend component under an output
    ctx.sync()
    ctx.close()


def test_refuses_bad_arguments_and_accepts_n_0():
    from homulator_amd import hip
    ctx = hip.Context(13, NQ, NP)
    src, out = ctx.alloc(12), ctx.alloc(6)
    ctx.fill_uniform(src, [0] * 12, 5)
    q0 = ctx.moduli[0]
    null = types.SimpleNamespace(ptr=None)
    ok = [[0], [1], [2], [3], [0], [1], [2]]
    call = lambda a=src, b=src, c=src, d=src, x=src, o0=out, o1=out, o2=out, mods=(0,), T=1, A=1, lx0=(4,), lx1=(5,), s=None, u=(1,), k=None, limbs=None: \
        ctx.tensor_dotadd(a, b, c, d, x, o0, o1, o2, list(mods), T, A, None if lx0 is None else list(lx0), None if lx1 is None else list(lx1), s,
                          None if u is None else list(u), k, limbs=limbs or ok)
    for kw in ("a", "b", "c", "d", "o0", "o1", "o2"):
        with pytest.raises(hip.HmError, match="hm_tensor_dotadd: null buffer"):
            call(**{kw: null})
    with pytest.raises(hip.HmError, match="hm_tensor_dotadd: null buffer"):
        call(x=None)
    with pytest.raises(hip.HmError, match="hm_tensor_dotadd: x0_limbs or x1_limbs is null"):
        call(lx0=None)
    with pytest.raises(hip.HmError, match="hm_tensor_dotadd: x0_limbs or x1_limbs is null"):
        call(lx1=None)
    with pytest.raises(hip.HmError, match="hm_tensor_dotadd: add_scale is null"):
        call(u=None)
    with pytest.raises(hip.HmError, match="hm_tensor_dotadd: mod_ids is null"):
        ctx._ck(ctx.L.hm_tensor_dotadd(ctx.h, src.ptr, None, src.ptr, None, src.ptr, None, src.ptr, None, None, None, None, out.ptr, None, out.ptr, None,
                                       out.ptr, None, None, 1, 1, 0, None, None, None))
    two = [[0, 6], [1, 7], [2, 8], [3, 9], [0], [1], [2]]
    for T in (0, 17):
        with pytest.raises(hip.HmError, match=rf"hm_tensor_dotadd: n_terms = {T}, must be in \[1, 16\]"):
            call(T=T, limbs=[[0] * T, [1] * T, [2] * T, [3] * T, [0], [1], [2]])
    with pytest.raises(hip.HmError, match=r"hm_tensor_dotadd: n_addends = 9, must be in \[0, 8\]"):
        call(A=9, lx0=[4] * 9, lx1=[5] * 9, u=[1] * 9)
    with pytest.raises(hip.HmError, match="65535"):
        call(limbs=[[70000], [1], [2], [3], [0], [1], [2]])
    with pytest.raises(hip.HmError, match="65535"):
        call(T=2, limbs=[[0, 6], [1, 7], [2, 8], [3, 70000], [0], [1], [2]])       # the last pair's d
    with pytest.raises(hip.HmError, match="65535"):
        call(limbs=[[0], [1], [2], [3], [0], [1], [70000]])
    with pytest.raises(hip.HmError, match="65535"):
        call(lx1=[70000])
    with pytest.raises(hip.HmError, match="mod id"):
        call(mods=[NQ + NP])
    with pytest.raises(hip.HmError, match=r"scale\[0\]\[0\] is not reduced"):
        call(s=[q0])
    with pytest.raises(hip.HmError, match=r"scale\[0\]\[1\] is zero"):
        call(T=2, s=[1, 0], limbs=two)
    with pytest.raises(hip.HmError, match=r"scale\[0\]\[1\] is not reduced"):
        call(T=2, s=[1, q0], limbs=two)
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
    with pytest.raises(hip.HmError, match=r"overlaps an input limb-poly \(c\)"):     # the second pair's c under o1
        call(T=2, o1=src, limbs=[[0, 6], [1, 7], [2, 8], [3, 9], [0], [8], [2]])
    keep = [hip._u32([0])]
    ctx._ck(ctx.L.hm_tensor_dotadd(ctx.h, src.ptr, None, src.ptr, None, src.ptr, None, src.ptr, None, None, None, None, out.ptr, None, out.ptr, None,
                                   out.ptr, None, keep[0][1], 0, 1, 0, None, None, None))   # n = 0: nothing to do
    call(A=0, x=None, lx0=None, lx1=None, u=None)                    # all four may be null without addends
    call(T=2, s=[q0 - 1, 1], u=[0], k=[q0 - 1], limbs=two)           # and a call with nothing wrong is accepted
    ctx.sync()
    ctx.close()


@pytest.mark.parametrize("chain", CHAINS)
def test_a_captured_call_replays(envs, chain):
    """the records live in a cached device table: after one warm run the call is captured into a graph and replayed on new input data"""
    ctx, o = envs(13, chain)[:2]
    ctx.L.hm_graph_launch.argtypes = [C.c_void_p, C.c_void_p]
    ctx.L.hm_graph_destroy.argtypes = [C.c_void_p]
    T, A = 3, 2
    mods = [(3 * i + 1) % (NQ + NP) for i in range(70)]
    n = len(mods)
    fill_mods = [m for m in range(NQ + NP) for _ in range(PER_MOD)]
    rng = np.random.default_rng(3)
    ops, lx0, lx1, s, u, k = kernel_lists(mods, T, A, ctx.moduli, rng)
    src, out = ctx.alloc(len(fill_mods)), ctx.alloc(3 * n)
    lo = [list(range(n)), list(range(n, 2 * n)), list(range(2 * n, 3 * n))]
    run = lambda: ctx.tensor_dotadd(src, src, src, src, src, out, out, out, mods, T, A, lx0, lx1, s, u, k, limbs=ops + lo)
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
    host_src = src.download()
    exp = expected_rows(o, host_src, host_src, mods, T, A, ops, lx0, lx1, s, u, k)
    for i in range(3):
        assert np.array_equal(got[lo[i]], exp[i]), (chain, i)
    ctx.L.hm_graph_destroy(g)
    src.free(); out.free()


# ============================================================================================================================
# B. the op
# ============================================================================================================================
def read_out(op, copy=0, name="out"):
    return op.read(f"{name}.c0", copy=copy), op.read(f"{name}.c1", copy=copy)


SHAPES = [
    ("config_4_N15.cfg", 15, 16, 10, 4, 2),
    ("config_4_N15.cfg", 13, 6, 5, 2, 1),
    ("config_4.cfg", 16, 6, 3, 2, 1),           # N = 2^16 at a low level
]
KEYS = [(1, 0, 0, 0), (2, 1, 1, 1), (3, 2, 1, 0), (3, 2, 0, 1)]     # (terms, addends, da_scale, da_const): every (T, A), both values of either key
_ref = {}


def reference(chain, logN, L, ell, alpha, keys, copy=0, seed=SEED):
    """the reference output on the op's synthetic inputs, computed once per case"""
    from dotadd_ref import dotadd, synthetic_constants, synthetic_inputs
    key = (chain, logN, L, ell, alpha, keys, copy, seed)
    if key not in _ref:
        T, A, ds, dc = keys
        o = oracle(logN, L, alpha, chain, threads=16)
        pairs, adds, evk = synthetic_inputs(o, ell, seed, T, A, copy=copy)
        scales, us, const = synthetic_constants(o, ell, seed, T, A, ds, dc)
        _ref[key] = dotadd(o, ell, pairs, evk, adds, scales, us, const)
    return _ref[key]


def ov_of(keys, **more):
    return dict({"terms": keys[0], "addends": keys[1], "da_scale": keys[2], "da_const": keys[3]}, **more)


@pytest.mark.parametrize("chain", CHAINS)
@pytest.mark.parametrize("keys", KEYS)
@pytest.mark.parametrize("cfg,logN,L,ell,alpha,batch", SHAPES)
def test_op_fused_unfused_and_reference_agree(chain, keys, cfg, logN, L, ell, alpha, batch):
    """fused, unfused and fuse_dotadd = 0 against the reference; batch 2 (first shape): both copies, under the same constants"""
    from dotadd_ref import assert_ct
    ov = chain_ov(chain, ov_of(keys, batch=batch, N=1 << logN))
    for mode, fuse, extra in (("fused", True, {}), ("unfused", False, {}), ("fuse_dotadd = 0", True, {"fuse_dotadd": 0})):
        op = host.Op(cfg, "hdotadd", L, ell, alpha, fuse=fuse, overrides=dict(ov, **extra))
        op.execute(1)
        kinds = [ln.split()[0] for ln in op.plan()]
        assert kinds.count("TENSOR_DOTADD") == (1 if mode == "fused" else 0), (mode, kinds)
        for c in range(batch):
            got = read_out(op, c)
            assert got[0].shape[0] == ell - 1
            assert_ct(got, reference(chain, logN, L, ell, alpha, keys, copy=c), (mode, keys, c))
        op.close()


@pytest.mark.parametrize("chain", CHAINS)
def test_without_addends_and_keys_it_is_hdot_and_with_one_pair_hmuladd(chain):
    """the op-level identities, device output against device output: A = 0 without keys is hdot at the same T; T = 1 is hmuladd under the same
    constants (the two ops draw their synthetic constants from different streams, so both are handed the same ones)"""
    from dotadd_ref import assert_ct
    cfg, logN, L, ell, alpha, _ = SHAPES[1]
    ov = chain_ov(chain, {"N": 1 << logN})
    o = oracle(logN, L, alpha, chain)
    dot = host.Op(cfg, "hdot", L, ell, alpha, overrides=dict(ov, terms=3))
    mine = host.Op(cfg, "hdotadd", L, ell, alpha, overrides=dict(ov, terms=3, addends=0))
    dot.execute(1)
    mine.execute(1)
    assert_ct(read_out(mine), read_out(dot), "hdot")
    dot.close(); mine.close()
    scale = [o.moduli[j] - 2 - j for j in range(ell)]
    us = [[(5 << 40) % o.moduli[j] for j in range(ell)], [o.moduli[j] - 1 for j in range(ell)]]
    const = [(7 << 80) % o.moduli[j] for j in range(ell)]
    ma = host.Op(cfg, "hmuladd", L, ell, alpha, overrides=dict(ov, addends=2, ma_scale=1, ma_const=1))
    mine = host.Op(cfg, "hdotadd", L, ell, alpha, overrides=dict(ov, terms=1, addends=2, da_scale=1, da_const=1))
    for op, name in ((ma, "scale"), (mine, "scale1")):
        op.set_constants(name, scale)
        for r in range(2):
            op.set_constants(f"addscale{r + 1}", us[r])
        op.set_constants("const", const)
        op.execute(1)
    assert_ct(read_out(mine), read_out(ma), "hmuladd")
    ma.close(); mine.close()


def test_graph_replay_with_a_batch():
    """graph = 1: run 1 direct, run 2 captures, run 3 replays; both copies after the replay"""
    from dotadd_ref import assert_ct
    cfg, logN, L, ell, alpha, batch = SHAPES[0]
    keys = (3, 2, 1, 1)
    op = host.Op(cfg, "hdotadd", L, ell, alpha, overrides=ov_of(keys, batch=batch, graph=1))
    da = [ln for ln in op.plan() if ln.startswith("TENSOR_DOTADD")]
    assert len(da) == 1 and f" n={batch * ell} " in da[0] and " terms=3 addends=2 scale=1 const=1" in da[0]
    for _ in range(3):
        op.execute(1)
    for c in range(batch):
        assert_ct(read_out(op, c), reference("mont32", logN, L, ell, alpha, keys, copy=c), f"copy {c}")
    op.close()


@pytest.mark.parametrize("chain", CHAINS)
@pytest.mark.parametrize("fuse", [True, False])
def test_caller_constants(chain, fuse):
    from dotadd_ref import assert_ct, dotadd, synthetic_inputs
    L, ell, alpha, T, A = 6, 5, 2, 2, 3
    o = oracle(13, L, alpha, chain)
    scales = [[2, o.moduli[1] - 1, 1, 12345, o.moduli[4] // 2], [o.moduli[j] - 2 for j in range(ell)]]
    us = [[3, o.moduli[1] - 1, 1, 54321, o.moduli[4] // 3], [0] * ell, [o.moduli[j] - 3 for j in range(ell)]]
    const = [(7 << 40) % o.moduli[j] for j in range(ell)]
    op = host.Op("config_4_N15.cfg", "hdotadd", L, ell, alpha, fuse=fuse, overrides=chain_ov(chain, ov_of((T, A, 1, 1), N=1 << 13)))
    for t in range(T):
        op.set_constants(f"scale{t + 1}", scales[t])
    for r in range(A):
        op.set_constants(f"addscale{r + 1}", us[r])
    op.set_constants("const", const)
    op.execute(1)
    pairs, adds, evk = synthetic_inputs(o, ell, SEED, T, A)
    assert_ct(read_out(op), dotadd(o, ell, pairs, evk, adds, scales, us, const), ("caller constants", chain, fuse))
    with pytest.raises(host.HostError, match=r'hdotadd: set_constants\("addscale2"\) after prepare'):
        op.set_constants("addscale2", us[1])
    op.close()


def test_reim_then_re_squared_minus_im_squared_link_by_link():
    """hreim -> hdotadd (T = 2, s = (1, -1)): both outputs of an hreim bound to the pairs (re, re) and (im, im) of an hdotadd, checked link by link
    against the references on the oracle's hreim outputs; then the pairs (re, im), (re, im): two pairs of the same two ciphertexts"""
    from dotadd_ref import assert_ct, dotadd
    import reim_ref
    L, ell, alpha = 6, 5, 2
    o = oracle(13, L, alpha)
    src = host.Op("config_4_N15.cfg", "hreim", L, ell, alpha, overrides={"N": 1 << 13})
    src.execute(1)
    re, im, _ = reim_ref.reim(o, ell, *reim_ref.synthetic_input(o, ell, SEED))
    assert_ct(read_out(src), re, "link 0")
    assert_ct(read_out(src, name="out_im"), im, "link 0, imaginary")
    seed = SEED + 31
    evk = o.synth_evk(ell, seed + 10000)
    scales = [[1] * ell, [o.moduli[j] - 1 for j in range(ell)]]
    for binds, pairs in (((("ct1", "out"), ("ct2", "out"), ("ct3", "out_im"), ("ct4", "out_im")), [(re, re), (im, im)]),
                         ((("ct1", "out"), ("ct2", "out_im"), ("ct3", "out"), ("ct4", "out_im")), [(re, im), (re, im)])):
        for fuse in (True, False):
            op = host.Op("config_4_N15.cfg", "hdotadd", L, ell, alpha, fuse=fuse, overrides={"N": 1 << 13, "terms": 2, "addends": 0, "da_scale": 1, "seed": seed})
            for t in range(2):
                op.set_constants(f"scale{t + 1}", scales[t])
            for name, output in binds:
                op.bind_input(name, src, output=output)
            op.execute(1)
            assert_ct(read_out(op), dotadd(o, ell, pairs, evk, scales=scales), ("link 1", binds[1], fuse))
            op.close()
    src.close()


def test_real_data_decrypts_within_the_bound():
    """3 m1 m2 - 2 m3 m4 + 5 m5 + 7 on toy-scheme data: five uploaded ciphertexts and the key.  The output is the reference's bit for bit and decrypts
    within the bound the reference is held to first (tests/dotadd_ref.py)"""
    from dotadd_ref import assert_ct, decryption_error, dotadd, real_case
    from toy_ckks import Toy
    LOGN, L, ELL, ALPHA = 13, 6, 5, 2
    o = oracle(LOGN, L, ALPHA)
    toy = Toy(o, seed=4251)
    cts, evk, scales, u, const, exact = real_case(toy, ELL)
    ref = dotadd(o, ELL, [(cts[0], cts[1]), (cts[2], cts[3])], evk, [cts[4]], scales, [u], const)
    ref_err, bound = decryption_error(toy, ref, ELL, exact)
    print(f"reference: max |dec q_4 - exact| = 2^{ref_err.bit_length()} (bound 2^{bound.bit_length() - 1})")
    assert ref_err <= bound
    op = host.Op("config_4_N15.cfg", "hdotadd", L, ELL, ALPHA, overrides={"N": 1 << LOGN, "terms": 2, "addends": 1, "da_scale": 1, "da_const": 1})
    op.set_constants("scale1", scales[0])          # (the constants first: writing a buffer prepares the op)
    op.set_constants("scale2", scales[1])
    op.set_constants("addscale1", u)
    op.set_constants("const", const)
    for i, ct in enumerate(cts):
        op.write(f"ct{i + 1}.c0", ct[0])
        op.write(f"ct{i + 1}.c1", ct[1])
    for j in range(evk.shape[0]):
        for k in range(2):
            op.write(f"IP_Key{k}_{j}", evk[j][k])
    op.execute(1)
    out = read_out(op)
    op.close()
    gpu_err, _ = decryption_error(toy, out, ELL, exact)
    print(f"GPU: max |dec q_4 - exact| = 2^{gpu_err.bit_length()} (bound 2^{bound.bit_length() - 1})")
    assert gpu_err <= bound
    assert_ct(out, ref, "real data")
