"""hsquare on the GPU, on both arithmetic back-ends (mont32 and chain_bits = 60), bit for bit:
 A. hm_tensor_square and the element-wise opcode ADD_CONST through the ABI: against tests/square_ref.py and against hm_tensor(a, a, c, c) + MUL_CONST
    x 3 + ADD_CONST on the same device data, on permuted and repeated limb lists with guard limb-polys; the refusals; a captured call replayed;
 B. the op, fused (one TENSOR_SQUARE launch), unfused (one launch per stage) and with fuse_square = 0, over the four key combinations, against the
    reference; batch 2, graph = 1, caller constants, a chain of three squares link by link, and real data (tests/toy_ckks.py)."""
import ctypes as C
import itertools
import types

import numpy as np
import pytest

from homulator_amd import host
from oracle.homoracle import Oracle, chain_below

pytestmark = pytest.mark.gpu
CHAINS = ["mont32", "survey"]
SEED = host.SEED
NQ, NP = 6, 3
GUARD = 0x5A5A5A5A5A5A5A5A
KEYS = [(0, 0), (0, 1), (1, 0), (1, 1)]
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


def constants(kind, mods, moduli, rng, lo):
    """per-entry scalars (lo = 1) or constants (lo = 0) of the named kind; None: no list"""
    if kind is None:
        return None
    return [{"0": 0, "1": 1, "2": 2, "q-1": moduli[m] - 1}[kind] if kind != "random" else int(rng.integers(lo, moduli[m])) for m in mods]


def run_kernel_case(ctx, o, mods, seed, fill="uniform", scale="random", const="random", composed=True):
    """one hm_tensor_square call: a and c hold n limb-polys each, the three output buffers n and one guard limb-poly; the output lists are random
    permutations, the input lists random permutations in which an entry may repeat the limb of an earlier entry of its modulus.
    fill: "uniform" (device fill), "q-1" or "zero"."""
    from homulator_amd import hip
    from square_ref import square_tensor
    n, N = len(mods), ctx.N
    rng = np.random.default_rng(seed)
    ins = [ctx.alloc(n) for _ in range(2)]
    outs = [ctx.alloc(n + 1) for _ in range(3)]
    il = []
    for _ in range(2):
        ls = [int(v) for v in rng.permutation(n)]
        for i in range(1, n):
            same = [j for j in range(i) if mods[j] == mods[i]]
            if same and rng.integers(0, 2):
                ls[i] = ls[same[0]]
        il.append(ls)
    operm = [[int(v) for v in rng.permutation(n + 1)] for _ in range(3)]
    ol = [pm[:n] for pm in operm]
    for k, (buf, ls) in enumerate(zip(ins, il)):
        m = {ls[i]: mods[i] for i in range(n)}
        if fill == "uniform":
            ctx.fill_uniform(buf, [m[x] for x in sorted(m)], seed * 13 + k, out_limbs=sorted(m))
        else:
            host_data = np.zeros((n, N), dtype=np.uint64)
            for x in m:
                host_data[x] = ctx.moduli[m[x]] - 1 if fill == "q-1" else 0
            buf.upload(host_data)
    for buf in outs:
        buf.upload(np.full((n + 1, N), GUARD, dtype=np.uint64))
    s, k = constants(scale, mods, ctx.moduli, rng, 1), constants(const, mods, ctx.moduli, rng, 0)
    ctx.tensor_square(*ins, *outs, mods, scale=s, addend=k, limbs=il + ol)
    A, Cc = (b.download() for b in ins)
    got = [b.download() for b in outs]
    a_rows, c_rows = np.stack([A[il[0][i]] for i in range(n)]), np.stack([Cc[il[1][i]] for i in range(n)])
    exp = square_tensor(o, mods, a_rows, c_rows, s, k)
    what = (n, fill, scale, const)
    for t in range(3):
        assert np.array_equal(got[t][ol[t]], exp[t]), (what, f"d{t}")
        assert np.all(got[t][operm[t][n]] == GUARD), "a guard limb-poly was written"
    if composed:   # the same from the calls it replaces, on the same device data
        ref = [ctx.alloc(n) for _ in range(3)]
        ctx.tensor(ins[0], ins[0], ins[1], ins[1], *ref, mods, limbs=[il[0], il[0], il[1], il[1], None, None, None])
        if s is not None:
            for r in ref:
                ctx.ewe(hip.OP_MUL_CONST, r, mods, a=r, k=s)
        if k is not None:
            ctx.ewe(hip.OP_ADD_CONST, ref[0], mods, a=ref[0], k=k)
        for t in range(3):
            assert np.array_equal(ref[t].download(), exp[t]), (what, f"composed d{t}")
        for b in ref:
            b.free()
    for b in ins + outs:
        b.free()


@pytest.mark.parametrize("chain", CHAINS)
@pytest.mark.parametrize("n", [1, 3, 65, 130])
def test_kernel_entry_counts(envs, chain, n):
    """across the 64- and 128-entry cuts of the launches whose records travel as kernel arguments: this one is ONE launch for any n; Q and P
    limbs, repeated moduli"""
    ctx, o = envs(13, chain)
    run_kernel_case(ctx, o, [(5 * i + 2) % (NQ + NP) for i in range(n)], 40 + n)


@pytest.mark.parametrize("chain", CHAINS)
@pytest.mark.parametrize("fill", ["uniform", "zero", "q-1"])
def test_kernel_fills_scalars_and_constants(envs, chain, fill):
    """every scalar (1, 2, q - 1, random, no list) with every constant (0, q - 1, random, no list), 5 entries"""
    ctx, o = envs(13, chain)
    mods = [0, NQ + NP - 1, 3, 0, NQ]
    for i, (s, k) in enumerate(itertools.product(["1", "2", "q-1", "random", None], ["0", "q-1", "random", None])):
        run_kernel_case(ctx, o, mods, 7 + i, fill=fill, scale=s, const=k, composed=(fill == "uniform" and i % 5 == 3))


@pytest.mark.parametrize("chain", CHAINS)
@pytest.mark.parametrize("logN", [15, 16])
def test_kernel_at_larger_rings(envs, chain, logN):
    ctx, o = envs(logN, chain)
    run_kernel_case(ctx, o, [0, 5, NQ, 5, 2], logN)


@pytest.mark.parametrize("chain", CHAINS)
def test_ewe_add_const_alone(envs, chain):
    from homulator_amd import hip
    ctx, o = envs(13, chain)
    ids = [0, 3, NQ, NQ + NP - 1]
    A = o.fill_uniform(ids, 21)
    for r, m in enumerate(ids):
        A[r, :4] = [0, 1, o.moduli[m] - 2, o.moduli[m] - 1]
    da, out = ctx.from_host(A), ctx.alloc(len(ids) + 1)
    out.upload(np.full((len(ids) + 1, ctx.N), GUARD, dtype=np.uint64))
    for ks in ([0] * 4, [o.moduli[m] - 1 for m in ids], [1, 2, 3, 4], [o.moduli[m] // 3 for m in ids]):
        ctx.ewe(hip.OP_ADD_CONST, out, ids, a=da, k=ks, lo=[4, 2, 0, 1])
        got = out.download()
        for r, (m, k) in enumerate(zip(ids, ks)):
            q = o.moduli[m]
            t = A[r] + np.uint64(k)
            assert np.array_equal(got[[4, 2, 0, 1][r]], np.where(t >= np.uint64(q), t - np.uint64(q), t)), (chain, r, k)
        assert np.all(got[3] == GUARD)
    with pytest.raises(hip.HmError, match="needs constants"):
        ctx.ewe(hip.OP_ADD_CONST, out, ids, a=da)
    with pytest.raises(hip.HmError, match="not reduced"):
        ctx.ewe(hip.OP_ADD_CONST, out, ids, a=da, k=[0, 0, o.moduli[NQ], 0])
    with pytest.raises(hip.HmError, match="missing an operand"):
        ctx.ewe(hip.OP_ADD_CONST, out, ids, k=[0] * 4)
    with pytest.raises(hip.HmError, match="bad opcode"):
        ctx.ewe(hip.OP_ADD_CONST + 1, out, ids, a=da, k=[0] * 4)
    da.free(); out.free()


def _alias_call(ctx, big, o0=40, o1=44, o2=48):
    """n = 4 entries in ONE allocation, each operand through a base pointer of its own: a limbs 0..3, c 8..11; the outputs from limbs o0, o1, o2"""
    at = lambda limb: types.SimpleNamespace(ptr=big.limb_ptr(limb))
    ctx.tensor_square(big, at(8), at(o0), at(o1), at(o2), [0] * 4)


@pytest.mark.parametrize("where,what", [({"o0": 3}, r"output.*\(o0\).*input.*\(a\)"), ({"o1": 9}, r"\(o1\).*\(c\)"), ({"o2": 0}, r"\(o2\).*\(a\)"),
                                        ({"o1": 42}, "two output"), ({"o2": 47}, "two output")])
def test_refuses_an_output_over_another_operand_through_another_base_pointer(where, what):
    from homulator_amd import hip
    ctx = hip.Context(13, NQ, NP)
    big = ctx.alloc(64)
    ctx.fill_uniform(big, [0] * 64, 5)
    _alias_call(ctx, big)                                   # disjoint: accepted
    with pytest.raises(hip.HmError, match=what):
        _alias_call(ctx, big, **where)
    ctx.sync()
    ctx.close()


def test_refuses_bad_arguments():
    from homulator_amd import hip
    ctx = hip.Context(13, NQ, NP)
    b = [ctx.alloc(4) for _ in range(5)]
    q0 = ctx.moduli[0]
    null = types.SimpleNamespace(ptr=None)
    for k in range(5):
        with pytest.raises(hip.HmError, match="null buffer"):
            ctx.tensor_square(*[null if j == k else x for j, x in enumerate(b)], [0])
    for k in range(5):
        limbs = [None] * 5
        limbs[k] = [70000]
        with pytest.raises(hip.HmError, match="65535"):
            ctx.tensor_square(*b, [0], limbs=limbs)
    with pytest.raises(hip.HmError, match="mod id"):
        ctx.tensor_square(*b, [NQ + NP])
    with pytest.raises(hip.HmError, match=r"scale\[1\] is not reduced"):
        ctx.tensor_square(*b, [0, 0], scale=[1, q0])
    with pytest.raises(hip.HmError, match=r"scale\[0\] is zero"):
        ctx.tensor_square(*b, [0, 0], scale=[0, 1])
    with pytest.raises(hip.HmError, match=r"addend\[1\] is not reduced"):
        ctx.tensor_square(*b, [0, 0], addend=[0, q0])
    with pytest.raises(hip.HmError, match="two output"):
        ctx.tensor_square(b[0], b[1], b[2], b[2], b[4], [0])
    with pytest.raises(hip.HmError, match="two output limb-polys overlap"):   # through a limb list: entries 0 and 2 of o1, no input touched
        ctx.tensor_square(*b, [0, 0, 0], limbs=[None, None, None, [2, 0, 2], None])
    with pytest.raises(hip.HmError, match="overlaps an input"):
        ctx.tensor_square(b[0], b[1], b[0], b[3], b[4], [0])
    ctx.tensor_square(*b, [])                               # n = 0: nothing to do
    ctx.tensor_square(*b, [0, 0], scale=[1, q0 - 1], addend=[0, q0 - 1])   # and a call with nothing wrong is accepted
    ctx.sync()
    ctx.close()


@pytest.mark.parametrize("chain", CHAINS)
def test_a_captured_call_replays(envs, chain):
    """the records live in a cached device table: after one run the call is captured into a graph and replayed on new input data"""
    from square_ref import square_tensor
    ctx, o = envs(13, chain)
    ctx.L.hm_graph_launch.argtypes = [C.c_void_p, C.c_void_p]
    ctx.L.hm_graph_destroy.argtypes = [C.c_void_p]
    mods = [(3 * i + 1) % (NQ + NP) for i in range(70)]
    rng = np.random.default_rng(3)
    s, k = constants("random", mods, ctx.moduli, rng, 1), constants("random", mods, ctx.moduli, rng, 0)
    a, c = ctx.alloc(len(mods)), ctx.alloc(len(mods))
    outs = [ctx.alloc(len(mods)) for _ in range(3)]
    run = lambda: ctx.tensor_square(a, c, *outs, mods, scale=s, addend=k)
    ctx.fill_uniform(a, mods, 1); ctx.fill_uniform(c, mods, 2)
    run()
    g = C.c_void_p()
    ctx._ck(ctx.L.hm_capture_begin(ctx.h))
    run()
    ctx._ck(ctx.L.hm_capture_end(ctx.h, C.byref(g)))
    ctx.fill_uniform(a, mods, 3); ctx.fill_uniform(c, mods, 4)
    for b in outs:
        b.upload(np.full((len(mods), ctx.N), GUARD, dtype=np.uint64))
    ctx._ck(ctx.L.hm_graph_launch(ctx.h, g))
    ctx.sync()
    exp = square_tensor(o, mods, a.download(), c.download(), s, k)
    for t in range(3):
        assert np.array_equal(outs[t].download(), exp[t]), (chain, t)
    ctx.L.hm_graph_destroy(g)
    for b in [a, c] + outs:
        b.free()


# ============================================================================================================================
# B. the op
# ============================================================================================================================
def read_out(op, copy=0):
    return op.read("out.c0", copy=copy), op.read("out.c1", copy=copy)


SHAPES = [
    ("config_4_N15.cfg", 15, 16, 10, 4, 2),
    ("config_4_N15.cfg", 15, 8, 8, 8, 1),       # beta = 1
    ("config_4_N15.cfg", 13, 6, 5, 1, 1),       # beta = 5: element-wise key products behind the one TENSOR_SQUARE launch
]
_ref = {}


def reference(chain, logN, L, ell, alpha, keys, copy=0, seed=SEED):
    """the reference output on the op's synthetic inputs, computed once per case"""
    from square_ref import square, synthetic_constants, synthetic_inputs
    key = (chain, logN, L, ell, alpha, keys, copy, seed)
    if key not in _ref:
        o = oracle(logN, L, alpha, chain, threads=16)
        _ref[key] = square(o, ell, *synthetic_inputs(o, ell, seed, copy=copy), *synthetic_constants(o, ell, seed, *keys))
    return _ref[key]


@pytest.mark.parametrize("chain", CHAINS)
@pytest.mark.parametrize("keys", KEYS)
@pytest.mark.parametrize("cfg,logN,L,ell,alpha,batch", SHAPES)
def test_op_fused_unfused_and_reference_agree(chain, keys, cfg, logN, L, ell, alpha, batch):
    """fused, unfused and fuse_square = 0 against the reference; batch 2 (first shape): both copies, under the same constants"""
    from square_ref import assert_ct
    ov = chain_ov(chain, {"sq_scale": keys[0], "sq_const": keys[1], "batch": batch, "N": 1 << logN})
    for mode, fuse, extra in (("fused", True, {}), ("unfused", False, {}), ("fuse_square = 0", True, {"fuse_square": 0})):
        op = host.Op(cfg, "hsquare", L, ell, alpha, fuse=fuse, overrides=dict(ov, **extra))
        op.execute(1)
        kinds = [ln.split()[0] for ln in op.plan()]
        assert kinds.count("TENSOR_SQUARE") == (1 if mode == "fused" else 0), (mode, kinds)
        assert kinds.count("TENSOR") == (1 if mode == "fuse_square = 0" else 0), (mode, kinds)
        for c in range(batch):
            assert_ct(read_out(op, c), reference(chain, logN, L, ell, alpha, keys, copy=c), (mode, keys, c))
        op.close()


@pytest.mark.parametrize("chain", CHAINS)
def test_without_constants_it_is_the_hmult_of_the_ciphertext_with_itself(chain):
    from square_ref import assert_ct, synthetic_inputs
    L, ell, alpha = 6, 5, 2
    o = oracle(15, L, alpha, chain)
    op = host.Op("config_4_N15.cfg", "hsquare", L, ell, alpha, overrides=chain_ov(chain, {}))
    op.execute(1)
    ct, evk = synthetic_inputs(o, ell, SEED)
    assert_ct(read_out(op), o.hmult(ell, ct, ct, evk), "hsquare without constants against the oracle's hmult")
    op.close()


def test_graph_replay_with_a_batch():
    """graph = 1: run 1 direct, run 2 captures, run 3 replays; both copies after the replay"""
    from square_ref import assert_ct
    cfg, logN, L, ell, alpha, batch = SHAPES[0]
    op = host.Op(cfg, "hsquare", L, ell, alpha, overrides={"sq_scale": 1, "sq_const": 1, "batch": batch, "graph": 1})
    sq = [ln for ln in op.plan() if ln.startswith("TENSOR_SQUARE")]
    assert len(sq) == 1 and f" n={batch * ell} " in sq[0] and " scale=1 const=1" in sq[0]
    for _ in range(3):
        op.execute(1)
    for c in range(batch):
        assert_ct(read_out(op, c), reference("mont32", logN, L, ell, alpha, (1, 1), copy=c), f"copy {c}")
    op.close()


@pytest.mark.parametrize("chain", CHAINS)
@pytest.mark.parametrize("fuse", [True, False])
def test_caller_constants(chain, fuse):
    from square_ref import assert_ct, square, synthetic_inputs
    L, ell, alpha = 6, 5, 2
    o = oracle(13, L, alpha, chain)
    scale = [2, o.moduli[1] - 1, 1, 12345, o.moduli[4] // 2]
    const = [(-(1 << 80)) % o.moduli[j] for j in range(ell)]
    op = host.Op("config_4_N15.cfg", "hsquare", L, ell, alpha, fuse=fuse, overrides=chain_ov(chain, {"sq_scale": 1, "sq_const": 1, "N": 1 << 13}))
    op.set_constants("scale", scale)
    op.set_constants("const", const)
    op.execute(1)
    assert_ct(read_out(op), square(o, ell, *synthetic_inputs(o, ell, SEED), scale, const), ("caller constants", chain, fuse))
    with pytest.raises(host.HostError, match=r'hsquare: set_constants\("scale"\) after prepare'):
        op.set_constants("scale", scale)
    op.close()


def test_chain_of_three_squares_link_by_link():
    """hsquare,hsquare,hsquare at N = 2^13: link k runs under seed + 31 k (OpChain): its key and its constants are drawn from there, its input is
    the link before's output"""
    from square_ref import assert_ct, square, synthetic_constants, synthetic_inputs
    L, ell, alpha = 6, 5, 2
    o = oracle(13, L, alpha)
    chain = host.Chain("config_4_N15.cfg", "hsquare,hsquare,hsquare", L, ell, alpha, overrides={"sq_scale": 1, "sq_const": 1, "N": 1 << 13})
    chain.execute(1)
    ct = synthetic_inputs(o, ell, SEED)[0]
    for k in range(3):
        lvl, seed = ell - k, SEED + 31 * k
        out = square(o, lvl, ct, o.synth_evk(lvl, seed + 10000), *synthetic_constants(o, lvl, seed, 1, 1))
        assert [ln.split()[0] for ln in chain[k].plan()].count("TENSOR_SQUARE") == 1
        assert_ct(read_out(chain[k]), out, f"link {k}")
        ct = np.stack(out)
    chain.close()


def test_real_data_decrypts_to_the_double_angle_step():
    """a toy ciphertext, the relinearisation key and the constants s = 2, k = -2^80 written into the op: the output is the reference's bit for bit
    and decrypts to (2 m m 2^80 - 2^80) / q_last within twice the bound tests/test_gpu_real_data.py holds one hmult to; the reference is held to it first"""
    from square_ref import assert_ct, decryption_error, real_case, square
    from toy_ckks import Toy
    LOGN, L, ELL, ALPHA = 13, 6, 5, 2
    o = oracle(LOGN, L, ALPHA)
    toy = Toy(o, seed=4246)
    ct, evk, scale, const, exact = real_case(toy, ELL)
    ref = square(o, ELL, ct, evk, scale, const)
    ref_err, bound = decryption_error(toy, ref, ELL, exact)
    print(f"reference: max |dec q_last - exact| = 2^{ref_err.bit_length()} (bound 2^{bound.bit_length() - 1})")
    assert ref_err <= bound
    op = host.Op("config_4_N15.cfg", "hsquare", L, ELL, ALPHA, overrides={"N": 1 << LOGN, "sq_scale": 1, "sq_const": 1})
    op.set_constants("scale", scale)
    op.set_constants("const", const)
    op.write("ct1.c0", ct[0])
    op.write("ct1.c1", ct[1])
    for j in range(evk.shape[0]):
        for k in range(2):
            op.write(f"IP_Key{k}_{j}", evk[j][k])
    op.execute(1)
    out = read_out(op)
    op.close()
    gpu_err, _ = decryption_error(toy, out, ELL, exact)
    print(f"GPU: max |dec q_last - exact| = 2^{gpu_err.bit_length()} (bound 2^{bound.bit_length() - 1})")
    assert gpu_err <= bound
    assert_ct(out, ref, "real data")
