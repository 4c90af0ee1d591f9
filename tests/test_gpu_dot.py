"""hdot on the GPU, on both arithmetic back-ends (mont32 and chain_bits = 60), bit for bit:
 A. hm_tensor_dot against the oracle's MUL / MAC2 / ADD, on permuted limb lists with guard limb-polys, and its refusals;
 B. the op, fused (one TENSOR_DOT launch) and unfused (one launch per stage), against tests/dot_ref.py; terms = 1 against the hmult op;
 C. the op as the middle link of a chain;
 D. on real data (tests/toy_ckks.py) out decrypts to sum_t m_t m'_t / q_last."""
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


def run_kernel_case(ctx, o, mods, T, seed, fill="uniform"):
    """one hm_tensor_dot call: the four operand buffers hold n T limb-polys each, the three output buffers n and one guard limb-poly; every limb
    list is a random permutation of its buffer.  fill: "uniform" (device fill), "q-1" or "zero" (every operand)."""
    from dot_ref import tensor_sum
    n, N = len(mods), ctx.N
    rng = np.random.default_rng(seed)
    ins = [ctx.alloc(n * T) for _ in range(4)]
    outs = [ctx.alloc(n + 1) for _ in range(3)]
    il = [[int(v) for v in rng.permutation(n * T)] for _ in range(4)]
    operm = [[int(v) for v in rng.permutation(n + 1)] for _ in range(3)]
    ol = [pm[:n] for pm in operm]
    for k, (buf, ls) in enumerate(zip(ins, il)):
        m = {ls[i * T + t]: mods[i] for i in range(n) for t in range(T)}
        if fill == "uniform":
            ctx.fill_uniform(buf, [m[x] for x in sorted(m)], seed * 13 + k, out_limbs=sorted(m))
        else:
            buf.upload(np.stack([np.full(N, ctx.moduli[m[x]] - 1 if fill == "q-1" else 0, dtype=np.uint64) for x in sorted(m)]))
    for buf in outs:
        buf.upload(np.full((n + 1, N), GUARD, dtype=np.uint64))
    ctx.tensor_dot(*ins, *outs, mods, T, limbs=il + ol)
    A, B, Cc, D = (b.download() for b in ins)
    got = [b.download() for b in outs]
    for b in ins + outs:
        b.free()
    rows = lambda X, ls, t: np.stack([X[ls[i * T + t]] for i in range(n)])
    # roles: a = c00, b = c10, c = c01, d = c11
    exp = tensor_sum(o, mods, [(rows(A, il[0], t), rows(Cc, il[2], t), rows(B, il[1], t), rows(D, il[3], t)) for t in range(T)])
    for k in range(3):
        assert np.array_equal(got[k][ol[k]], exp[k]), (T, n, fill, f"d{k}")
        assert np.all(got[k][operm[k][n]] == GUARD), "a guard limb-poly was written"
        if fill == "zero":
            assert not got[k][ol[k]].any()


@pytest.mark.parametrize("chain", CHAINS)
@pytest.mark.parametrize("T", [1, 2, 3, 16])
def test_kernel_against_the_oracle(envs, chain, T):
    """7 entries with repeated moduli, Q and P limbs"""
    ctx, o = envs(13, chain)
    mods = [int(x) for x in np.random.default_rng(T).integers(0, NQ + NP, 7)]
    assert len(set(mods)) < 7
    run_kernel_case(ctx, o, mods, T, 100 + T)


@pytest.mark.parametrize("chain", CHAINS)
@pytest.mark.parametrize("fill", ["q-1", "zero"])
def test_kernel_worst_case_operands(envs, chain, fill):
    """16 pairs with every operand q - 1: 32 (q - 1)^2 in d1's accumulator, the largest value the wide reduction ever sees; and all zeros"""
    ctx, o = envs(13, chain)
    run_kernel_case(ctx, o, [0, NQ + NP - 1, 3], 16, 7, fill=fill)


@pytest.mark.parametrize("chain", CHAINS)
@pytest.mark.parametrize("n", [1, 65, 130])
def test_kernel_entry_counts(envs, chain, n):
    """across the 64- and 128-entry cuts of the launches whose records travel as kernel arguments: this one is ONE launch for any n"""
    ctx, o = envs(13, chain)
    run_kernel_case(ctx, o, [i % (NQ + NP) for i in range(n)], 2, 40 + n)


@pytest.mark.parametrize("chain", CHAINS)
def test_kernel_at_n_2_16(envs, chain):
    ctx, o = envs(16, chain)
    run_kernel_case(ctx, o, [0, 5, NQ, 5, 2], 3, 16)


def _alias_call(ctx, big, o0=40, o1=44, o2=48):
    """n = 4 entries of 2 pairs in ONE allocation, each operand through a base pointer of its own: a limbs 0..7, b 8..15, c 16..23, d 24..31;
    the outputs from limbs o0, o1, o2 (4 limb-polys each)"""
    at = lambda limb: types.SimpleNamespace(ptr=big.limb_ptr(limb))
    ctx.tensor_dot(big, at(8), at(16), at(24), at(o0), at(o1), at(o2), [0] * 4, 2)


@pytest.mark.parametrize("where,what", [({"o0": 5}, r"output.*\(o0\).*input.*\(a\)"), ({"o1": 13}, r"\(o1\).*\(b\)"), ({"o2": 21}, r"\(o2\).*\(c\)"),
                                        ({"o0": 29}, r"\(o0\).*\(d\)"), ({"o1": 42}, "two output"), ({"o2": 47}, "two output")])
def test_refuses_an_output_over_another_operand_through_another_base_pointer(where, what):
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
    b = [ctx.alloc(16) for _ in range(7)]
    null = types.SimpleNamespace(ptr=None)
    for k in range(7):
        with pytest.raises(hip.HmError, match="null buffer"):
            ctx.tensor_dot(*[null if j == k else x for j, x in enumerate(b)], [0], 1)
    for T in (0, 17):
        with pytest.raises(hip.HmError, match=r"n_terms.*\[1, 16\]"):
            ctx.tensor_dot(*b, [0], T)
    for k in range(7):
        limbs = [None] * 7
        limbs[k] = [70000]
        with pytest.raises(hip.HmError, match="65535"):
            ctx.tensor_dot(*b, [0], 1, limbs=limbs)
    with pytest.raises(hip.HmError, match="mod id"):
        ctx.tensor_dot(*b, [NQ + NP], 1)
    with pytest.raises(hip.HmError, match="two output"):
        ctx.tensor_dot(*b[:4], b[4], b[4], b[6], [0], 1)
    with pytest.raises(hip.HmError, match="two output limb-polys overlap"):   # through a limb list: entries 0 and 2 of o0, no input touched
        ctx.tensor_dot(*b, [0, 0, 0], 1, limbs=[None] * 4 + [[0, 1, 0], None, None])
    with pytest.raises(hip.HmError, match="overlaps an input"):
        ctx.tensor_dot(*b[:4], b[0], b[5], b[6], [0], 1)
    ctx.tensor_dot(*b, [0], 1)                              # and the same call with nothing wrong is accepted
    ctx.sync()
    ctx.close()


# ============================================================================================================================
# B. the op
# ============================================================================================================================
def read_out(op, copy=0):
    return op.read("out.c0", copy=copy), op.read("out.c1", copy=copy)


@pytest.mark.parametrize("chain", CHAINS)
@pytest.mark.parametrize("cfg,logN,L,ell,alpha,T,batch", [
    ("config_4_N15.cfg", 15, 16, 10, 4, 3, 2),
    ("config_4_N15.cfg", 15, 8, 8, 8, 2, 1),       # beta = 1
    ("config_4_N15.cfg", 13, 6, 5, 1, 2, 1),       # beta = 5: element-wise key products behind the one TENSOR_DOT launch
    ("config_4.cfg", 16, 45, 35, 15, 4, 1),        # the headline shape
])
def test_op_fused_unfused_and_reference_agree(chain, cfg, logN, L, ell, alpha, T, batch):
    from dot_ref import assert_ct, dot, synthetic_inputs
    o = oracle(logN, L, alpha, chain, threads=16)
    ov = chain_ov(chain, {"terms": T, "batch": batch, "N": 1 << logN})
    got = {}
    for fuse in (True, False):
        op = host.Op(cfg, "hdot", L, ell, alpha, fuse=fuse, overrides=ov)
        op.execute(1)
        got[fuse] = [read_out(op, c) for c in range(batch)]
        kinds = [ln.split()[0] for ln in op.plan()]
        assert kinds.count("TENSOR_DOT") == (1 if fuse else 0) and "TENSOR" not in kinds
        op.close()
    for c in range(batch):
        exp = dot(o, ell, *synthetic_inputs(o, ell, T, SEED, copy=c))
        assert_ct(got[True][c], exp, ("fused", c))
        assert_ct(got[False][c], exp, ("unfused", c))


@pytest.mark.parametrize("chain", CHAINS)
def test_one_term_is_the_hmult_op(chain):
    """terms = 1: the TENSOR_DOT launch in hmult's plan gives hmult's output on the same seed (and both are the reference's)"""
    from dot_ref import assert_ct, dot, synthetic_inputs
    L, ell, alpha = 6, 5, 2
    o = oracle(15, L, alpha, chain)
    out = {}
    for name, ov in (("hmult", {}), ("hdot", {"terms": 1})):
        op = host.Op("config_4_N15.cfg", name, L, ell, alpha, overrides=chain_ov(chain, ov))
        op.execute(1)
        out[name] = read_out(op)
        assert [ln.split()[0] for ln in op.plan()][0] == ("TENSOR" if name == "hmult" else "TENSOR_DOT")
        op.close()
    assert_ct(out["hdot"], out["hmult"], "hdot at one term against hmult")
    assert_ct(out["hdot"], dot(o, ell, *synthetic_inputs(o, ell, 1, SEED)), "reference")


def test_fuse_dot_off_computes_the_same():
    """fuse_dot = 0: a TENSOR launch and element-wise launches in front of the fused key switch"""
    from dot_ref import assert_ct, dot, synthetic_inputs
    L, ell, alpha, T = 16, 10, 4, 3
    o = oracle(15, L, alpha, threads=16)
    op = host.Op("config_4_N15.cfg", "hdot", L, ell, alpha, overrides={"terms": T, "fuse_dot": 0})
    kinds = [ln.split()[0] for ln in op.plan()]
    assert "TENSOR_DOT" not in kinds and kinds.count("TENSOR") == 1 and "EWE" in kinds
    op.execute(1)
    assert_ct(read_out(op), dot(o, ell, *synthetic_inputs(o, ell, T, SEED)), "fuse_dot = 0")
    op.close()


def test_bench_shape_batch_10_graph_replay():
    """config_4.cfg 45/35/15, 10 ops per launch, 4 pairs, the plan captured into a HIP graph (run 1 direct, run 2 captures, run 3 replays): copies 0
    and 9 of the batch after the replay"""
    from dot_ref import assert_ct, dot, synthetic_inputs
    cfg, logN, L, ell, alpha, T, B = "config_4.cfg", 16, 45, 35, 15, 4, 10
    o = oracle(logN, L, alpha, threads=16)
    op = host.Op(cfg, "hdot", L, ell, alpha, overrides={"terms": T, "batch": B, "graph": 1})
    dots = [ln for ln in op.plan() if ln.startswith("TENSOR_DOT")]
    assert len(dots) == 1 and f" n={B * ell} " in dots[0] and f" terms={T}" in dots[0] + " " and op.launch_count() == 6
    for _ in range(3):
        op.execute(1)
    for c in (0, 9):
        assert_ct(read_out(op, c), dot(o, ell, *synthetic_inputs(o, ell, T, SEED, copy=c)), f"copy {c}")
    op.close()


# ============================================================================================================================
# C. in a chain
# ============================================================================================================================
def test_middle_link_of_a_chain():
    """hmult,hdot,hadd at N = 2^15 against the same sequence of reference calls.  Link k runs under seed + 31 k (OpChain): its key and its
    synthetic operands ct2 .. ct<2T> are drawn from there, ct1 is the link before's output."""
    from dot_ref import assert_ct, dot, synthetic_inputs
    L, ell, alpha, T = 6, 5, 2, 2
    o = oracle(15, L, alpha)
    chain = host.Chain("config_4_N15.cfg", "hmult,hdot,hadd", L, ell, alpha, overrides={"terms": T})
    chain.execute(1)
    a = o.hmult(ell, o.synth_ct(ell, SEED), o.synth_ct(ell, SEED + 2000), o.synth_evk(ell, SEED + 10000))
    cts, evk = synthetic_inputs(o, ell - 1, T, SEED + 31)
    b = dot(o, ell - 1, [np.stack(a)] + cts[1:], evk)
    c = o.hadd(ell - 2, np.stack(b), o.synth_ct(ell - 2, SEED + 62 + 2000))
    assert [ln.split()[0] for ln in chain[1].plan()].count("TENSOR_DOT") == 1
    assert_ct(read_out(chain[0]), a, "hmult")
    assert_ct(read_out(chain[1]), b, "hdot")
    assert_ct(read_out(chain[2]), c, "hadd")
    chain.close()


# ============================================================================================================================
# D. real data
# ============================================================================================================================
def test_real_data_decrypts_to_the_sum_of_products():
    """T = 3 pairs of toy ciphertexts and the relinearisation key written with op.write: the output is the reference's bit for bit and decrypts to
    sum_t m_t m'_t / q_last within T x the bound tests/test_gpu_real_data.py holds one hmult to; the reference is held to it on the CPU first"""
    from dot_ref import assert_ct, decryption_error, dot, real_pairs
    from toy_ckks import Toy
    LOGN, L, ELL, ALPHA, T = 13, 6, 5, 2, 3
    o = oracle(LOGN, L, ALPHA)
    toy = Toy(o, seed=4245)
    cts, evk, exact = real_pairs(toy, T, ELL)
    ref = dot(o, ELL, cts, evk)
    ref_err, one = decryption_error(toy, ref, ELL, exact)
    print(f"reference: max |dec q_last - exact| = 2^{ref_err.bit_length()} (bound {T} x 2^{one.bit_length() - 1})")
    assert ref_err < T * one
    op = host.Op("config_4_N15.cfg", "hdot", L, ELL, ALPHA, overrides={"N": 1 << LOGN, "terms": T})
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
    print(f"GPU: max |dec q_last - exact| = 2^{gpu_err.bit_length()} (bound {T} x 2^{one.bit_length() - 1})")
    assert gpu_err < T * one
    assert_ct(out, ref, "real data")
