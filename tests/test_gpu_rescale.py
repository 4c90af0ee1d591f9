"""Rescale on the GPU, on both arithmetic back-ends (mont32 and chain_bits = 60), bit for bit:
 A. hm_ntt_mix_sub_scale_mul and hm_ntt_mul against the oracle's element-wise MUL followed by the reference of the base call, on permuted limb lists
    with a guard limb-poly, in every form of the transform (16-coefficient and 8-coefficient two-kernel forms, the one-launch form), their refusals,
    and one captured call replayed;
 B. hrescale and pmult / hlintrans / hrotsum / hbsgs with rescale = 1, fused and unfused, against tests/rescale_ref.py;
 C. chains: every link against the same sequence of reference calls;
 D. on real data (tests/toy_ckks.py) the rescaled result decrypts to the unrescaled one divided by q_last, within 1 + ||s||_1."""
import ctypes as C
import types

import numpy as np
import pytest

from homulator_amd import host
from oracle.homoracle import EWE_ADD, EWE_MUL, EWE_MUL_CONST, EWE_SUB_SCALE, Oracle, chain_below

pytestmark = pytest.mark.gpu
CHAINS = ["mont32", "survey"]
SEED = host.SEED
BATCH_SEED_STRIDE = 100000   # host/src/Arch.cpp kBatchSeedStride
NQ, NP = 6, 3
GUARD = 0x5A5A5A5A5A5A5A5A
_oracles = {}


def oracle(logN, L, K, chain="mont32", threads=16):
    key = (logN, L, K, chain)
    if key not in _oracles:
        _oracles[key] = Oracle(logN, L, K, chain=chain)
    _oracles[key].set_threads(threads)
    return _oracles[key]


def chain_ov(chain, base):
    return dict(base, chain_bits=60) if chain != "mont32" else dict(base)


# ============================================================================================================================
# A. the kernels
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


def operands(ctx, o, rng, mods, count, fill):
    """`count` buffers of len(mods) limb-polys each, every limb list a random permutation: [(device buffer, limb list, host rows in entry order)]"""
    n, N = len(mods), ctx.N
    out = []
    for _ in range(count):
        limbs = [int(v) for v in rng.permutation(n)]
        if fill == "uniform":
            rows = np.stack([rng.integers(0, o.moduli[m], N, dtype=np.uint64) for m in mods])
        else:
            rows = np.stack([np.full(N, o.moduli[m] - 1 if fill == "q-1" else 0, dtype=np.uint64) for m in mods])
        stored = np.empty_like(rows)
        stored[limbs] = rows
        out.append((ctx.from_host(stored), limbs, rows))
    return out


def guarded_output(ctx, rng, n):
    buf = ctx.alloc(n + 1)
    buf.upload(np.full((n + 1, ctx.N), GUARD, dtype=np.uint64))
    perm = [int(v) for v in rng.permutation(n + 1)]
    return buf, perm[:n], perm[n]


def forward_case(ctx, o, mods, seed, mix=False, addend=False, addend_k=False, plain=(), fill="uniform", replay=False):
    """one hm_ntt_mix_sub_scale_mul call against EWE_MUL + the reference of hm_ntt_mix_sub_scale; plain: entries with HM_NO_LIMB in minuend_b_limbs"""
    from homulator_amd import hip
    n = len(mods)
    rng = np.random.default_rng(seed)
    (dx, xl, x), (dmn, ml, mn), (dmb, bl, mb), (dad, al, ad), (dmx, xml, mx) = operands(ctx, o, rng, mods, 5, fill)
    out, ol, guard = guarded_output(ctx, rng, n)
    k = [int(rng.integers(1, o.moduli[m])) for m in mods]
    mk = [int(rng.integers(1, o.moduli[m])) for m in mods]
    ak = [int(rng.integers(1, o.moduli[m])) for m in mods]
    bll = [hip.NO_LIMB if i in plain else bl[i] for i in range(n)]
    kw = dict(in_limbs=xl, minuend_limbs=ml, out_limbs=ol)
    if mix:
        kw.update(mix=dmx, mix_k=mk, mix_limbs=xml)
    if addend:
        kw.update(addend=dad, addend_limbs=al)
        if addend_k:
            kw.update(addend_k=ak)
    call = lambda: ctx.ntt_mix_sub_scale_mul(dx, dmn, dmb, out, mods, k, minuend_b_limbs=bll, **kw)
    call()
    if replay:   # the launch tables are cached now: capture the same call and replay it onto a cleared output
        out.upload(np.full((n + 1, ctx.N), GUARD, dtype=np.uint64))
        g = C.c_void_p()
        ctx._ck(ctx.L.hm_capture_begin(ctx.h))
        call()
        ctx._ck(ctx.L.hm_capture_end(ctx.h, C.byref(g)))
        assert np.all(out.download() == GUARD)      # captured, not run
        ctx._ck(ctx.L.hm_graph_launch(ctx.h, g))
        ctx.sync()
        ctx.L.hm_graph_destroy(g)
    got = out.download()
    prod = o.ewe(EWE_MUL, mods, mn, mb)
    minuend = np.stack([mn[i] if i in plain else prod[i] for i in range(n)])
    xin = o.ewe(EWE_ADD, mods, x, None, o.ewe(EWE_MUL_CONST, mods, mx, k=mk)) if mix else x
    exp = o.ewe(EWE_SUB_SCALE, mods, minuend, None, o.ntt(mods, xin), k=k)
    if addend:
        exp = o.ewe(EWE_ADD, mods, exp, None, o.ewe(EWE_MUL_CONST, mods, ad, k=ak) if addend_k else ad)
    assert np.array_equal(got[ol], exp), (mods, mix, addend, addend_k, plain, fill)
    assert np.all(got[guard] == GUARD), "the guard limb-poly was written"
    for b in (dx, dmn, dmb, dad, dmx, out):
        b.free()


def inverse_case(ctx, o, mods, seed, scale=False, packed=(), fill="uniform"):
    """one hm_ntt_mul call against EWE_MUL + the reference of hm_ntt_ex; packed: entries stored in the split-30 form"""
    n = len(mods)
    rng = np.random.default_rng(seed)
    (da, al, a), (db, bl, b) = operands(ctx, o, rng, mods, 2, fill)
    out, ol, guard = guarded_output(ctx, rng, n)
    sc = [int(rng.integers(1, o.moduli[m])) for m in mods] if scale else None
    pk = [1 if i in packed else 0 for i in range(n)] if packed else None
    ctx.ntt_mul(da, db, out, mods, in_limbs=al, in_b_limbs=bl, out_limbs=ol, scale=sc, out_packed=pk)
    got = out.download()
    exp = o.ntt(mods, o.ewe(EWE_MUL, mods, a, b), inverse=True)
    if scale:
        exp = o.ewe(EWE_MUL_CONST, mods, exp, k=sc)
    for i in packed:
        exp[i] = (exp[i] & np.uint64(0x3FFFFFFF)) | ((exp[i] >> np.uint64(30)) << np.uint64(32))
    assert np.array_equal(got[ol], exp), (mods, scale, packed, fill)
    assert np.all(got[guard] == GUARD), "the guard limb-poly was written"
    for buf in (da, db, out):
        buf.free()


@pytest.mark.parametrize("chain", CHAINS)
def test_smallest_ring_every_operand_combination(envs, chain):
    """N = 2^13 (the smallest ring the transforms serve), n = 1 and n = 3: with and without mix, addend, addend_k, HM_NO_LIMB entries, out_packed"""
    ctx, o = envs(13, chain)
    s = 0
    for mods in ([NQ + 1], [0, NQ + NP - 1, 0]):
        for mix in (False, True):
            for addend, addend_k in ((False, False), (True, False), (True, True)):
                s += 1
                forward_case(ctx, o, mods, s, mix=mix, addend=addend, addend_k=addend_k, plain=(1,) if len(mods) > 1 and s % 2 else ())
        inverse_case(ctx, o, mods, 100 + s)
        inverse_case(ctx, o, mods, 200 + s, scale=True, packed=(0,))
    forward_case(ctx, o, [2, 2, 5], 99, plain=(0, 1, 2))     # every minuend plain: hm_ntt_sub_scale's result


@pytest.mark.parametrize("chain", CHAINS)
@pytest.mark.parametrize("fill", ["q-1", "zero"])
def test_worst_case_operands(envs, chain, fill):
    ctx, o = envs(13, chain)
    forward_case(ctx, o, [0, NQ + NP - 1, 3], 7, mix=True, addend=True, addend_k=True, fill=fill)
    forward_case(ctx, o, [0, NQ + NP - 1, 3], 8, fill=fill)
    inverse_case(ctx, o, [0, NQ + NP - 1, 3], 9, scale=True, fill=fill)


@pytest.mark.parametrize("chain", CHAINS)
@pytest.mark.parametrize("logN", [16, 15])
@pytest.mark.parametrize("form", ["one-launch", "two-kernel-8", "two-kernel-16"])
def test_every_form_of_the_transform(chain, logN, form):
    """n = 3 once per geometry, forced with the existing options: the one-launch form (default), the 8-coefficient two-kernel form
    (ntt_fused_small = 0) and the 16-coefficient one (ntt_small_limbs = 0 as well).  The inverse call has all three; the forward call's table leaves
    out the geometries in which the product epilogue costs a wave per SIMD, so there the options must fall back to the
    16-coefficient form and give the same bits"""
    from homulator_amd import hip
    o = oracle(logN, NQ, NP, chain)
    mods_all = o.moduli
    ctx = hip.Context(logN, NQ, NP) if chain == "mont32" else hip.Context(logN, NQ, NP, q=mods_all[:NQ], p=mods_all[NQ:])   # its own: the options stay with it
    try:
        assert ctx.moduli == o.moduli
        if form != "one-launch":
            ctx.set_option("ntt_fused_small", 0)
        if form == "two-kernel-16":
            ctx.set_option("ntt_small_limbs", 0)
        mods = [1, NQ, 1]
        forward_case(ctx, o, mods, logN, mix=True, addend=True, addend_k=True, plain=(2,))
        forward_case(ctx, o, mods, logN + 1)
        inverse_case(ctx, o, mods, logN + 2, scale=True, packed=(1,))
        inverse_case(ctx, o, mods, logN + 3)
    finally:
        ctx.close()


def test_more_entries_than_one_group_of_workgroups(envs):
    """70 limb-polys with repeated moduli (pmult's final launch at 45/35/15 has 68): above the one-launch form's limit, several same-modulus groups"""
    ctx, o = envs(13, "mont32")
    mods = [i % (NQ + NP) for i in range(70)]
    forward_case(ctx, o, mods, 70, plain=tuple(range(0, 70, 7)))
    inverse_case(ctx, o, mods, 71)


@pytest.mark.parametrize("chain", CHAINS)
def test_a_captured_call_replays(envs, chain):
    ctx, o = envs(15, chain)
    forward_case(ctx, o, [0, 4, NQ], 31, addend=True, replay=True)


def test_refusals():
    """what the two calls refuse.  The wrappers of homulator_amd/hip.py offer only what the calls serve, so the descs of the unserved combinations
    are built here"""
    from homulator_amd import hip
    ctx = hip.Context(13, NQ, NP)
    big = ctx.alloc(16)
    ctx.fill_uniform(big, [0] * 16, 5)
    at = lambda limb: types.SimpleNamespace(ptr=big.limb_ptr(limb))
    u32 = lambda v: np.array(v, dtype=np.uint32)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    mods, k, two = [0, 0], [3, 4], [0, 1]
    # in: limbs 0, 1; minuend: 2, 3; minuend_b: 4, 5; addend: 6, 7; out: 8, 9 — each through a base pointer of its own
    fwd = lambda out=8: ctx.ntt_mix_sub_scale_mul(big, at(2), at(4), at(out), mods, k, minuend_b_limbs=two, in_limbs=two, minuend_limbs=two, out_limbs=two)
    fwd()                                                                    # disjoint: accepted
    with pytest.raises(hip.HmError, match="minuend_b"):
        fwd(out=5)                                                           # out[0] is minuend_b[1], through another base pointer

    def fwd_desc(**kw):
        d, keep = ctx._fused_desc(big, at(2), at(8), mods, k, in_limbs=two, minuend_limbs=two, out_limbs=two, **kw)
        lb = u32(two)
        m = hip.hm_ntt_fused_mul_desc(d, at(4).ptr, p(lb))
        ctx._ck(ctx.L.hm_ntt_mix_sub_scale_mul(ctx.h, C.byref(m)))
    fwd_desc()
    with pytest.raises(hip.HmError, match="conv"):
        fwd_desc(conv=[(at(10), two, [NQ, NQ + 1], two, [0, 0])])
    with pytest.raises(hip.HmError, match="addend_galois"):
        fwd_desc(addend=at(6), addend_limbs=two, addend_galois=[5, 5])

    inv = lambda out=8: ctx.ntt_mul(big, at(4), at(out), mods, in_limbs=two, in_b_limbs=two, out_limbs=two)
    inv()
    with pytest.raises(hip.HmError, match="in_b"):
        inv(out=5)                                                           # out[0] is in_b[1], through another base pointer

    def inv_desc(inverse=1, second_pass_only=0, in_galois=None):
        arrs = [u32(two), u32(two), u32(mods), u32(two)] + ([u32(in_galois)] if in_galois else [])
        t = hip.hm_ntt_desc(big.ptr, p(arrs[0]), at(8).ptr, p(arrs[1]), p(arrs[2]), 2, inverse, None, second_pass_only, None, p(arrs[4]) if in_galois else None)
        m = hip.hm_ntt_mul_desc(t, at(4).ptr, p(arrs[3]))
        ctx._ck(ctx.L.hm_ntt_mul(ctx.h, C.byref(m)))
    inv_desc()
    with pytest.raises(hip.HmError, match="inverse"):
        inv_desc(inverse=0)
    with pytest.raises(hip.HmError, match="second_pass_only"):
        inv_desc(second_pass_only=1)
    with pytest.raises(hip.HmError, match="in_galois"):
        inv_desc(in_galois=[5, 5])
    ctx.close()


# ============================================================================================================================
# B. the ops
# ============================================================================================================================
ROWS = [("config_4_N15.cfg", 15, 16, 10, 4), ("config_4_N15.cfg", 15, 8, 8, 8), ("config_4_N15.cfg", 13, 6, 5, 1), ("config_4.cfg", 16, 45, 35, 15)]
R, G = 2, 2


def read_out(op, copy=0):
    return op.read("out.c0", copy=copy), op.read("out.c1", copy=copy)


def assert_ct(got, exp, what):
    assert got[0].shape == exp[0].shape, (what, got[0].shape, exp[0].shape)
    assert np.array_equal(got[0], exp[0]), (what, "c0")
    assert np.array_equal(got[1], exp[1]), (what, "c1")


def lintrans_inputs(o, ell, seed, copy=0):
    c = copy * BATCH_SEED_STRIDE
    ids = o.ext_ids(ell)
    return ([o.synth_evk(ell, seed + 10000 + 100000 * r) for r in range(1, R + 1)], [o.fill_uniform(ids, seed + 4000 + 100000 * r + c) for r in range(1, R + 1)],
            o.fill_uniform(ids, seed + 4300 + c))


def reference(o, op, ell, identity=False, seed=SEED, copy=0, ct=None):
    """the op with rescale = 1 on its synthetic streams (tests/rescale_ref.py); ct: the first operand, if it is not the op's own stream"""
    import rescale_ref as rr
    from bsgs_ref import synthetic_inputs as bsgs_inputs
    from identity_ref import bsgs_id_inputs
    from rotsum_ref import synthetic_inputs as rotsum_inputs
    c = copy * BATCH_SEED_STRIDE
    ct1 = o.synth_ct(ell, seed + c) if ct is None else ct
    if op == "hrescale":
        return rr.rescale_ct(o, ell, ct1)
    if op == "pmult":
        return rr.pmult_rescaled(o, ell, ct1, o.fill_uniform(list(range(ell)), seed + 4000 + c))
    if op == "hlintrans":
        keys, pts, pt0 = lintrans_inputs(o, ell, seed, copy)
        return rr.lintrans_rescaled(o, ell, ct1, 5, keys, pts, pt0 if identity else None)
    if op == "hrotsum":
        cts, keys = rotsum_inputs(o, ell, G, seed, copy)
        return rr.rotsum_rescaled(o, ell, [ct1] + cts[1:], 5, keys)
    _, bk, gk, pts = bsgs_inputs(o, ell, R, G, seed, copy)
    if not identity:
        return rr.bsgs_rescaled(o, ell, ct1, 5, pow(5, R, 2 * o.N), bk, gk, pts)
    pt0s, ptgs = bsgs_id_inputs(o, ell, R, G, seed, copy)
    return rr.bsgs_rescaled(o, ell, ct1, 5, pow(5, R + 1, 2 * o.N), bk, gk, pts, pt0s, ptgs)


def overrides(op, chain, logN, **extra):
    ov = {"N": 1 << logN}
    if op != "hrescale":
        ov["rescale"] = 1
    if op in ("hlintrans", "hbsgs"):
        ov["rotations"] = R
    if op == "hrotsum":
        ov["rotations"] = G
    if op == "hbsgs":
        ov["giants"] = G
    return chain_ov(chain, dict(ov, **extra))


def run_op(cfg, op, L, ell, alpha, ov, fuse=True, runs=1, copies=1):
    o = host.Op(cfg, op, L, ell, alpha, fuse=fuse, overrides=ov)
    try:
        for _ in range(runs):
            o.execute(1)
        return [read_out(o, c) for c in range(copies)], [ln.split()[0] for ln in o.plan()], o.plan()
    finally:
        o.close()


@pytest.mark.parametrize("chain", CHAINS)
@pytest.mark.parametrize("cfg,logN,L,ell,alpha", ROWS)
@pytest.mark.parametrize("op", ["hrescale", "pmult", "hlintrans", "hrotsum", "hbsgs"])
def test_op_fused_unfused_and_reference_agree(chain, cfg, logN, L, ell, alpha, op):
    o = oracle(logN, L, alpha, chain)
    exp = reference(o, op, ell)
    extra = {"fuse_pmul_rescale": 1} if op == "pmult" else {}     # said, not left to the default: the product kernels run on both back-ends
    for fuse in (True, False):
        got, kinds, plan = run_op(cfg, op, L, ell, alpha, overrides(op, chain, logN, **extra), fuse=fuse)
        assert_ct(got[0], exp, (op, "fused" if fuse else "unfused"))
        if op == "pmult":
            assert (kinds == ["INTT", "NTT_SUBSCALE"] and all("mul=1" in ln for ln in plan)) if fuse else "mul=1" not in "".join(plan)


@pytest.mark.parametrize("chain", CHAINS)
@pytest.mark.parametrize("op", ["hlintrans", "hbsgs"])
def test_identity_composes_with_the_rescale(chain, op):
    """W is the c1 addend of the merged transform, as d1 is in hmult"""
    cfg, logN, L, ell, alpha = ROWS[0]
    o = oracle(logN, L, alpha, chain)
    exp = reference(o, op, ell, identity=True)
    for fuse in (True, False):
        got, _, _ = run_op(cfg, op, L, ell, alpha, overrides(op, chain, logN, identity=1), fuse=fuse)
        assert_ct(got[0], exp, (op, fuse))


@pytest.mark.parametrize("chain", CHAINS)
def test_pmult_with_one_output_limb_and_with_the_pass_off(chain):
    cfg, logN, L, alpha = "config_4_N15.cfg", 15, 16, 4
    o = oracle(logN, L, alpha, chain)
    got, kinds, _ = run_op(cfg, "pmult", L, 2, alpha, overrides("pmult", chain, logN, fuse_pmul_rescale=1))
    assert_ct(got[0], reference(o, "pmult", 2), "l = 2")
    assert kinds == ["INTT", "NTT_SUBSCALE"]
    got, kinds, plan = run_op(cfg, "pmult", L, 10, alpha, overrides("pmult", chain, logN, fuse_pmul_rescale=0))
    assert_ct(got[0], reference(o, "pmult", 10), "pass off")
    assert kinds == ["EWE", "INTT", "NTT_SUBSCALE"] and "mul=1" not in "".join(plan)


def test_pmult_default_on_the_generic_back_end():
    """fuse_pmul_rescale not given, chain_bits = 60: the three-launch plan inside the one-launch limit (18 limb-polys), the product transforms above it
    (batch 11: 198 > 192 at N = 2^15); both against the reference"""
    cfg, logN, L, ell, alpha = ROWS[0]
    o = oracle(logN, L, alpha, "survey")
    got, kinds, _ = run_op(cfg, "pmult", L, ell, alpha, overrides("pmult", "survey", logN))
    assert kinds == ["EWE", "INTT", "NTT_SUBSCALE"]
    assert_ct(got[0], reference(o, "pmult", ell), "small launch")
    got, kinds, plan = run_op(cfg, "pmult", L, ell, alpha, overrides("pmult", "survey", logN, batch=11), copies=11)
    assert kinds == ["INTT", "NTT_SUBSCALE"] and all("mul=1" in ln for ln in plan)
    for c in (0, 10):
        assert_ct(got[c], reference(o, "pmult", ell, copy=c), ("batch 11, copy", c))


@pytest.mark.parametrize("op", ["hrescale", "pmult", "hlintrans", "hrotsum", "hbsgs"])
def test_batch_of_three(op):
    cfg, logN, L, ell, alpha = ROWS[0]
    o = oracle(logN, L, alpha)
    got, _, _ = run_op(cfg, op, L, ell, alpha, overrides(op, "mont32", logN, batch=3), copies=3)
    for c in range(3):
        assert_ct(got[c], reference(o, op, ell, copy=c), (op, "copy", c))


@pytest.mark.parametrize("op", ["hrescale", "pmult", "hlintrans", "hrotsum", "hbsgs"])
def test_graph_replay(op):
    """run 1 direct, run 2 captures, run 3 replays"""
    cfg, logN, L, ell, alpha = ROWS[0]
    o = oracle(logN, L, alpha)
    got, _, _ = run_op(cfg, op, L, ell, alpha, overrides(op, "mont32", logN, graph=1), runs=3)
    assert_ct(got[0], reference(o, op, ell), (op, "graph"))


@pytest.mark.parametrize("op", ["pmult", "hlintrans", "hrotsum", "hbsgs"])
def test_rescale_0_is_the_op_without_the_key(op):
    cfg, logN, L, ell, alpha = ROWS[0]
    base = {k: v for k, v in overrides(op, "mont32", logN).items() if k != "rescale"}
    a, _, pa = run_op(cfg, op, L, ell, alpha, base)
    b, _, pb = run_op(cfg, op, L, ell, alpha, dict(base, rescale=0))
    assert pa == pb and a[0][0].shape[0] == ell
    assert_ct(a[0], b[0], op)


# ============================================================================================================================
# C. chains
# ============================================================================================================================
def test_chain_pmult_hrescale_hmult():
    """link k runs under seed + 31 k (OpChain): its second operand and keys are drawn from there, its first operand is the link before's output"""
    L, ell, alpha = 6, 5, 2
    o = oracle(15, L, alpha)
    chain = host.Chain("config_4_N15.cfg", "pmult,hrescale,hmult", L, ell, alpha)
    chain.execute(1)
    a = o.pmult(ell, o.synth_ct(ell, SEED), o.fill_uniform(list(range(ell)), SEED + 4000))
    b = reference(o, "hrescale", ell, ct=np.stack(a))
    c = o.hmult(ell - 1, np.stack(b), o.synth_ct(ell - 1, SEED + 62 + 2000), o.synth_evk(ell - 1, SEED + 62 + 10000))
    assert c[0].shape[0] == ell - 2
    for i, (exp, what) in enumerate(((a, "pmult"), (b, "hrescale"), (c, "hmult"))):
        assert_ct(read_out(chain[i]), exp, what)
    chain.close()


def test_chain_hlintrans_with_rescale_then_hadd():
    L, ell, alpha = 6, 5, 2
    o = oracle(15, L, alpha)
    chain = host.Chain("config_4_N15.cfg", "hlintrans,hadd", L, ell, alpha, overrides={"rotations": R, "rescale": 1})
    chain.execute(1)
    a = reference(o, "hlintrans", ell)
    b = o.hadd(ell - 1, np.stack(a), o.synth_ct(ell - 1, SEED + 31 + 2000))
    assert_ct(read_out(chain[0]), a, "hlintrans")
    assert_ct(read_out(chain[1]), b, "hadd")
    chain.close()


# ============================================================================================================================
# D. real data
# ============================================================================================================================
@pytest.mark.parametrize("op", ["pmult", "hlintrans"])
def test_real_data_decrypts_to_the_unrescaled_result_over_q_last(op):
    """The same real inputs with rescale = 1 and rescale = 0.  out'_k = (out_k - [out_k]_{q_last}) / q_last = out_k / q_last - f_k with every
    coefficient of f_k in [0, 1), so Dec(out') - Dec(out) / q_last = -(f_0 + f_1 s) mod Q': below 1 + ||s||_1 in every coefficient (f_1 s is a
    negacyclic product with a ternary s).  A derived bound, computed from the toy key; compared as integers, times q_last, centred mod Q = q_last Q'."""
    from toy_ckks import Toy
    LOGN, L, ELL, ALPHA, g = 13, 6, 5, 2, 5
    o = oracle(LOGN, L, ALPHA)
    toy = Toy(o, seed=4243)
    s1 = int(sum(abs(int(v)) for v in toy.s))
    m = toy.rng.integers(-1000, 1000, o.N).astype(object) * (1 << 30)
    ct = toy.encrypt(m, ELL)
    ids = o.ext_ids(ELL)

    def plaintext():
        p = np.zeros(o.N, dtype=object)
        for i in toy.rng.choice(o.N, 8, replace=False):
            p[int(i)] = int(toy.rng.integers(-(1 << 10), (1 << 10) + 1))
        return p
    writes = {"ct1.c0": ct[0], "ct1.c1": ct[1]}
    ov = {"N": 1 << LOGN}
    if op == "pmult":
        writes["pt"] = toy.to_rns_eval(plaintext(), ids[:ELL])
    else:
        ov.update(rotations=R, galois=g)
        for r in range(1, R + 1):
            writes[f"pt{r}"] = toy.to_rns_eval(plaintext(), ids)
            key = toy.evk_at_level(toy.gen_evk(toy.automorph(toy.s, pow(g, r, 2 * o.N))), ELL)
            for j in range(key.shape[0]):
                for k in range(2):
                    writes[f"IP_Rot{r}_Key{k}_{j}"] = key[j][k]
    dec = {}
    for rescale in (0, 1):
        h = host.Op("config_4_N15.cfg", op, L, ELL, ALPHA, overrides=dict(ov, rescale=rescale))
        for name, data in writes.items():
            h.write(name, data)
        h.execute(1)
        dec[rescale] = toy.decrypt(np.stack(read_out(h)), ELL - rescale)
        h.close()
    (d0, Q), (d1, Q1) = dec[0], dec[1]
    qlast = o.moduli[ELL - 1]
    assert Q == Q1 * qlast
    worst = 0
    for a, b in zip(d1, d0):
        num = (qlast * int(a) - int(b)) % Q
        worst = max(worst, min(num, Q - num))
    print(f"{op}: max |q_last Dec(out') - Dec(out)| / q_last = {worst / qlast:.3f} (bound 1 + ||s||_1 = {1 + s1})")
    assert worst < qlast * (1 + s1)
