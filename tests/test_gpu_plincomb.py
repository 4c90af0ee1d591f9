"""hplincomb on the GPU, on both arithmetic back-ends (mont32 and chain_bits = 60), bit for bit:
 A. hm_plincomb through the ABI: against the reference's primitives (oracle MUL and ADD, and Python integers on some entries) and against the
    element-wise chain through hm_ewe (MUL, MAC_ADD per term and component, ADD for the addend) on the same device data, on permuted and repeated
    limbs with mixed moduli, the plaintexts in an allocation of their own and a guard limb-poly in the output buffer; the refusals; n = 0; a
    captured call replayed;
 B. the op, fused (one PLINCOMB launch), unfused (one launch per stage) and with fuse_plincomb = 0, against the reference; batch 2, graph = 1,
    caller-written plaintexts, T = 1 against pmult on the device, hrotate_hoisted -> hplincomb link by link, and real data (tests/toy_ckks.py)."""
import ctypes as C
import types

import numpy as np
import pytest

from homulator_amd import host
from oracle.homoracle import EWE_ADD, EWE_MUL, Oracle, chain_below

pytestmark = pytest.mark.gpu
CHAINS = ["mont32", "survey"]
SEED = host.SEED
NQ, NP = 6, 3
PER_MOD = 3            # ciphertext limb-polys per modulus in the kernel cases: term lists draw from them with repetition
PT_PER_MOD = 2         # plaintext limb-polys per modulus, in another allocation: shared by records and terms
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
    """(hip context, oracle on the same moduli, the ciphertext pool and the plaintext pool on the device and on the host) per (logN, chain), made
    on first use.  Limb m * PER_MOD + r of the ciphertext pool and limb m * PT_PER_MOD + r of the plaintext pool are filled for modulus m; neither
    is written again"""
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
            pool, pts = ctx.alloc((NQ + NP) * PER_MOD), ctx.alloc((NQ + NP) * PT_PER_MOD)
            ctx.fill_uniform(pool, [m for m in range(NQ + NP) for _ in range(PER_MOD)], 1900 + logN)
            ctx.fill_uniform(pts, [m for m in range(NQ + NP) for _ in range(PT_PER_MOD)], 2900 + logN)
            made[(logN, chain)] = (ctx, o, pool, pool.download(), pts, pts.download())
        return made[(logN, chain)]
    yield get
    for ctx, _, pool, _, pts, _ in made.values():
        pool.free()
        pts.free()
        ctx.close()


def kernel_lists(mods, T, rng, addend=True):
    """per record and term a plaintext limb and two ciphertext limbs of its modulus from the pools (repeats allowed), and an addend limb"""
    n = len(mods)
    lp = [mods[i] * PT_PER_MOD + int(rng.integers(0, PT_PER_MOD)) for i in range(n) for _ in range(T)]
    lx0 = [mods[i] * PER_MOD + int(rng.integers(0, PER_MOD)) for i in range(n) for _ in range(T)]
    lx1 = [mods[i] * PER_MOD + int(rng.integers(0, PER_MOD)) for i in range(n) for _ in range(T)]
    la = [m * PT_PER_MOD + int(rng.integers(0, PT_PER_MOD)) for m in mods] if addend else None
    return lp, lx0, lx1, la


def expected_rows(o, host_pool, host_pts, mods, T, lp, lx0, lx1, la):
    """the Python-side reference, from the reference's primitives: MUL per term, ADD between the terms and for the addend"""
    n, ids = len(mods), list(mods)
    out = []
    for lx, add in ((lx0, la), (lx1, None)):
        acc = None
        for t in range(T):
            term = o.ewe(EWE_MUL, ids, np.stack([host_pool[lx[i * T + t]] for i in range(n)]), np.stack([host_pts[lp[i * T + t]] for i in range(n)]))
            acc = term if acc is None else o.ewe(EWE_ADD, ids, acc, None, term)
        if add is not None:
            acc = o.ewe(EWE_ADD, ids, acc, None, np.stack([host_pts[a] for a in add]))
        out.append(acc)
    return out


def run_kernel_case(env, mods, T, seed, addend=True, composed=True):
    """one hm_plincomb call: the output buffer holds 2 n limb-polys and one guard limb-poly, the output lists are a random permutation"""
    from homulator_amd import hip
    ctx, o, pool, host_pool, pts, host_pts = env
    n, N = len(mods), ctx.N
    rng = np.random.default_rng(seed)
    lp, lx0, lx1, la = kernel_lists(mods, T, rng, addend)
    perm = [int(v) for v in rng.permutation(2 * n + 1)]
    l0, l1 = perm[:n], perm[n:2 * n]
    out = ctx.alloc(2 * n + 1)
    out.upload(np.full((2 * n + 1, N), GUARD, dtype=np.uint64))
    ctx.plincomb(pts, lp, pool, lx0, lx1, out, l0, l1, mods, T, addend=pts if addend else None, addend_limbs=la)
    got = out.download()
    exp = expected_rows(o, host_pool, host_pts, mods, T, lp, lx0, lx1, la)
    what = (n, T, addend)
    assert np.array_equal(got[l0], exp[0]), (what, "c0")
    assert np.array_equal(got[l1], exp[1]), (what, "c1")
    assert np.all(got[perm[2 * n]] == GUARD), "the guard limb-poly was written"
    if T <= 3:   # the definition in Python integers on a stretch of some records
        for i in sorted({0, n // 2, n - 1}):
            q = int(ctx.moduli[mods[i]])
            for x in (0, 1, N // 2 - 1, N // 2, N - 1):
                e0 = sum(int(host_pts[lp[i * T + t]][x]) * int(host_pool[lx0[i * T + t]][x]) for t in range(T)) + (int(host_pts[la[i]][x]) if addend else 0)
                e1 = sum(int(host_pts[lp[i * T + t]][x]) * int(host_pool[lx1[i * T + t]][x]) for t in range(T))
                assert (int(got[l0[i]][x]), int(got[l1[i]][x])) == (e0 % q, e1 % q), (what, i, x)
    if composed:   # the same from the calls it replaces, on the same device data
        acc = [ctx.alloc(n), ctx.alloc(n)]
        for k, lx in enumerate((lx0, lx1)):
            for t in range(T):
                lxa, lpb = [lx[i * T + t] for i in range(n)], [lp[i * T + t] for i in range(n)]
                if t == 0:
                    ctx.ewe(hip.OP_MUL, acc[k], mods, a=pool, la=lxa, b=pts, lb=lpb)
                else:
                    ctx.ewe(hip.OP_MAC_ADD, acc[k], mods, a=pool, la=lxa, b=pts, lb=lpb, c=acc[k])
        if addend:
            ctx.ewe(hip.OP_ADD, acc[0], mods, a=acc[0], c=pts, lc=la)
        assert np.array_equal(acc[0].download(), got[l0]) and np.array_equal(acc[1].download(), got[l1]), (what, "composed")
        for buf in acc:
            buf.free()
    out.free()


@pytest.mark.parametrize("chain", CHAINS)
@pytest.mark.parametrize("T", [1, 2, 3, 16])
@pytest.mark.parametrize("n", [1, 3, 65, 130])
def test_kernel_entry_and_term_counts(envs, chain, n, T):
    """ONE launch for any n (across the 64- and 128-entry cuts of the launches whose records travel as kernel arguments); T = 1 runs no round of
    the two-term loop, 2 the tail behind it, 3 one round, 16 the most; Q and P limbs, mixed moduli, permuted and repeated limbs, the plaintexts in
    an allocation of their own.  With the addend, and without at the odd sizes"""
    mods = [(5 * i + 2) % (NQ + NP) for i in range(n)]
    run_kernel_case(envs(13, chain), mods, T, 40 + 17 * n + T, addend=True)
    if n in (3, 65):
        run_kernel_case(envs(13, chain), mods, T, 90 + 17 * n + T, addend=False)


@pytest.mark.parametrize("chain", CHAINS)
@pytest.mark.parametrize("logN", [15, 16])
def test_kernel_at_larger_rings(envs, chain, logN):
    run_kernel_case(envs(logN, chain), [0, 5, NQ, 5, 2], 3, logN + 3)
    run_kernel_case(envs(logN, chain), [0, 5, NQ, 5, 2], 16, logN + 16, composed=False)


def test_plaintexts_and_ciphertexts_may_share_an_allocation(envs):
    """p, x and addend through one base pointer: plaintext limbs drawn from the ciphertext pool itself"""
    ctx, o, pool, host_pool, _, _ = envs(13, "mont32")
    mods, T = [0, 3, NQ, 1], 2
    lp = [m * PER_MOD + 2 for m in mods for _ in range(T)]
    lx0 = [m * PER_MOD for m in mods for _ in range(T)]
    lx1 = [m * PER_MOD + 1 for m in mods for _ in range(T)]
    la = [m * PER_MOD + 1 for m in mods]
    out = ctx.alloc(8)
    ctx.plincomb(pool, lp, pool, lx0, lx1, out, [0, 1, 2, 3], [4, 5, 6, 7], mods, T, addend=pool, addend_limbs=la)
    got = out.download()
    pt_of = {a: a for a in range(len(host_pool))}
    exp = expected_rows(o, host_pool, host_pool, mods, T, [pt_of[a] for a in lp], lx0, lx1, la)
    assert np.array_equal(got[:4], exp[0]) and np.array_equal(got[4:], exp[1])
    out.free()


def _alias_call(ctx, big, out_at=40, n=4, T=2, addend=False, l0_from=0, l1_from=4):
    """n = 4 records of 2 terms in ONE allocation: plaintext limbs 0 .. 7, ciphertext limbs 8 .. 23 and addend limbs 24 .. 27 through the
    allocation's base, the outputs through a base pointer of their own at limb `out_at`: c0's n limbs from `l0_from` behind it, c1's from `l1_from`"""
    at = lambda limb: types.SimpleNamespace(ptr=big.limb_ptr(limb))
    ctx.plincomb(big, list(range(n * T)), big, list(range(8, 8 + n * T)), list(range(16, 16 + n * T)), at(out_at), list(range(l0_from, l0_from + n)), list(range(l1_from, l1_from + n)), [0] * n, T,
                 addend=big if addend else None, addend_limbs=list(range(24, 24 + n)) if addend else None)


def test_refuses_an_output_over_an_input_through_another_base_pointer():
    from homulator_amd import hip
    ctx = hip.Context(13, NQ, NP)
    big = ctx.alloc(64)
    ctx.fill_uniform(big, [0] * 64, 5)
    _alias_call(ctx, big)                                   # disjoint: accepted
    _alias_call(ctx, big, out_at=24)                        # over limbs that are an addend only when one is passed: accepted
    for out_at, name in ((0, "p"), (4, "p"), (5, "p"), (8, "x"), (12, "x"), (20, "x")):
        with pytest.raises(hip.HmError, match=rf"hm_plincomb: an output limb-poly \(out\) overlaps an input limb-poly \({name}\)"):
            _alias_call(ctx, big, out_at=out_at)
    for out_at in (24, 21, 27):
        with pytest.raises(hip.HmError, match=r"hm_plincomb: an output limb-poly \(out\) overlaps an input limb-poly \((x|addend)\)"):
            _alias_call(ctx, big, out_at=out_at, addend=True)
    with pytest.raises(hip.HmError, match=r"overlaps an input limb-poly \(addend\)"):
        _alias_call(ctx, big, out_at=24, l0_from=4, l1_from=0, addend=True)     # c1's outputs alone over the addend
    with pytest.raises(hip.HmError, match="hm_plincomb: two output limb-polys overlap"):
        _alias_call(ctx, big, out_at=40, l1_from=3)                 # c1's first output is c0's last
    ctx.sync()
    ctx.close()


def test_refuses_bad_arguments_and_accepts_n_0():
    from homulator_amd import hip
    ctx = hip.Context(13, NQ, NP)
    src, pts, out = ctx.alloc(4), ctx.alloc(4), ctx.alloc(4)
    ctx.fill_uniform(src, [0] * 4, 5)
    ctx.fill_uniform(pts, [0] * 4, 6)
    null = types.SimpleNamespace(ptr=None)
    one, zero = hip._u32([1]), hip._u32([0])      # (kept alive: the raw calls below take their addresses)
    call = lambda p=pts, lp=(0,), x=src, lx0=(0,), lx1=(1,), o=out, l0=(0,), l1=(1,), mods=(0,), T=1, **kw: ctx.plincomb(
        p, list(lp), x, list(lx0), list(lx1), o, list(l0), list(l1), list(mods), T, **kw)
    for kw in ({"p": null}, {"x": null}, {"o": null}):
        with pytest.raises(hip.HmError, match="hm_plincomb: null buffer"):
            call(**kw)
    with pytest.raises(hip.HmError, match="hm_plincomb: mod_ids is null"):
        ctx._ck(ctx.L.hm_plincomb(ctx.h, pts.ptr, None, src.ptr, None, one[1], None, None, out.ptr, None, one[1], None, 1, 1))
    for T in (0, 17):
        with pytest.raises(hip.HmError, match=rf"hm_plincomb: n_terms = {T}, must be in \[1, 16\]"):
            call(lp=[0] * T, lx0=[0] * T, lx1=[1] * T, T=T)
    for kw in ({"lp": (0, 70000), "lx0": (0, 1), "lx1": (2, 3), "T": 2}, {"lx0": (70000,)}, {"lx1": (70000,)}, {"l0": (70000,)}, {"l1": (70000,)},
               {"addend": pts, "addend_limbs": [70000]}):
        with pytest.raises(hip.HmError, match="65535"):
            call(**kw)
    with pytest.raises(hip.HmError, match="mod id"):
        call(mods=(NQ + NP,))
    with pytest.raises(hip.HmError, match="two output limb-polys overlap"):     # the two outputs of one record
        call(l0=(2,), l1=(2,))
    with pytest.raises(hip.HmError, match="two output limb-polys overlap"):     # null output lists: both the identity
        ctx._ck(ctx.L.hm_plincomb(ctx.h, pts.ptr, None, src.ptr, None, one[1], None, None, out.ptr, None, None, zero[1], 1, 1))
    with pytest.raises(hip.HmError, match="two output limb-polys overlap"):     # c0 of entry 0 and c1 of entry 1
        call(lp=(0, 1), lx0=(0, 1), lx1=(2, 3), l0=(0, 1), l1=(2, 0), mods=(0, 0))
    with pytest.raises(hip.HmError, match=r"overlaps an input limb-poly \(x\)"):
        call(o=src, l0=(3,), l1=(1,))
    with pytest.raises(hip.HmError, match=r"overlaps an input limb-poly \(p\)"):
        call(o=pts, l0=(0,), l1=(1,))
    with pytest.raises(hip.HmError, match=r"overlaps an input limb-poly \(addend\)"):
        call(o=pts, l0=(2,), l1=(3,), addend=pts, addend_limbs=[3])
    call(o=pts, l0=(2,), l1=(3,))                                               # ... the same outputs without the addend: accepted
    ctx._ck(ctx.L.hm_plincomb(ctx.h, pts.ptr, None, src.ptr, None, None, None, None, out.ptr, None, None, zero[1], 0, 3))   # n = 0: nothing to do
    call(lp=(0, 0, 0, 1), lx0=(0, 1, 1, 0), lx1=(2, 2, 3, 3), l0=(3, 0), l1=(1, 2), mods=(0, 0), T=2, addend=src, addend_limbs=[0, 0])   # nothing wrong
    ctx.sync()
    ctx.close()


@pytest.mark.parametrize("chain", CHAINS)
def test_a_captured_call_replays(envs, chain):
    """the records live in a cached device table: after one warm run the call is captured into a graph and replayed on new input data"""
    ctx, o, _, _, _, _ = envs(13, chain)
    ctx.L.hm_graph_launch.argtypes = [C.c_void_p, C.c_void_p]
    ctx.L.hm_graph_destroy.argtypes = [C.c_void_p]
    T = 3
    mods = [(3 * i + 1) % (NQ + NP) for i in range(70)]
    x_mods = [m for m in range(NQ + NP) for _ in range(PER_MOD)]
    p_mods = [m for m in range(NQ + NP) for _ in range(PT_PER_MOD)]
    lp, lx0, lx1, la = kernel_lists(mods, T, np.random.default_rng(3))
    src, pts, out = ctx.alloc(len(x_mods)), ctx.alloc(len(p_mods)), ctx.alloc(2 * len(mods))
    l0, l1 = list(range(0, 140, 2)), list(range(1, 140, 2))
    run = lambda: ctx.plincomb(pts, lp, src, lx0, lx1, out, l0, l1, mods, T, addend=pts, addend_limbs=la)
    ctx.fill_uniform(src, x_mods, 1)
    ctx.fill_uniform(pts, p_mods, 11)
    run()
    g = C.c_void_p()
    ctx._ck(ctx.L.hm_capture_begin(ctx.h))
    run()
    ctx._ck(ctx.L.hm_capture_end(ctx.h, C.byref(g)))
    ctx.fill_uniform(src, x_mods, 2)
    ctx.fill_uniform(pts, p_mods, 12)
    out.upload(np.full((2 * len(mods), ctx.N), GUARD, dtype=np.uint64))
    ctx._ck(ctx.L.hm_graph_launch(ctx.h, g))
    ctx.sync()
    exp = expected_rows(o, src.download(), pts.download(), mods, T, lp, lx0, lx1, la)
    got = out.download()
    assert np.array_equal(got[l0], exp[0]) and np.array_equal(got[l1], exp[1]), chain
    ctx.L.hm_graph_destroy(g)
    for buf in (src, pts, out):
        buf.free()


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
KEYS = [(1, 0, 0), (2, 1, 1), (4, 1, 0), (4, 0, 1)]     # (terms, pl_addend, rescale): every T, both values of either key
_ref = {}


def reference(chain, logN, L, ell, alpha, keys, copy=0, seed=SEED):
    """the reference output on the op's synthetic inputs, computed once per case"""
    from plincomb_ref import plincomb, synthetic_plaintexts
    from lincomb_ref import synthetic_inputs
    key = (chain, logN, L, ell, alpha, keys, copy, seed)
    if key not in _ref:
        T, pa, rs = keys
        o = oracle(logN, L, alpha, chain, threads=16)
        _ref[key] = plincomb(o, ell, synthetic_inputs(o, ell, seed, T, copy=copy), *synthetic_plaintexts(o, ell, seed, T, pa, copy=copy), rescale=bool(rs))
    return _ref[key]


@pytest.mark.parametrize("chain", CHAINS)
@pytest.mark.parametrize("keys", KEYS)
@pytest.mark.parametrize("cfg,logN,L,ell,alpha,batch", SHAPES)
def test_op_fused_unfused_and_reference_agree(chain, keys, cfg, logN, L, ell, alpha, batch):
    """fused, unfused and fuse_plincomb = 0 against the reference; batch 2 (first shape): both copies, each under its own plaintexts"""
    from plincomb_ref import assert_ct
    T, pa, rs = keys
    ov = chain_ov(chain, {"terms": T, "pl_addend": pa, "rescale": rs, "batch": batch, "N": 1 << logN})
    for mode, fuse, extra in (("fused", True, {}), ("unfused", False, {}), ("fuse_plincomb = 0", True, {"fuse_plincomb": 0})):
        op = host.Op(cfg, "hplincomb", L, ell, alpha, fuse=fuse, overrides=dict(ov, **extra))
        op.execute(1)
        kinds = [ln.split()[0] for ln in op.plan()]
        assert kinds.count("PLINCOMB") == (1 if mode == "fused" else 0), (mode, kinds)
        for c in range(batch):
            got = read_out(op, c)
            assert got[0].shape[0] == ell - rs
            assert_ct(got, reference(chain, logN, L, ell, alpha, keys, copy=c), (mode, keys, c))
        op.close()


def test_graph_replay_with_a_batch():
    """graph = 1: run 1 direct, run 2 captures, run 3 replays; both copies after the replay"""
    from plincomb_ref import assert_ct
    cfg, logN, L, ell, alpha, batch = SHAPES[0]
    keys = (2, 1, 1)
    op = host.Op(cfg, "hplincomb", L, ell, alpha, overrides={"terms": 2, "pl_addend": 1, "rescale": 1, "batch": batch, "graph": 1})
    lc = [ln for ln in op.plan() if ln.startswith("PLINCOMB")]
    assert len(lc) == 1 and f" n={batch * ell} " in lc[0] and " terms=2 addend=1" in lc[0]
    for _ in range(3):
        op.execute(1)
    for c in range(batch):
        assert_ct(read_out(op, c), reference("mont32", logN, L, ell, alpha, keys, copy=c), f"copy {c}")
    op.close()


@pytest.mark.parametrize("chain", CHAINS)
@pytest.mark.parametrize("fuse", [True, False])
def test_caller_written_plaintexts(chain, fuse):
    """pt1 .. pt3 and pt0 written with Op.write: constant polynomials, a sparse one and uniform ones"""
    from plincomb_ref import assert_ct, constant_plaintext, encode, plincomb
    from lincomb_ref import synthetic_inputs
    L, ell, alpha, T = 6, 5, 2, 3
    o = oracle(13, L, alpha, chain)
    q = [int(v) for v in o.moduli]
    ids = list(range(ell))
    pts = [constant_plaintext(o, ell, [q[j] - 1 for j in range(ell)]), encode(o, ell, {0: 3, 5: -2, o.N // 2: 1}), o.fill_uniform(ids, 77)]
    addend = o.fill_uniform(ids, 78)
    op = host.Op("config_4_N15.cfg", "hplincomb", L, ell, alpha, fuse=fuse, overrides=chain_ov(chain, {"terms": T, "pl_addend": 1, "N": 1 << 13}))
    for t in range(T):
        op.write(f"pt{t + 1}", pts[t])
    op.write("pt0", addend)
    op.execute(1)
    assert_ct(read_out(op), plincomb(o, ell, synthetic_inputs(o, ell, SEED, T), pts, addend), ("caller plaintexts", chain, fuse))
    op.close()


@pytest.mark.parametrize("chain", CHAINS)
def test_one_term_is_pmult_on_the_device(chain):
    """T = 1 without the addend, fed pmult's ciphertext (the same stream) and pmult's plaintext read back from the device: pmult's output bit
    for bit"""
    from plincomb_ref import assert_ct
    L, ell, alpha = 6, 5, 2
    ov = chain_ov(chain, {"N": 1 << 13})
    pm = host.Op("config_4_N15.cfg", "pmult", L, ell, alpha, overrides=ov)
    pm.execute(1)
    op = host.Op("config_4_N15.cfg", "hplincomb", L, ell, alpha, overrides=dict(ov, terms=1))
    op.write("pt1", pm.read("pt"))
    op.execute(1)
    assert np.array_equal(op.read("ct1.c0"), pm.read("ct1.c0")) and np.array_equal(op.read("ct1.c1"), pm.read("ct1.c1"))
    assert [ln.split()[0] for ln in op.plan()] == ["PLINCOMB"]
    got = read_out(op)
    assert got[0].any()
    assert_ct(got, read_out(pm), ("T = 1 is pmult", chain))
    op.close()
    pm.close()


@pytest.mark.parametrize("chain", CHAINS)
def test_chain_hoisted_rotations_into_hplincomb(chain):
    """the inner sum of a baby-step/giant-step transform over rotations that exist: ct<t> of hplincomb bound to output t of ONE hrotate_hoisted.
    Link by link: the rotations against the reference's hrotate, the sum against plincomb_ref on those rotations"""
    from hoisted_ref import hoisted_rotations
    from plincomb_ref import assert_ct, plincomb, synthetic_plaintexts
    L, ell, alpha, R = 6, 5, 2, 3
    o = oracle(13, L, alpha, chain)
    ov = chain_ov(chain, {"N": 1 << 13})
    rot = host.Op("config_4_N15.cfg", "hrotate_hoisted", L, ell, alpha, overrides=dict(ov, rotations=R, galois=5))
    op = host.Op("config_4_N15.cfg", "hplincomb", L, ell, alpha, overrides=dict(ov, terms=R, pl_addend=1, seed=SEED + 31))
    for t in range(1, R + 1):
        op.bind_input(f"ct{t}", rot, output=f"out{t}")
    rot.execute(1)
    op.execute(1)
    assert [ln.split()[0] for ln in op.plan()] == ["PLINCOMB"]
    rots = [np.stack([rot.read(f"out{t}.c0"), rot.read(f"out{t}.c1")]) for t in range(1, R + 1)]
    keys = [o.synth_evk(ell, SEED + 10000 + 100000 * r) for r in range(1, R + 1)]
    exp = hoisted_rotations(o, ell, o.synth_ct(ell, SEED), 5, keys)
    for r in range(R):
        assert_ct(rots[r], exp[r], ("hrotate_hoisted", chain, r))
    pts, addend = synthetic_plaintexts(o, ell, SEED + 31, R, 1)
    assert_ct(read_out(op), plincomb(o, ell, rots, pts, addend), ("hrotate_hoisted -> hplincomb", chain))
    op.close()
    rot.close()


def test_real_data_decrypts_to_the_plaintext_weighted_sum():
    """two fresh toy ciphertexts, p_1 = 3 - 2 X^5 + X^(N/2), p_2 = 1 + 5 X^(N-1) and the addend 7 Delta written into the op: the output is the
    reference's bit for bit and decrypts to sum_t p_t m_t Delta + 7 Delta within sum_t ||p_t||_1 times the bound of one fresh error; the
    reference is held to it first"""
    from plincomb_ref import REAL_BOUND, assert_ct, decryption_error, real_reference
    LOGN, L, ELL, ALPHA = 13, 6, 5, 2
    _, toy, cts, pts, addend, ref, exact = real_reference(LOGN, L, ELL, ALPHA)
    ref_err = decryption_error(toy, ref, ELL, exact)
    print(f"reference: max |dec - exact| = {ref_err} (bound {REAL_BOUND})")
    assert REAL_BOUND == 312 and ref_err <= REAL_BOUND
    op = host.Op("config_4_N15.cfg", "hplincomb", L, ELL, ALPHA, overrides={"N": 1 << LOGN, "terms": len(cts), "pl_addend": 1})
    for t, (ct, pt) in enumerate(zip(cts, pts)):
        op.write(f"ct{t + 1}.c0", ct[0])
        op.write(f"ct{t + 1}.c1", ct[1])
        op.write(f"pt{t + 1}", pt)
    op.write("pt0", addend)
    op.execute(1)
    out = read_out(op)
    op.close()
    gpu_err = decryption_error(toy, out, ELL, exact)
    print(f"GPU: max |dec - exact| = {gpu_err} (bound {REAL_BOUND})")
    assert gpu_err <= REAL_BOUND
    assert_ct(out, ref, "real data")
