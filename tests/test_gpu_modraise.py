"""ModRaise on the GPU, on both arithmetic back-ends, bit for bit:
 A. hm_ntt_lift against tests/modraise_ref.py (the centring with integers, then the oracle's transform): permuted limb lists, several entries that
    read one source, a guard limb-poly behind the output, the five fills, every form of the transform (16-coefficient and 8-coefficient two-kernel
    forms, the one-launch form), a mixed-width chain on the generic back-end, more entries than one group of workgroups, one captured call replayed,
    and the refusals;
 B. the op hmodraise, fused and unfused, with raise_to, as a batch, with graph = 1, and as the first link of a chain;
 C. on real data (tests/toy_ckks.py) the raised ciphertext decrypts to the input's plaintext plus a small multiple of q_0."""
import ctypes as C
import types

import numpy as np
import pytest

import modraise_ref as mr
from homulator_amd import host
from oracle.homoracle import Oracle, chain_below

pytestmark = pytest.mark.gpu
CHAINS = ["mont32", "survey"]
SEED = host.SEED
BATCH_SEED_STRIDE = 100000   # host/src/Arch.cpp kBatchSeedStride
NQ, NP = 6, 3
GUARD = 0x5A5A5A5A5A5A5A5A
FILLS = ["uniform", "zero", "qs-1", "half", "half+1"]
_oracles = {}


def oracle(logN, L, K, chain="mont32", threads=16):
    key = (logN, L, K, chain if isinstance(chain, str) else tuple(chain))
    if key not in _oracles:
        _oracles[key] = Oracle(logN, L, K, chain=chain)
    _oracles[key].set_threads(threads)
    return _oracles[key]


def make_context(logN, chain):
    from homulator_amd import hip
    if chain == "mont32":
        return hip.Context(logN, NQ, NP)
    mods = chain_below(logN, 60, NQ + NP) if chain == "survey" else list(chain)
    return hip.Context(logN, NQ, NP, q=mods[:NQ], p=mods[NQ:])


# ============================================================================================================================
# A. the kernel
# ============================================================================================================================
@pytest.fixture(scope="module")
def envs():
    """(hip context, oracle on the same moduli) per (logN, chain), made on first use"""
    made = {}

    def get(logN, chain):
        key = (logN, chain if isinstance(chain, str) else tuple(chain))
        if key not in made:
            ctx, o = make_context(logN, chain), oracle(logN, NQ, NP, chain)
            assert ctx.moduli == o.moduli
            made[key] = (ctx, o)
        return made[key]
    yield get
    for ctx, _ in made.values():
        ctx.close()


def source_rows(o, rng, src_mods, fill):
    rows = []
    for m in src_mods:
        qs = o.moduli[m]
        if fill == "uniform":
            r = rng.integers(0, qs, o.N, dtype=np.uint64)
            r[:5] = [0, (qs - 1) // 2, (qs + 1) // 2, qs - 1, 1]
        else:
            r = np.full(o.N, {"zero": 0, "qs-1": qs - 1, "half": (qs - 1) // 2, "half+1": (qs + 1) // 2}[fill], dtype=np.uint64)
        rows.append(r)
    return np.stack(rows)


def lift_case(ctx, o, src_mods, entries, seed, fill="uniform", replay=False):
    """one hm_ntt_lift call.  src_mods: the modulus of every source limb-poly; entries: (source index, target modulus) per output limb-poly.  The
    sources sit at permuted limbs of their buffer, the outputs at permuted limbs of a buffer with one limb-poly more, which must keep its fill"""
    rng = np.random.default_rng(seed)
    ns, n, N = len(src_mods), len(entries), ctx.N
    rows = source_rows(o, rng, src_mods, fill)
    sl = [int(v) for v in rng.permutation(ns)]
    stored = np.empty_like(rows)
    stored[sl] = rows
    src = ctx.from_host(stored)
    out = ctx.alloc(n + 1)
    out.upload(np.full((n + 1, N), GUARD, dtype=np.uint64))
    perm = [int(v) for v in rng.permutation(n + 1)]
    ol, guard = perm[:n], perm[n]
    mods = [m for _, m in entries]
    call = lambda: ctx.ntt_lift(src, out, mods, [src_mods[s] for s, _ in entries], in_limbs=[sl[s] for s, _ in entries], out_limbs=ol)
    call()
    if replay:   # the launch table is cached now: capture the same call and replay it onto a cleared output
        out.upload(np.full((n + 1, N), GUARD, dtype=np.uint64))
        g = C.c_void_p()
        ctx._ck(ctx.L.hm_capture_begin(ctx.h))
        call()
        ctx._ck(ctx.L.hm_capture_end(ctx.h, C.byref(g)))
        assert np.all(out.download() == GUARD)      # captured, not run
        ctx._ck(ctx.L.hm_graph_launch(ctx.h, g))
        ctx.sync()
        ctx.L.hm_graph_destroy(g)
    got = out.download()
    assert np.array_equal(src.download(), stored), "a source was written"
    for s in range(ns):   # the reference once per source, for all of its targets
        idx = [i for i, (si, _) in enumerate(entries) if si == s]
        if not idx:
            continue
        exp = mr.lift(o, src_mods[s], [mods[i] for i in idx], rows[s])
        for e, i in zip(exp, idx):
            assert np.array_equal(got[ol[i]], e), (src_mods, entries[i], fill, "entry", i)
            if src_mods[s] == mods[i]:   # the identity lift is the plain transform of the stored coefficients
                assert np.array_equal(e, o.ntt([mods[i]], rows[s][None, :])[0])
    assert np.all(got[guard] == GUARD), "the guard limb-poly was written"
    src.free()
    out.free()


def raise_entries(n_src, T, extra=()):
    """every source into moduli 0 .. T-1 (ModRaise's own shape), then further (source, modulus) pairs"""
    return [(s, j) for s in range(n_src) for j in range(T)] + list(extra)


@pytest.mark.parametrize("chain", CHAINS)
def test_smallest_ring_eight_and_nine_entries(envs, chain):
    """N = 2^13: 8 entries fill one group of eight, 9 leave seven empty slots; sources of a Q modulus and of a special modulus (target above, below, equal)"""
    ctx, o = envs(13, chain)
    lift_case(ctx, o, [0, NQ + NP - 1], raise_entries(2, 4), 1)
    lift_case(ctx, o, [0, NQ + NP - 1], raise_entries(2, 4, [(1, NQ + NP - 1)]), 2)
    lift_case(ctx, o, [3], [(0, 3)], 3)                          # one entry, source = target
    lift_case(ctx, o, [5, 1, 2], [(2, 0), (0, 7), (1, 1), (0, 5), (2, 2), (1, 8)], 4)


@pytest.mark.parametrize("chain", CHAINS)
@pytest.mark.parametrize("fill", FILLS[1:])
def test_constant_fills_at_the_ends_and_the_centring_boundary(envs, chain, fill):
    ctx, o = envs(13, chain)
    lift_case(ctx, o, [0, NQ + NP - 1, 3], raise_entries(3, 3, [(0, NQ + NP - 1), (1, NQ)]), 5, fill=fill)


@pytest.mark.parametrize("chain", CHAINS)
@pytest.mark.parametrize("logN", [16, 15])
@pytest.mark.parametrize("form", ["one-launch", "two-kernel-8", "two-kernel-16"])
def test_every_form_of_the_transform(chain, logN, form):
    """once per geometry, forced with the existing options: the one-launch form (default), the 8-coefficient two-kernel form (ntt_fused_small = 0)
    and the 16-coefficient one (ntt_small_limbs = 0 as well): the lifted form has all three on both back-ends"""
    o = oracle(logN, NQ, NP, chain)
    ctx = make_context(logN, chain)   # its own: the options stay with it
    try:
        assert ctx.moduli == o.moduli
        if form != "one-launch":
            ctx.set_option("ntt_fused_small", 0)
        if form == "two-kernel-16":
            ctx.set_option("ntt_small_limbs", 0)
        lift_case(ctx, o, [0, NQ], raise_entries(2, 3, [(1, NQ)]), logN)
        lift_case(ctx, o, [2], [(0, 1), (0, 2)], logN + 1, fill="half+1")
    finally:
        ctx.close()


def test_mixed_width_chain_on_the_generic_back_end(envs):
    """a chain of a 60-bit, a 21-bit and 36-bit moduli: 60 -> 21 bits and back, the 36-bit pairs, every fill"""
    logN = 13
    chain = chain_below(logN, 60, 2) + chain_below(logN, 21, 1) + chain_below(logN, 36, NQ + NP - 3)
    ctx, o = envs(logN, chain)
    pairs = [(s, m) for s in range(4) for m in (0, 2, 3, 4)]
    for i, fill in enumerate(FILLS):
        lift_case(ctx, o, [0, 2, 3, 4], pairs, 40 + i, fill=fill)


def test_more_entries_than_one_group_of_workgroups(envs):
    """two sources into 35 moduli each with repeated moduli: 70 limb-polys, above the one-launch form's limit at N = 2^16, several same-modulus groups"""
    ctx, o = envs(13, "mont32")
    lift_case(ctx, o, [0, 4], [(i % 2, (i // 2) % (NQ + NP)) for i in range(70)], 70)


@pytest.mark.parametrize("chain", CHAINS)
def test_a_captured_call_replays(envs, chain):
    ctx, o = envs(15, chain)
    lift_case(ctx, o, [0, 1], raise_entries(2, 5), 31, replay=True)


def test_refusals():
    from homulator_amd import hip
    ctx = hip.Context(13, NQ, NP)
    big = ctx.alloc(8)
    ctx.fill_uniform(big, [0] * 8, 5)
    at = lambda limb: types.SimpleNamespace(ptr=big.limb_ptr(limb))
    mods, two = [0, 1], [0, 1]
    call = lambda out=4, src_mods=(0, 0), mod_ids=mods, **kw: ctx.ntt_lift(big, at(out), mod_ids, list(src_mods), in_limbs=[0, 0], out_limbs=two, **kw)
    call()                                                       # in: limb 0 twice; out: limbs 4, 5
    with pytest.raises(hip.HmError, match="hm_ntt_lift.*overlaps the input"):
        ctx.ntt_lift(big, at(1), mods, [0, 0], in_limbs=[2, 2], out_limbs=two)      # out[1] is the source, through another base pointer
    with pytest.raises(hip.HmError, match="hm_ntt_lift.*overlaps the input"):
        ctx.ntt_lift(big, big, mods, [0, 0], in_limbs=[0, 0], out_limbs=two)        # in place
    for kw, what in (({"inverse": 1}, "forward"), ({"second_pass_only": 1}, "second_pass_only"), ({"in_galois": [5, 5]}, "in_galois"),
                     ({"scale": [3, 4]}, "scale"), ({"out_packed": [1, 0]}, "out_packed")):
        with pytest.raises(hip.HmError, match="hm_ntt_lift.*" + what):
            call(**kw)
    with pytest.raises(hip.HmError, match="hm_ntt_lift: mod id"):
        call(src_mods=(0, NQ + NP))
    with pytest.raises(hip.HmError, match="hm_ntt_lift: mod id"):
        call(mod_ids=[NQ + NP, 0])
    call()                                                       # the context is as usable as before
    ctx.close()


# ============================================================================================================================
# B. the op
# ============================================================================================================================
ROWS = [("config_4_N15.cfg", 13, 6, 1, 1), ("config_4_N15.cfg", 15, 16, 1, 4), ("config_4.cfg", 16, 45, 1, 15)]


def read_out(op, copy=0):
    return op.read("out.c0", copy=copy), op.read("out.c1", copy=copy)


def assert_ct(got, exp, what):
    assert got[0].shape == exp[0].shape, (what, got[0].shape, exp[0].shape)
    assert np.array_equal(got[0], exp[0]), (what, "c0")
    assert np.array_equal(got[1], exp[1]), (what, "c1")


def reference(o, T, seed=SEED, copy=0):
    return mr.modraise_ct(o, T, o.synth_ct(1, seed + copy * BATCH_SEED_STRIDE))


def run_op(cfg, L, alpha, ov, fuse=True, runs=1, copies=1):
    op = host.Op(cfg, "hmodraise", L, 1, alpha, fuse=fuse, overrides=ov)
    try:
        for _ in range(runs):
            op.execute(1)
        return [read_out(op, c) for c in range(copies)], op.plan(), op.output_level()
    finally:
        op.close()


def overrides(chain, logN, **extra):
    return dict({"N": 1 << logN}, **(dict(extra, chain_bits=60) if chain != "mont32" else extra))


@pytest.mark.parametrize("chain", CHAINS)
@pytest.mark.parametrize("cfg,logN,L,ell,alpha", ROWS)
def test_op_fused_unfused_and_reference_agree(chain, cfg, logN, L, ell, alpha):
    o = oracle(logN, L, alpha, chain)
    exp = reference(o, L)
    for fuse in (True, False):
        got, plan, level = run_op(cfg, L, alpha, overrides(chain, logN), fuse=fuse)
        assert level == L and len(plan) == 2 and "lift=1" in plan[1], plan
        assert_ct(got[0], exp, ("fused" if fuse else "unfused", chain))
    src = o.synth_ct(1, SEED)
    assert np.array_equal(got[0][0][0], src[0][0]) and np.array_equal(got[0][1][0], src[1][0]), "limb 0 is the input, bit for bit"


@pytest.mark.parametrize("chain", CHAINS)
def test_raise_to_below_the_top(chain):
    cfg, logN, L, _, alpha = ROWS[1]
    o = oracle(logN, L, alpha, chain)
    for T in (2, 9):
        got, _, level = run_op(cfg, L, alpha, overrides(chain, logN, raise_to=T))
        assert level == T
        assert_ct(got[0], reference(o, T), ("raise_to", T))


def test_batch_of_three():
    cfg, logN, L, _, alpha = ROWS[1]
    o = oracle(logN, L, alpha)
    got, plan, _ = run_op(cfg, L, alpha, overrides("mont32", logN, batch=3), copies=3)
    assert len(plan) == 2
    for c in range(3):
        assert_ct(got[c], reference(o, L, copy=c), ("copy", c))


def test_graph_replay():
    """run 1 direct, run 2 captures, run 3 replays"""
    cfg, logN, L, _, alpha = ROWS[1]
    o = oracle(logN, L, alpha)
    got, _, _ = run_op(cfg, L, alpha, overrides("mont32", logN, graph=1), runs=3)
    assert_ct(got[0], reference(o, L), "graph")


def test_chain_hmodraise_hrotate():
    """link k runs under seed + 31 k (OpChain): hrotate's keys are drawn from there, its operand is hmodraise's output at level T"""
    L, alpha, T = 6, 2, 5
    o = oracle(15, L, alpha)
    chain = host.Chain("config_4_N15.cfg", "hmodraise,hrotate", L, 1, alpha, overrides={"raise_to": T})
    chain.execute(1)
    a = reference(o, T)
    b = o.hrotate(T, np.stack(a), 5, o.synth_evk(T, SEED + 31 + 10000))
    assert chain[0].output_level() == T and chain[1].output_level() == T
    assert_ct(read_out(chain[0]), a, "hmodraise")
    assert_ct(read_out(chain[1]), (b[0], b[1]), "hrotate")
    chain.close()


# ============================================================================================================================
# C. real data
# ============================================================================================================================
def test_real_data_decrypts_to_the_input_plus_a_small_multiple_of_q0():
    """Encrypt at level 1, raise, decrypt at level T.  Dec_T(out) is the INTEGER polynomial c0' + c1' s with every coefficient of c0', c1' at most
    q_0 / 2 in magnitude, so it is at most (q_0 / 2)(1 + ||s||_1), far below Q_T / 2: no wrap.  Dec_1(in) is its centred residue mod q_0, at most
    q_0 / 2.  So D = Dec_T(out) - Dec_1(in) is divisible by q_0 in every coefficient and |D / q_0| <= (1 + ||s||_1) / 2 + 1 / 2 = 1 + ||s||_1 / 2:
    a derived bound, computed from the toy key."""
    from toy_ckks import Toy
    LOGN, L, ALPHA = 13, 6, 2
    o = oracle(LOGN, L, ALPHA)
    toy = Toy(o, seed=4244)
    s1 = int(sum(abs(int(v)) for v in toy.s))
    q0 = o.moduli[0]
    m = toy.rng.integers(-1000, 1000, o.N).astype(object) * (1 << 30)
    ct = toy.encrypt(m, 1)
    d_in, Q1 = toy.decrypt(ct, 1)
    assert Q1 == q0
    for T in (L, 3):
        h = host.Op("config_4_N15.cfg", "hmodraise", L, 1, ALPHA, overrides={"N": 1 << LOGN, "raise_to": T})
        h.write("ct1.c0", ct[0])
        h.write("ct1.c1", ct[1])
        h.execute(1)
        out = np.stack(read_out(h))
        h.close()
        assert out.shape == (2, T, o.N)
        d_out, QT = toy.decrypt(out, T)
        assert q0 * (1 + s1) < QT, "the bound needs room below Q_T / 2"
        worst = 0
        for a, b in zip(d_out, d_in):
            D = int(a) - int(b)
            assert D % q0 == 0
            worst = max(worst, abs(D // q0))
        print(f"T = {T}: max |Dec_T(out) - Dec_1(in)| / q_0 = {worst} (bound 1 + ||s||_1 / 2 = {1 + s1 / 2})")
        assert 2 * worst <= 2 + s1
