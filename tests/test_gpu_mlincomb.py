"""hmlincomb on the GPU, on both arithmetic back-ends (mont32 and chain_bits = 60), bit for bit:
 A. hm_lincomb_multi through the ABI, with both built tiles: against the oracle's MUL_CONST / ADD (tests/lincomb_ref.py's primitives) and against
    n_out calls of hm_lincomb on the same device data, on permuted and repeated input limbs with mixed and repeated moduli and a guard limb-poly; the
    worst case and all zeros; the refusals; n = 0; a captured call replayed;
 B. the op, fused (one LINCOMB_MULTI launch), unfused (one launch per stage) and with fuse_mlincomb = 0, against the reference; batch 3, graph = 1
    with batch 2, caller constants, M = 1 against hlincomb, the Paterson-Stockmeyer shape hmlincomb -> hdotadd link by link, and real data
    (tests/toy_ckks.py)."""
import ctypes as C
import types

import numpy as np
import pytest

from homulator_amd import hip, host
from oracle.homoracle import EWE_ADD, EWE_MUL_CONST, Oracle, chain_below

pytestmark = pytest.mark.gpu
CHAINS = ["mont32", "survey"]
SEED = host.SEED
NQ, NP = 6, 3
PER_MOD = 3            # input limb-polys per modulus in the kernel cases: term lists draw from them with repetition
GUARD = 0x5A5A5A5A5A5A5A5A
TILE = hip.LINCOMB_MULTI_TILE
TILES = [4, 8]
OUTS = sorted({m for t in TILES for m in (1, t - 1, t, t + 1, 16)})     # M in {1, TILE - 1, TILE, TILE + 1, 16} of both tiles
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
        ctx.set_option("lincomb_multi_tile", 0)
        pool.free()
        ctx.close()


def add_const_rows(x, ks, qs):
    out = np.empty_like(x)
    for i, (k, q) in enumerate(zip(ks, qs)):
        t = x[i] + np.uint64(k)
        out[i] = np.where(t >= np.uint64(q), t - np.uint64(q), t)
    return out


def kernel_lists(mods, T, M, moduli, rng, scale="random", const="random"):
    """per entry T input limbs of its modulus from the pool (repeats allowed), M rows of T scalars and M constants of the named kinds (const None: no
    list)"""
    n = len(mods)
    li = [mods[i] * PER_MOD + int(rng.integers(0, PER_MOD)) for i in range(n) for _ in range(T)]
    val = lambda kind, q: {"0": 0, "1": 1, "q-1": q - 1}[kind] if kind != "random" else int(rng.integers(0, q))
    s = [val(scale, moduli[mods[i]]) for i in range(n) for _ in range(M * T)]
    k = None if const is None else [val(const, moduli[mods[i]]) for i in range(n) for _ in range(M)]
    return li, s, k


def expected_rows(o, host_pool, mods, T, M, li, s, k):
    """the Python-side reference, [n * M] rows in the order of the output list: MUL_CONST per term, ADD between them (the oracle's element-wise
    primitives) on one row per (entry, output), the constants by numpy"""
    n = len(mods)
    rmods = [mods[i] for i in range(n) for _ in range(M)]
    acc = None
    for t in range(T):
        rows = np.stack([host_pool[li[i * T + t]] for i in range(n) for _ in range(M)])
        term = o.ewe(EWE_MUL_CONST, rmods, rows, k=[s[(i * M + m) * T + t] for i in range(n) for m in range(M)])
        acc = term if acc is None else o.ewe(EWE_ADD, rmods, acc, None, term)
    return acc if k is None else add_const_rows(acc, k, [o.moduli[m] for m in rmods])


def set_tile(ctx, tile):
    ctx.set_option("lincomb_multi_tile", tile)


def run_kernel_case(env, mods, T, M, seed, scale="random", const="random", integers=True):
    """one list of entries through hm_lincomb_multi with either tile: the output buffer holds n M limb-polys and one guard limb-poly, the output
    list is a random permutation; then the same from M calls of hm_lincomb on the same device data"""
    ctx, o, pool, host_pool = env
    n, N = len(mods), ctx.N
    rng = np.random.default_rng(seed)
    li, s, k = kernel_lists(mods, T, M, ctx.moduli, rng, scale, const)
    perm = [int(v) for v in rng.permutation(n * M + 1)]
    lo = perm[:n * M]
    exp = expected_rows(o, host_pool, mods, T, M, li, s, k)
    what = (n, T, M, scale, const)
    out = ctx.alloc(n * M + 1)
    got = None
    for tile in TILES:
        out.upload(np.full((n * M + 1, N), GUARD, dtype=np.uint64))
        set_tile(ctx, tile)
        ctx.lincomb_multi(pool, li, out, lo, mods, T, M, s, k)
        got = out.download()
        assert np.array_equal(got[lo], exp), (what, tile)
        assert np.all(got[perm[n * M]] == GUARD), "the guard limb-poly was written"
    set_tile(ctx, 0)
    if integers and T <= 3:   # the definition in Python integers on a stretch of some rows
        for i in sorted({0, n // 2, n - 1}):
            q = ctx.moduli[mods[i]]
            for m in sorted({0, M - 1}):
                for x in (0, 1, N - 1):
                    e = (sum(s[(i * M + m) * T + t] * int(host_pool[li[i * T + t]][x]) for t in range(T)) + (k[i * M + m] if k else 0)) % q
                    assert int(got[lo[i * M + m]][x]) == e, (what, i, m, x)
    single = ctx.alloc(n)   # M calls of hm_lincomb that differ in out, scale and addend
    for m in range(M):
        ctx.lincomb(pool, li, single, None, mods, T, [s[(i * M + m) * T + t] for i in range(n) for t in range(T)],
                    None if k is None else [k[i * M + m] for i in range(n)])
        assert np.array_equal(single.download(), got[[lo[i * M + m] for i in range(n)]]), (what, "hm_lincomb", m)
    single.free()
    out.free()


@pytest.mark.parametrize("chain", CHAINS)
@pytest.mark.parametrize("T", [1, 2, 3, 16])
@pytest.mark.parametrize("n", [1, 3, 65])
def test_kernel_entry_term_and_output_counts(envs, chain, n, T):
    """ONE launch for any n; T = 1 runs no round of the two-term loop, 2 the tail behind it, 3 one round, 16 the most; M = 1, a short tile, a full
    one, a full one and a tile of one output, 16, for both tiles; Q and P limbs, mixed and repeated moduli"""
    for M in OUTS:
        run_kernel_case(envs(13, chain), [(5 * i + 2) % (NQ + NP) for i in range(n)], T, M, 40 + 17 * n + T + 1000 * M)


@pytest.mark.parametrize("chain", CHAINS)
def test_kernel_scalars_and_constants_at_the_ends_of_the_range(envs, chain):
    """every scalar kind (0, 1, q - 1, random) with every constant kind (none, 0, q - 1, random), 5 entries, T = 3 with M = TILE + 1"""
    mods = [0, NQ + NP - 1, 3, 0, NQ]
    i = 0
    for s in ("0", "1", "q-1", "random"):
        for k in (None, "0", "q-1", "random"):
            run_kernel_case(envs(13, chain), mods, 3, TILE + 1, 7 + i, scale=s, const=k)
            i += 1


@pytest.mark.parametrize("chain", CHAINS)
def test_kernel_worst_case_and_all_zeros(envs, chain):
    """T = 16, M = 16 with every input, scalar and constant q - 1 (16 (q - 1)^2 + q - 1 in every accumulator), and with everything zero"""
    ctx, o, _, _ = envs(13, chain)
    T = M = 16
    mods = [NQ + NP - 1, 0, 2]
    n, N = len(mods), ctx.N
    src, out = ctx.alloc(n), ctx.alloc(n * M)
    li = [i for i in range(n) for _ in range(T)]
    for worst in (True, False):
        qs = [ctx.moduli[m] for m in mods]
        src.upload(np.stack([np.full(N, q - 1 if worst else 0, dtype=np.uint64) for q in qs]))
        s = [q - 1 if worst else 0 for q in qs for _ in range(M * T)]
        k = [q - 1 if worst else 0 for q in qs for _ in range(M)]
        for tile in TILES:
            out.upload(np.full((n * M, N), GUARD, dtype=np.uint64))
            set_tile(ctx, tile)
            ctx.lincomb_multi(src, li, out, None, mods, T, M, s, k)
            got = out.download()
            for i, q in enumerate(qs):
                want = (16 * (q - 1) ** 2 + q - 1) % q if worst else 0
                assert np.all(got[i * M:(i + 1) * M] == np.uint64(want)), (chain, worst, tile, i)
    set_tile(ctx, 0)
    src.free(); out.free()


@pytest.mark.parametrize("chain", CHAINS)
@pytest.mark.parametrize("logN", [15, 16])
def test_kernel_at_larger_rings(envs, chain, logN):
    run_kernel_case(envs(logN, chain), [0, NQ, 5], 3, TILE + 1, logN, integers=True)


def test_the_tile_option_takes_the_built_sizes_only():
    ctx = hip.Context(13, NQ, NP)
    for v in (0, 4, 8):
        ctx.set_option("lincomb_multi_tile", v)
    for v in (1, 2, 16):
        with pytest.raises(hip.HmError, match="hm_set_option: lincomb_multi_tile is 0 .the default tile., 4 or 8"):
            ctx.set_option("lincomb_multi_tile", v)
    ctx.close()


def _alias_call(ctx, big, out_at=40, n=2, T=2, M=2, out_lo=None):
    """n = 2 entries of 2 terms and 2 outputs in ONE allocation: the inputs are limbs 0 .. 3 through the allocation's base, the outputs n M limbs
    from `out_at` through a base pointer of their own"""
    at = lambda limb: types.SimpleNamespace(ptr=big.limb_ptr(limb))
    ctx.lincomb_multi(big, list(range(n * T)), at(out_at), out_lo, [0] * n, T, M, [1] * (n * M * T))


def test_refuses_an_output_over_an_input_or_another_output_through_another_base_pointer():
    ctx = hip.Context(13, NQ, NP)
    big = ctx.alloc(64)
    ctx.fill_uniform(big, [0] * 64, 5)
    _alias_call(ctx, big)                                   # disjoint: accepted
    for out_at in (3, 2, 0):
        with pytest.raises(hip.HmError, match=r"hm_lincomb_multi: an output limb-poly \(out\) overlaps an input limb-poly \(in\)"):
            _alias_call(ctx, big, out_at=out_at)
    with pytest.raises(hip.HmError, match="hm_lincomb_multi: two output limb-polys overlap"):     # outputs 1 and 2 of different entries
        _alias_call(ctx, big, out_lo=[0, 1, 1, 2])
    with pytest.raises(hip.HmError, match="hm_lincomb_multi: two output limb-polys overlap"):     # both outputs of entry 0
        _alias_call(ctx, big, out_lo=[5, 5, 1, 2])
    ctx.sync()
    ctx.close()


def test_refuses_bad_arguments_and_accepts_n_0():
    ctx = hip.Context(13, NQ, NP)
    src, out = ctx.alloc(4), ctx.alloc(8)
    ctx.fill_uniform(src, [0] * 4, 5)
    q0 = ctx.moduli[0]
    null = types.SimpleNamespace(ptr=None)
    what = "hm_lincomb_multi"
    with pytest.raises(hip.HmError, match=f"{what}: null buffer"):
        ctx.lincomb_multi(null, [0], out, [0], [0], 1, 1, [1])
    with pytest.raises(hip.HmError, match=f"{what}: null buffer"):
        ctx.lincomb_multi(src, [0], null, [0], [0], 1, 1, [1])
    with pytest.raises(hip.HmError, match=f"{what}: scale is null"):
        ctx.lincomb_multi(src, [0], out, [0], [0], 1, 1, None)
    with pytest.raises(hip.HmError, match=f"{what}: mod_ids is null"):
        ctx._ck(ctx.L.hm_lincomb_multi(ctx.h, src.ptr, None, out.ptr, None, None, 1, 1, 1, hip._u64([1])[1], None))
    for T in (0, 17):
        with pytest.raises(hip.HmError, match=rf"{what}: n_terms = {T}, must be in \[1, 16\]"):
            ctx.lincomb_multi(src, [0] * T, out, [0], [0], T, 1, [1] * max(T, 1))
    for M in (0, 17):
        with pytest.raises(hip.HmError, match=rf"{what}: n_out = {M}, must be in \[1, 16\]"):
            ctx.lincomb_multi(src, [0], out, [0] * M, [0], 1, M, [1] * max(M, 1))
    with pytest.raises(hip.HmError, match="65535"):
        ctx.lincomb_multi(src, [0, 70000], out, [0], [0], 2, 1, [1, 1])
    with pytest.raises(hip.HmError, match="65535"):
        ctx.lincomb_multi(src, [0, 1], out, [0, 70000], [0], 2, 2, [1] * 4)
    with pytest.raises(hip.HmError, match="mod id"):
        ctx.lincomb_multi(src, [0], out, [0], [NQ + NP], 1, 1, [1])
    with pytest.raises(hip.HmError, match=r"scale\[1\]\[2\] is not reduced"):        # entry 1, output 1, term 0 of [n][n_out][n_terms]
        ctx.lincomb_multi(src, [0, 1, 2, 3], out, [0, 1, 2, 3], [0, 0], 2, 2, [1, 0, 1, 1, 1, 1, q0, 1])
    with pytest.raises(hip.HmError, match=r"addend\[1\]\[1\] is not reduced"):
        ctx.lincomb_multi(src, [0, 1], out, [0, 1, 2, 3], [0, 0], 1, 2, [1] * 4, [0, 0, 0, q0])
    with pytest.raises(hip.HmError, match="too many for one call"):                # a record table beyond 2^32 words; refused before any list is read
        ctx._ck(ctx.L.hm_lincomb_multi(ctx.h, src.ptr, None, out.ptr, None, hip._u32([0])[1], 1 << 24, 16, 16, hip._u64([1])[1], None))
    with pytest.raises(hip.HmError, match="two output limb-polys overlap"):
        ctx.lincomb_multi(src, [0, 1], out, [2, 3, 4, 2], [0, 0], 1, 2, [1] * 4)
    with pytest.raises(hip.HmError, match="overlaps an input"):
        ctx.lincomb_multi(src, [0, 1], src, [3, 1], [0, 0], 1, 1, [1, 1])
    keep = [hip._u32([0]), hip._u64([1, 1, 1])]
    ctx._ck(ctx.L.hm_lincomb_multi(ctx.h, src.ptr, None, out.ptr, None, keep[0][1], 0, 3, 1, keep[1][1], None))   # n = 0: nothing to do
    ctx.lincomb_multi(src, [0, 1, 1, 0], out, [3, 0, 7, 5], [0, 0], 2, 2, [0, q0 - 1, 1, 0, 0, 0, 1, 1], [0, q0 - 1, 0, 1])   # nothing wrong: accepted
    ctx.sync()
    ctx.close()


@pytest.mark.parametrize("chain", CHAINS)
def test_a_captured_call_replays(envs, chain):
    """the records live in a cached device table: after one warm run the call is captured into a graph and replayed on new input data"""
    ctx, o, _, _ = envs(13, chain)
    ctx.L.hm_graph_launch.argtypes = [C.c_void_p, C.c_void_p]
    ctx.L.hm_graph_destroy.argtypes = [C.c_void_p]
    T, M = 3, TILE + 1
    mods = [(3 * i + 1) % (NQ + NP) for i in range(20)]
    fill_mods = [m for m in range(NQ + NP) for _ in range(PER_MOD)]
    rng = np.random.default_rng(3)
    li, s, k = kernel_lists(mods, T, M, ctx.moduli, rng)
    src, out = ctx.alloc(len(fill_mods)), ctx.alloc(len(mods) * M)
    run = lambda: ctx.lincomb_multi(src, li, out, None, mods, T, M, s, k)
    ctx.fill_uniform(src, fill_mods, 1)
    run()
    g = C.c_void_p()
    ctx._ck(ctx.L.hm_capture_begin(ctx.h))
    run()
    ctx._ck(ctx.L.hm_capture_end(ctx.h, C.byref(g)))
    ctx.fill_uniform(src, fill_mods, 2)
    out.upload(np.full((len(mods) * M, ctx.N), GUARD, dtype=np.uint64))
    ctx._ck(ctx.L.hm_graph_launch(ctx.h, g))
    ctx.sync()
    assert np.array_equal(out.download(), expected_rows(o, src.download(), mods, T, M, li, s, k)), chain
    ctx.L.hm_graph_destroy(g)
    src.free(); out.free()


# ============================================================================================================================
# B. the op
# ============================================================================================================================
def read_out(op, m=None, copy=0):
    name = "out" if m is None else f"out{m}"
    return op.read(f"{name}.c0", copy=copy), op.read(f"{name}.c1", copy=copy)


def read_all(op, M, copy=0):
    return [read_out(op, m, copy) for m in range(1, M + 1)]


SHAPES = [
    ("config_4_N15.cfg", 13, 13, 7, 3, 1),
    ("config_4_N15.cfg", 13, 13, 13, 13, 1),
    ("config_4_N15.cfg", 15, 16, 10, 4, 3),
]
KEYS = [(1, 1, 0, 0), (3, 2, 1, 1), (4, 5, 1, 0), (4, 5, 0, 1)]     # (terms, outputs, ml_const, rescale): every (T, M), both values of either key
_ref = {}


def reference(chain, logN, L, ell, alpha, keys, copy=0, seed=SEED):
    """the reference outputs on the op's synthetic inputs, computed once per case"""
    from mlincomb_ref import mlincomb, synthetic_constants, synthetic_inputs
    key = (chain, logN, L, ell, alpha, keys, copy, seed)
    if key not in _ref:
        T, M, mc, rs = keys
        o = oracle(logN, L, alpha, chain, threads=16)
        _ref[key] = mlincomb(o, ell, synthetic_inputs(o, ell, seed, T, copy=copy), *synthetic_constants(o, ell, seed, T, M, mc), rescale=bool(rs))
    return _ref[key]


@pytest.mark.parametrize("chain", CHAINS)
@pytest.mark.parametrize("keys", KEYS)
@pytest.mark.parametrize("cfg,logN,L,ell,alpha,batch", SHAPES)
def test_op_fused_unfused_and_reference_agree(chain, keys, cfg, logN, L, ell, alpha, batch):
    """fused, unfused and fuse_mlincomb = 0 against the reference; batch 3 (last shape): every copy, under the same constants"""
    from mlincomb_ref import assert_outputs
    T, M, mc, rs = keys
    ov = chain_ov(chain, {"terms": T, "outputs": M, "ml_const": mc, "rescale": rs, "batch": batch, "N": 1 << logN})
    for mode, fuse, extra in (("fused", True, {}), ("unfused", False, {}), ("fuse_mlincomb = 0", True, {"fuse_mlincomb": 0})):
        op = host.Op(cfg, "hmlincomb", L, ell, alpha, fuse=fuse, overrides=dict(ov, **extra))
        op.execute(1)
        kinds = [ln.split()[0] for ln in op.plan()]
        assert kinds.count("LINCOMB_MULTI") == (1 if mode == "fused" and M > 1 else 0), (mode, kinds)
        assert kinds.count("LINCOMB") == (1 if mode == "fuse_mlincomb = 0" or (mode == "fused" and M == 1) else 0), (mode, kinds)
        for c in range(batch):
            got = read_all(op, M, c)
            assert got[0][0].shape[0] == ell - rs
            assert_outputs(got, reference(chain, logN, L, ell, alpha, keys, copy=c), (mode, keys, c))
        first = read_out(op)                                   # "out" names out1
        assert np.array_equal(first[0], op.read("out1.c0")) and np.array_equal(first[1], op.read("out1.c1"))
        op.close()


def test_graph_replay_with_a_batch():
    """graph = 1: run 1 direct, run 2 captures, run 3 replays; both copies after the replay"""
    from mlincomb_ref import assert_outputs
    cfg, logN, L, ell, alpha, _ = SHAPES[2]
    keys, batch = (3, 2, 1, 1), 2
    op = host.Op(cfg, "hmlincomb", L, ell, alpha, overrides={"terms": 3, "outputs": 2, "ml_const": 1, "rescale": 1, "batch": batch, "graph": 1})
    lc = [ln for ln in op.plan() if ln.startswith("LINCOMB_MULTI")]
    assert len(lc) == 1 and " terms=3 out=2 const=1" in lc[0]
    for _ in range(3):
        op.execute(1)
    for c in range(batch):
        assert_outputs(read_all(op, 2, c), reference("mont32", logN, L, ell, alpha, keys, copy=c), f"copy {c}")
    op.close()


@pytest.mark.parametrize("chain", CHAINS)
@pytest.mark.parametrize("fuse", [True, False])
def test_caller_constants(chain, fuse):
    from mlincomb_ref import assert_outputs, mlincomb, synthetic_inputs
    L, ell, alpha, T, M = 6, 5, 2, 3, 2
    o = oracle(13, L, alpha, chain)
    scales = [[[2, o.moduli[1] - 1, 1, 12345, o.moduli[4] // 2], [0] * ell, [o.moduli[j] - 3 for j in range(ell)]],
              [[0] * ell, [0] * ell, [0] * ell]]                                  # a zero row: output 2 is its constant alone
    consts = [[(7 << 40) % o.moduli[j] for j in range(ell)], [o.moduli[j] - 1 for j in range(ell)]]
    op = host.Op("config_4_N15.cfg", "hmlincomb", L, ell, alpha, fuse=fuse,
                 overrides=chain_ov(chain, {"terms": T, "outputs": M, "ml_const": 1, "N": 1 << 13}))
    for m in range(M):
        for t in range(T):
            op.set_constants(f"scale{m + 1}_{t + 1}", scales[m][t])
        op.set_constants(f"const{m + 1}", consts[m])
    op.execute(1)
    got = read_all(op, M)
    assert_outputs(got, mlincomb(o, ell, synthetic_inputs(o, ell, SEED, T), scales, consts), ("caller constants", chain, fuse))
    for j in range(ell):
        assert np.all(got[1][0][j] == np.uint64(consts[1][j])) and np.all(got[1][1][j] == 0)
    with pytest.raises(host.HostError, match=r'hmlincomb: set_constants\("scale2_1"\) after prepare'):
        op.set_constants("scale2_1", scales[1][0])
    op.close()


@pytest.mark.parametrize("chain", CHAINS)
def test_one_output_is_hlincomb_bit_for_bit(chain):
    """M = 1 with hlincomb's constants written into it, against the hlincomb op itself"""
    from lincomb_ref import synthetic_constants
    L, ell, alpha, T = 6, 5, 2, 4
    o = oracle(13, L, alpha, chain)
    scales, const = synthetic_constants(o, ell, SEED, T, 1)
    a = host.Op("config_4_N15.cfg", "hlincomb", L, ell, alpha, overrides=chain_ov(chain, {"terms": T, "lc_const": 1, "N": 1 << 13}))
    b = host.Op("config_4_N15.cfg", "hmlincomb", L, ell, alpha, overrides=chain_ov(chain, {"terms": T, "outputs": 1, "ml_const": 1, "N": 1 << 13}))
    for t in range(T):
        b.set_constants(f"scale1_{t + 1}", scales[t])
    b.set_constants("const1", const)
    a.execute(1); b.execute(1)
    for k in range(2):
        assert np.array_equal(a.read(f"out.c{k}"), b.read(f"out1.c{k}")), (chain, k)
    a.close(); b.close()


def test_paterson_stockmeyer_shape_link_by_link():
    """p = q_1(x) G_1 G_1' + q_2(x) G_2 G_2' + r(x) in two ops: hmlincomb (T = 3, M = 3, ml_const = 1) forms q_1, q_2 and r from three baby powers;
    hdotadd (terms = 2, addends = 1) takes out1 as ct1, out2 as ct3 and out3 as its addend ct5, with synthetic giant powers ct2 and ct4.  Both ops
    against their references link by link"""
    import dotadd_ref
    from mlincomb_ref import assert_outputs, mlincomb, synthetic_constants, synthetic_inputs
    L, ell, alpha = 6, 5, 2
    o = oracle(13, L, alpha)
    src = host.Op("config_4_N15.cfg", "hmlincomb", L, ell, alpha, overrides={"N": 1 << 13, "terms": 3, "outputs": 3, "ml_const": 1})
    src.execute(1)
    blocks = mlincomb(o, ell, synthetic_inputs(o, ell, SEED, 3), *synthetic_constants(o, ell, SEED, 3, 3, 1))
    assert_outputs(read_all(src, 3), blocks, "link 0")
    seed = SEED + 31
    for fuse in (True, False):
        op = host.Op("config_4_N15.cfg", "hdotadd", L, ell, alpha, fuse=fuse,
                     overrides={"N": 1 << 13, "terms": 2, "addends": 1, "da_scale": 1, "da_const": 1, "seed": seed})
        for name, output in (("ct1", "out1"), ("ct3", "out2"), ("ct5", "out3")):
            op.bind_input(name, src, output=output)
        op.execute(1)
        pairs, addends, evk = dotadd_ref.synthetic_inputs(o, ell, seed, 2, 1)
        pairs = [(np.stack(blocks[0]), pairs[0][1]), (np.stack(blocks[1]), pairs[1][1])]
        want = dotadd_ref.dotadd(o, ell, pairs, evk, [np.stack(blocks[2])], *dotadd_ref.synthetic_constants(o, ell, seed, 2, 1, 1, 1))
        dotadd_ref.assert_ct(read_out(op), want, ("link 1", fuse))
        op.close()
    wrong = host.Op("config_4_N15.cfg", "hdotadd", L, ell - 1, alpha, overrides={"N": 1 << 13, "terms": 2, "addends": 1})
    with pytest.raises(host.HostError, match="levels differ"):
        wrong.bind_input("ct1", src, output="out2")
    wrong.close()
    src.close()


def test_real_data_decrypts_to_the_linear_combinations():
    """three fresh toy ciphertexts, two rows of small signed scalars and the constants 7 Delta written into the op: every output is the reference's
    bit for bit and decrypts to sum_t s_{m,t} m_t Delta + 7 Delta within sum_t |s_{m,t}| times the bound of one fresh error (156 and 286); the
    reference is held to the bounds first"""
    from mlincomb_ref import REAL_ROWS, assert_outputs, decryption_errors, mlincomb, real_bounds, real_case
    from toy_ckks import Toy
    LOGN, L, ELL, ALPHA = 13, 6, 5, 2
    o = oracle(LOGN, L, ALPHA)
    toy = Toy(o, seed=4249)
    cts, scales, consts, exact = real_case(toy, ELL)
    ref = mlincomb(o, ELL, cts, scales, consts)
    bounds = real_bounds()
    ref_errs = decryption_errors(toy, ref, ELL, exact)
    print(f"reference: max |dec - exact| per output = {ref_errs} (bounds {bounds})")
    assert bounds == [156, 286] and all(e <= b for e, b in zip(ref_errs, bounds))
    T, M = len(REAL_ROWS[0]), len(REAL_ROWS)
    op = host.Op("config_4_N15.cfg", "hmlincomb", L, ELL, ALPHA, overrides={"N": 1 << LOGN, "terms": T, "outputs": M, "ml_const": 1})
    for m in range(M):                          # (the constants first: writing a buffer prepares the op)
        for t in range(T):
            op.set_constants(f"scale{m + 1}_{t + 1}", scales[m][t])
        op.set_constants(f"const{m + 1}", consts[m])
    for t, ct in enumerate(cts):
        op.write(f"ct{t + 1}.c0", ct[0])
        op.write(f"ct{t + 1}.c1", ct[1])
    op.execute(1)
    out = read_all(op, M)
    op.close()
    gpu_errs = decryption_errors(toy, out, ELL, exact)
    print(f"GPU: max |dec - exact| per output = {gpu_errs} (bounds {bounds})")
    assert all(e <= b for e, b in zip(gpu_errs, bounds))
    assert_outputs(out, ref, "real data")
