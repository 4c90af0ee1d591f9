"""hreim on the GPU, on both arithmetic back-ends (mont32 and chain_bits = 60), bit for bit:
 A. hm_reim_split through the ABI: against the oracle's ADD / SUB / MUL by U = NTT(-X^(N/2)) (tests/reim_ref.py's primitives) and against ADD, SUB
    and MUL through hm_ewe with an uploaded U on the same device data, on permuted and repeated input limbs with mixed moduli and a guard
    limb-poly; at N = 2^15 and 2^16, where the half boundary lies elsewhere; the refusals; n = 0; a captured call replayed;
 B. the op, fused (hrotate's launches and one REIM launch), unfused (one launch per stage) and with fuse_reim = 0, against the reference; the stored
    unit; batch 2 and graph = 1; the 2 ct1 identity and out = hrotate's output + ct1 on device output; a chain hreim,hsquare link by link; an
    hsquare bound to out_im; and real data (tests/toy_ckks.py)."""
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
PER_MOD = 3            # input limb-polys per modulus in the kernel cases: the records draw from them with repetition
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
    """(hip context, oracle on the same moduli, two input pools on the device and on the host, the oracle's U per modulus) per (logN, chain), made
    on first use.  A pool holds PER_MOD limb-polys per modulus, limb m * PER_MOD + r filled for modulus m; neither is written again"""
    from homulator_amd import hip
    from reim_ref import unit
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
            fill = [m for m in range(NQ + NP) for _ in range(PER_MOD)]
            px, py = ctx.alloc(len(fill)), ctx.alloc(len(fill))
            ctx.fill_uniform(px, fill, 700 + logN)
            ctx.fill_uniform(py, fill, 800 + logN)
            made[(logN, chain)] = (ctx, o, px, py, px.download(), py.download(), unit(o, list(range(NQ + NP))))
        return made[(logN, chain)]
    yield get
    for ctx, _, px, py, *_ in made.values():
        px.free(); py.free()
        ctx.close()


def expected_rows(o, hx, hy, U, mods, lx, ly):
    from reim_ref import split
    n = len(mods)
    x, y = np.stack([hx[lx[i]] for i in range(n)]), np.stack([hy[ly[i]] for i in range(n)])
    re, im = split(o, mods, x, y)
    assert np.array_equal(im, o.ewe(EWE_MUL, mods, o.ewe(4, mods, x, None, y), np.stack([U[m] for m in mods])))
    return re, im


def run_kernel_case(env, mods, seed, composed=True):
    """one hm_reim_split call: the two outputs share ONE buffer of 2n limb-polys and one guard limb-poly, at a random permutation"""
    from homulator_amd import hip
    from reim_ref import split_integers
    ctx, o, px, py, hx, hy, U = env
    n, N = len(mods), ctx.N
    rng = np.random.default_rng(seed)
    lx = [mods[i] * PER_MOD + int(rng.integers(0, PER_MOD)) for i in range(n)]
    ly = [mods[i] * PER_MOD + int(rng.integers(0, PER_MOD)) for i in range(n)]
    perm = [int(v) for v in rng.permutation(2 * n + 1)]
    lre, lim = perm[:n], perm[n:2 * n]
    out = ctx.alloc(2 * n + 1)
    out.upload(np.full((2 * n + 1, N), GUARD, dtype=np.uint64))
    ctx.reim_split(px, py, out, out, mods, limbs=[lx, ly, lre, lim])
    got = out.download()
    re, im = expected_rows(o, hx, hy, U, mods, lx, ly)
    assert np.array_equal(got[lre], re), (n, "re")
    assert np.array_equal(got[lim], im), (n, "im")
    assert np.all(got[perm[2 * n]] == GUARD), "the guard limb-poly was written"
    h = N // 2
    cols = [0, 1, 511, 512, h - 513, h - 512, h - 1, h, h + 511, h + 512, N - 1]     # either side of N/2, chunk by chunk
    for i in sorted({0, n // 2, n - 1}):       # the definition in Python integers on some records
        e_re, e_im = split_integers(o, mods[i], hx[lx[i]], hy[ly[i]], cols)
        assert [int(got[lre[i]][c]) for c in cols] == e_re and [int(got[lim[i]][c]) for c in cols] == e_im, (n, i)
    if composed:   # the same from the calls it replaces, on the same device data, with an uploaded U
        u, s, d, p = ctx.alloc(n), ctx.alloc(n), ctx.alloc(n), ctx.alloc(n)
        u.upload(np.stack([U[m] for m in mods]))
        ctx.ewe(hip.OP_ADD, s, mods, a=px, la=lx, c=py, lc=ly)
        ctx.ewe(hip.OP_SUB, d, mods, a=px, la=lx, c=py, lc=ly)
        ctx.ewe(hip.OP_MUL, p, mods, a=d, b=u)
        assert np.array_equal(s.download(), got[lre]) and np.array_equal(p.download(), got[lim]), (n, "composed")
        for b in (u, s, d, p):
            b.free()
    out.free()


@pytest.mark.parametrize("chain", CHAINS)
@pytest.mark.parametrize("n", [1, 3, 65, 130])
def test_kernel_entry_counts(envs, chain, n):
    """ONE launch for any n (across the 64- and 128-entry cuts of the launches whose records travel as kernel arguments); Q and P limbs, mixed
    moduli, repeated input limbs"""
    run_kernel_case(envs(13, chain), [(5 * i + 2) % (NQ + NP) for i in range(n)], 40 + 17 * n)


@pytest.mark.parametrize("chain", CHAINS)
@pytest.mark.parametrize("logN", [15, 16])
def test_kernel_at_larger_rings(envs, chain, logN):
    """the half boundary moves with N: chunk N/1024 is the first of the second half"""
    run_kernel_case(envs(logN, chain), [0, 5, NQ, 5, 2], logN)


def test_refuses_bad_arguments_and_accepts_n_0():
    from homulator_amd import hip
    ctx = hip.Context(13, NQ, NP)
    big = ctx.alloc(64)
    ctx.fill_uniform(big, [0] * 64, 5)
    x, y, out = ctx.alloc(4), ctx.alloc(4), ctx.alloc(8)
    ctx.fill_uniform(x, [0] * 4, 6)
    ctx.fill_uniform(y, [0] * 4, 7)
    null = types.SimpleNamespace(ptr=None)
    at = lambda limb: types.SimpleNamespace(ptr=big.limb_ptr(limb))
    ok = dict(limbs=[[0, 1], [0, 1], [0, 1], [2, 3]])
    for bufs in ((null, y, out, out), (x, null, out, out), (x, y, null, out), (x, y, out, null)):
        with pytest.raises(hip.HmError, match="hm_reim_split: null buffer"):
            ctx.reim_split(*bufs, [0, 0], **ok)
    with pytest.raises(hip.HmError, match="hm_reim_split: mod_ids is null"):
        ctx._ck(ctx.L.hm_reim_split(ctx.h, x.ptr, None, y.ptr, None, out.ptr, None, at(0).ptr, None, None, 1))
    for bad in range(4):
        ls = [[0], [0], [0], [1]]
        ls[bad] = [70000]
        with pytest.raises(hip.HmError, match="65535"):
            ctx.reim_split(x, y, out, out, [0], limbs=ls)
    with pytest.raises(hip.HmError, match="mod id"):
        ctx.reim_split(x, y, out, out, [NQ + NP], limbs=[[0], [0], [0], [1]])
    with pytest.raises(hip.HmError, match="hm_reim_split: two output"):
        ctx.reim_split(x, y, out, out, [0, 0], limbs=[[0, 1], [0, 1], [0, 1], [2, 1]])
    with pytest.raises(hip.HmError, match="hm_reim_split: two output"):
        ctx.reim_split(x, y, out, out, [0, 0], limbs=[[0, 1], [0, 1], [2, 2], [0, 1]])
    with pytest.raises(hip.HmError, match=r"hm_reim_split: an output limb-poly \(o_re\) overlaps an input limb-poly \(x\)"):
        ctx.reim_split(x, y, x, out, [0, 0], limbs=[[0, 1], [0, 1], [3, 1], [0, 1]])
    with pytest.raises(hip.HmError, match=r"hm_reim_split: an output limb-poly \(o_im\) overlaps an input limb-poly \(y\)"):
        ctx.reim_split(x, y, out, y, [0, 0], limbs=[[0, 1], [0, 1], [0, 1], [2, 0]])
    # by address range, not by base pointer: everything in ONE allocation, x = limbs 0..3, y = limbs 8..11 through bases of their own
    call = lambda re_at, im_at: ctx.reim_split(big, at(8), at(re_at), at(im_at), [0] * 4)
    call(16, 24)                                                # disjoint: accepted
    for re_at, im_at, what in ((3, 24, r"\(o_re\) overlaps an input limb-poly \(x\)"), (16, 11, r"\(o_im\) overlaps an input limb-poly \(y\)"),
                               (5, 24, r"\(o_re\) overlaps an input limb-poly \(y\)"), (16, 19, "two output")):
        with pytest.raises(hip.HmError, match="hm_reim_split: .*" + what):
            call(re_at, im_at)
    keep = hip._u32([0])
    ctx._ck(ctx.L.hm_reim_split(ctx.h, x.ptr, None, y.ptr, None, out.ptr, None, at(0).ptr, None, keep[1], 0))   # n = 0: nothing to do
    ctx.reim_split(x, y, out, out, [0, 0, 0], limbs=[[0, 1, 1], [3, 3, 0], [0, 2, 4], [1, 3, 5]])   # and a call with nothing wrong is accepted
    ctx.sync()
    ctx.close()


@pytest.mark.parametrize("chain", CHAINS)
def test_a_captured_call_replays(envs, chain):
    """the records live in a cached device table: after one warm run the call is captured into a graph and replayed on new input data"""
    ctx, o, _, _, _, _, U = envs(13, chain)
    ctx.L.hm_graph_launch.argtypes = [C.c_void_p, C.c_void_p]
    ctx.L.hm_graph_destroy.argtypes = [C.c_void_p]
    mods = [(3 * i + 1) % (NQ + NP) for i in range(70)]
    n = len(mods)
    fill_mods = [m for m in range(NQ + NP) for _ in range(PER_MOD)]
    rng = np.random.default_rng(3)
    lx = [m * PER_MOD + int(rng.integers(0, PER_MOD)) for m in mods]
    ly = [m * PER_MOD + int(rng.integers(0, PER_MOD)) for m in mods]
    x, y, re, im = ctx.alloc(len(fill_mods)), ctx.alloc(len(fill_mods)), ctx.alloc(n), ctx.alloc(n)
    run = lambda: ctx.reim_split(x, y, re, im, mods, limbs=[lx, ly, None, None])
    ctx.fill_uniform(x, fill_mods, 1)
    ctx.fill_uniform(y, fill_mods, 2)
    run()
    g = C.c_void_p()
    ctx._ck(ctx.L.hm_capture_begin(ctx.h))
    run()
    ctx._ck(ctx.L.hm_capture_end(ctx.h, C.byref(g)))
    ctx.fill_uniform(x, fill_mods, 3)
    ctx.fill_uniform(y, fill_mods, 4)
    for b in (re, im):
        b.upload(np.full((n, ctx.N), GUARD, dtype=np.uint64))
    ctx._ck(ctx.L.hm_graph_launch(ctx.h, g))
    ctx.sync()
    e_re, e_im = expected_rows(o, x.download(), y.download(), U, mods, lx, ly)
    assert np.array_equal(re.download(), e_re) and np.array_equal(im.download(), e_im), chain
    ctx.L.hm_graph_destroy(g)
    for b in (x, y, re, im):
        b.free()


# ============================================================================================================================
# B. the op
# ============================================================================================================================
def read_ct(op, name="out", copy=0):
    return op.read(name + ".c0", copy=copy), op.read(name + ".c1", copy=copy)


SHAPES = [
    ("config_4_N15.cfg", 13, 6, 5, 2, 2),       # beta = 3 with an uneven last digit, a batch of two
    ("config_4_N15.cfg", 13, 6, 3, 2, 1),
    ("config_4_N15.cfg", 13, 4, 4, 4, 1),       # one digit
]
_ref = {}


def reference(chain, logN, L, ell, alpha, copy=0, seed=SEED):
    """(out, out_im, conj) of the reference on the op's synthetic inputs, computed once per case"""
    from reim_ref import reim, synthetic_input
    key = (chain, logN, L, ell, alpha, copy, seed)
    if key not in _ref:
        o = oracle(logN, L, alpha, chain, threads=16)
        _ref[key] = reim(o, ell, *synthetic_input(o, ell, seed, copy=copy))
    return _ref[key]


@pytest.mark.parametrize("chain", CHAINS)
@pytest.mark.parametrize("cfg,logN,L,ell,alpha,batch", SHAPES)
def test_op_fused_unfused_and_reference_agree(chain, cfg, logN, L, ell, alpha, batch):
    """fused, unfused and fuse_reim = 0 against the reference, every copy of the batch; the stored unit is the oracle's U in every copy"""
    from reim_ref import assert_ct, unit
    ov = chain_ov(chain, {"batch": batch, "N": 1 << logN})
    U = unit(oracle(logN, L, alpha, chain), list(range(ell)))
    for mode, fuse, extra in (("fused", True, {}), ("unfused", False, {}), ("fuse_reim = 0", True, {"fuse_reim": 0})):
        op = host.Op(cfg, "hreim", L, ell, alpha, fuse=fuse, overrides=dict(ov, **extra))
        op.execute(1)
        kinds = [ln.split()[0] for ln in op.plan()]
        assert kinds.count("REIM") == (1 if mode == "fused" else 0), (mode, kinds)
        for c in range(batch):
            out, out_im, conj = reference(chain, logN, L, ell, alpha, copy=c)
            assert_ct(read_ct(op, "conj", c), conj, (mode, c, "conj"))
            assert_ct(read_ct(op, "out", c), out, (mode, c, "out"))
            assert_ct(read_ct(op, "out_im", c), out_im, (mode, c, "out_im"))
            assert np.array_equal(op.read("unit", copy=c), U), (mode, c, "unit")
        op.close()


def test_graph_replay_with_a_batch():
    """graph = 1: run 1 direct, run 2 captures, run 3 replays; both copies after the replay"""
    from reim_ref import assert_ct
    cfg, logN, L, ell, alpha, batch = SHAPES[0]
    op = host.Op(cfg, "hreim", L, ell, alpha, overrides={"batch": batch, "graph": 1, "N": 1 << logN})
    ln = [x for x in op.plan() if x.startswith("REIM")]
    assert len(ln) == 1 and f" n={2 * batch * ell} " in ln[0]
    for _ in range(3):
        op.execute(1)
    for c in range(batch):
        out, out_im, _ = reference("mont32", logN, L, ell, alpha, copy=c)
        assert_ct(read_ct(op, "out", c), out, f"copy {c}")
        assert_ct(read_ct(op, "out_im", c), out_im, f"copy {c}, imaginary")
    op.close()


@pytest.mark.parametrize("chain", CHAINS)
def test_device_output_against_hrotate_and_the_identity(chain):
    """on device output only: out = hrotate's output (galois = 2N - 1, same seed) + ct1, and out + X^(N/2) out_im = 2 ct1, X^(N/2) = q - U"""
    from reim_ref import unit
    cfg, logN, L, ell, alpha, _ = SHAPES[0]
    o = oracle(logN, L, alpha, chain)
    ids = list(range(ell))
    ov = chain_ov(chain, {"N": 1 << logN})
    rot = host.Op(cfg, "hrotate", L, ell, alpha, overrides=dict(ov, galois=2 * (1 << logN) - 1))
    rot.execute(1)
    op = host.Op(cfg, "hreim", L, ell, alpha, overrides=ov)
    op.execute(1)
    U = unit(o, ids)
    neg = np.stack([np.uint64(o.moduli[j]) - U[j] for j in ids])
    for k in range(2):
        ct, out, out_im = op.read(f"ct1.c{k}"), op.read(f"out.c{k}"), op.read(f"out_im.c{k}")
        assert np.array_equal(rot.read(f"ct1.c{k}"), ct)
        assert np.array_equal(out, o.ewe(EWE_ADD, ids, ct, None, rot.read(f"out.c{k}"))), (chain, k, "hrotate + ct1")
        assert np.array_equal(o.ewe(EWE_ADD, ids, out, None, o.ewe(EWE_MUL, ids, out_im, neg)), o.ewe(EWE_ADD, ids, ct, None, ct)), (chain, k, "2 ct1")
    rot.close()
    op.close()


def test_chain_reim_square_link_by_link():
    """hreim,hsquare at N = 2^13: link k runs under seed + 31 k (OpChain); the square's ct1 is the real part"""
    from reim_ref import assert_ct
    import square_ref
    cfg, logN, L, ell, alpha, _ = SHAPES[0]
    o = oracle(logN, L, alpha)
    chain = host.Chain(cfg, "hreim,hsquare", L, ell, alpha, overrides={"N": 1 << logN, "sq_scale": 1, "sq_const": 1})
    chain.execute(1)
    out, out_im, _ = reference("mont32", logN, L, ell, alpha)
    assert_ct(read_ct(chain[0], "out"), out, "link 0")
    assert_ct(read_ct(chain[0], "out_im"), out_im, "link 0, imaginary")
    seed = SEED + 31
    evk = square_ref.synthetic_inputs(o, ell, seed)[1]
    assert_ct(read_ct(chain[1]), square_ref.square(o, ell, out, evk, *square_ref.synthetic_constants(o, ell, seed, 1, 1)), "link 1 (hsquare)")
    chain.close()


def test_a_square_bound_to_the_imaginary_part():
    """the second output by name: an hsquare whose ct1 is out_im, beside one whose ct1 is out; a wrong name and a wrong level are refused"""
    from reim_ref import assert_ct
    import square_ref
    cfg, logN, L, ell, alpha, _ = SHAPES[0]
    o = oracle(logN, L, alpha)
    src = host.Op(cfg, "hreim", L, ell, alpha, overrides={"N": 1 << logN})
    src.execute(1)
    seeds = {"out_im": SEED + 31, "out": SEED + 62}
    sq = {name: host.Op(cfg, "hsquare", L, ell, alpha, overrides={"N": 1 << logN, "sq_scale": 1, "sq_const": 1, "seed": s}) for name, s in seeds.items()}
    sq["out_im"].bind_input("ct1", src, output="out_im")
    sq["out"].bind_input("ct1", src)
    ref = dict(zip(("out", "out_im"), reference("mont32", logN, L, ell, alpha)[:2]))
    for name, op in sq.items():
        op.execute(1)
        evk = square_ref.synthetic_inputs(o, ell, seeds[name])[1]
        assert_ct(read_ct(op), square_ref.square(o, ell, ref[name], evk, *square_ref.synthetic_constants(o, ell, seeds[name], 1, 1)), name)
    wrong = host.Op(cfg, "hsquare", L, ell - 1, alpha, overrides={"N": 1 << logN})
    with pytest.raises(host.HostError, match="levels differ"):
        wrong.bind_input("ct1", src, output="out_im")
    with pytest.raises(host.HostError, match="HREIM has no output ciphertext out_re"):
        wrong.bind_input("ct1", src, output="out_re")
    for x in (src, wrong, *sq.values()):
        x.close()


def test_real_data_decrypts_to_both_parts():
    """a fresh toy ciphertext and the conjugation key written into the op: both outputs are the reference's bit for bit and decrypt to
    m + sigma(m) and -X^(N/2) (m - sigma(m)) inside the derived bound; the reference is held to it first"""
    from reim_ref import REAL_BOUND, assert_ct, decryption_errors, real_reference
    LOGN, L, ELL, ALPHA = 13, 6, 5, 2
    o, toy, ct, evk, out, out_im, exact_re, exact_im = real_reference(LOGN, L, ELL, ALPHA)
    ref_errs = decryption_errors(toy, out, out_im, ELL, exact_re, exact_im)
    print(f"reference: max |dec - exact| = {ref_errs} (bound {REAL_BOUND})")
    assert max(ref_errs) < REAL_BOUND
    op = host.Op("config_4_N15.cfg", "hreim", L, ELL, ALPHA, overrides={"N": 1 << LOGN})
    op.write("ct1.c0", ct[0])
    op.write("ct1.c1", ct[1])
    for j in range(evk.shape[0]):
        for k in range(2):
            op.write(f"IP_Key{k}_{j}", evk[j][k])
    op.execute(1)
    got, got_im = read_ct(op, "out"), read_ct(op, "out_im")
    op.close()
    gpu_errs = decryption_errors(toy, got, got_im, ELL, exact_re, exact_im)
    print(f"GPU: max |dec - exact| = {gpu_errs} (bound {REAL_BOUND})")
    assert max(gpu_errs) < REAL_BOUND
    assert_ct(got, out, "real data, real part")
    assert_ct(got_im, out_im, "real data, imaginary part")
