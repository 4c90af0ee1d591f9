"""hm_encode / hm_decode on the MI355X, on both arithmetic back-ends.
 A. the calls: the coefficients hm_encode stores are the emulator's (tests/emu/hm_emu_slots.cpp: the same header compiled for the host) bit for
    bit, the limbs are the oracle's transform of them bit for bit, hm_decode is the emulator's bit for bit and inverts hm_encode within
    N (1/2 + B) / Delta + F (B, F as measured: tests/test_emu_slots.py), hm_automorph in between rotates and conjugates the slots; every refusal, the
    overflow counter, n_vec = 0, a captured call replayed, an input that is already on the device.
 B. the ops on slots (tests/toy_ckks.py ciphertexts and keys at N = 2^13): pmult with an encoded plaintext, hrotate, hreim, and hlintrans with
    three encoded diagonals.  Each result is first the CPU oracle's on the same buffers bit for bit, then the statement about the slots: within
    4 x the error the CPU reference pipeline (tests/slots_ref.py's encoding, the oracle's op) makes against that statement, measured on the CPU
    and written down below (REF_ERR), where each test prints its own figure before it asserts."""
import ctypes as C

import numpy as np
import pytest

import slots_ref as R
from oracle.homoracle import Oracle, chain_below
from test_emu_slots import B_MEASURED, F_MEASURED, emu_decode, emu_encode, fill

pytestmark = pytest.mark.gpu
NQ, NP = 3, 1
GUARD = 0x5A5A5A5A5A5A5A5A
_made = {}


def env(logN, chain):
    """(hip context, oracle on the same moduli), made on first use and kept for the module"""
    from homulator_amd import hip
    if (logN, chain) not in _made:
        if chain == "mont32":
            ctx, o = hip.Context(logN, NQ, NP), Oracle(logN, NQ, NP)
        else:   # 36-bit words: the generic back-end
            mods = chain_below(logN, 36, NQ + NP)
            ctx, o = hip.Context(logN, NQ, NP, q=mods[:NQ], p=mods[NQ:]), Oracle(logN, NQ, NP, chain=mods)
        assert ctx.moduli == o.moduli and ctx.counter("arith") == (0 if chain == "mont32" else 1)
        o.set_threads(8)
        _made[(logN, chain)] = (ctx, o)
    return _made[(logN, chain)]


@pytest.fixture(scope="module", autouse=True)
def close_contexts():
    yield
    for ctx, _ in _made.values():
        ctx.close()
    _made.clear()


def scale_for(chain):
    return 2.0 ** 40 if chain == "mont32" else 2.0 ** 24   # |c| <= Delta must stay below half a 36-bit modulus


def vectors(logN, n_vec):
    return np.stack([fill(logN, "uniform", seed=10 + v) for v in range(n_vec)])


def tolerance(N, scale):
    """the issue's bound with B and F as measured: each of the N coefficients is off by at most 1/2 + B, every root has modulus 1"""
    return N * (0.5 + B_MEASURED) / scale + F_MEASURED


# ============================================================================================================================
# A. the calls
# ============================================================================================================================
# N = 2^14 and 2^16 have an odd log n, where the transform's two passes split unevenly (6 and 7 at 2^14)
SHAPES = [("mont32", 13, 1), ("mont32", 13, 3), ("generic", 13, 1), ("generic", 13, 3), ("mont32", 14, 2), ("generic", 14, 1), ("mont32", 15, 1),
          ("mont32", 16, 1), ("mont32", 17, 1)]


@pytest.mark.parametrize("chain,logN,n_vec", SHAPES)
def test_the_stored_coefficients_are_the_emulators(chain, logN, n_vec):
    ctx, _ = env(logN, chain)
    z, scale, src = vectors(logN, n_vec), scale_for(chain), ctx.largest_modulus()
    got = ctx.encode(z, scale, [])
    exp, ovf = emu_encode(logN, z, scale, ctx.moduli[src])
    assert ovf == 0 and ctx.counter("encode_overflow") == 0
    assert np.array_equal(got, exp)
    if chain == "mont32":   # and at the scale where the double transform is coarsest
        assert np.array_equal(ctx.encode(z[0], 2.0 ** 50, []), emu_encode(logN, z[0], 2.0 ** 50, ctx.moduli[src])[0])


@pytest.mark.parametrize("chain", ["mont32", "generic"])
def test_the_limbs_are_the_oracle_transform_of_the_coefficients(chain):
    """n_mod = 3 on permuted out_limbs of a buffer with one limb-poly more, which keeps its fill; the source modulus is not one of the three"""
    logN, n_vec, mods = 13, 2, [2, 0, 3]
    ctx, o = env(logN, chain)
    z, scale, src = vectors(logN, n_vec), scale_for(chain), 1
    rng = np.random.default_rng(5)
    out = ctx.alloc(n_vec * 3 + 1)
    out.upload(np.full((n_vec * 3 + 1, ctx.N), GUARD, dtype=np.uint64))
    perm = [int(v) for v in rng.permutation(n_vec * 3 + 1)]
    work = ctx.alloc(4)
    zb = ctx.from_host(z.view(np.uint64).reshape(n_vec, ctx.N))
    res = ctx.encode(zb, scale, mods, src_mod=src, n_vec=n_vec, work=work, work_limbs=[3, 1], out=out, out_limbs=perm[:-1])
    assert res is out
    got, coef = out.download(), work.download()
    exp_coef, _ = emu_encode(logN, z, scale, ctx.moduli[src])
    assert np.array_equal(coef[3], exp_coef[0]) and np.array_equal(coef[1], exp_coef[1])
    for v in range(n_vec):
        c = R.centre(exp_coef[v], ctx.moduli[src])
        exp = o.ntt(mods, np.stack([R.residues(c, o.moduli[m]) for m in mods]))
        for i in range(3):
            assert np.array_equal(got[perm[v * 3 + i]], exp[i]), (v, i)
    assert np.all(got[perm[-1]] == GUARD), "the guard limb-poly was written"
    # the host path of the binding returns the same limbs
    assert np.array_equal(ctx.encode(z, scale, mods, src_mod=src), np.stack([got[perm[v * 3:v * 3 + 3]] for v in range(n_vec)]))
    for b in (zb, out, work):
        b.free()


@pytest.mark.parametrize("chain,logN,n_vec", SHAPES)
def test_decode_is_the_emulators_and_inverts_encode(chain, logN, n_vec):
    ctx, _ = env(logN, chain)
    z, scale, m = vectors(logN, n_vec), scale_for(chain), 1
    limbs = ctx.encode(z, scale, [m])[:, 0, :]
    got = ctx.decode(limbs, None, m, scale)
    coef = np.stack([R.residues(R.centre(c, ctx.moduli[ctx.largest_modulus()]), ctx.moduli[m]) for c in ctx.encode(z, scale, [])])
    assert np.array_equal(got.view(np.uint64), emu_decode(logN, coef, scale, ctx.moduli[m]).view(np.uint64))
    err = float(np.abs(got - z).max())
    print(f"round trip {chain} 2^{logN} x{n_vec}: max |decode(encode z) - z| = {err:.4g}, tolerance {tolerance(ctx.N, scale):.4g}")
    assert err <= tolerance(ctx.N, scale)


@pytest.mark.parametrize("chain", ["mont32", "generic"])
@pytest.mark.parametrize("what,k", [("rotate", 1), ("rotate", 7), ("conjugate", 0)])
def test_an_automorphism_between_encode_and_decode_acts_on_the_slots(chain, what, k):
    """g = 5^k mod 2N rotates the slots left by k, g = 2N - 1 conjugates them: the automorphism permutes and negates coefficients, so the round
    trip's tolerance holds unchanged"""
    logN = 13
    ctx, _ = env(logN, chain)
    z, scale, m = vectors(logN, 1)[0], scale_for(chain), 0
    g = pow(5, k, 2 * ctx.N) if what == "rotate" else 2 * ctx.N - 1
    pt = ctx.from_host(ctx.encode(z, scale, [m])[0])
    rot = ctx.alloc(1)
    ctx.automorph(pt, rot, 1, g)
    got = ctx.decode(rot.download(), None, m, scale)[0]
    want = np.roll(z, -k) if what == "rotate" else np.conj(z)
    err = float(np.abs(got - want).max())
    print(f"{what} {k} {chain}: max error {err:.4g}, tolerance {tolerance(ctx.N, scale):.4g}")
    assert err <= tolerance(ctx.N, scale)
    assert float(np.abs(got - z).max()) > 0.1   # and it did move them
    pt.free()
    rot.free()


def test_every_refusal():
    from homulator_amd import hip
    ctx, _ = env(13, "mont32")
    N, h, L = ctx.N, ctx.h, ctx.L
    zb, work, out = ctx.alloc(1), ctx.alloc(2), ctx.alloc(4)
    u32 = lambda a: np.asarray(a, dtype=np.uint32).ctypes.data_as(C.c_void_p)
    mods = u32([0, 1])

    def enc(what, slots=zb.ptr, n_vec=1, scale=2.0 ** 30, wk=work.ptr, wl=None, src=0, o=out.ptr, ol=None, md=mods, n_mod=2):
        with pytest.raises(hip.HmError, match="hm_encode.*" + what):
            ctx._ck(L.hm_encode(h, slots, n_vec, scale, wk, wl, src, o, ol, md, n_mod))

    def dec(what, src=out.ptr, il=None, mod=0, scale=2.0 ** 30, wk=work.ptr, wl=None, slots=zb.ptr, n_vec=1):
        with pytest.raises(hip.HmError, match="hm_decode.*" + what):
            ctx._ck(L.hm_decode(h, src, il, mod, scale, wk, wl, slots, n_vec))

    enc("null buffer", slots=None)
    enc("null buffer", wk=None)
    enc("null buffer", o=None)
    enc("mod_ids is null", md=None)
    enc("limb index", wl=u32([1 << 16]))
    enc("limb index", ol=u32([0, 1 << 16]))
    enc("mod id", src=NQ + NP)
    enc("mod id", md=u32([0, NQ + NP]))
    for bad in (0.0, -1.0, float("inf"), float("nan"), 1e308 * 10):
        enc("scale must be finite and positive", scale=bad)
    enc("16-byte aligned", slots=zb.ptr + 8)
    enc("overlaps work", wk=out.ptr, wl=u32([1]), ol=u32([0, 1]))
    enc("overlaps work", wk=out.ptr + 8 * N // 2, wl=u32([0]), ol=u32([2, 1]))   # half a limb-poly in: touches out limbs 0 and 1
    dec("null buffer", src=None)
    dec("null buffer", wk=None)
    dec("null buffer", slots=None)
    dec("limb index", il=u32([1 << 16]))
    dec("limb index", wl=u32([1 << 16]))
    dec("mod id", mod=NQ + NP)
    for bad in (0.0, -2.0, float("inf"), float("nan")):
        dec("scale must be finite and positive", scale=bad)
    dec("16-byte aligned", slots=zb.ptr + 8)
    dec("work overlaps the input", wk=out.ptr, wl=u32([0]))
    dec("work overlaps the input", src=work.ptr + 8, wl=u32([1]))
    assert L.hm_encode(None, zb.ptr, 1, 1.0, work.ptr, None, 0, out.ptr, None, mods, 2) != 0
    # n_vec = 0 is no work and no error, whatever else is passed
    assert L.hm_encode(h, None, 0, 0.0, None, None, 99, None, None, None, 5) == 0
    assert L.hm_decode(h, None, None, 99, 0.0, None, None, None, 0) == 0
    assert ctx.encode(np.zeros((0, N // 2), dtype=np.complex128), 2.0 ** 30, [0]).shape == (0, 1, N)
    for b in (zb, work, out):
        b.free()


@pytest.mark.parametrize("chain", ["mont32", "generic"])
def test_the_overflow_counter(chain):
    """the constant slot vector v encodes to the constant polynomial rint(Delta v) exactly (tests/test_emu_slots.py): (q_s - 1) / 2 is kept,
    one more raises the counter, is stored as 0, and reading the counter clears it"""
    ctx, _ = env(13, chain)
    src = NQ - 1 if chain == "generic" else None
    q = ctx.moduli[ctx.largest_modulus() if src is None else src]
    half = (q - 1) // 2
    lg = max(half.bit_length() - 52, 0)               # Delta = 2^lg: v and v + 1 below are integers of at most 52 bits, exact doubles,
    scale, n = 2.0 ** lg, ctx.N // 2                  # and Delta v is the largest multiple of Delta that half the modulus holds
    v = float(half >> lg)
    kept = int(v) << lg
    assert kept <= half < kept + (1 << lg)
    coef = ctx.encode(np.full(n, v), scale, [], src_mod=src)
    assert ctx.counter("encode_overflow") == 0 and int(coef[0, 0]) == kept and not coef[0, 1:].any()
    over = v + 1
    coef = ctx.encode(np.full(n, -over), scale, [], src_mod=src)
    assert not coef.any()
    assert ctx.counter("encode_overflow") == 1 and ctx.counter("encode_overflow") == 0
    assert np.array_equal(coef, emu_encode(13, np.full(n, -over), scale, q)[0])


@pytest.mark.parametrize("chain", ["mont32", "generic"])
def test_a_captured_encode_and_decode_replay(chain):
    logN, mods = 13, [0, 2]
    ctx, _ = env(logN, chain)
    z, scale = vectors(logN, 2), scale_for(chain)
    exp = ctx.encode(z, scale, mods)                  # the first run makes the tables
    exp_z = ctx.decode(exp[:, 1, :], None, 2, scale)
    zb = ctx.from_host(z.view(np.uint64).reshape(2, ctx.N))
    work, out, back, w2 = ctx.alloc(2), ctx.alloc(4), ctx.alloc(2), ctx.alloc(2)
    for b, k in ((out, 4), (back, 2)):
        b.upload(np.full((k, ctx.N), GUARD, dtype=np.uint64))
    run = lambda: (ctx.encode(zb, scale, mods, n_vec=2, work=work, out=out), ctx.decode(out, [1, 3], 2, scale, work=w2, out=back))
    run()                                             # the launch tables of exactly these calls are cached now
    for b, k in ((out, 4), (back, 2)):
        b.upload(np.full((k, ctx.N), GUARD, dtype=np.uint64))
    g = C.c_void_p()
    ctx._ck(ctx.L.hm_capture_begin(ctx.h))
    run()
    ctx._ck(ctx.L.hm_capture_end(ctx.h, C.byref(g)))
    assert np.all(out.download() == GUARD)            # captured, not run
    ctx._ck(ctx.L.hm_graph_launch(ctx.h, g))
    ctx.sync()
    ctx.L.hm_graph_destroy(g)
    assert np.array_equal(out.download().reshape(2, 2, ctx.N), exp)
    assert np.array_equal(back.download(), exp_z.view(np.uint64).reshape(2, ctx.N))
    for b in (zb, work, out, back, w2):
        b.free()


def test_a_captured_encode_survives_a_larger_eager_call():
    """a graph keeps the address of the hand-off between hm_encode's two launches.  Captured with n_vec = 1 on a context of its own (whose
    hand-off holds one vector), then an eager call with n_vec = 3 outgrows that hand-off: it is kept while the graph lives, so the replay
    writes the expected limbs, before and after another eager call; once the graph is gone a still larger call runs as well"""
    from homulator_amd import hip
    logN, mods, scale = 13, [0, 2], 2.0 ** 40
    ctx = hip.Context(logN, NQ, NP)
    z = vectors(logN, 4)
    exp1 = ctx.encode(z[0], scale, mods)
    zb = ctx.from_host(z[:1].view(np.uint64).reshape(1, ctx.N))
    work, out = ctx.alloc(1), ctx.alloc(2)
    ctx.encode(zb, scale, mods, n_vec=1, work=work, out=out)
    g = C.c_void_p()
    ctx._ck(ctx.L.hm_capture_begin(ctx.h))
    ctx.encode(zb, scale, mods, n_vec=1, work=work, out=out)
    ctx._ck(ctx.L.hm_capture_end(ctx.h, C.byref(g)))
    exp3 = ctx.encode(z[:3], scale, mods)             # eager, three vectors: a larger hand-off
    assert np.array_equal(exp3[0], exp1[0])
    for again in range(2):
        out.upload(np.full((2, ctx.N), GUARD, dtype=np.uint64))
        ctx._ck(ctx.L.hm_graph_launch(ctx.h, g))
        ctx.sync()
        assert np.array_equal(out.download(), exp1[0]), again
        assert np.array_equal(ctx.encode(z[1:3], scale, mods), exp3[1:])
    ctx.L.hm_graph_destroy(g)
    assert np.array_equal(ctx.encode(z, scale, mods)[:3], exp3)
    for b in (zb, work, out):
        b.free()
    ctx.close()


def test_a_tensor_in_host_memory_is_refused():
    import torch
    ctx, _ = env(13, "mont32")
    t = torch.zeros(1 << 12, dtype=torch.complex128)
    with pytest.raises(ValueError, match="must be on the GPU"):
        ctx.encode(t, 2.0 ** 40, [0])
    with pytest.raises(ValueError, match="must be on the GPU"):
        ctx.decode(t, [0], 0, 2.0 ** 40)


def test_an_input_that_is_already_on_the_device():
    """a torch tensor in HBM goes in through data_ptr(); the result stays on the device and equals the host path's"""
    import torch
    logN = 13
    ctx, _ = env(logN, "mont32")
    z, scale = vectors(logN, 2), 2.0 ** 40
    t = torch.from_numpy(z).to("cuda")
    torch.cuda.synchronize()
    assert t.is_contiguous() and t.dtype == torch.complex128
    res = ctx.encode(t, scale, [0, 1])
    assert hasattr(res, "ptr")
    exp = ctx.encode(z, scale, [0, 1])
    assert np.array_equal(res.download().reshape(2, 2, ctx.N), exp)
    back = torch.zeros_like(t)
    torch.cuda.synchronize()
    assert ctx.decode(res, [0, 2], 0, scale, out=back) is back
    ctx.sync()
    assert np.array_equal(back.cpu().numpy(), ctx.decode(exp[:, 0, :], None, 0, scale))
    res.free()


# ============================================================================================================================
# B. the ops on slots
# ============================================================================================================================
LOGN, L, ELL, ALPHA = 13, 6, 5, 2
SCALE = 2.0 ** 30
OV = {"N": 1 << LOGN}
# max |slots of the CPU reference pipeline - the slot statement|, measured on the CPU with the seeds below (print_reference_errors()); the GPU
# tests assert 4 x these.  pmult meets no key: its error is the fresh noise times the plaintext; the others carry a key switch's noise, which the
# evaluation at N / 2 roots of modulus 1 spreads over the slots
REF_ERR = {"pmult": 6.34e-7, "hrotate": 1.79e-3, "hreim": 2.98e-3, "hlintrans": 2.04e-3}
_ops = {}


def ops_env():
    """(oracle, toy, z, a fresh encryption of the exact encoding of z at level ELL), once per process"""
    if not _ops:
        from toy_ckks import Toy
        o = Oracle(LOGN, L, ALPHA)
        o.set_threads(8)
        toy = Toy(o, seed=4261)
        z = fill(LOGN, "uniform", seed=77)
        _ops["env"] = (o, toy, z, toy.encrypt(R.encode_int(z, LOGN, SCALE, R.fft_coeffs), ELL))
    return _ops["env"]


def slots_of(toy, ct, level, scale):
    """decrypt with Python integers, decode with the longdouble reference"""
    dec, _ = toy.decrypt(np.stack(ct), level)
    return R.decode_int(dec, LOGN, scale, R.fft_slots)


def diagonals(count, seed=303):
    rng = np.random.default_rng(seed)
    n = 1 << (LOGN - 1)
    return [np.sqrt(rng.uniform(0, 1, n)) * np.exp(2j * np.pi * rng.uniform(0, 1, n)) for _ in range(count)]


def rotation_key(toy, g, level=ELL):
    return toy.evk_at_level(toy.gen_evk(toy.automorph(toy.s, g)), level)


def reference(name):
    """the op through the CPU alone: (what the slot statement says, the slots the reference pipeline gives, the key(s) it used)"""
    import reim_ref
    from identity_ref import lintrans_id
    if name in _ops:
        return _ops[name]
    o, toy, z, ct = ops_env()
    N = o.N
    if name == "pmult":
        w = diagonals(1)[0]
        out = o.pmult(ELL, ct, R.encode_limbs(o, w, SCALE, range(ELL), R.fft_coeffs))
        res = ([z * w], [slots_of(toy, out, ELL, SCALE * SCALE)], None)
    elif name == "hrotate":
        evk = rotation_key(toy, 5)
        res = ([np.roll(z, -1)], [slots_of(toy, o.hrotate(ELL, ct, 5, evk), ELL, SCALE)], evk)
    elif name == "hreim":
        evk = rotation_key(toy, 2 * N - 1)
        out, out_im, _ = reim_ref.reim(o, ELL, ct, evk)
        res = ([2 * z.real + 0j, 2 * z.imag + 0j], [slots_of(toy, out, ELL, SCALE), slots_of(toy, out_im, ELL, SCALE)], evk)
    else:   # hlintrans, R = 2, identity = 1: y = d0 (.) z + d1 (.) rot_1(z) + d2 (.) rot_2(z), the matrix with the three diagonals 0, 1, 2
        d = diagonals(3)
        keys = [rotation_key(toy, pow(5, r, 2 * N)) for r in (1, 2)]
        pts = [R.encode_limbs(o, dr, SCALE, o.ext_ids(ELL), R.fft_coeffs) for dr in d]
        out = lintrans_id(o, ELL, ct, 5, keys, pts[1:], pts[0])
        res = ([d[0] * z + d[1] * np.roll(z, -1) + d[2] * np.roll(z, -2)], [slots_of(toy, out, ELL, SCALE * SCALE)], keys)
    _ops[name] = res
    return res


def print_reference_errors():
    for name in REF_ERR:
        want, got, _ = reference(name)
        print(name, max(float(np.abs(g - w).max()) for g, w in zip(got, want)))


def check_slots(name, toy, outs, level, scale):
    want, ref, _ = reference(name)
    ref_err = max(float(np.abs(g - w).max()) for g, w in zip(ref, want))
    err = max(float(np.abs(slots_of(toy, out, level, scale) - w).max()) for out, w in zip(outs, want))
    print(f"{name}: max |slots - statement| = {err:.4g} on the GPU, {ref_err:.4g} through the CPU reference (recorded {REF_ERR[name]:.4g})")
    assert err <= 4 * REF_ERR[name]


def read_ct(op, name="out"):
    return np.stack([op.read(name + ".c0"), op.read(name + ".c1")])


def write_ct_and_keys(op, ct, keys):
    """keys: {buffer name stem: evk}"""
    op.write("ct1.c0", ct[0])
    op.write("ct1.c1", ct[1])
    for stem, evk in keys.items():
        for j in range(evk.shape[0]):
            for k in range(2):
                op.write(f"{stem}Key{k}_{j}", evk[j][k])


def assert_encoding(o, got, z, mods):
    """a plaintext buffer the op encoded on the device against the reference encoding: the same integers but for coefficients whose exact value
    lies within the double transform's error of a half-integer, where the two may round apart by one"""
    ref = R.encode_int(z, LOGN, SCALE, R.fft_coeffs)
    for r, m in enumerate(mods):
        c = R.centre(o.ntt([m], got[r][None, :], inverse=True)[0], o.moduli[m])
        diff = np.array([int(a) - int(b) for a, b in zip(c, ref)])
        assert np.abs(diff).max() <= 1 and np.count_nonzero(diff) <= 8, (m, np.count_nonzero(diff))


def test_pmult_with_an_encoded_plaintext_multiplies_the_slots():
    from homulator_amd import host
    o, toy, z, ct = ops_env()
    w = diagonals(1)[0]
    op = host.Op("config_4_N15.cfg", "pmult", L, ELL, ALPHA, overrides=OV)
    write_ct_and_keys(op, ct, {})
    op.encode_plaintext("pt", w, SCALE)
    op.execute(1)
    out, pt = read_ct(op), op.read("pt")
    op.close()
    assert_encoding(o, pt, w, range(ELL))
    exp = o.pmult(ELL, ct, pt)
    assert np.array_equal(out[0], exp[0]) and np.array_equal(out[1], exp[1])
    check_slots("pmult", toy, [out], ELL, SCALE * SCALE)


def test_hrotate_rotates_the_slots_by_one():
    from homulator_amd import host
    o, toy, z, ct = ops_env()
    evk = reference("hrotate")[2]
    op = host.Op("config_4_N15.cfg", "hrotate", L, ELL, ALPHA, overrides=dict(OV, galois=5))
    write_ct_and_keys(op, ct, {"IP_": evk})
    op.execute(1)
    out = read_ct(op)
    op.close()
    exp = o.hrotate(ELL, ct, 5, evk)
    assert np.array_equal(out[0], exp[0]) and np.array_equal(out[1], exp[1])
    check_slots("hrotate", toy, [out], ELL, SCALE)


def test_hreim_gives_twice_the_real_and_twice_the_imaginary_part():
    import reim_ref
    from homulator_amd import host
    o, toy, z, ct = ops_env()
    evk = reference("hreim")[2]
    op = host.Op("config_4_N15.cfg", "hreim", L, ELL, ALPHA, overrides=OV)
    write_ct_and_keys(op, ct, {"IP_": evk})
    op.execute(1)
    out, out_im = read_ct(op), read_ct(op, "out_im")
    op.close()
    exp, exp_im, _ = reim_ref.reim(o, ELL, ct, evk)
    reim_ref.assert_ct(out, exp, "real part")
    reim_ref.assert_ct(out_im, exp_im, "imaginary part")
    check_slots("hreim", toy, [out, out_im], ELL, SCALE)


def test_hlintrans_with_three_encoded_diagonals_is_the_matrix_vector_product():
    from homulator_amd import host
    from identity_ref import lintrans_id
    o, toy, z, ct = ops_env()
    d, keys = diagonals(3), reference("hlintrans")[2]
    op = host.Op("config_4_N15.cfg", "hlintrans", L, ELL, ALPHA, overrides=dict(OV, rotations=2, galois=5, identity=1))
    write_ct_and_keys(op, ct, {f"IP_Rot{r}_": keys[r - 1] for r in (1, 2)})
    for r in range(3):
        op.encode_plaintext(f"pt{r}", d[r], SCALE)
    op.execute(1)
    out, pts = read_ct(op), [op.read(f"pt{r}") for r in range(3)]
    op.close()
    for r in range(3):
        assert_encoding(o, pts[r], d[r], o.ext_ids(ELL))
    exp = lintrans_id(o, ELL, ct, 5, keys, pts[1:], pts[0])
    assert np.array_equal(out[0], exp[0]) and np.array_equal(out[1], exp[1])
    check_slots("hlintrans", toy, [out], ELL, SCALE * SCALE)


def test_encode_plaintext_refusals():
    from homulator_amd import host
    n = 1 << (LOGN - 1)
    op = host.Op("config_4_N15.cfg", "pmult", L, ELL, ALPHA, overrides=OV)
    z = np.zeros(n, dtype=np.complex128)
    for name, what in (("nothing", "has no buffer nothing"), ("ct1.c0", "is no plaintext"), ("out.c0", "is no plaintext")):
        with pytest.raises(host.HostError, match="encode_plaintext:.*" + what):
            op.encode_plaintext(name, z, SCALE)
    with pytest.raises(host.HostError, match="encode_plaintext:.*slots given"):
        op.encode_plaintext("pt", z[:-1], SCALE)
    with pytest.raises(host.HostError, match="encode_plaintext:.*hm_encode.*scale"):
        op.encode_plaintext("pt", z, -1.0)
    with pytest.raises(host.HostError, match="encode_plaintext:.*copy"):
        op.encode_plaintext("pt", z, SCALE, copy=1)
    with pytest.raises(host.HostError, match="encode_plaintext:.*exceeds half"):
        op.encode_plaintext("pt", np.full(n, 4.0), 2.0 ** 60)
    op.encode_plaintext("pt", z, SCALE)
    assert not op.read("pt").any()
    op.close()


def test_encode_plaintext_addresses_the_ops_of_a_batch():
    """batch = 2: the plaintext of copy 1 is encoded into copy 1's limb-polys (the copy's own base of the pool), copy 0 keeps its own"""
    from homulator_amd import host
    d = diagonals(2, seed=404)
    op = host.Op("config_4_N15.cfg", "pmult", L, ELL, ALPHA, overrides=dict(OV, batch=2))
    op.encode_plaintext("pt", d[0], SCALE)
    first = op.read("pt")
    op.encode_plaintext("pt", d[1], SCALE, copy=1)
    assert np.array_equal(op.read("pt"), first)
    second = op.read("pt", copy=1)
    op.encode_plaintext("pt", d[1], SCALE)
    assert np.array_equal(op.read("pt"), second) and not np.array_equal(first, second)
    assert_encoding(ops_env()[0], second, d[1], range(ELL))
    op.close()
