"""CPU reference of hsquare from oracle primitives only, following the definition literally and independent of the host plan:
tensor the ciphertext with itself (MUL, MAC2, MUL), multiply the three polynomials by the per-limb scalars (MUL_CONST), add the per-limb constants to
every evaluation-form entry of d0 (numpy: the oracle has no such opcode), then hmult's tail: key switch of d2, the two adds, the two rescales."""
import numpy as np

from oracle.homoracle import EWE_ADD, EWE_MAC2, EWE_MUL, EWE_MUL_CONST

SCALE_STREAM, CONST_STREAM = 6000, 6100


def add_const(x, ks, moduli):
    """x[j] + ks[j] mod moduli[j] on every entry (canonical residues in, canonical residues out)"""
    x = np.ascontiguousarray(x, dtype=np.uint64)
    out = np.empty_like(x)
    for j, (k, q) in enumerate(zip(ks, moduli)):
        t = x[j] + np.uint64(k)               # below 2^61
        out[j] = np.where(t >= np.uint64(q), t - np.uint64(q), t)
    return out


def square_tensor(o, mods, a, c, scale=None, const=None):
    """(d0, d1, d2) = (s a a + k, 2 s a c, s c c) on the limbs `mods`; scale / const: per-limb lists or None"""
    d0, d1, d2 = o.ewe(EWE_MUL, mods, a, a), o.ewe(EWE_MAC2, mods, a, c, c, a), o.ewe(EWE_MUL, mods, c, c)
    if scale is not None:
        d0, d1, d2 = (o.ewe(EWE_MUL_CONST, mods, d, k=scale) for d in (d0, d1, d2))
    if const is not None:
        d0 = add_const(d0, const, [o.moduli[m] for m in mods])
    return d0, d1, d2


def square(o, ell, ct, evk, scale=None, const=None):
    """ct: [2][ell][N] at level ell; evk: hmult's key.  Returns (out.c0, out.c1) at level ell - 1"""
    ids = list(range(ell))
    d0, d1, d2 = square_tensor(o, ids, ct[0], ct[1], scale, const)
    ks0, ks1 = o.keyswitch(ell, d2, evk)
    return (o.rescale(ell, o.ewe(EWE_ADD, ids, d0, None, ks0)), o.rescale(ell, o.ewe(EWE_ADD, ids, d1, None, ks1)))


def synthetic_constants(o, ell, seed, sq_scale, sq_const):
    """the op's synthetic constants: word 0 of limb j of the streams seed + 6000 (a 0 replaced by 1) and seed + 6100; None where the key is 0"""
    ids = list(range(ell))
    scale = [int(v) or 1 for v in o.fill_uniform(ids, seed + SCALE_STREAM)[:, 0]] if sq_scale else None
    const = [int(v) for v in o.fill_uniform(ids, seed + CONST_STREAM)[:, 0]] if sq_const else None
    return scale, const


def synthetic_inputs(o, ell, seed, copy=0, batch_seed_stride=100000):
    """the op's synthetic streams: ct1 from seed (c1: + 1000), op `copy` of a batch + copy * stride; the key from seed + 10000"""
    return o.synth_ct(ell, seed + copy * batch_seed_stride), o.synth_evk(ell, seed + 10000)


def assert_ct(got, exp, what):
    assert np.array_equal(got[0], exp[0]), (what, "c0")
    assert np.array_equal(got[1], exp[1]), (what, "c1")


# ---- real data (tests/toy_ckks.py): one double-angle step y <- 2 y^2 - 1 at scale Delta = 2^40
def real_case(toy, ell):
    """a toy ciphertext of small messages m 2^40 (|m| < 50), the relinearisation key, the constants s_j = 2 and k_j = -2^80 mod q_j, and the exact
    result 2 m m 2^80 - 2^80 X^0"""
    from dot_ref import negacyclic_small
    s = np.array([int(x) for x in toy.s])
    evk = toy.evk_at_level(toy.gen_evk(negacyclic_small(s, s).astype(object)), ell)
    m = toy.rng.integers(-50, 50, toy.N)
    ct = toy.encrypt(m.astype(object) * (1 << 40), ell)
    exact = 2 * negacyclic_small(m, m).astype(object) * (1 << 80)
    exact[0] -= 1 << 80
    scale = [2] * ell
    const = [(-(1 << 80)) % toy.o.moduli[j] for j in range(ell)]
    return ct, evk, scale, const, exact


def decryption_error(toy, out, ell, exact):
    """max |Dec(out) q_last - exact|, and the bound: twice the one tests/test_gpu_real_data.py holds a single hmult to (q_last << 12): the scalar
    2 multiplies the key-switch noise by 2, the constant is added exactly"""
    got, _ = toy.decrypt(np.stack(out), ell - 1)
    ql = toy.o.moduli[ell - 1]
    assert max(abs(int(g)) for g in got) > 1 << 30   # a signal, not zeros
    return max(abs(int(g) * ql - int(e)) for g, e in zip(got, exact)), 2 * (ql << 12)
