"""CPU reference of hlincomb from oracle primitives only, following the definition literally and independent of the host plan:
per component, MUL_CONST of every term by its per-limb scalars, ADD of the terms, the per-limb constants on every evaluation-form entry of c0 (numpy:
the oracle has no such opcode), and with rescale the oracle's rescale of both sums."""
import numpy as np

from oracle.homoracle import EWE_ADD, EWE_MUL_CONST
from square_ref import add_const

SCALE_STREAM, SCALE_STRIDE, CONST_STREAM = 6200, 100, 6290
FRESH_SIGMA = 3.2          # tests/toy_ckks.py Toy.small_err: the error of a fresh ciphertext is rint(normal(0, 3.2)) per coefficient
FRESH_BOUND = 26           # 8 sigma, rounded up: one coefficient exceeds it with probability below 2^-49


def lincomb(o, ell, cts, scales, const=None, rescale=False):
    """cts: T ciphertexts [2][ell][N] at level ell; scales[t]: ell residues; const: ell residues or None.  Returns (out.c0, out.c1) at level ell,
    or ell - 1 with rescale"""
    ids = list(range(ell))
    out = []
    for k in range(2):
        acc = None
        for ct, s in zip(cts, scales):
            term = o.ewe(EWE_MUL_CONST, ids, ct[k], k=s)
            acc = term if acc is None else o.ewe(EWE_ADD, ids, acc, None, term)
        if k == 0 and const is not None:
            acc = add_const(acc, const, [o.moduli[m] for m in ids])
        out.append(o.rescale(ell, acc) if rescale else acc)
    return out[0], out[1]


def lincomb_integers(o, ell, cts, scales, const, k, j, cols):
    """the definition in Python integers: component k, limb j, the entries `cols`"""
    q = o.moduli[j]
    add = const[j] if (const is not None and k == 0) else 0
    return [(sum(int(s[j]) * int(ct[k][j][x]) for ct, s in zip(cts, scales)) + add) % q for x in cols]


def synthetic_constants(o, ell, seed, T, lc_const):
    """the op's synthetic constants: word 0 of limb j of the streams seed + 6200 + 100 t (t = 1 .. T) and seed + 6290; const None where the key is 0"""
    ids = list(range(ell))
    scales = [[int(v) for v in o.fill_uniform(ids, seed + SCALE_STREAM + SCALE_STRIDE * t)[:, 0]] for t in range(1, T + 1)]
    const = [int(v) for v in o.fill_uniform(ids, seed + CONST_STREAM)[:, 0]] if lc_const else None
    return scales, const


def synthetic_inputs(o, ell, seed, T, copy=0, batch_seed_stride=100000):
    """the op's synthetic streams: ct<t> from seed + 2000 (t - 1) (c1: + 1000), op `copy` of a batch + copy * stride"""
    return [o.synth_ct(ell, seed + copy * batch_seed_stride + 2000 * t) for t in range(T)]


def assert_ct(got, exp, what):
    assert np.array_equal(got[0], exp[0]), (what, "c0")
    assert np.array_equal(got[1], exp[1]), (what, "c1")


# ---- real data (tests/toy_ckks.py): sum_t s_t m_t + c at scale Delta = 2^40
REAL_SCALARS, REAL_CONST, DELTA = [3, -2, 1, -5], 7, 1 << 40


def real_case(toy, ell):
    """T = 4 fresh toy ciphertexts of small messages m_t Delta (|m_t| < 50), small signed integer scalars s_t stored as q_j - |s_t| when negative,
    the constant k_j = c Delta mod q_j, and the exact result (sum_t s_t m_t) Delta + c Delta X^0"""
    ms = [toy.rng.integers(-50, 50, toy.N) for _ in REAL_SCALARS]
    cts = [toy.encrypt(m.astype(object) * DELTA, ell) for m in ms]
    scales = [[s % toy.o.moduli[j] for j in range(ell)] for s in REAL_SCALARS]
    const = [REAL_CONST * DELTA % toy.o.moduli[j] for j in range(ell)]
    exact = sum(s * m.astype(object) for s, m in zip(REAL_SCALARS, ms)) * DELTA
    exact[0] += REAL_CONST * DELTA
    return cts, scales, const, exact


def decryption_error(toy, out, ell, exact):
    """max |Dec(out) - exact|, and the bound.  The op is linear and meets no key: Dec(out) = sum_t s_t (m_t Delta + e_t) + c Delta exactly, so the
    error is sum_t s_t e_t with e_t the errors of the fresh inputs, at most sum_t |s_t| times the bound of one fresh error (FRESH_BOUND)"""
    got, _ = toy.decrypt(np.stack(out), ell)
    assert max(abs(int(g)) for g in got) > 1 << 30   # a signal, not zeros
    return max(abs(int(g) - int(e)) for g, e in zip(got, exact)), sum(abs(s) for s in REAL_SCALARS) * FRESH_BOUND
