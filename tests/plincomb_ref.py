"""CPU reference of hplincomb from oracle primitives only, following the definition literally and independent of the host plan:
per component the MUL of every ciphertext limb-poly by its plaintext's, the ADD of the terms, the ADD of the plaintext addend onto c0, and with
rescale the oracle's rescale of both sums.  Nothing here comes from the code under test."""
import numpy as np

from oracle.homoracle import EWE_ADD, EWE_MUL
from lincomb_ref import FRESH_BOUND

PT_STREAM, PT_STRIDE, ADDEND_T = 4000, 100000, 17


def plincomb(o, ell, cts, pts, addend=None, rescale=False):
    """cts: T ciphertexts [2][ell][N] at level ell; pts: T plaintexts [ell][N] in evaluation form; addend: [ell][N] or None.  Returns (out.c0,
    out.c1) at level ell, or ell - 1 with rescale"""
    ids = list(range(ell))
    out = []
    for k in range(2):
        acc = None
        for ct, p in zip(cts, pts):
            term = o.ewe(EWE_MUL, ids, ct[k], p)
            acc = term if acc is None else o.ewe(EWE_ADD, ids, acc, None, term)
        if k == 0 and addend is not None:
            acc = o.ewe(EWE_ADD, ids, acc, None, addend)
        out.append(o.rescale(ell, acc) if rescale else acc)
    return out[0], out[1]


def plincomb_integers(o, cts, pts, addend, k, j, cols):
    """the definition in Python integers: component k, limb j, the entries `cols`"""
    q = int(o.moduli[j])
    return [(sum(int(p[j][x]) * int(ct[k][j][x]) for ct, p in zip(cts, pts)) + (int(addend[j][x]) if (addend is not None and k == 0) else 0)) % q
            for x in cols]


def pt_stream(t):
    """the offset from the seed of the stream of pt<t>; pt0 is numbered 17"""
    return PT_STREAM + PT_STRIDE * (t if t else ADDEND_T)


def synthetic_plaintexts(o, ell, seed, T, pl_addend, copy=0, batch_seed_stride=100000):
    """the op's synthetic plaintexts: pt<t> = stream seed + 4000 + 100000 t (t = 1 .. T), pt0 = seed + 4000 + 100000 * 17; op `copy` of a batch
    + copy * stride; the addend None where the key is 0"""
    ids = list(range(ell))
    pts = [o.fill_uniform(ids, seed + copy * batch_seed_stride + pt_stream(t)) for t in range(1, T + 1)]
    return pts, (o.fill_uniform(ids, seed + copy * batch_seed_stride + pt_stream(0)) if pl_addend else None)


def constant_plaintext(o, ell, s):
    """the evaluation form of the constant polynomial with residues s[j]: every entry s[j]"""
    return np.stack([np.full(o.N, int(s[j]), dtype=np.uint64) for j in range(ell)])


def assert_ct(got, exp, what):
    assert np.array_equal(got[0], exp[0]), (what, "c0")
    assert np.array_equal(got[1], exp[1]), (what, "c1")


# ---- real data (tests/toy_ckks.py): sum_t p_t m_t + p_0 at scale Delta = 2^40, the products taken in the ring Z[X] / (X^N + 1)
DELTA, REAL_ADDEND = 1 << 40, 7


def real_plain_coeffs(N):
    """the sparse plaintext polynomials, {exponent: coefficient}: p_1 = 3 - 2 X^5 + X^(N/2), p_2 = 1 + 5 X^(N-1)"""
    return [{0: 3, 5: -2, N // 2: 1}, {0: 1, N - 1: 5}]


# Bound per coefficient of the decrypted output: the op is linear and meets no key, so Dec(out) - exact = sum_t p_t e_t with e_t the errors of
# the fresh inputs.  A coefficient of p_t e_t is a signed sum of the coefficients of e_t weighted by those of p_t: at most ||p_t||_1 times the
# bound of one fresh error coefficient (FRESH_BOUND, 8 sigma).  ||p_1||_1 = 6, ||p_2||_1 = 6.
REAL_BOUND = sum(sum(abs(c) for c in p.values()) for p in real_plain_coeffs(1 << 13)) * FRESH_BOUND


def negacyclic(p, m):
    """p m in Z[X] / (X^N + 1) for a sparse p {exponent: coefficient} and m an object array of N Python integers"""
    N = len(m)
    out = np.zeros(N, dtype=object)
    for e, c in p.items():
        out += c * np.concatenate([-m[N - e:], m[:N - e]]) if e else c * m
    return out


def encode(o, ell, p):
    """the evaluation form [ell][N] of the sparse integer polynomial p on the limbs 0 .. ell - 1"""
    a = np.zeros((ell, o.N), dtype=np.uint64)
    for j in range(ell):
        for e, c in p.items():
            a[j][e] = c % int(o.moduli[j])
    return o.ntt(list(range(ell)), a)


def real_case(toy, ell):
    """T = 2 fresh toy ciphertexts of small messages m_t Delta (|m_t| < 50), the two sparse plaintexts and the addend 7 Delta in evaluation
    form, and the exact result (sum_t p_t m_t) Delta + 7 Delta X^0"""
    ps = real_plain_coeffs(toy.N)
    ms = [toy.rng.integers(-50, 50, toy.N).astype(object) for _ in ps]
    cts = [toy.encrypt(m * DELTA, ell) for m in ms]
    pts = [encode(toy.o, ell, p) for p in ps]
    addend = encode(toy.o, ell, {0: REAL_ADDEND * DELTA})
    exact = sum(negacyclic(p, m) for p, m in zip(ps, ms)) * DELTA
    exact[0] += REAL_ADDEND * DELTA
    return cts, pts, addend, exact


def decryption_error(toy, out, ell, exact):
    """max |Dec(out) - exact|"""
    got, _ = toy.decrypt(np.stack(out), ell)
    assert max(abs(int(g)) for g in got) > 1 << 30   # a signal, not zeros
    return max(abs(int(g) - int(e)) for g, e in zip(got, exact))


_REAL = {}


def real_reference(logN=13, L=6, ell=5, alpha=2, seed=4271):
    """the real-data case and its reference, computed once per process: (oracle, toy, cts, pts, addend, out, exact)"""
    key = (logN, L, ell, alpha, seed)
    if key not in _REAL:
        from oracle.homoracle import Oracle
        from toy_ckks import Toy
        orc = Oracle(logN, L, alpha)
        orc.set_threads(8)
        toy = Toy(orc, seed=seed)
        cts, pts, addend, exact = real_case(toy, ell)
        _REAL[key] = (orc, toy, cts, pts, addend, plincomb(orc, ell, cts, pts, addend), exact)
    return _REAL[key]
