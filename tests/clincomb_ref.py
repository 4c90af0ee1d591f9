"""CPU reference of hclincomb from oracle primitives only, following the definition literally and independent of the host plan:
per component and term MUL_CONST by a_t, MUL by the oracle's NTT of the monomial X^(N/2) and MUL_CONST by b_t, ADD of the two and of the terms, the
per-limb constants on every evaluation-form entry of c0 (numpy: the oracle has no such opcode), and with rescale the oracle's rescale of both sums.
Nothing here comes from the code under test."""
import numpy as np

from oracle.homoracle import EWE_ADD, EWE_MUL, EWE_MUL_CONST
from lincomb_ref import FRESH_BOUND
from square_ref import add_const

RE_STREAM, IM_STREAM, STRIDE, CONST_STREAM = 6450, 8150, 100, 9850


def monomial(o, ids):
    """NTT_{q_j}(X^(N/2)) for the limbs `ids`: [len(ids)][N]"""
    p = np.zeros((len(ids), o.N), dtype=np.uint64)
    p[:, o.N // 2] = 1
    return o.ntt(ids, p)


def halves(o, j):
    """X^(N/2) under q_j in Python integers: (v, q - v), its values on entries [0, N/2) and [N/2, N); v = psi^(N/2)"""
    q = int(o.moduli[j])
    v = pow(int(o.psis[j]), o.N // 2, q)
    return v, q - v


def clincomb_poly(o, ids, xs, re, im, const=None, mono=None):
    """sum_t (re[t] + im[t] X^(N/2)) xs[t] + const for limb-polys xs[t] [len(ids)][N]; re[t], im[t], const: one residue per limb of `ids`"""
    mono = monomial(o, ids) if mono is None else mono
    acc = None
    for x, a, b in zip(xs, re, im):
        term = o.ewe(EWE_ADD, ids, o.ewe(EWE_MUL_CONST, ids, x, k=a), None, o.ewe(EWE_MUL_CONST, ids, o.ewe(EWE_MUL, ids, x, mono), k=b))
        acc = term if acc is None else o.ewe(EWE_ADD, ids, acc, None, term)
    if const is not None:
        acc = add_const(acc, const, [o.moduli[m] for m in ids])
    return acc


def clincomb(o, ell, cts, re, im, const=None, rescale=False):
    """cts: T ciphertexts [2][ell][N] at level ell; re[t], im[t]: ell residues; const: ell residues or None.  Returns (out.c0, out.c1) at level
    ell, or ell - 1 with rescale"""
    ids = list(range(ell))
    mono = monomial(o, ids)
    out = []
    for k in range(2):
        acc = clincomb_poly(o, ids, [ct[k] for ct in cts], re, im, const if k == 0 else None, mono)
        out.append(o.rescale(ell, acc) if rescale else acc)
    return out[0], out[1]


def clincomb_integers(o, cts, re, im, const, k, j, cols):
    """the definition in Python integers: component k, limb j, the entries `cols`"""
    q = int(o.moduli[j])
    v, w = halves(o, j)
    add = int(const[j]) if (const is not None and k == 0) else 0
    return [(sum((int(a[j]) + int(b[j]) * (v if x < o.N // 2 else w)) * int(ct[k][j][x]) for ct, a, b in zip(cts, re, im)) + add) % q for x in cols]


def synthetic_constants(o, ell, seed, T, cl_const):
    """the op's synthetic constants: word 0 of limb j of the streams seed + 6450 + 100 t (a_t), seed + 8150 + 100 t (b_t), t = 1 .. T, and
    seed + 9850 (k); const None where the key is 0"""
    ids = list(range(ell))
    word0 = lambda s: [int(v) for v in o.fill_uniform(ids, seed + s)[:, 0]]
    re = [word0(RE_STREAM + STRIDE * t) for t in range(1, T + 1)]
    im = [word0(IM_STREAM + STRIDE * t) for t in range(1, T + 1)]
    return re, im, word0(CONST_STREAM) if cl_const else None


def assert_ct(got, exp, what):
    assert np.array_equal(got[0], exp[0]), (what, "c0")
    assert np.array_equal(got[1], exp[1]), (what, "c1")


# ---- real data (tests/toy_ckks.py): sum_t (a_t + b_t X^(N/2)) m_t + c at scale Delta = 2^40
REAL_SCALARS, REAL_CONST, DELTA = [(3, -2), (1, 5)], 7, 1 << 40
# Bound per coefficient of the decrypted output (derived as lincomb_ref's): the op is linear and meets no key, and the monomial only permutes and
# negates coefficients, so Dec(out) - exact = sum_t (a_t e_t + b_t X^(N/2) e_t) with e_t the errors of the fresh inputs, each coefficient of which is
# at most FRESH_BOUND (8 sigma): at most sum_t (|a_t| + |b_t|) FRESH_BOUND
REAL_BOUND = sum(abs(a) + abs(b) for a, b in REAL_SCALARS) * FRESH_BOUND


def times_monomial(m):
    """X^(N/2) m in the ring: coefficient i goes to i + N/2, and wraps round X^N = -1 with a minus sign"""
    h = len(m) // 2
    return np.concatenate([-m[h:], m[:h]])


def real_case(toy, ell):
    """T = 2 fresh toy ciphertexts of small messages m_t Delta (|m_t| < 50), small signed scalars stored as q_j - |s| when negative, the constant
    k_j = c Delta mod q_j, and the exact result sum_t (a_t m_t + b_t X^(N/2) m_t) Delta + c Delta X^0"""
    ms = [toy.rng.integers(-50, 50, toy.N).astype(object) for _ in REAL_SCALARS]
    cts = [toy.encrypt(m * DELTA, ell) for m in ms]
    re = [[a % int(toy.o.moduli[j]) for j in range(ell)] for a, _ in REAL_SCALARS]
    im = [[b % int(toy.o.moduli[j]) for j in range(ell)] for _, b in REAL_SCALARS]
    const = [REAL_CONST * DELTA % int(toy.o.moduli[j]) for j in range(ell)]
    exact = sum(a * m + b * times_monomial(m) for (a, b), m in zip(REAL_SCALARS, ms)) * DELTA
    exact[0] += REAL_CONST * DELTA
    return cts, re, im, const, exact


def decryption_error(toy, out, ell, exact):
    """max |Dec(out) - exact|"""
    got, _ = toy.decrypt(np.stack(out), ell)
    assert max(abs(int(g)) for g in got) > 1 << 30   # a signal, not zeros
    return max(abs(int(g) - int(e)) for g, e in zip(got, exact))


_REAL = {}


def real_reference(logN=13, L=6, ell=5, alpha=2, seed=4259):
    """the real-data case and its reference, computed once per process: (oracle, toy, cts, re, im, const, out, exact)"""
    key = (logN, L, ell, alpha, seed)
    if key not in _REAL:
        from oracle.homoracle import Oracle
        from toy_ckks import Toy
        orc = Oracle(logN, L, alpha)
        orc.set_threads(8)
        toy = Toy(orc, seed=seed)
        cts, re, im, const, exact = real_case(toy, ell)
        _REAL[key] = (orc, toy, cts, re, im, const, clincomb(orc, ell, cts, re, im, const), exact)
    return _REAL[key]
