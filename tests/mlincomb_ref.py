"""CPU reference of hmlincomb: M calls of the reference of hlincomb (tests/lincomb_ref.py) over the same T ciphertexts, one per
output, with the op's own synthetic streams.  Independent of the host plan."""
import numpy as np

from lincomb_ref import DELTA, FRESH_BOUND, lincomb, synthetic_inputs  # noqa: F401  (synthetic_inputs: the op's inputs are hlincomb's)

BASE, PER_OUTPUT, SCALE_AT, SCALE_STRIDE, CONST_AT = 8000, 1000, 100, 50, 950


def scale_stream(seed, m, t):
    """the stream of s_{m,t}, m and t from 1"""
    return seed + BASE + PER_OUTPUT * m + SCALE_AT + SCALE_STRIDE * t


def const_stream(seed, m):
    return seed + BASE + PER_OUTPUT * m + CONST_AT


def mlincomb(o, ell, cts, scales, consts=None, rescale=False):
    """cts: T ciphertexts [2][ell][N] at level ell; scales[m][t]: ell residues; consts[m]: ell residues, or consts None.  Returns the M outputs
    [(c0, c1)] at level ell, or ell - 1 with rescale"""
    return [lincomb(o, ell, cts, scales[m], None if consts is None else consts[m], rescale) for m in range(len(scales))]


def synthetic_constants(o, ell, seed, T, M, ml_const):
    """the op's synthetic constants: word 0 of limb j of the streams above; consts None where the key is 0"""
    ids = list(range(ell))
    word0 = lambda stream: [int(v) for v in o.fill_uniform(ids, stream)[:, 0]]
    scales = [[word0(scale_stream(seed, m, t)) for t in range(1, T + 1)] for m in range(1, M + 1)]
    consts = [word0(const_stream(seed, m)) for m in range(1, M + 1)] if ml_const else None
    return scales, consts


def assert_outputs(got, exp, what):
    assert len(got) == len(exp), what
    for m, (g, e) in enumerate(zip(got, exp)):
        assert np.array_equal(g[0], e[0]), (what, f"out{m + 1}.c0")
        assert np.array_equal(g[1], e[1]), (what, f"out{m + 1}.c1")


# ---- real data (tests/toy_ckks.py): out_m = sum_t s_{m,t} m_t + 7 at scale Delta = 2^40
REAL_ROWS, REAL_CONST = [[3, -2, 1], [-5, 4, 2]], 7


def real_case(toy, ell):
    """T = 3 fresh toy ciphertexts of small messages m_t Delta (|m_t| < 50), M = 2 rows of small signed integer scalars stored as q_j - |s| when
    negative, the constants k_{m,j} = 7 Delta mod q_j, and per output the exact result (sum_t s_{m,t} m_t) Delta + 7 Delta X^0"""
    ms = [toy.rng.integers(-50, 50, toy.N) for _ in REAL_ROWS[0]]
    cts = [toy.encrypt(m.astype(object) * DELTA, ell) for m in ms]
    scales = [[[s % toy.o.moduli[j] for j in range(ell)] for s in row] for row in REAL_ROWS]
    consts = [[REAL_CONST * DELTA % toy.o.moduli[j] for j in range(ell)] for _ in REAL_ROWS]
    exact = []
    for row in REAL_ROWS:
        e = sum(s * m.astype(object) for s, m in zip(row, ms)) * DELTA
        e[0] += REAL_CONST * DELTA
        exact.append(e)
    return cts, scales, consts, exact


def real_bounds():
    """per output sum_t |s_{m,t}| times the bound of one fresh error (hlincomb's derivation: the op meets no key, so the error of output m is
    sum_t s_{m,t} e_t with e_t = rint(normal(0, 3.2)), and FRESH_BOUND = 26 is 8 sigma rounded up): 156 and 286"""
    return [sum(abs(s) for s in row) * FRESH_BOUND for row in REAL_ROWS]


def decryption_errors(toy, outs, ell, exact):
    """max |Dec(out_m) - exact_m| per output"""
    errs = []
    for out, e in zip(outs, exact):
        got, _ = toy.decrypt(np.stack(out), ell)
        assert max(abs(int(g)) for g in got) > 1 << 30   # a signal, not zeros
        errs.append(max(abs(int(g) - int(x)) for g, x in zip(got, e)))
    return errs
