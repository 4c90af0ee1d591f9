"""CPU reference of hreim from oracle primitives only, following the definition literally and independent of the host plan:
conj = Oracle.hrotate(ell, ct, 2N - 1, evk), then per component Oracle.ewe ADD, SUB and MUL by U, the oracle's NTT of the polynomial whose
coefficient N/2 is q_j - 1 (that is -X^(N/2)).  Nothing here comes from the code under test."""
import numpy as np

from oracle.homoracle import EWE_ADD, EWE_MUL, EWE_SUB

KEY_STREAM = 10000         # hrotate's key: stream seed + 10 000
FRESH_BOUND = 26           # tests/lincomb_ref.py: 8 sigma of a fresh toy ciphertext's error, rounded up
# Bound per coefficient on both decrypted outputs (derived, not tuned): out = ct + conj and out_im = -X^(N/2) (ct - conj) are linear in ct and
# conj, and the monomial only permutes and negates coefficients.  So each error is at most the error of conj = hrotate(ct), bounded by 2^16 in
# tests/test_gpu_real_data.py, plus the fresh error of ct itself, at most FRESH_BOUND: 2^16 + 26 < 2^17.
REAL_BOUND = 1 << 17


def unit(o, ids):
    """U_j = NTT_{q_j}(-X^(N/2)) for the limbs `ids`: [len(ids)][N]"""
    p = np.zeros((len(ids), o.N), dtype=np.uint64)
    for r, m in enumerate(ids):
        p[r][o.N // 2] = o.moduli[m] - 1
    return o.ntt(ids, p)


def split(o, ids, x, y):
    """(x + y, U (.) (x - y)) per limb, by the oracle's element-wise primitives"""
    return o.ewe(EWE_ADD, ids, x, None, y), o.ewe(EWE_MUL, ids, o.ewe(EWE_SUB, ids, x, None, y), unit(o, ids))


def reim(o, ell, ct, evk):
    """ct [2][ell][N] at level ell, evk the conjugation key [beta][2][ell + K][N].  Returns (out, out_im, conj), each [2][ell][N]"""
    ids = list(range(ell))
    conj = o.hrotate(ell, ct, 2 * o.N - 1, evk)
    parts = [split(o, ids, ct[k], conj[k]) for k in range(2)]
    return np.stack([parts[0][0], parts[1][0]]), np.stack([parts[0][1], parts[1][1]]), conj


def split_integers(o, j, x, y, cols):
    """the definition in Python integers for limb j and the entries `cols`: w = -psi^(N/2) on [0, N/2), q - w on [N/2, N)"""
    q = o.moduli[j]
    w = q - pow(o.psis[j], o.N // 2, q)
    return ([(int(x[e]) + int(y[e])) % q for e in cols],
            [(w if e < o.N // 2 else q - w) * (int(x[e]) - int(y[e])) % q for e in cols])


def synthetic_input(o, ell, seed, copy=0, batch_seed_stride=100000):
    """the op's synthetic streams: ct1 from seed (c1: + 1000), the key from seed + 10 000; op `copy` of a batch draws ct1 from + copy * stride"""
    return o.synth_ct(ell, seed + copy * batch_seed_stride), o.synth_evk(ell, seed + KEY_STREAM)


def assert_ct(got, exp, what):
    assert np.array_equal(got[0], exp[0]), (what, "c0")
    assert np.array_equal(got[1], exp[1]), (what, "c1")


# ---- real data (tests/toy_ckks.py)
def real_case(toy, ell):
    """m = integers in (-1000, 1000) times 2^30, a fresh encryption of it, the conjugation key gen_evk(automorph(s, 2N - 1)) at the level, and the
    two exact results m + sigma(m) and -X^(N/2) (m - sigma(m))"""
    N = toy.N
    g = 2 * N - 1
    evk = toy.evk_at_level(toy.gen_evk(toy.automorph(toy.s, g)), ell)
    m = toy.rng.integers(-999, 1000, N).astype(object) * (1 << 30)
    ct = toy.encrypt(m, ell)
    sm = toy.automorph(m, g)
    d = m - sm
    # -X^(N/2) d: coefficient i goes to i + N/2 with a minus sign, and wraps round X^N = -1 with a plus sign
    im = np.concatenate([d[N // 2:], -d[:N // 2]])
    return ct, evk, m + sm, im


def decryption_errors(toy, out, out_im, ell, exact_re, exact_im):
    """max |Dec(out) - exact_re|, max |Dec(out_im) - exact_im|"""
    errs = []
    for ct, exact in ((out, exact_re), (out_im, exact_im)):
        got, _ = toy.decrypt(np.stack(ct), ell)
        assert max(abs(int(g)) for g in got) > 1 << 30   # a signal, not zeros
        errs.append(max(abs(int(g) - int(e)) for g, e in zip(got, exact)))
    return errs


_REAL = {}


def real_reference(logN=13, L=6, ell=5, alpha=2, seed=4253):
    """the real-data case and its reference, computed once per process: (oracle, toy, ct, evk, out, out_im, exact_re, exact_im)"""
    key = (logN, L, ell, alpha, seed)
    if key not in _REAL:
        from oracle.homoracle import Oracle
        from toy_ckks import Toy
        orc = Oracle(logN, L, alpha)
        orc.set_threads(8)
        toy = Toy(orc, seed=seed)
        ct, evk, exact_re, exact_im = real_case(toy, ell)
        out, out_im, _ = reim(orc, ell, ct, evk)
        _REAL[key] = (orc, toy, ct, evk, out, out_im, exact_re, exact_im)
    return _REAL[key]
