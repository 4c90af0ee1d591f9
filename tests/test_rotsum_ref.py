"""tests/rotsum_ref.py (the CPU reference the hrotsum GPU tests compare against) against a recomputation in the coefficient domain with Python
integers — decompose, extend, rotate, multiply by the key, sum, and the ModDown by its formula — and against hoisted_ref at G = 1.  No GPU."""
import numpy as np
import pytest

from oracle.homoracle import Oracle
from hoisted_ref import hoisted_rotations
from rotsum_ref import rotsum

LOGN, L, ALPHA = 11, 5, 2


@pytest.fixture(scope="module")
def oracle():
    o = Oracle(LOGN, L, ALPHA)
    o.set_threads(8)
    return o


def _automorph_coef(a, g):
    """sigma_g in the coefficient domain, explicitly: X^i -> X^(i g mod 2N), with X^N = -1"""
    N = len(a)
    out = np.zeros(N, dtype=object)
    for i in range(N):
        e = i * g % (2 * N)
        out[e % N] = a[i] if e < N else -a[i]
    return out


def _prod(v):
    p = 1
    for x in v:
        p *= x
    return p


def _convert(rows, src, dst):
    """the fast base conversion of the coefficient rows `rows` (one per modulus of `src`) to the moduli `dst`:
    sum_i [x_i (M / m_i)^-1]_{m_i} (M / m_i) mod t — the representative below len(src) M, not M's canonical one"""
    M = _prod(src)
    y = [r * pow(M // m % m, -1, m) % m for r, m in zip(rows, src)]
    return [sum(yi * (M // m) for yi, m in zip(y, src)) % t for t in dst]


@pytest.mark.parametrize("ell,G", [(3, 2), (4, 3), (5, 2)], ids=["beta2-short-last", "beta2", "beta3-one-limb-last"])
def test_reference_helper_against_integer_recomputation(oracle, ell, G):
    o, g = oracle, 5
    N, ids = o.N, o.ext_ids(ell)
    mod = [o.moduli[m] for m in ids]
    Q, P = mod[:ell], mod[ell:]
    cts = [o.synth_ct(ell, 91 + 2000 * i) for i in range(G)]
    keys = [o.synth_evk(ell, 7000 + 100000 * i) for i in range(1, G + 1)]
    got = rotsum(o, ell, cts, g, keys)

    def to_coef(mods, a):
        return [c.astype(object) for c in o.ntt(mods, a, inverse=True)]

    def to_eval(mods, rows):
        return o.ntt(mods, np.stack([np.array([int(x) for x in r], dtype=np.uint64) for r in rows]))

    S = [[np.zeros(N, dtype=object) for _ in ids] for _ in range(2)]
    U = [np.zeros(N, dtype=object) for _ in Q]
    for i, (ct, evk) in enumerate(zip(cts, keys), start=1):
        gi = pow(g, i, 2 * N)
        c1 = to_coef(ids[:ell], ct[1])
        for j in range(o.beta(ell)):
            lo, hi = j * ALPHA, min(ell, (j + 1) * ALPHA)
            conv = _convert(c1[lo:hi], Q[lo:hi], mod)
            digit = [c1[t] if lo <= t < hi else conv[t] for t in range(len(ids))]
            X = to_eval(ids, [_automorph_coef(d, gi) % q for d, q in zip(digit, mod)])
            for k in range(2):
                for e, q in enumerate(mod):   # the key product stays element-wise, in evaluation form, with Python integers
                    S[k][e] = (S[k][e] + X[e].astype(object) * evk[j][k][e].astype(object)) % q
        for e, (c, q) in enumerate(zip(to_coef(ids[:ell], ct[0]), Q)):
            U[e] = (U[e] + _automorph_coef(c, gi)) % q
    pinv = [pow(_prod(P) % q, -1, q) for q in Q]
    exp = []
    for k in range(2):
        s = to_coef(ids, np.stack([np.array([int(x) for x in r], dtype=np.uint64) for r in S[k]]))
        down = [(a - c) * pi % q for a, c, pi, q in zip(s[:ell], _convert(s[ell:], P, Q), pinv, Q)]
        exp.append([d if k else (d + u) % q for d, u, q in zip(down, U, Q)])
    assert np.array_equal(got[0], to_eval(ids[:ell], exp[0])) and np.array_equal(got[1], to_eval(ids[:ell], exp[1]))


def test_one_ciphertext_is_the_hoisted_rotation(oracle):
    o, ell = oracle, 4
    ct = o.synth_ct(ell, 17)
    key = o.synth_evk(ell, 7000 + 100000)
    got = rotsum(o, ell, [ct], 5, [key])
    exp = hoisted_rotations(o, ell, ct, 5, [key])[0]
    assert np.array_equal(got[0], exp[0]) and np.array_equal(got[1], exp[1])
