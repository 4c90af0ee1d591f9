"""tests/bsgs_ref.py (the CPU reference the hbsgs GPU tests compare against) against a recomputation in the coefficient domain with Python
integers — decompose and extend ONCE, rotate, multiply by the key, weight by the plaintexts, the ModDown by its formula, then the giant step the
same way on the intermediate ciphertexts — and against lintrans + rotsum called separately.  No GPU."""
import numpy as np
import pytest

from oracle.homoracle import Oracle
from bsgs_ref import baby_step, bsgs, synthetic_inputs
from lintrans_ref import lintrans
from rotsum_ref import rotsum

LOGN, L, ALPHA = 10, 5, 2


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


class Ints:
    """the pieces of a key switch on Python integers; polynomials travel as coefficient rows (one object array per modulus)"""

    def __init__(self, o, ell):
        self.o, self.ell, self.ids = o, ell, o.ext_ids(ell)
        self.mod = [o.moduli[m] for m in self.ids]
        self.Q, self.P = self.mod[:ell], self.mod[ell:]

    def to_coef(self, mods, a):
        return [c.astype(object) for c in self.o.ntt(mods, a, inverse=True)]

    def to_eval(self, mods, rows):
        return self.o.ntt(mods, np.stack([np.array([int(x) for x in r], dtype=np.uint64) for r in rows]))

    def digits(self, c1):
        """the extended digits of the coefficient rows c1 (ModUp)"""
        out = []
        for j in range(self.o.beta(self.ell)):
            lo, hi = j * ALPHA, min(self.ell, (j + 1) * ALPHA)
            conv = _convert(c1[lo:hi], self.Q[lo:hi], self.mod)
            out.append([c1[t] if lo <= t < hi else conv[t] for t in range(len(self.ids))])
        return out

    def key_product(self, digits, g, evk):
        """acc_k[e] = sum_j NTT(sigma_g(D_j))[e] * evk[j][k][e] mod q_e: element-wise, in evaluation form (object arrays)"""
        acc = [[np.zeros(self.o.N, dtype=object) for _ in self.ids] for _ in range(2)]
        for j, d in enumerate(digits):
            X = self.to_eval(self.ids, [_automorph_coef(r, g) % q for r, q in zip(d, self.mod)])
            for k in range(2):
                for e, q in enumerate(self.mod):
                    acc[k][e] = (acc[k][e] + X[e].astype(object) * evk[j][k][e].astype(object)) % q
        return acc

    def moddown(self, s_eval):
        """coefficient rows mod Q of ModDown(S), S given in evaluation form as object arrays per extended limb"""
        s = self.to_coef(self.ids, np.stack([np.array([int(x) for x in r], dtype=np.uint64) for r in s_eval]))
        pinv = [pow(_prod(self.P) % q, -1, q) for q in self.Q]
        return [(a - c) * pi % q for a, c, pi, q in zip(s[:self.ell], _convert(s[self.ell:], self.P, self.Q), pinv, self.Q)]


def integer_bsgs(o, ell, ct, g, h, baby, giant, pts):
    z = Ints(o, ell)
    N, R, G = o.N, len(baby), len(giant)
    c0, c1 = z.to_coef(z.ids[:ell], ct[0]), z.to_coef(z.ids[:ell], ct[1])
    D = z.digits(c1)                                         # ONE ModUp
    gs = [pow(g, r, 2 * N) for r in range(1, R + 1)]
    acc = [z.key_product(D, gr, evk) for gr, evk in zip(gs, baby)]      # once per baby rotation
    rc0 = [z.to_eval(z.ids[:ell], [_automorph_coef(c, gr) % q for c, q in zip(c0, z.Q)]) for gr in gs]
    v = []
    for i in range(G):
        S = [[sum(pts[i][r][e].astype(object) * acc[r][k][e] for r in range(R)) % q for e, q in enumerate(z.mod)] for k in range(2)]
        U = [sum(pts[i][r][e].astype(object) * rc0[r][e].astype(object) for r in range(R)) % q for e, q in enumerate(z.Q)]
        Uc = z.to_coef(z.ids[:ell], np.stack([np.array([int(x) for x in r], dtype=np.uint64) for r in U]))
        v.append(([(d + u) % q for d, u, q in zip(z.moddown(S[0]), Uc, z.Q)], z.moddown(S[1])))
    T = [[np.zeros(N, dtype=object) for _ in z.ids] for _ in range(2)]
    V = [np.zeros(N, dtype=object) for _ in z.Q]
    for i, ((vc0, vc1), evk) in enumerate(zip(v, giant), start=1):
        hi = pow(h, i, 2 * N)
        a = z.key_product(z.digits(vc1), hi, evk)
        T = [[(t + x) % q for t, x, q in zip(T[k], a[k], z.mod)] for k in range(2)]
        V = [(s + _automorph_coef(c, hi)) % q for s, c, q in zip(V, vc0, z.Q)]
    out0 = [(d + u) % q for d, u, q in zip(z.moddown(T[0]), V, z.Q)]
    return z.to_eval(z.ids[:ell], out0), z.to_eval(z.ids[:ell], z.moddown(T[1]))


@pytest.mark.parametrize("ell,R,G", [(3, 2, 2), (4, 3, 2), (5, 2, 3)], ids=["beta2-short-last", "beta2", "beta3-one-limb-last"])
def test_reference_helper_against_integer_recomputation(oracle, ell, R, G):
    o, g = oracle, 5
    h = pow(g, R, 2 * o.N)
    ct, baby, giant, pts = synthetic_inputs(o, ell, R, G, 91)
    got = bsgs(o, ell, ct, g, h, baby, giant, pts)
    exp = integer_bsgs(o, ell, ct, g, h, baby, giant, pts)
    assert np.array_equal(got[0], exp[0]) and np.array_equal(got[1], exp[1])


def test_a_giant_element_of_its_own(oracle):
    o, ell, R, G = oracle, 4, 2, 2
    ct, baby, giant, pts = synthetic_inputs(o, ell, R, G, 17)
    got = bsgs(o, ell, ct, 5, 2 * o.N - 1, baby, giant[:1], pts[:1])
    exp = integer_bsgs(o, ell, ct, 5, 2 * o.N - 1, baby, giant[:1], pts[:1])
    assert np.array_equal(got[0], exp[0]) and np.array_equal(got[1], exp[1])


@pytest.mark.parametrize("ell,R,G", [(4, 3, 4), (5, 1, 2), (2, 2, 1)])
def test_equals_lintrans_and_rotsum_called_separately(oracle, ell, R, G):
    """G hlintrans references on ct with the plaintexts pt_{i,.} and the shared baby keys, then one hrotsum reference with galois = h"""
    o, g = oracle, 5
    h = pow(g, R, 2 * o.N)
    ct, baby, giant, pts = synthetic_inputs(o, ell, R, G, 5)
    inner = [lintrans(o, ell, ct, g, baby, pts[i]) for i in range(G)]
    for a, b in zip(inner, baby_step(o, ell, ct, g, baby, pts)):
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    got, exp = bsgs(o, ell, ct, g, h, baby, giant, pts), rotsum(o, ell, inner, h, giant)
    assert np.array_equal(got[0], exp[0]) and np.array_equal(got[1], exp[1])


def test_synthetic_inputs_use_the_op_s_streams(oracle):
    o, ell, R, G, seed = oracle, 3, 2, 3, 1000
    ct, baby, giant, pts = synthetic_inputs(o, ell, R, G, seed, copy=2)
    assert np.array_equal(ct, o.synth_ct(ell, seed + 200000))
    assert np.array_equal(baby[1], o.synth_evk(ell, seed + 10000 + 200000)) and np.array_equal(giant[2], o.synth_evk(ell, seed + 10000 + 1900000))
    assert np.array_equal(pts[2][1], o.fill_uniform(o.ext_ids(ell), seed + 4000 + 100000 * 6 + 200000))
