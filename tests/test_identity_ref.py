"""tests/identity_ref.py (the CPU reference the identity-step GPU tests compare against) at the smallest ring the oracle serves: against a
recomputation in the coefficient domain with Python integers (decompose and extend once, rotate, multiply by the key, weight by the
plaintexts, the ModDown by its formula, then the unrotated products pt_0 * c0 and pt_0 * c1 as negacyclic convolutions), and against
tests/lintrans_ref.py with a zero identity plaintext.  No GPU."""
import numpy as np
import pytest

from oracle.homoracle import Oracle
from bsgs_ref import bsgs, synthetic_inputs
from identity_ref import PT0_STREAM, bsgs_id, bsgs_id_inputs, lintrans_id
from lintrans_ref import lintrans
from test_bsgs_ref import Ints, _automorph_coef

LOGN, L, ALPHA = 10, 5, 2


@pytest.fixture(scope="module")
def oracle():
    o = Oracle(LOGN, L, ALPHA)
    o.set_threads(8)
    return o


def inputs(o, ell, R, seed):
    ids = o.ext_ids(ell)
    return (o.synth_ct(ell, seed), [o.synth_evk(ell, seed + 10000 + 100000 * r) for r in range(1, R + 1)],
            [o.fill_uniform(ids, seed + 4000 + 100000 * r) for r in range(1, R + 1)], o.fill_uniform(ids, seed + PT0_STREAM))


def _negacyclic(a, b, q):
    """a * b in Z_q[X] / (X^N + 1) on Python integers, by the definition"""
    N = len(a)
    full = np.convolve(np.asarray(a, dtype=object), np.asarray(b, dtype=object))   # exact: Python integers, 2N - 1 coefficients
    out = full[:N].copy()
    out[:N - 1] -= full[N:]                                                        # X^N = -1
    return out % q


def integer_lintrans_id(o, ell, ct, g, keys, pts, pt0):
    z = Ints(o, ell)
    N, R, Qids = o.N, len(keys), z.ids[:ell]
    c0, c1 = z.to_coef(Qids, ct[0]), z.to_coef(Qids, ct[1])
    D = z.digits(c1)
    gs = [pow(g, r, 2 * N) for r in range(1, R + 1)]
    acc = [z.key_product(D, gr, evk) for gr, evk in zip(gs, keys)]
    S = [[sum(pts[r][e].astype(object) * acc[r][k][e] for r in range(R)) % q for e, q in enumerate(z.mod)] for k in range(2)]
    p0 = z.to_coef(Qids, pt0[:ell])
    # the identity step: no automorphism, no key — pt_0 * c_k as negacyclic convolutions
    out = [[_negacyclic(p0[e], c[e], q) for e, q in enumerate(z.Q)] for c in (c0, c1)]
    # U's rotated terms, in evaluation form (element-wise), then to coefficients
    rc0 = [z.to_eval(Qids, [_automorph_coef(c, gr) % q for c, q in zip(c0, z.Q)]) for gr in gs]
    U = [sum(pts[r][e].astype(object) * rc0[r][e].astype(object) for r in range(R)) % q for e, q in enumerate(z.Q)]
    Uc = z.to_coef(Qids, np.stack([np.array([int(x) for x in r], dtype=np.uint64) for r in U]))
    d0, d1 = z.moddown(S[0]), z.moddown(S[1])
    out0 = [(d + u + w) % q for d, u, w, q in zip(d0, Uc, out[0], z.Q)]
    out1 = [(d + w) % q for d, w, q in zip(d1, out[1], z.Q)]
    return z.to_eval(Qids, out0), z.to_eval(Qids, out1)


@pytest.mark.parametrize("ell,R", [(3, 1), (4, 3), (5, 2)], ids=["beta2-short-last", "beta2", "beta3-one-limb-last"])
def test_reference_helper_against_integer_recomputation(oracle, ell, R):
    o = oracle
    ct, keys, pts, pt0 = inputs(o, ell, R, 91)
    got = lintrans_id(o, ell, ct, 5, keys, pts, pt0)
    exp = integer_lintrans_id(o, ell, ct, 5, keys, pts, pt0)
    assert np.array_equal(got[0], exp[0]) and np.array_equal(got[1], exp[1])


@pytest.mark.parametrize("ell,R", [(4, 3), (2, 1)])
def test_a_zero_identity_plaintext_gives_lintrans(oracle, ell, R):
    o = oracle
    ct, keys, pts, pt0 = inputs(o, ell, R, 17)
    exp = lintrans(o, ell, ct, 5, keys, pts)
    got = lintrans_id(o, ell, ct, 5, keys, pts, np.zeros_like(pt0))
    assert np.array_equal(got[0], exp[0]) and np.array_equal(got[1], exp[1])
    moved = lintrans_id(o, ell, ct, 5, keys, pts, pt0)                           # ... and a non-zero one moves both components
    assert not np.array_equal(moved[0], exp[0]) and not np.array_equal(moved[1], exp[1])


def test_the_identity_term_is_the_plain_product(oracle):
    """out(identity) - out(no identity) = pt_0[Q] * (c0, c1), element-wise in evaluation form: linearity of everything behind the sums"""
    o, ell, R = oracle, 3, 2
    ct, keys, pts, pt0 = inputs(o, ell, R, 5)
    base, got = lintrans(o, ell, ct, 5, keys, pts), lintrans_id(o, ell, ct, 5, keys, pts, pt0)
    for k in range(2):
        for e in range(ell):
            q = o.moduli[e]
            exp = (base[k][e].astype(object) + pt0[e].astype(object) * ct[k][e].astype(object)) % q
            assert [int(v) for v in got[k][e]] == [int(v) for v in exp]


# ---- hbsgs with the identity steps
def _eval_mul(a, b, q):
    return (a.astype(object) * b.astype(object)) % q


@pytest.mark.parametrize("ell,R,G", [(3, 2, 2), (5, 1, 1)], ids=["beta2-short-last", "beta3-1x1"])
def test_bsgs_id_against_integer_recomputation(oracle, ell, R, G):
    """Python integers: integer_bsgs's pieces (tests/test_bsgs_ref.py) with the unrotated terms added element-wise in evaluation form on exact
    integers, group 0 joining the giant sums in front of the one final ModDown"""
    o, g = oracle, 5
    h = pow(g, R + 1, 2 * o.N)
    ct, baby, giant, pts = synthetic_inputs(o, ell, R, G, 91)
    pt0s, ptgs = bsgs_id_inputs(o, ell, R, G, 91)
    got = bsgs_id(o, ell, ct, g, h, baby, giant, pts, pt0s, ptgs)
    z = Ints(o, ell)
    N, Qids = o.N, z.ids[:ell]
    u64 = lambda rows: np.stack([np.array([int(x) for x in r], dtype=np.uint64) for r in rows])
    c0, c1 = z.to_coef(Qids, ct[0]), z.to_coef(Qids, ct[1])
    D = z.digits(c1)
    gs = [pow(g, r, 2 * N) for r in range(1, R + 1)]
    acc = [z.key_product(D, gr, evk) for gr, evk in zip(gs, baby)]
    rc0 = [z.to_eval(Qids, [_automorph_coef(c, gr) % q for c, q in zip(c0, z.Q)]) for gr in gs]
    S, U, W = [], [], []
    for i in range(G + 1):
        p = pts[i - 1] if i else ptgs
        S.append([[sum(p[r][e].astype(object) * acc[r][k][e] for r in range(R)) % q for e, q in enumerate(z.mod)] for k in range(2)])
        U.append([(_eval_mul(pt0s[i][e], ct[0][e], q) + sum(p[r][e].astype(object) * rc0[r][e].astype(object) for r in range(R))) % q
                  for e, q in enumerate(z.Q)])
        W.append([_eval_mul(pt0s[i][e], ct[1][e], q) for e, q in enumerate(z.Q)])
    coef = lambda rows: z.to_coef(Qids, u64(rows))
    T = [[S[0][k][e] for e in range(len(z.ids))] for k in range(2)]
    V = coef(U[0])
    for i in range(1, G + 1):
        vc0 = [(d + u) % q for d, u, q in zip(z.moddown(S[i][0]), coef(U[i]), z.Q)]
        vc1 = [(d + w) % q for d, w, q in zip(z.moddown(S[i][1]), coef(W[i]), z.Q)]
        hi = pow(h, i, 2 * N)
        a = z.key_product(z.digits(vc1), hi, giant[i - 1])
        T = [[(t + x) % q for t, x, q in zip(T[k], a[k], z.mod)] for k in range(2)]
        V = [(s + _automorph_coef(c, hi)) % q for s, c, q in zip(V, vc0, z.Q)]
    out0 = [(d + u) % q for d, u, q in zip(z.moddown(T[0]), V, z.Q)]
    out1 = [(d + w) % q for d, w, q in zip(z.moddown(T[1]), coef(W[0]), z.Q)]
    assert np.array_equal(got[0], z.to_eval(Qids, out0)) and np.array_equal(got[1], z.to_eval(Qids, out1))


@pytest.mark.parametrize("ell,R,G", [(4, 3, 2), (2, 1, 1)])
def test_bsgs_id_with_zeroed_identity_and_group_0_plaintexts_is_bsgs(oracle, ell, R, G):
    o, g = oracle, 5
    h = pow(g, R + 1, 2 * o.N)
    ct, baby, giant, pts = synthetic_inputs(o, ell, R, G, 17)
    pt0s, ptgs = bsgs_id_inputs(o, ell, R, G, 17)
    zero = lambda v: [np.zeros_like(x) for x in v]
    exp = bsgs(o, ell, ct, g, h, baby, giant, pts)
    got = bsgs_id(o, ell, ct, g, h, baby, giant, pts, zero(pt0s), zero(ptgs))
    assert np.array_equal(got[0], exp[0]) and np.array_equal(got[1], exp[1])
    moved = bsgs_id(o, ell, ct, g, h, baby, giant, pts, pt0s, ptgs)
    assert not np.array_equal(moved[0], exp[0]) and not np.array_equal(moved[1], exp[1])


def test_one_giant_step_reduces_to_lintrans_id_then_a_hoisted_rotation(oracle):
    """G = 1 with ptg* = 0: v_1 = lintrans_id(ct; pt_{1,.}, pt0_1); out = its rotation by h (one key product, one ModDown, tests/rotsum_ref.py
    with one ciphertext) with pt0_0 * (c0, c1) added: to c0 behind the ModDown, and to c1 behind the ModDown"""
    from rotsum_ref import rotsum
    o, ell, R, g = oracle, 4, 2, 5
    h = pow(g, R + 1, 2 * o.N)
    Q = o.ext_ids(ell)[:ell]
    ct, baby, giant, pts = synthetic_inputs(o, ell, R, 1, 5)
    pt0s, ptgs = bsgs_id_inputs(o, ell, R, 1, 5)
    got = bsgs_id(o, ell, ct, g, h, baby, giant, pts, pt0s, [np.zeros_like(x) for x in ptgs])
    v1 = lintrans_id(o, ell, ct, g, baby, pts[0], pt0s[1])
    rot = rotsum(o, ell, [v1], h, giant)
    for k in range(2):
        for e, m in enumerate(Q):
            q = o.moduli[m]
            exp = (rot[k][e].astype(object) + pt0s[0][e].astype(object) * ct[k][e].astype(object)) % q
            assert [int(x) for x in got[k][e]] == [int(x) for x in exp], (k, e)
