"""tests/rescale_ref.py (the CPU reference the rescale GPU tests compare against) against a recomputation in the coefficient domain with Python
integers: out_i = (x_i - [x]_{q_last}) * q_last^-1 mod q_i with [.] taken in [0, q_last), at N = 2^13, l = 3 and l = 2, on both chains, for every
helper including the identity forms.  No GPU."""
import numpy as np
import pytest

from oracle.homoracle import Oracle
from bsgs_ref import bsgs, synthetic_inputs as bsgs_inputs
from identity_ref import bsgs_id, bsgs_id_inputs, lintrans_id
from lintrans_ref import lintrans
from rescale_ref import bsgs_rescaled, lintrans_rescaled, pmult_rescaled, rescale_ct, rotsum_rescaled
from rotsum_ref import rotsum, synthetic_inputs as rotsum_inputs

LOGN, L, ALPHA = 13, 3, 2
_oracles = {}


def oracle(chain):
    if chain not in _oracles:
        _oracles[chain] = Oracle(LOGN, L, ALPHA, chain=chain)
        _oracles[chain].set_threads(8)
    return _oracles[chain]


def rescale_int(o, ell, x):
    """the rescale of one polynomial ([ell][N], evaluation form) from its definition, with Python integers in the coefficient domain"""
    Q = list(range(ell))
    coef = [c.astype(object) for c in o.ntt(Q, x, inverse=True)]
    qlast = o.moduli[ell - 1]
    rows = []
    for i in range(ell - 1):
        q = o.moduli[i]
        inv = pow(qlast % q, -1, q)
        rows.append(np.array([int((int(a) - int(r)) * inv % q) for a, r in zip(coef[i], coef[ell - 1])], dtype=np.uint64))   # r in [0, q_last)
    return o.ntt(Q[:ell - 1], np.stack(rows))


def check(o, ell, got, unrescaled):
    assert got[0].shape == got[1].shape == (ell - 1, o.N)
    for k in range(2):
        assert np.array_equal(got[k], rescale_int(o, ell, unrescaled[k])), k


@pytest.mark.parametrize("chain", ["mont32", "survey"])
@pytest.mark.parametrize("ell", [3, 2])
def test_helpers_against_integer_recomputation(chain, ell):
    o, g, R, G = oracle(chain), 5, 2, 2
    ids = o.ext_ids(ell)
    ct = o.synth_ct(ell, 91)
    check(o, ell, rescale_ct(o, ell, ct), ct)
    pt = o.fill_uniform(ids[:ell], 17)
    check(o, ell, pmult_rescaled(o, ell, ct, pt), o.pmult(ell, ct, pt))
    keys = [o.synth_evk(ell, 7000 + 100000 * r) for r in range(1, R + 1)]
    pts = [o.fill_uniform(ids, 300 + r) for r in range(R)]
    pt0 = o.fill_uniform(ids, 299)
    check(o, ell, lintrans_rescaled(o, ell, ct, g, keys, pts), lintrans(o, ell, ct, g, keys, pts))
    check(o, ell, lintrans_rescaled(o, ell, ct, g, keys, pts, pt0), lintrans_id(o, ell, ct, g, keys, pts, pt0))
    cts, rkeys = rotsum_inputs(o, ell, G, 55)
    check(o, ell, rotsum_rescaled(o, ell, cts, g, rkeys), rotsum(o, ell, cts, g, rkeys))
    bct, bk, gk, bpts = bsgs_inputs(o, ell, R, G, 77)
    h = pow(g, R, 2 * o.N)
    check(o, ell, bsgs_rescaled(o, ell, bct, g, h, bk, gk, bpts), bsgs(o, ell, bct, g, h, bk, gk, bpts))
    pt0s, ptgs = bsgs_id_inputs(o, ell, R, G, 77)
    h1 = pow(g, R + 1, 2 * o.N)
    check(o, ell, bsgs_rescaled(o, ell, bct, g, h1, bk, gk, bpts, pt0s, ptgs), bsgs_id(o, ell, bct, g, h1, bk, gk, bpts, pt0s, ptgs))


def test_the_zero_polynomial_and_the_largest_residues():
    """all zero stays zero; every residue q_i - 1 (the constant -1 in evaluation form on every limb): x = -1 on all limbs, [x]_{q_last} = q_last - 1,
    so out_i = (-1 - (q_last - 1)) / q_last = -1"""
    o, ell = oracle("mont32"), 3
    zero = np.zeros((ell, o.N), dtype=np.uint64)
    assert not rescale_ct(o, ell, (zero, zero))[0].any()
    top = np.stack([np.full(o.N, o.moduli[i] - 1, dtype=np.uint64) for i in range(ell)])
    got = rescale_ct(o, ell, (top, top))
    assert np.array_equal(got[0], top[:ell - 1]) and np.array_equal(got[1], rescale_int(o, ell, top))
