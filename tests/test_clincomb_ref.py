"""The CPU reference of hclincomb (tests/clincomb_ref.py), pinned without a GPU at N = 2^13, l = 3, on both chains: it is the definition in Python
integers with X^(N/2) the two halves v and q - v, v = psi^(N/2), v^2 = -1; with every b = 0 it is lincomb_ref; i applied twice negates; on reim_ref's
two outputs (1, i) gives back 2 ct1 and (h, i h), h = (q + 1) / 2, gives back ct1; with rescale it is the oracle's rescale of the sum; and on real
data (tests/toy_ckks.py) it decrypts to sum_t (a_t + b_t X^(N/2)) m_t + c within the derived bound."""
import numpy as np
import pytest

from homulator_amd import host
from oracle.homoracle import EWE_ADD, Oracle
from clincomb_ref import (REAL_BOUND, assert_ct, clincomb, clincomb_integers, decryption_error, halves, monomial, real_reference,
                          synthetic_constants)
from lincomb_ref import lincomb, synthetic_inputs
import lincomb_ref
import reim_ref

LOGN, ELL = 13, 3
CHAINS = ["mont32", "survey"]


@pytest.fixture(scope="module", params=CHAINS)
def o(request):
    orc = Oracle(LOGN, 4, 2, chain=request.param)
    orc.set_threads(8)
    return orc


def test_the_monomial_is_two_constant_halves(o):
    mono = monomial(o, list(range(ELL)))
    for j in range(ELL):
        q = int(o.moduli[j])
        v, w = halves(o, j)
        assert v * v % q == q - 1 and w == q - v
        assert (mono[j][:o.N // 2] == v).all() and (mono[j][o.N // 2:] == w).all()


@pytest.mark.parametrize("T,cl", [(1, 0), (3, 1), (4, 0), (16, 1)])
def test_it_is_the_definition_in_python_integers(o, T, cl):
    cts = synthetic_inputs(o, ELL, host.SEED, T)
    re, im, const = synthetic_constants(o, ELL, host.SEED, T, cl)
    assert all(0 <= s[j] < o.moduli[j] for s in re + im for j in range(ELL))
    got = clincomb(o, ELL, cts, re, im, const)
    h = o.N // 2
    cols = list(range(24)) + list(range(h - 12, h + 12)) + list(range(o.N - 16, o.N))
    for k in range(2):
        for j in range(ELL):
            assert [int(got[k][j][x]) for x in cols] == clincomb_integers(o, cts, re, im, const, k, j, cols), (T, cl, k, j)
            assert int(got[k][j].max()) < o.moduli[j]
    if cl:     # the constant goes on c0 only, on every entry
        plain = clincomb(o, ELL, cts, re, im, None)
        assert np.array_equal(plain[1], got[1]) and not np.array_equal(plain[0], got[0])


@pytest.mark.parametrize("T,cl", [(1, 0), (4, 1), (16, 0)])
def test_with_every_b_zero_it_is_lincomb_ref(o, T, cl):
    cts = synthetic_inputs(o, ELL, host.SEED, T)
    re, _, const = synthetic_constants(o, ELL, host.SEED, T, cl)
    assert_ct(clincomb(o, ELL, cts, re, [[0] * ELL] * T, const), lincomb(o, ELL, cts, re, const), "b = 0")


def test_i_applied_twice_negates(o):
    ct = synthetic_inputs(o, ELL, host.SEED, 1)[0]
    zero, one = [[0] * ELL], [[1] * ELL]
    once = np.stack(clincomb(o, ELL, [ct], zero, one))
    twice = clincomb(o, ELL, [once], zero, one)
    assert not np.array_equal(once, ct)
    for k in range(2):
        back = o.ewe(EWE_ADD, list(range(ELL)), twice[k], None, ct[k])
        assert not back.any(), k


def test_it_puts_reims_outputs_back_together(o):
    """hreim gives out = ct + conj and out_im = -i (ct - conj): out + i out_im = 2 ct, and with h = 1/2 mod q, h out + i h out_im = ct bit for bit"""
    ct, evk = reim_ref.synthetic_input(o, ELL, host.SEED)
    out, out_im, _ = reim_ref.reim(o, ELL, ct, evk)
    ids = list(range(ELL))
    one, zero = [1] * ELL, [0] * ELL
    twice = clincomb(o, ELL, [out, out_im], [one, zero], [zero, one])
    assert_ct(twice, [o.ewe(EWE_ADD, ids, ct[k], None, ct[k]) for k in range(2)], "2 ct1")
    h = [(int(o.moduli[j]) + 1) // 2 for j in range(ELL)]
    assert_ct(clincomb(o, ELL, [out, out_im], [h, zero], [zero, h]), ct, "ct1")


def test_with_rescale_it_is_the_oracles_rescale_of_the_sum(o):
    cts = synthetic_inputs(o, ELL, host.SEED, 4)
    re, im, const = synthetic_constants(o, ELL, host.SEED, 4, 1)
    plain = clincomb(o, ELL, cts, re, im, const)
    got = clincomb(o, ELL, cts, re, im, const, rescale=True)
    assert got[0].shape == (ELL - 1, o.N)
    assert_ct(got, (o.rescale(ELL, plain[0]), o.rescale(ELL, plain[1])), "rescale")


def test_reference_on_real_data_decrypts_to_the_complex_combination():
    _, toy, _, _, _, _, out, exact = real_reference()
    err = decryption_error(toy, out, 5, exact)
    print(f"reference: max |dec - exact| = {err} (bound {REAL_BOUND})")
    assert REAL_BOUND == 11 * lincomb_ref.FRESH_BOUND == 286
    assert err <= REAL_BOUND
