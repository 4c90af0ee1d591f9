"""The CPU reference of hreim (tests/reim_ref.py), pinned without a GPU at N = 2^13, l = 3, on both chains: U, the oracle's transform of -X^(N/2),
is two constant halves w, q - w with w^2 = -1; the element-wise part is the definition in Python integers; out + (q - U) (.) out_im is 2 ct1 bit for
bit; out is the oracle's hrotate by 2N - 1 plus ct1; and on real data (tests/toy_ckks.py) the two outputs decrypt to m + sigma(m) and
-X^(N/2) (m - sigma(m)) inside the derived bound 2^17."""
import numpy as np
import pytest

from homulator_amd import host
from oracle.homoracle import EWE_ADD, EWE_MUL, Oracle
from reim_ref import REAL_BOUND, assert_ct, decryption_errors, real_reference, reim, split_integers, synthetic_input, unit

LOGN, ELL = 13, 3
CHAINS = ["mont32", "survey"]


@pytest.fixture(scope="module", params=CHAINS)
def o(request):
    orc = Oracle(LOGN, 4, 2, chain=request.param)
    orc.set_threads(8)
    return orc


@pytest.fixture(scope="module")
def case(o):
    ct, evk = synthetic_input(o, ELL, host.SEED)
    return (ct,) + tuple(reim(o, ELL, ct, evk))


def test_unit_is_two_constant_halves_that_sum_to_q_and_square_to_minus_one(o):
    ids = list(range(o.L + o.K))     # every modulus of the chain, the special primes too
    U = unit(o, ids)
    for j in ids:
        q, h = o.moduli[j], o.N // 2
        w = int(U[j][0])
        assert np.all(U[j][:h] == np.uint64(w)) and np.all(U[j][h:] == np.uint64(q - w)), j
        assert 0 < w < q and w * w % q == q - 1, j
        assert w == q - pow(o.psis[j], h, q), j


def test_the_elementwise_part_is_the_definition_in_python_integers(o, case):
    ct, out, out_im, conj = case
    h = o.N // 2
    cols = list(range(24)) + list(range(h - 12, h + 12)) + list(range(o.N - 12, o.N))
    for k in range(2):
        for j in range(ELL):
            re, im = split_integers(o, j, ct[k][j], conj[k][j], cols)
            assert [int(out[k][j][e]) for e in cols] == re, (k, j)
            assert [int(out_im[k][j][e]) for e in cols] == im, (k, j)
            assert int(out[k][j].max()) < o.moduli[j] and int(out_im[k][j].max()) < o.moduli[j]


def test_real_part_plus_the_rotated_imaginary_part_is_twice_the_input(o, case):
    """(x + y) + X^(N/2) (-X^(N/2)) (x - y) = 2 x, with X^(N/2) = q - U in evaluation form"""
    ct, out, out_im, _ = case
    ids = list(range(ELL))
    U = unit(o, ids)
    neg = np.stack([np.uint64(o.moduli[j]) - U[j] for j in ids])
    for k in range(2):
        got = o.ewe(EWE_ADD, ids, out[k], None, o.ewe(EWE_MUL, ids, out_im[k], neg))
        assert np.array_equal(got, o.ewe(EWE_ADD, ids, ct[k], None, ct[k])), k


def test_the_real_part_is_the_oracles_conjugation_plus_the_input(o, case):
    ct, out, _, conj = case
    _, evk = synthetic_input(o, ELL, host.SEED)
    assert_ct(conj, o.hrotate(ELL, ct, 2 * o.N - 1, evk), "conj")
    assert_ct(out, o.hadd(ELL, ct, conj), "out")


def test_reference_on_real_data_decrypts_to_both_parts():
    orc, toy, ct, evk, out, out_im, exact_re, exact_im = real_reference()
    ell = ct.shape[1]
    errs = decryption_errors(toy, out, out_im, ell, exact_re, exact_im)
    print(f"reference: max |dec - exact| = {errs[0]} (real), {errs[1]} (imaginary), bound {REAL_BOUND}")
    assert errs[0] < REAL_BOUND and errs[1] < REAL_BOUND
    assert max(abs(int(v)) for v in exact_im) > 1 << 30
