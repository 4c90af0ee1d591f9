"""The CPU reference of hlincomb (tests/lincomb_ref.py), pinned without a GPU at N = 2^13, l = 3, on both chains: it is the definition in Python
integers, the identity at T = 1 with s = 1, the oracle's hadd at T = 2 with s = (1, 1), a zero scalar drops its term, with rescale it is the oracle's
rescale of the sum, and on real data (tests/toy_ckks.py) it decrypts to sum_t s_t m_t + c."""
import numpy as np
import pytest

from homulator_amd import host
from oracle.homoracle import Oracle
from lincomb_ref import assert_ct, decryption_error, lincomb, lincomb_integers, real_case, synthetic_constants, synthetic_inputs

LOGN, ELL = 13, 3
CHAINS = ["mont32", "survey"]


@pytest.fixture(scope="module", params=CHAINS)
def o(request):
    orc = Oracle(LOGN, 4, 2, chain=request.param)
    orc.set_threads(8)
    return orc


@pytest.mark.parametrize("T,lc", [(1, 0), (3, 1), (4, 0), (16, 1)])
def test_it_is_the_definition_in_python_integers(o, T, lc):
    cts = synthetic_inputs(o, ELL, host.SEED, T)
    scales, const = synthetic_constants(o, ELL, host.SEED, T, lc)
    assert all(0 <= s[j] < o.moduli[j] for s in scales for j in range(ELL))
    got = lincomb(o, ELL, cts, scales, const)
    cols = list(range(48)) + list(range(o.N - 16, o.N))
    for k in range(2):
        for j in range(ELL):
            assert [int(got[k][j][x]) for x in cols] == lincomb_integers(o, ELL, cts, scales, const, k, j, cols), (T, lc, k, j)
            assert int(got[k][j].max()) < o.moduli[j]
    if lc:     # the constant goes on c0 only, on every entry
        plain = lincomb(o, ELL, cts, scales, None)
        assert np.array_equal(plain[1], got[1]) and not np.array_equal(plain[0], got[0])


def test_one_term_with_scalar_one_is_the_identity(o):
    ct = synthetic_inputs(o, ELL, host.SEED, 1)
    assert_ct(lincomb(o, ELL, ct, [[1] * ELL]), ct[0], "identity")
    assert_ct(lincomb(o, ELL, ct, [[1] * ELL], [0] * ELL), ct[0], "identity, k = 0")


def test_two_terms_with_scalars_one_are_the_oracles_hadd(o):
    a, b = synthetic_inputs(o, ELL, host.SEED, 2)
    assert_ct(lincomb(o, ELL, [a, b], [[1] * ELL] * 2), o.hadd(ELL, a, b), "hadd")


def test_a_zero_scalar_drops_its_term(o):
    cts = synthetic_inputs(o, ELL, host.SEED, 3)
    scales, const = synthetic_constants(o, ELL, host.SEED, 3, 1)
    scales[1] = [0] * ELL
    assert_ct(lincomb(o, ELL, cts, scales, const), lincomb(o, ELL, [cts[0], cts[2]], [scales[0], scales[2]], const), "zero")


def test_with_rescale_it_is_the_oracles_rescale_of_the_sum(o):
    cts = synthetic_inputs(o, ELL, host.SEED, 4)
    scales, const = synthetic_constants(o, ELL, host.SEED, 4, 1)
    plain = lincomb(o, ELL, cts, scales, const)
    got = lincomb(o, ELL, cts, scales, const, rescale=True)
    assert got[0].shape == (ELL - 1, o.N)
    assert_ct(got, (o.rescale(ELL, plain[0]), o.rescale(ELL, plain[1])), "rescale")


def test_reference_on_real_data_decrypts_to_the_linear_combination():
    from toy_ckks import Toy
    L, ell, ALPHA = 6, 5, 2
    orc = Oracle(LOGN, L, ALPHA)
    orc.set_threads(8)
    toy = Toy(orc, seed=4247)
    cts, scales, const, exact = real_case(toy, ell)
    err, bound = decryption_error(toy, lincomb(orc, ell, cts, scales, const), ell, exact)
    print(f"reference: max |dec - exact| = {err} (bound {bound})")
    assert err <= bound
