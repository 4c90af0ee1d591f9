"""The CPU reference of hplincomb (tests/plincomb_ref.py), pinned without a GPU at N = 2^13, l = 3, on both chains: it is the definition in Python
integers; T = 1 without the addend is the oracle's pmult bit for bit; with every plaintext the constant polynomial s_t it is lincomb_ref; with
rescale it is the oracle's rescale of the sum; and on real data (tests/toy_ckks.py) it decrypts to sum_t p_t m_t + p_0, the negacyclic product in
Python integers, within the derived bound."""
import numpy as np
import pytest

from homulator_amd import host
from oracle.homoracle import Oracle
from plincomb_ref import (REAL_BOUND, assert_ct, constant_plaintext, decryption_error, plincomb, plincomb_integers, pt_stream, real_reference,
                          synthetic_plaintexts)
from lincomb_ref import lincomb, synthetic_inputs
import lincomb_ref

LOGN, ELL = 13, 3
CHAINS = ["mont32", "survey"]


@pytest.fixture(scope="module", params=CHAINS)
def o(request):
    orc = Oracle(LOGN, 4, 2, chain=request.param)
    orc.set_threads(8)
    return orc


@pytest.mark.parametrize("T,pa", [(1, 0), (3, 1), (4, 0), (16, 1)])
def test_it_is_the_definition_in_python_integers(o, T, pa):
    cts = synthetic_inputs(o, ELL, host.SEED, T)
    pts, addend = synthetic_plaintexts(o, ELL, host.SEED, T, pa)
    got = plincomb(o, ELL, cts, pts, addend)
    cols = list(range(24)) + list(range(o.N // 2 - 12, o.N // 2 + 12)) + list(range(o.N - 16, o.N))
    for k in range(2):
        for j in range(ELL):
            assert [int(got[k][j][x]) for x in cols] == plincomb_integers(o, cts, pts, addend, k, j, cols), (T, pa, k, j)
            assert int(got[k][j].max()) < o.moduli[j]
    if pa:     # the addend goes on c0 only
        plain = plincomb(o, ELL, cts, pts, None)
        assert np.array_equal(plain[1], got[1]) and not np.array_equal(plain[0], got[0])


def test_one_term_without_the_addend_is_the_oracles_pmult(o):
    ct = synthetic_inputs(o, ELL, host.SEED, 1)[0]
    pt = o.fill_uniform(list(range(ELL)), host.SEED + pt_stream(1))
    assert_ct(plincomb(o, ELL, [ct], [pt]), o.pmult(ELL, ct, pt), "pmult")
    # ... and pmult's own synthetic plaintext (stream seed + 4000) serves as well as any
    pt = o.fill_uniform(list(range(ELL)), host.SEED + 4000)
    assert_ct(plincomb(o, ELL, [ct], [pt]), o.pmult(ELL, ct, pt), "pmult, its own plaintext")


@pytest.mark.parametrize("T,const", [(1, 0), (4, 1), (16, 0)])
def test_with_constant_plaintexts_it_is_lincomb_ref(o, T, const):
    cts = synthetic_inputs(o, ELL, host.SEED, T)
    scales, k = lincomb_ref.synthetic_constants(o, ELL, host.SEED, T, const)
    pts = [constant_plaintext(o, ELL, s) for s in scales]
    addend = constant_plaintext(o, ELL, k) if const else None
    assert_ct(plincomb(o, ELL, cts, pts, addend), lincomb(o, ELL, cts, scales, k), "constant plaintexts")


def test_with_rescale_it_is_the_oracles_rescale_of_the_sum(o):
    cts = synthetic_inputs(o, ELL, host.SEED, 4)
    pts, addend = synthetic_plaintexts(o, ELL, host.SEED, 4, 1)
    plain = plincomb(o, ELL, cts, pts, addend)
    got = plincomb(o, ELL, cts, pts, addend, rescale=True)
    assert got[0].shape == (ELL - 1, o.N)
    assert_ct(got, (o.rescale(ELL, plain[0]), o.rescale(ELL, plain[1])), "rescale")


def test_reference_on_real_data_decrypts_to_the_plaintext_weighted_sum():
    _, toy, _, _, _, out, exact = real_reference()
    err = decryption_error(toy, out, 5, exact)
    print(f"reference: max |dec - exact| = {err} (bound {REAL_BOUND})")
    assert REAL_BOUND == 12 * lincomb_ref.FRESH_BOUND == 312
    assert err <= REAL_BOUND
