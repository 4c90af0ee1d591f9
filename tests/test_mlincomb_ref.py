"""The CPU reference of hmlincomb (tests/mlincomb_ref.py), pinned without a GPU at N = 2^13, l = 3, on both chains: it is M calls of the reference of
hlincomb with the op's streams, M = 1 is hlincomb's, a zero scalar row gives the constant alone, with rescale every output is the oracle's rescale of
its sum, and on real data (tests/toy_ckks.py) output m decrypts to sum_t s_{m,t} m_t + 7 within sum_t |s_{m,t}| 26."""
import numpy as np
import pytest

from homulator_amd import host
from oracle.homoracle import Oracle
from lincomb_ref import assert_ct, lincomb, lincomb_integers
from mlincomb_ref import (assert_outputs, const_stream, decryption_errors, mlincomb, real_bounds, real_case, scale_stream, synthetic_constants,
                          synthetic_inputs)

LOGN, ELL = 13, 3
CHAINS = ["mont32", "survey"]


@pytest.fixture(scope="module", params=CHAINS)
def o(request):
    orc = Oracle(LOGN, 4, 2, chain=request.param)
    orc.set_threads(8)
    return orc


@pytest.mark.parametrize("T,M,mc", [(1, 1, 0), (3, 2, 1), (4, 5, 0), (16, 16, 1)])
def test_every_output_is_the_definition_in_python_integers(o, T, M, mc):
    cts = synthetic_inputs(o, ELL, host.SEED, T)
    scales, consts = synthetic_constants(o, ELL, host.SEED, T, M, mc)
    assert len(scales) == M and all(len(row) == T for row in scales) and all(0 <= s[j] < o.moduli[j] for row in scales for s in row for j in range(ELL))
    got = mlincomb(o, ELL, cts, scales, consts)
    cols = list(range(16)) + list(range(o.N - 8, o.N))
    for m in (0, M - 1):
        for k in range(2):
            for j in range(ELL):
                want = lincomb_integers(o, ELL, cts, scales[m], None if consts is None else consts[m], k, j, cols)
                assert [int(got[m][k][j][x]) for x in cols] == want, (T, M, mc, m, k, j)
    if M > 1:   # every output has constants of its own
        assert scales[0] != scales[1] and not np.array_equal(got[0][1], got[1][1])


def test_the_streams_are_the_issues():
    assert scale_stream(host.SEED, 1, 1) == host.SEED + 9150 and scale_stream(host.SEED, 16, 16) == host.SEED + 24900
    assert const_stream(host.SEED, 1) == host.SEED + 9950 and const_stream(host.SEED, 16) == host.SEED + 24950


def test_one_output_is_the_reference_of_hlincomb(o):
    cts = synthetic_inputs(o, ELL, host.SEED, 4)
    scales, consts = synthetic_constants(o, ELL, host.SEED, 4, 1, 1)
    assert_ct(mlincomb(o, ELL, cts, scales, consts)[0], lincomb(o, ELL, cts, scales[0], consts[0]), "M = 1")


def test_a_zero_scalar_row_gives_the_constant_alone(o):
    cts = synthetic_inputs(o, ELL, host.SEED, 3)
    scales, consts = synthetic_constants(o, ELL, host.SEED, 3, 2, 1)
    scales[1] = [[0] * ELL] * 3
    out = mlincomb(o, ELL, cts, scales, consts)[1]
    for j in range(ELL):
        assert np.all(out[0][j] == np.uint64(consts[1][j])) and np.all(out[1][j] == 0)


def test_with_rescale_every_output_is_the_oracles_rescale_of_its_sum(o):
    cts = synthetic_inputs(o, ELL, host.SEED, 4)
    scales, consts = synthetic_constants(o, ELL, host.SEED, 4, 3, 1)
    plain = mlincomb(o, ELL, cts, scales, consts)
    got = mlincomb(o, ELL, cts, scales, consts, rescale=True)
    assert got[0][0].shape == (ELL - 1, o.N)
    assert_outputs(got, [(o.rescale(ELL, p[0]), o.rescale(ELL, p[1])) for p in plain], "rescale")


def test_reference_on_real_data_decrypts_to_the_linear_combinations():
    from toy_ckks import Toy
    L, ell, ALPHA = 6, 5, 2
    orc = Oracle(LOGN, L, ALPHA)
    orc.set_threads(8)
    toy = Toy(orc, seed=4249)
    cts, scales, consts, exact = real_case(toy, ell)
    errs = decryption_errors(toy, mlincomb(orc, ell, cts, scales, consts), ell, exact)
    assert real_bounds() == [156, 286]
    print(f"reference: max |dec - exact| per output = {errs} (bounds {real_bounds()})")
    assert all(e <= b for e, b in zip(errs, real_bounds()))
