"""The CPU reference of hmuladd (tests/muladd_ref.py), pinned without a GPU at N = 2^13, l = 3, on both chains: without addends and constants it is
the oracle's hmult; with ct2 = ct1 and no addends it is the reference of hsquare (tests/square_ref.py) with the same constants; an addend with a zero
scalar is an addend dropped; its three polynomials are the definition in Python integers; and on real data (tests/toy_ckks.py) an hsquare followed by
an hmuladd evaluates T_3 = 2 T_2 x - x within the bound derived in tests/muladd_ref.py."""
import numpy as np
import pytest

from homulator_amd import host
from muladd_ref import (decryption_error, muladd, muladd_integers, muladd_tensor, real_case, synthetic_constants, synthetic_inputs)
from oracle.homoracle import Oracle
from square_ref import square

LOGN = 13
CHAINS = ["mont32", "survey"]
ELL = 3


@pytest.fixture(scope="module", params=CHAINS)
def o(request):
    orc = Oracle(LOGN, 4, 2, chain=request.param)
    orc.set_threads(8)
    return orc


def test_without_addends_and_constants_it_is_the_oracles_hmult(o):
    ct1, ct2, _, evk = synthetic_inputs(o, ELL, host.SEED, 0)
    exp = o.hmult(ELL, ct1, ct2, evk, rescale=True)
    got = muladd(o, ELL, ct1, ct2, evk)
    assert np.array_equal(got[0], exp[0]) and np.array_equal(got[1], exp[1])
    ones = muladd(o, ELL, ct1, ct2, evk, scale=[1] * ELL, const=[0] * ELL)     # the neutral constants change nothing
    assert np.array_equal(ones[0], exp[0]) and np.array_equal(ones[1], exp[1])


def test_with_ct2_equal_to_ct1_it_is_the_reference_of_hsquare(o):
    ct1, _, _, evk = synthetic_inputs(o, ELL, host.SEED, 0)
    scale, _, const = synthetic_constants(o, ELL, host.SEED, 0, 1, 1)
    for s, k in ((None, None), (scale, None), (None, const), (scale, const)):
        exp = square(o, ELL, ct1, evk, s, k)
        got = muladd(o, ELL, ct1, ct1, evk, scale=s, const=k)
        assert np.array_equal(got[0], exp[0]) and np.array_equal(got[1], exp[1])


def test_a_zero_scalar_is_an_addend_dropped(o):
    ct1, ct2, adds, evk = synthetic_inputs(o, ELL, host.SEED, 2)
    scale, us, const = synthetic_constants(o, ELL, host.SEED, 2, 1, 1)
    exp = muladd(o, ELL, ct1, ct2, evk, adds[:1], scale, us[:1], const)
    got = muladd(o, ELL, ct1, ct2, evk, adds, scale, [us[0], [0] * ELL], const)
    assert np.array_equal(got[0], exp[0]) and np.array_equal(got[1], exp[1])
    other = muladd(o, ELL, ct1, ct2, evk, adds, scale, us, const)             # ... and a nonzero one is not
    assert not np.array_equal(other[0], exp[0]) and not np.array_equal(other[1], exp[1])


def test_the_constants_act_as_defined(o):
    ids = list(range(ELL))
    ct1, ct2, adds, _ = synthetic_inputs(o, ELL, host.SEED, 3)
    scale, us, const = synthetic_constants(o, ELL, host.SEED, 3, 1, 1)
    assert all(1 <= s < o.moduli[j] for j, s in enumerate(scale)) and all(0 <= k < o.moduli[j] for j, k in enumerate(const))
    assert scale == [int(o.fill_uniform(ids, host.SEED + 6400)[j][0]) or 1 for j in ids]
    assert us[1] == [int(o.fill_uniform(ids, host.SEED + 6420)[j][0]) for j in ids]
    assert const == [int(o.fill_uniform(ids, host.SEED + 6490)[j][0]) for j in ids]
    cols = list(range(64)) + [o.N - 1]
    for s, u, k, n in ((None, [], None, 0), (scale, us, const, 3), (None, us[:1], const, 1), (scale, us[:2], None, 2)):
        d = muladd_tensor(o, ids, ct1, ct2, adds[:n], s, u, k)
        for j in ids:       # against Python integers on a stretch of every limb
            e = muladd_integers(o, ct1, ct2, adds[:n], s, u, k, j, cols)
            for i in range(3):
                assert [int(d[i][j][x]) for x in cols] == e[i], (n, j, i)


def test_reference_on_real_data_decrypts_to_t3():
    from toy_ckks import Toy
    L, ELL5, ALPHA = 6, 5, 2
    orc = Oracle(LOGN, L, ALPHA)
    orc.set_threads(8)
    toy = Toy(orc, seed=4247)
    x, evk_full, sq_scale, sq_const, scale, u1, D, exact = real_case(toy, ELL5)
    t2 = square(orc, ELL5, x, toy.evk_at_level(evk_full, ELL5), sq_scale, sq_const)
    x4 = np.ascontiguousarray(x[:, :ELL5 - 1])
    out = muladd(orc, ELL5 - 1, np.stack(t2), x4, toy.evk_at_level(evk_full, ELL5 - 1), [x4], scale, [u1], None)
    err, bound = decryption_error(toy, out, ELL5, D, exact)
    print(f"reference: max |dec q_3 q_4 - exact| = 2^{err.bit_length()} (bound 2^{bound.bit_length() - 1})")
    assert err <= bound
