"""The CPU reference of hsquare (tests/square_ref.py), pinned without a GPU at N = 2^13: with both constants absent it is the oracle's hmult of the
ciphertext with itself, its d1 is twice the product, and on real data (tests/toy_ckks.py) one double-angle step 2 y^2 - 1 decrypts correctly."""
import numpy as np
import pytest

from homulator_amd import host
from oracle.homoracle import EWE_MUL, Oracle
from square_ref import decryption_error, real_case, square, square_tensor, synthetic_constants, synthetic_inputs

LOGN = 13
CHAINS = ["mont32", "survey"]


@pytest.fixture(scope="module", params=CHAINS)
def o(request):
    orc = Oracle(LOGN, 4, 2, chain=request.param)
    orc.set_threads(8)
    return orc


def test_without_constants_it_is_the_oracles_hmult_of_the_ciphertext_with_itself(o):
    ell = 3
    ct, evk = synthetic_inputs(o, ell, host.SEED)
    exp = o.hmult(ell, ct, ct, evk, rescale=True)
    got = square(o, ell, ct, evk)
    assert np.array_equal(got[0], exp[0]) and np.array_equal(got[1], exp[1])
    ones = square(o, ell, ct, evk, scale=[1] * ell, const=[0] * ell)     # the neutral constants change nothing
    assert np.array_equal(ones[0], exp[0]) and np.array_equal(ones[1], exp[1])


def test_d1_is_twice_the_product_and_the_constants_act_as_defined(o):
    ell = 3
    ids = list(range(ell))
    ct, _ = synthetic_inputs(o, ell, host.SEED)
    scale, const = synthetic_constants(o, ell, host.SEED, 1, 1)
    assert all(1 <= s < o.moduli[j] for j, s in enumerate(scale)) and all(0 <= k < o.moduli[j] for j, k in enumerate(const))
    assert scale == [int(o.fill_uniform(range(ell), host.SEED + 6000)[j][0]) or 1 for j in ids]
    prod = o.ewe(EWE_MUL, ids, ct[0], ct[1])
    d0, d1, d2 = square_tensor(o, ids, ct[0], ct[1])
    for j in ids:
        q = o.moduli[j]
        assert [int(v) for v in d1[j][:64]] == [2 * int(p) % q for p in prod[j][:64]]
    twice = np.stack([np.where(prod[j] * np.uint64(2) >= np.uint64(o.moduli[j]), prod[j] * np.uint64(2) - np.uint64(o.moduli[j]), prod[j] * np.uint64(2)) for j in ids])
    assert np.array_equal(d1, twice)
    e0, e1, e2 = square_tensor(o, ids, ct[0], ct[1], scale, const)
    for j in ids:       # against Python integers on a stretch of every limb
        q, s, k = o.moduli[j], scale[j], const[j]
        a, c = [int(v) for v in ct[0][j][:64]], [int(v) for v in ct[1][j][:64]]
        assert [int(v) for v in e0[j][:64]] == [(s * x * x + k) % q for x in a]
        assert [int(v) for v in e1[j][:64]] == [2 * s * x * y % q for x, y in zip(a, c)]
        assert [int(v) for v in e2[j][:64]] == [s * y * y % q for y in c]


def test_reference_on_real_data_decrypts_to_the_double_angle_step():
    from toy_ckks import Toy
    L, ELL, ALPHA = 6, 5, 2
    orc = Oracle(LOGN, L, ALPHA)
    orc.set_threads(8)
    toy = Toy(orc, seed=4246)
    ct, evk, scale, const, exact = real_case(toy, ELL)
    err, bound = decryption_error(toy, square(orc, ELL, ct, evk, scale, const), ELL, exact)
    print(f"reference: max |dec q_last - exact| = 2^{err.bit_length()} (bound 2^{bound.bit_length() - 1})")
    assert err <= bound
