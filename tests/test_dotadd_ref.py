"""The CPU reference of hdotadd (tests/dotadd_ref.py), pinned without a GPU at N = 2^13, l = 3, on both chains: without addends and constants it is
the reference of hdot; with one pair it is the reference of hmuladd with the same constants; with one pair and nothing else it is the oracle's hmult;
an addend with a zero scalar is an addend dropped; scalars that are all 1 are no scalars; its three polynomials are the definition in Python integers;
and on real data (tests/toy_ckks.py) it decrypts to 3 m1 m2 - 2 m3 m4 + 5 m5 + 7 within the bound derived in tests/dotadd_ref.py."""
import numpy as np
import pytest

from dot_ref import dot
from dotadd_ref import (decryption_error, dotadd, dotadd_integers, dotadd_tensor, real_case, synthetic_constants, synthetic_inputs)
from homulator_amd import host
from muladd_ref import muladd
from oracle.homoracle import Oracle

LOGN = 13
CHAINS = ["mont32", "survey"]
ELL = 3


@pytest.fixture(scope="module", params=CHAINS)
def o(request):
    orc = Oracle(LOGN, 4, 2, chain=request.param)
    orc.set_threads(8)
    return orc


def same(a, b):
    return np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


def test_without_addends_and_constants_it_is_the_reference_of_hdot(o):
    for T in (1, 3):
        pairs, _, evk = synthetic_inputs(o, ELL, host.SEED, T, 0)
        assert same(dotadd(o, ELL, pairs, evk), dot(o, ELL, [ct for p in pairs for ct in p], evk)), T


def test_with_one_pair_it_is_the_reference_of_hmuladd(o):
    pairs, adds, evk = synthetic_inputs(o, ELL, host.SEED, 1, 2)
    scales, us, const = synthetic_constants(o, ELL, host.SEED, 1, 2, 1, 1)
    for s, n, k in ((None, 0, None), (scales, 2, const), (None, 1, const), (scales, 2, None)):
        exp = muladd(o, ELL, pairs[0][0], pairs[0][1], evk, adds[:n], None if s is None else s[0], us[:n], k)
        assert same(dotadd(o, ELL, pairs, evk, adds[:n], s, us[:n], k), exp), (n, s is None, k is None)


def test_with_one_pair_and_nothing_else_it_is_the_oracles_hmult(o):
    pairs, _, evk = synthetic_inputs(o, ELL, host.SEED, 1, 0)
    assert same(dotadd(o, ELL, pairs, evk), o.hmult(ELL, pairs[0][0], pairs[0][1], evk, rescale=True))


def test_a_zero_scalar_is_an_addend_dropped(o):
    pairs, adds, evk = synthetic_inputs(o, ELL, host.SEED, 2, 2)
    scales, us, const = synthetic_constants(o, ELL, host.SEED, 2, 2, 1, 1)
    exp = dotadd(o, ELL, pairs, evk, adds[:1], scales, us[:1], const)
    assert same(dotadd(o, ELL, pairs, evk, adds, scales, [us[0], [0] * ELL], const), exp)
    other = dotadd(o, ELL, pairs, evk, adds, scales, us, const)             # ... and a nonzero one is not
    assert not np.array_equal(other[0], exp[0]) and not np.array_equal(other[1], exp[1])


def test_scalars_that_are_all_one_are_no_scalars(o):
    pairs, adds, evk = synthetic_inputs(o, ELL, host.SEED, 2, 1)
    _, us, const = synthetic_constants(o, ELL, host.SEED, 2, 1, 0, 1)
    assert same(dotadd(o, ELL, pairs, evk, adds, [[1] * ELL] * 2, us, const), dotadd(o, ELL, pairs, evk, adds, None, us, const))


def test_the_constants_act_as_defined(o):
    ids = list(range(ELL))
    pairs, adds, _ = synthetic_inputs(o, ELL, host.SEED, 3, 3)
    scales, us, const = synthetic_constants(o, ELL, host.SEED, 3, 3, 1, 1)
    assert all(1 <= s < o.moduli[j] for sc in scales for j, s in enumerate(sc)) and all(0 <= k < o.moduli[j] for j, k in enumerate(const))
    assert scales[1] == [int(o.fill_uniform(ids, host.SEED + 6150)[j][0]) or 1 for j in ids]
    assert us[2] == [int(o.fill_uniform(ids, host.SEED + 7200)[j][0]) for j in ids]
    assert const == [int(o.fill_uniform(ids, host.SEED + 7900)[j][0]) for j in ids]
    cols = list(range(64)) + [o.N - 1]
    for T, s, u, k, n in ((1, None, [], None, 0), (3, scales, us, const, 3), (2, None, us[:1], const, 1), (3, scales, us[:2], None, 2)):
        d = dotadd_tensor(o, ids, pairs[:T], adds[:n], s, u, k)
        for j in ids:       # against Python integers on a stretch of every limb
            e = dotadd_integers(o, pairs[:T], adds[:n], s, u, k, j, cols)
            for i in range(3):
                assert [int(d[i][j][x]) for x in cols] == e[i], (T, n, j, i)


def test_reference_on_real_data_decrypts_within_the_bound():
    from toy_ckks import Toy
    L, ELL5, ALPHA = 6, 5, 2
    orc = Oracle(LOGN, L, ALPHA)
    orc.set_threads(8)
    toy = Toy(orc, seed=4251)
    cts, evk, scales, u, const, exact = real_case(toy, ELL5)
    out = dotadd(orc, ELL5, [(cts[0], cts[1]), (cts[2], cts[3])], evk, [cts[4]], scales, [u], const)
    err, bound = decryption_error(toy, out, ELL5, exact)
    print(f"reference: max |dec q_4 - exact| = 2^{err.bit_length()} (bound 2^{bound.bit_length() - 1})")
    assert err <= bound
