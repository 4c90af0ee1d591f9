"""tests/slots_ref.py against itself (CPU, N = 2^13): what follows from the definition of the slot encoding must hold for the
reference before anything is compared with it.  With g = 5^k mod 2N the automorphism X -> X^g rotates the slots left by k, g = 2N - 1 conjugates
them, the monomial X^(N/2) multiplies every slot by i, and the negacyclic product of two encodings decodes at Delta^2 to the slot-wise product.
The automorphism and the product are tests/toy_ckks.py's, on Python integers.

Tolerances are derived, not measured.  Encoding rounds each of the N coefficients by at most 1/2 and every root has modulus 1, so a decoded
slot is off by at most N / 2 / Delta; an automorphism or a monomial only permutes and negates coefficients, which keeps that bound.  For the
product, slot(c1) = Delta z + E1 and slot(c2) = Delta w + E2 with |E| <= N / 2, so the decoded product is off by at most
(|z| + |w|) (N / 2) / Delta + (N / 2)^2 / Delta^2.  SLACK covers the longdouble evaluation itself (N terms of 2^-64 relative each)."""
import numpy as np
import pytest

import slots_ref as R
from oracle.homoracle import Oracle
from toy_ckks import Toy

LOGN = 13
N, n = 1 << LOGN, 1 << (LOGN - 1)
SCALE = 2.0 ** 30
TOL = N / 2 / SCALE
SLACK = 1e-12


@pytest.fixture(scope="module")
def env():
    o = Oracle(LOGN, 3, 1)
    rng = np.random.default_rng(2027)
    z = (rng.uniform(-1, 1, n) + 1j * rng.uniform(-1, 1, n)) / np.sqrt(2)
    return o, Toy(o, seed=5), z, R.encode_int(z, LOGN, SCALE)


def test_the_transform_path_agrees_with_the_definition(env):
    _, _, z, _ = env
    m, mf = R.exact_coeffs(z, LOGN), R.fft_coeffs(z, LOGN)
    assert float(np.abs(m - mf).max()) < 1e-17
    re, im = R.exact_slots(m, LOGN)
    ref, imf = R.fft_slots(m, LOGN)
    assert float(max(np.abs(re - ref).max(), np.abs(im - imf).max())) < 1e-15
    # and decode inverts encode: no rounding in between
    assert float(np.abs(re.astype(np.float64) + 1j * im.astype(np.float64) - z).max()) < 1e-15


def test_encode_then_decode_is_within_the_rounding_bound(env):
    _, _, z, c = env
    assert np.abs(R.decode_int(c, LOGN, SCALE) - z).max() <= TOL + SLACK
    assert np.abs(R.decode_int(c, LOGN, SCALE, R.fft_slots) - z).max() <= TOL + SLACK


@pytest.mark.parametrize("k", [1, 2])
def test_the_automorphism_of_5_to_the_k_rotates_left_by_k(env, k):
    _, toy, z, c = env
    got = R.decode_int(toy.automorph(c, pow(5, k, 2 * N)), LOGN, SCALE, R.fft_slots)
    assert np.abs(got - np.roll(z, -k)).max() <= TOL + SLACK


def test_the_automorphism_of_2N_minus_1_conjugates(env):
    _, toy, z, c = env
    got = R.decode_int(toy.automorph(c, 2 * N - 1), LOGN, SCALE, R.fft_slots)
    assert np.abs(got - np.conj(z)).max() <= TOL + SLACK


def test_the_monomial_of_degree_half_N_multiplies_by_i(env):
    _, _, z, c = env
    shifted = np.concatenate([-c[N // 2:], c[:N // 2]])   # X^(N/2) c mod X^N + 1
    got = R.decode_int(shifted, LOGN, SCALE, R.fft_slots)
    assert np.abs(got - 1j * z).max() <= TOL + SLACK


def test_the_negacyclic_product_of_two_encodings_is_the_slot_wise_product(env):
    """the second factor is the slot vector of a polynomial with 24 coefficients (its encoding has 24 non-zero integers, so the schoolbook product
    of Toy stays quick); its slots are as generic as any"""
    _, toy, z, c = env
    rng = np.random.default_rng(99)
    sparse = np.zeros(N, dtype=np.int64)
    sparse[rng.choice(N, 24, replace=False)] = rng.integers(-2 ** 25, 2 ** 25, 24)
    w = R.decode_int(sparse.astype(object), LOGN, SCALE)
    cw = R.encode_int(w, LOGN, SCALE)
    assert [int(v) for v in cw] == [int(v) for v in sparse]      # encode inverts decode on integers
    prod = toy.negacyclic_mul(cw, c)   # the loop runs over the first factor's non-zero coefficients
    got = R.decode_int(prod, LOGN, SCALE * SCALE, R.fft_slots)
    bound = (np.abs(z).max() + np.abs(w).max()) * TOL + TOL * TOL
    assert np.abs(got - z * w).max() <= bound + SLACK


def test_the_limbs_are_the_oracle_transform_of_the_residues(env):
    o, toy, z, c = env
    ids = [0, 2, 3]
    assert np.array_equal(R.encode_limbs(o, z, SCALE, ids), toy.to_rns_eval(c, ids))
    x = R.encode_limbs(o, z, SCALE, [1])[0]
    assert np.abs(R.decode_limb(o, x, 1, SCALE, R.fft_slots) - z).max() <= TOL + SLACK
