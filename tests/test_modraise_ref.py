"""tests/modraise_ref.py against Python big integers in the coefficient domain (no GPU): N = 2^13, T = 3, both chains of tests/test_gpu_rescale.py.
The reference's output, taken back to coefficient form limb by limb, must be the residues of ONE integer polynomial v with |v_i| <= (q_0 - 1) / 2 and
v = c mod q_0, where c is the input in coefficient form; and limb 0 of the result equals the input."""
import numpy as np
import pytest

import modraise_ref as mr
from oracle.homoracle import Oracle

LOGN, L, K, T = 13, 6, 3, 3
CHAINS = ["mont32", "survey"]   # as tests/test_gpu_rescale.py


@pytest.fixture(scope="module", params=CHAINS)
def o(request):
    orc = Oracle(LOGN, L, K, chain=request.param)
    orc.set_threads(8)
    return orc


def test_centring_boundary():
    for qs in (97, 1152921504606584833):
        half = (qs - 1) // 2
        got = mr.centred(np.array([0, 1, half, half + 1, qs - 1], dtype=object), qs)
        assert [int(x) for x in got] == [0, 1, half, -half, -1]


def test_reference_is_the_centred_polynomial_on_every_limb(o):
    ct = o.synth_ct(1, 77)
    out = mr.modraise_ct(o, T, ct)
    q0 = o.moduli[0]
    for k in range(2):
        assert out[k].shape == (T, o.N) and out[k].dtype == np.uint64
        assert np.array_equal(out[k][0], ct[k][0]), "limb 0 is the input, bit for bit"
        c = [int(x) for x in o.ntt([0], ct[k][:1], inverse=True)[0]]
        v = [x if x <= (q0 - 1) // 2 else x - q0 for x in c]            # big integers, no helper of the reference
        assert all(abs(x) <= (q0 - 1) // 2 and (x - y) % q0 == 0 for x, y in zip(v, c))
        back = o.ntt(list(range(T)), out[k], inverse=True)
        for j in range(T):
            qj = o.moduli[j]
            assert [int(x) for x in back[j]] == [x % qj for x in v], (k, j)


def test_lift_between_any_two_moduli_of_the_chain(o):
    """source wider, narrower or equal: the helper the kernel tests use, on special moduli too"""
    rng = np.random.default_rng(5)
    for src, dst in ((0, L + K - 1), (L + K - 1, 0), (2, 2)):
        qs, qd = o.moduli[src], o.moduli[dst]
        c = rng.integers(0, qs, o.N, dtype=np.uint64)
        c[:5] = [0, 1, (qs - 1) // 2, (qs + 1) // 2, qs - 1]
        got = o.ntt([dst], mr.lift(o, src, [dst], c), inverse=True)[0]
        exp = [(int(x) if int(x) <= (qs - 1) // 2 else int(x) - qs) % qd for x in c]
        assert [int(x) for x in got] == exp, (src, dst)
