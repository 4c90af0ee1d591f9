"""Op.encode_plaintext's refusals that need no GPU (the count backend builds the op and its plan, and holds no values): every message begins
`encode_plaintext:` and names what is wrong.  The names and the length are checked before the backend is asked; then world > 1, then the backend.
What it encodes is tests/test_gpu_slots.py's."""
import numpy as np
import pytest

from homulator_amd import host

LOGN, L, ELL, ALPHA = 13, 6, 5, 2
n = 1 << (LOGN - 1)
Z = np.zeros(n, dtype=np.complex128)


def make(op="pmult", **ov):
    return host.Op("config_4_N15.cfg", op, L, ELL, ALPHA, backend=host.BACKEND_COUNT, overrides=dict({"N": 1 << LOGN}, **ov))


def test_the_backend_that_holds_no_values_is_refused():
    op = make()
    with pytest.raises(host.HostError, match="^encode_plaintext:.*hip backend"):
        op.encode_plaintext("pt", Z, 2.0 ** 30)
    op.close()


def test_a_sharded_plan_is_refused():
    op = make(world=2, rank=0)
    with pytest.raises(host.HostError, match=r"^encode_plaintext:.*world > 1"):
        op.encode_plaintext("pt", Z, 2.0 ** 30)
    op.close()


@pytest.mark.parametrize("op,name,what", [("pmult", "nothing", "has no buffer nothing"), ("pmult", "ct1.c0", "is no plaintext"),
                                          ("pmult", "out.c1", "is no plaintext"), ("hlintrans", "pt9", "has no buffer pt9"),
                                          ("hlintrans", "ct1.c1", "is no plaintext")])
def test_names_that_are_no_plaintext_input(op, name, what):
    o = make(op)
    with pytest.raises(host.HostError, match="^encode_plaintext:.*" + what):
        o.encode_plaintext(name, Z, 2.0 ** 30)
    o.close()


@pytest.mark.parametrize("op,name", [("pmult", "pt"), ("padd", "pt"), ("hlintrans", "pt1"), ("hplincomb", "pt2")])
def test_a_wrong_length_is_refused_for_every_kind_of_plaintext(op, name):
    """... and the right length gets as far as the backend's refusal: the name is a plaintext input of the op"""
    o = make(op)
    for bad in (Z[:-1], np.zeros(2 * n, dtype=np.complex128)):
        with pytest.raises(host.HostError, match="^encode_plaintext:.*slots given, the ring has 4096"):
            o.encode_plaintext(name, bad, 2.0 ** 30)
    with pytest.raises(host.HostError, match="^encode_plaintext:.*hip backend"):
        o.encode_plaintext(name, Z, 2.0 ** 30)
    o.close()


def test_the_capability_names_the_rings_the_slot_transform_serves():
    from homulator_amd import hip
    assert [hip.capability(logN, "cap_slot_transform") for logN in range(11, 20)] == [0, 0, 1, 1, 1, 1, 1, 0, 0]
