"""hdot on the count backend (no GPU): sum_t ct<2t-1> * ct<2t> with one key switch and one rescale.  The fused plan is
hmult's with the first launch swapped for ONE TENSOR_DOT launch whatever T is, its instruction total is the unfused plan's, the op chains, and the
CPU reference the GPU tests compare against (tests/dot_ref.py) is hmult at T = 1 and decrypts to the sum of products on real data."""
import re

import numpy as np
import pytest

from homulator_amd import host

FUSED = ["TENSOR_DOT", "INTT", "NTT_IP", "INTT", "BCONV", "NTT_SUBSCALE"]


def build(cfg, op, L, ell, alpha, fuse=True, **ov):
    o = host.Op(cfg, op, L, ell, alpha, backend=host.BACKEND_COUNT, fuse=fuse, overrides=ov or None)
    try:
        return o.plan(), o.total_instructions(), o.launch_count(), o.stage_bytes()
    finally:
        o.close()


def n_of(line):
    return int(re.search(r" n=(\d+)", line).group(1))


def ref_of(plan):
    return sum(int(re.search(r" ref=(\d+)", ln).group(1)) for ln in plan)


def kinds_of(plan):
    return [ln.split()[0] for ln in plan]


def assert_hmult_with_the_first_launch_swapped(p, hm, n_dot, T, what):
    """every launch behind the first has hmult's kind and entry count at the same point; the first is the one TENSOR_DOT"""
    assert len(p) == len(hm), (what, kinds_of(p), kinds_of(hm))
    assert kinds_of(hm)[0] == "TENSOR" and kinds_of(p)[0] == "TENSOR_DOT", (what, kinds_of(p))
    assert n_of(p[0]) == n_dot == n_of(hm[0]) and f" terms={T}" in p[0] + " ", (what, p[0])
    assert [(ln.split()[0], n_of(ln)) for ln in p[1:]] == [(ln.split()[0], n_of(ln)) for ln in hm[1:]], what
    assert "TENSOR" not in kinds_of(p), (what, kinds_of(p))


@pytest.mark.parametrize("T", [1, 2, 4, 8, 16])
def test_launch_list_at_45_35_15(T):
    ell = 35
    hm = build("config_4.cfg", "hmult", 45, ell, 15)[0]
    p, total, n, _ = build("config_4.cfg", "hdot", 45, ell, 15, terms=T)
    assert kinds_of(p) == FUSED and n == 6, (T, p)
    assert_hmult_with_the_first_launch_swapped(p, hm, ell, T, T)
    p0, total0, n0, _ = build("config_4.cfg", "hdot", 45, ell, 15, fuse=False, terms=T)
    assert total0 == total == ref_of(p) == ref_of(p0) and n0 > n      # fusion moves instructions, never drops them
    assert "TENSOR_DOT" not in kinds_of(p0) and "TENSOR" not in kinds_of(p0)
    pb = build("config_4.cfg", "hdot", 45, ell, 15, terms=T, batch=10)[0]
    assert kinds_of(pb) == FUSED and n_of(pb[0]) == 10 * ell and f" terms={T}" in pb[0] + " "


def test_default_terms_is_four():
    assert " terms=4" in build("config_4.cfg", "hdot", 45, 35, 15)[0][0] + " "


def test_byte_model_of_the_launch():
    """(4T + 3) limb-polys per record: every operand read once, the three sums written once"""
    for T, batch in ((1, 1), (4, 1), (4, 10), (16, 1)):
        o = host.Op("config_4.cfg", "hdot", 45, 35, 15, backend=host.BACKEND_COUNT, overrides={"terms": T, "batch": batch})
        line = [ln for ln in o.plan(full=True) if ln.startswith("TENSOR_DOT")][0]
        o.close()
        assert int(re.search(r" bytes=(\d+)", line).group(1)) == (4 * T + 3) * 35 * batch * 8 * (1 << 16), (T, batch)
        assert f" terms={T} " in line


def test_fuse_dot_off_gives_a_tensor_launch_and_element_wise_launches():
    for T in (2, 4):
        p, total, n, _ = build("config_4.cfg", "hdot", 45, 35, 15, terms=T, fuse_dot=0)
        kinds = kinds_of(p)
        assert "TENSOR_DOT" not in kinds and kinds.count("TENSOR") == 1 and "EWE" in kinds and n > 6, kinds
        assert total == ref_of(p) == build("config_4.cfg", "hdot", 45, 35, 15, terms=T)[1]
        assert kinds[-5:] == FUSED[1:]


@pytest.mark.parametrize("alpha", [1, 2, 3, 5, 13])
def test_every_level_of_a_13_limb_chain(alpha):
    """the grid of tests/test_host_hoisted_plan.py (N = 2^13, every level a rescale can start from): whatever plan hmult has at a point, hdot's is
    that plan with the first launch swapped, and the fused total is the unfused one"""
    L = 13
    for ell in range(2, L + 1):
        hm = build("config_4_N15.cfg", "hmult", L, ell, alpha, N=1 << 13)[0]
        for T in (1, 3):
            p, total, n, _ = build("config_4_N15.cfg", "hdot", L, ell, alpha, N=1 << 13, terms=T)
            assert n == len(p)
            assert_hmult_with_the_first_launch_swapped(p, hm, ell, T, (alpha, ell, T))
            p0, total0, _, _ = build("config_4_N15.cfg", "hdot", L, ell, alpha, fuse=False, N=1 << 13, terms=T)
            assert total0 == total == ref_of(p) == ref_of(p0), (alpha, ell, T)


@pytest.mark.parametrize("T", [0, 17])
def test_terms_out_of_range_is_a_clear_error(T):
    with pytest.raises(host.HostError, match=r"terms.*\[1, 16\]") as e:
        build("config_4_N15.cfg", "hdot", 16, 10, 4, terms=T)
    assert "hdot" in str(e.value)


def test_unserved_modes_are_clear_errors():
    with pytest.raises(host.HostError, match="hdot.*world"):
        host.Op("config_4_N15.cfg", "hdot", 16, 10, 4, backend=host.BACKEND_COUNT, world=2)
    with pytest.raises(host.HostError, match="hdot.*sim"):
        host.Op("config_4_N15.cfg", "hdot", 16, 10, 4, backend=host.BACKEND_SIM)


def test_middle_link_of_a_chain():
    """one output ciphertext a level down: any position of a chain; ct1 is the bound input"""
    c = host.Chain("config_4_N15.cfg", "hmult,hdot,hadd", 16, 10, 4, overrides={"backend": host.BACKEND_COUNT, "terms": 3})
    assert len(c) == 3
    p = c[1].plan()
    assert kinds_of(p)[0] == "TENSOR_DOT" and kinds_of(p).count("TENSOR_DOT") == 1 and n_of(p[0]) == 9 and " terms=3" in p[0] + " "   # hmult dropped a limb
    assert n_of(c[2].plan()[0]) == 2 * 8                                                                    # ... and so did hdot
    c.close()


def test_buffer_names():
    o = host.Op("config_4_N15.cfg", "hdot", 16, 10, 4, backend=host.BACKEND_COUNT, overrides={"terms": 3})
    names = set(o.buffer_names())
    o.close()
    assert {f"ct{i}.c{k}" for i in range(1, 7) for k in range(2)} | {"out.c0", "out.c1", "DotD0Out", "DotD1Out", "DotD2Out"} <= names
    assert "ct7.c0" not in names and "TensorD0Out" not in names
    assert {f"IP_Key{k}_{j}" for k in range(2) for j in range(3)} <= names


def test_the_other_ops_keep_their_tensor_launch():
    assert kinds_of(build("config_4.cfg", "hmult", 45, 35, 15)[0])[0] == "TENSOR"
    c = host.Chain("config_4_N15.cfg", "hmult,hmult", 16, 10, 4, overrides={"backend": host.BACKEND_COUNT})
    assert kinds_of(c[1].plan())[0] == "TENSOR"
    c.close()


# ---- the reference, pinned without a GPU at N = 2^13
LOGN, L, ELL, ALPHA = 13, 6, 5, 2


def test_reference_at_one_term_is_the_oracles_hmult():
    from dot_ref import dot, synthetic_inputs
    from oracle.homoracle import Oracle
    o = Oracle(LOGN, L, ALPHA)
    o.set_threads(8)
    cts, evk = synthetic_inputs(o, ELL, 1, host.SEED)
    exp = o.hmult(ELL, cts[0], cts[1], evk, rescale=True)
    got = dot(o, ELL, cts, evk)
    assert np.array_equal(got[0], exp[0]) and np.array_equal(got[1], exp[1])


def test_reference_on_real_data_decrypts_to_the_sum_of_products():
    from dot_ref import decryption_error, dot, real_pairs
    from oracle.homoracle import Oracle
    from toy_ckks import Toy
    T = 3
    o = Oracle(LOGN, L, ALPHA)
    o.set_threads(8)
    toy = Toy(o, seed=4244)
    cts, evk, exact = real_pairs(toy, T, ELL)
    err, one = decryption_error(toy, dot(o, ELL, cts, evk), ELL, exact)
    print(f"reference: max |dec q_last - exact| = 2^{err.bit_length()} (bound {T} x 2^{one.bit_length() - 1})")
    assert err < T * one
