"""hlintrans on the count backend (no GPU): sum_r pt_r * rot_r(ct) with one ModUp and one ModDown.  The fused plan has ONE launch between the
ModUp and the ModDown whatever R is, its instruction total is the unfused plan's, the op chains, and the CPU reference the GPU tests compare
against (tests/lintrans_ref.py) agrees with a recomputation of the weighted sum in the coefficient domain with Python integers."""
import re

import numpy as np
import pytest

from homulator_amd import host

FUSED = ["INTT", "BCONV", "NTT", "IP_LINTRANS", "INTT", "BCONV", "NTT_SUBSCALE"]


def build(cfg, L, ell, alpha, fuse=True, **ov):
    o = host.Op(cfg, "hlintrans", L, ell, alpha, backend=host.BACKEND_COUNT, fuse=fuse, overrides=ov or None)
    try:
        return o.plan(), o.total_instructions(), o.launch_count(), o.stage_bytes()
    finally:
        o.close()


def n_of(line):
    return int(re.search(r" n=(\d+)", line).group(1))


def kinds_of(plan):
    return [ln.split()[0] for ln in plan]


def test_launch_list_at_45_35_15():
    """ModUp (3 launches), the weighted sum of the rotations (1), ONE ModDown with the final add in its last transform (3)"""
    ell, alpha, beta = 35, 15, 3
    for R in (1, 2, 4, 8):
        p, total, n, _ = build("config_4.cfg", 45, ell, alpha, rotations=R)
        assert kinds_of(p) == FUSED and n == 7, (R, p)
        assert n_of(p[0]) == ell and n_of(p[1]) == n_of(p[2]) == beta * (ell + alpha) - ell
        g = ",".join(str(pow(5, r, 1 << 17)) for r in range(1, R + 1))
        assert n_of(p[3]) == ell + alpha and p[3].rstrip().endswith(f" rot={R} g={g} addend={ell}"), p[3]
        # one ModDown: the alpha special limbs of two polynomials in, the l limbs of two polynomials out, U added to c0 in the last transform
        assert n_of(p[4]) == 2 * alpha and n_of(p[5]) == 2 * ell and n_of(p[6]) == 2 * ell and "auto_addend" not in p[6]
        p0, total0, n0, _ = build("config_4.cfg", 45, ell, alpha, fuse=False, rotations=R)
        assert total0 == total and n0 > n
        assert "IP_LINTRANS" not in kinds_of(p0) and kinds_of(p0).count("AUTO") == R * (beta + 1)


@pytest.mark.parametrize("alpha", [1, 2, 3, 5, 13])
def test_route_by_digit_count_at_every_level(alpha):
    """every level of a 13-limb chain at N = 2^13 (the grid of tests/test_host_hoisted_plan.py): beta <= 4 merges everything between the ModUp and
    the ModDown into one launch; beta >= 5 (no key-product record to merge: pass 6 builds them of at most 4 terms) keeps separate launches.  Both
    keep the unfused plan's instruction total."""
    L = 13
    for ell in range(1, L + 1):
        beta = -(-ell // alpha)
        for R in (1, 4):
            p, total, n, _ = build("config_4_N15.cfg", L, ell, alpha, N=1 << 13, rotations=R)
            kinds = kinds_of(p)
            assert n == len(kinds)
            if beta <= 4:
                assert kinds.count("IP_LINTRANS") == 1 and "AUTO" not in kinds and "IP_HOISTED" not in kinds and "IP" not in kinds and "EWE" not in kinds, (ell, R, kinds)
                assert kinds == FUSED, (ell, R, kinds)
                assert n_of(p[3]) == ell + alpha and f" rot={R} " in p[3] and p[3].rstrip().endswith(f"addend={ell}")
                assert n_of(p[4]) == 2 * alpha and n_of(p[6]) == 2 * ell      # exactly one ModDown chain
            else:
                assert "IP_LINTRANS" not in kinds and kinds.count("AUTO") >= 1 and "EWE" in kinds, (ell, R, kinds)
            assert build("config_4_N15.cfg", L, ell, alpha, fuse=False, N=1 << 13, rotations=R)[1] == total, (ell, R)


def test_fuse_lintrans_off_gives_a_plan_without_the_launch():
    p, total, n, _ = build("config_4.cfg", 45, 35, 15, rotations=4, fuse_lintrans=0)
    kinds = kinds_of(p)
    assert "IP_LINTRANS" not in kinds and kinds.count("IP_HOISTED") == 1 and "EWE" in kinds   # (6h) then takes the key products
    assert total == build("config_4.cfg", 45, 35, 15, rotations=4)[1] and n > 7
    both_off = kinds_of(build("config_4.cfg", 45, 35, 15, rotations=4, fuse_lintrans=0, fuse_hoist=0)[0])
    assert "IP_LINTRANS" not in both_off and "IP_HOISTED" not in both_off
    only_lintrans = kinds_of(build("config_4.cfg", 45, 35, 15, rotations=4, fuse_hoist=0)[0])
    assert only_lintrans == FUSED


def test_batched_launch_carries_every_op():
    one = build("config_4.cfg", 45, 35, 15, rotations=4)
    p, _, n, nbytes = build("config_4.cfg", 45, 35, 15, rotations=4, batch=10)
    assert n == one[2] == 7 and nbytes == 10 * one[3]
    assert p[3].split()[0] == "IP_LINTRANS" and n_of(p[3]) == 10 * (35 + 15) and p[3].rstrip().endswith("addend=350")


def test_byte_model_of_the_launch():
    """limb-polys of the merged launch: n beta digits + 2 R n beta keys + R n plaintexts + n_Q c0 read, 2 n + n_Q written"""
    o = host.Op("config_4.cfg", "hlintrans", 45, 35, 15, backend=host.BACKEND_COUNT, overrides={"rotations": 4})
    line = [ln for ln in o.plan(full=True) if ln.startswith("IP_LINTRANS")][0]
    o.close()
    n, beta, R, nq = 50, 3, 4, 35
    assert int(re.search(r" bytes=(\d+)", line).group(1)) == (n * beta + 2 * R * n * beta + R * n + nq + 2 * n + nq) * 8 * (1 << 16)


@pytest.mark.parametrize("ov,what", [
    ({"rotations": 0}, r"\[1, 16\]"), ({"rotations": 17}, r"\[1, 16\]"), ({"galois": 4}, "odd"), ({"galois": 2 * 32768}, "odd"),
    ({"galois": 1}, "distinct"), ({"galois": 2 * 32768 - 1, "rotations": 2}, "distinct"),
])
def test_bad_parameters_are_clear_errors(ov, what):
    with pytest.raises(host.HostError, match=what) as e:
        build("config_4_N15.cfg", 16, 10, 4, **ov)
    assert "hlintrans" in str(e.value)


def test_unserved_modes_are_clear_errors():
    with pytest.raises(host.HostError, match="hlintrans.*world"):
        host.Op("config_4_N15.cfg", "hlintrans", 16, 10, 4, backend=host.BACKEND_COUNT, world=2)
    with pytest.raises(host.HostError, match="hlintrans.*sim"):
        host.Op("config_4_N15.cfg", "hlintrans", 16, 10, 4, backend=host.BACKEND_SIM)


def test_middle_link_of_a_chain():
    """one output ciphertext at the input's level: any position of a chain"""
    c = host.Chain("config_4_N15.cfg", "hmult,hlintrans,hadd", 16, 10, 4, overrides={"backend": host.BACKEND_COUNT, "rotations": 2})
    assert len(c) == 3
    assert kinds_of(c[1].plan()) == FUSED and n_of(c[1].plan()[3]) == 9 + 4      # the hmult's rescale dropped a limb
    assert n_of(c[2].plan()[0]) == 2 * 9                                          # ... and hlintrans kept the level
    c.close()


def test_buffer_names():
    o = host.Op("config_4_N15.cfg", "hlintrans", 16, 10, 4, backend=host.BACKEND_COUNT, overrides={"rotations": 2})
    names = set(o.buffer_names())
    o.close()
    assert {"ct1.c0", "ct1.c1", "out.c0", "out.c1", "pt1", "pt2"} <= names and "pt3" not in names and "pt" not in names
    for r in (1, 2):
        assert {f"IP_Rot{r}_Key{k}_{j}" for k in range(2) for j in range(3)} <= names
    assert "out1.c0" not in names


# ---- the reference helper against a recomputation in the coefficient domain, with Python integers
def _negacyclic_sparse(sparse, dense, q):
    """(sum_i sparse[i] X^i) * dense in Z_q[X] / (X^N + 1), schoolbook: one shifted, sign-wrapped copy of `dense` per non-zero coefficient"""
    N = len(dense)
    acc = np.zeros(N, dtype=object)
    for i, c in sparse.items():
        shifted = np.concatenate([-dense[N - i:], dense[:N - i]]) if i else dense
        acc = (acc + c * shifted) % q
    return acc


def _automorph_coef(a, g):
    """sigma_g in the coefficient domain, explicitly: X^i -> X^(i g mod 2N), with X^N = -1"""
    N = len(a)
    out = np.zeros(N, dtype=object)
    for i in range(N):
        e = i * g % (2 * N)
        out[e % N] = a[i] if e < N else -a[i]
    return out


def test_reference_helper_against_integer_recomputation():
    from oracle.homoracle import Oracle
    from hoisted_ref import EWE_ADD, EWE_MAC_ADD, EWE_MUL, modup_digits
    from lintrans_ref import lintrans, moddown
    LOGN, L, ell, alpha, R, g = 13, 4, 3, 2, 2, 5
    o = Oracle(LOGN, L, alpha)
    o.set_threads(8)
    N, ids = o.N, o.ext_ids(ell)
    Q = ids[:ell]
    ct = o.synth_ct(ell, 91)
    keys = [o.synth_evk(ell, 7000 + 100000 * r) for r in range(1, R + 1)]
    # plaintexts: 6 non-zero coefficients each, full-size residues (one integer per coefficient and modulus), given to the helper in evaluation form
    rng = np.random.default_rng(5)
    sparse = [{int(i): [int(rng.integers(0, o.moduli[m])) for m in ids] for i in rng.choice(N, 6, replace=False)} for _ in range(R)]
    sparse[0][0] = [o.moduli[m] - 1 for m in ids]      # a constant term too (no wrap) ...
    sparse[1][N - 1] = [1] * len(ids)                  # ... and the top coefficient (everything but one coefficient wraps)
    pts = []
    for sp in sparse:
        coef = np.zeros((len(ids), N), dtype=np.uint64)
        for i, vals in sp.items():
            coef[:, i] = vals
        pts.append(o.ntt(ids, coef))
    got = lintrans(o, ell, ct, g, keys, pts)

    def to_coef(mods, a):
        return [c.astype(object) for c in o.ntt(mods, a, inverse=True)]

    def to_eval(mods, rows):
        return o.ntt(mods, np.stack([np.array([int(x) for x in r], dtype=np.uint64) for r in rows]))

    gs = [pow(g, r, 2 * N) for r in range(1, R + 1)]
    D = modup_digits(o, ell, ct[1])
    S = [[np.zeros(N, dtype=object) for _ in ids] for _ in range(2)]
    U = [np.zeros(N, dtype=object) for _ in Q]
    for r in range(R):
        # sigma_r of every digit, limb by limb in the coefficient domain; the dense x dense key product stays element-wise
        X = [to_eval(ids, [_automorph_coef(c, gs[r]) % o.moduli[m] for c, m in zip(to_coef(ids, d), ids)]) for d in D]
        for k in range(2):
            acc = o.ewe(EWE_MUL, ids, X[0], keys[r][0][k])
            for j in range(1, len(X)):
                acc = o.ewe(EWE_MAC_ADD, ids, X[j], keys[r][j][k], acc)
            for e, (c, m) in enumerate(zip(to_coef(ids, acc), ids)):
                q = o.moduli[m]
                S[k][e] = (S[k][e] + _negacyclic_sparse({i: v[e] for i, v in sparse[r].items()}, c, q)) % q
        for e, (c, m) in enumerate(zip(to_coef(Q, ct[0]), Q)):
            q = o.moduli[m]
            U[e] = (U[e] + _negacyclic_sparse({i: v[e] for i, v in sparse[r].items()}, _automorph_coef(c, gs[r]) % q, q)) % q
    exp0 = o.ewe(EWE_ADD, Q, moddown(o, ell, to_eval(ids, S[0])), None, to_eval(Q, U))
    exp1 = moddown(o, ell, to_eval(ids, S[1]))
    assert np.array_equal(got[0], exp0) and np.array_equal(got[1], exp1)
