"""hrotate_hoisted on the GPU, on both arithmetic back-ends (mont32 and chain_bits = 60):
 1. hm_inner_product_hoisted is bit-identical to n_rot calls of hm_inner_product_ex(x_galois = g_r), and refuses outputs that overlap its inputs;
 2. the op, fused (one hoisted launch) and unfused (one launch per stage), equals a CPU reference composed from oracle primitives, bit for bit;
 3. on real data (tests/toy_ckks.py) every out<r> decrypts to sigma_{g^r}(m)."""
import types

import numpy as np
import pytest

from homulator_amd import host
from oracle.homoracle import Oracle, chain_below

pytestmark = pytest.mark.gpu
CHAINS = ["mont32", "survey"]
_oracles = {}


def oracle(logN, L, K, chain):
    key = (logN, L, K, chain)
    if key not in _oracles:
        _oracles[key] = Oracle(logN, L, K, chain=chain)
        _oracles[key].set_threads(8)
    return _oracles[key]


def context(logN, L, K, chain):
    from homulator_amd import hip
    if chain == "mont32":
        return hip.Context(logN, L, K), hip
    mods = chain_below(logN, 60, L + K)
    return hip.Context(logN, L, K, q=mods[:L], p=mods[L:]), hip


@pytest.mark.parametrize("chain", CHAINS)
@pytest.mark.parametrize("logN", [13, 16])
def test_hoisted_key_product_equals_gathered_inner_products(chain, logN):
    ctx, hip = context(logN, 6, 3, chain)
    rng = np.random.default_rng(logN)
    M = 9
    for terms in (1, 2, 3, 4):
        for n_rot in (1, 3, 16):
            n = 7
            mods = [int(x) for x in rng.integers(0, M, n)]
            galois = [pow(5, r + 1, 2 << logN) for r in range(n_rot)]
            if n_rot == 3:
                galois[2] = (2 << logN) - 1   # the conjugation too
            nx, ny, no = n * terms, n_rot * n * 2 * terms, n_rot * n * 2
            xb, yb, ob, rb = ctx.alloc(nx), ctx.alloc(ny), ctx.alloc(no), ctx.alloc(no)
            xl = [int(v) for v in rng.permutation(nx)]             # non-identity limb lists
            yl = [int(v) for v in rng.permutation(ny)]
            ol = [int(v) for v in rng.permutation(no)]
            ctx.fill_uniform(xb, [mods[i // terms] for i in range(nx)], 11 + terms, out_limbs=[xl[i] for i in range(nx)])
            ctx.fill_uniform(yb, [mods[(i // terms) % (2 * n) // 2] for i in range(ny)], 23 + n_rot, out_limbs=[yl[i] for i in range(ny)])
            ctx.inner_product_hoisted(xb, xl, yb, yl, ob, ol, mods, terms, galois)
            got = ob.download()
            for r, g in enumerate(galois):
                ctx.inner_product(xb, xl, yb, yl[r * n * 2 * terms:(r + 1) * n * 2 * terms], rb, ol[r * n * 2:(r + 1) * n * 2], mods, terms, 2,
                                  x_galois=g)
                exp = rb.download()
                rows = ol[r * n * 2:(r + 1) * n * 2]
                assert np.array_equal(got[rows], exp[rows]), (terms, n_rot, r)
            for b_ in (xb, yb, ob, rb):
                b_.free()
    ctx.close()


def _alias_setup(logN=13):
    ctx, hip = context(logN, 6, 3, "mont32")
    n, terms = 4, 2
    big = ctx.alloc(64)
    ctx.fill_uniform(big, [0] * 64, 5)
    return ctx, hip, big, n, terms


def test_hoisted_refuses_an_output_over_a_digit_through_another_base_pointer():
    ctx, hip, big, n, terms = _alias_setup()
    x = big                                                        # digits: limbs 0 .. 7 of the allocation
    out = types.SimpleNamespace(ptr=big.limb_ptr(40))             # outputs from limb 40 on ...
    y = types.SimpleNamespace(ptr=big.limb_ptr(16))
    xl, yl = list(range(n * terms)), list(range(n * 2 * terms))
    ctx.inner_product_hoisted(x, xl, y, yl, out, list(range(n * 2)), [0] * n, terms, [5])      # disjoint: fine
    with pytest.raises(hip.HmError, match="digit"):                # outputs from limb 5 on: over the digits' limbs 5 .. 7
        ctx.inner_product_hoisted(x, xl, y, yl, types.SimpleNamespace(ptr=big.limb_ptr(5)), list(range(n * 2)), [0] * n, terms, [5])
    ctx.close()


def test_hoisted_refuses_an_output_over_a_key_through_another_base_pointer():
    ctx, hip, big, n, terms = _alias_setup()
    x, y = big, types.SimpleNamespace(ptr=big.limb_ptr(16))      # keys: limbs 16 .. 31
    xl, yl = list(range(n * terms)), list(range(n * 2 * terms))
    with pytest.raises(hip.HmError, match="key"):
        ctx.inner_product_hoisted(x, xl, y, yl, types.SimpleNamespace(ptr=big.limb_ptr(30)), list(range(n * 2)), [0] * n, terms, [5])
    with pytest.raises(hip.HmError, match="key"):                  # a base off the limb grid: partial overlap of one limb-poly
        ctx.inner_product_hoisted(x, xl, y, yl, types.SimpleNamespace(ptr=big.limb_ptr(31) + 8 * 64), list(range(n * 2)), [0] * n, terms, [5])
    ctx.close()


@pytest.mark.parametrize("chain", CHAINS)
@pytest.mark.parametrize("cfg,logN,L,ell,alpha,R,batch", [
    ("config_4_N15.cfg", 15, 16, 10, 4, 3, 2),
    ("config_4.cfg", 16, 45, 35, 15, 4, 1),
    ("config_4_N15.cfg", 15, 8, 8, 8, 2, 1),      # beta = 1
])
def test_op_fused_unfused_and_reference_agree(chain, cfg, logN, L, ell, alpha, R, batch):
    from hoisted_ref import hoisted_rotations
    o = oracle(logN, L, alpha, chain)
    ov = {"rotations": R, "galois": 5, "batch": batch}
    if chain != "mont32":
        ov["chain_bits"] = 60
    got = {}
    for fuse in (True, False):
        op = host.Op(cfg, "hrotate_hoisted", L, ell, alpha, fuse=fuse, overrides=ov)
        op.execute(1)
        got[fuse] = [[(op.read(f"out{r}.c0", copy=c), op.read(f"out{r}.c1", copy=c)) for r in range(1, R + 1)] for c in range(batch)]
        kinds = [ln.split()[0] for ln in op.plan()]
        assert (kinds.count("IP_HOISTED") == 1) == fuse
        op.close()
    keys = [o.synth_evk(ell, host.SEED + 10000 + 100000 * r) for r in range(1, R + 1)]
    for c in range(batch):
        exp = hoisted_rotations(o, ell, o.synth_ct(ell, host.SEED + 100000 * c), 5, keys)
        for r in range(R):
            for k in range(2):
                assert np.array_equal(got[True][c][r][k], exp[r][k]), ("fused", c, r, k)
                assert np.array_equal(got[False][c][r][k], exp[r][k]), ("unfused", c, r, k)


def test_real_data_decrypts_to_every_rotation():
    from toy_ckks import Toy
    LOGN, L, ELL, ALPHA, R, g = 13, 6, 5, 2, 3, 5
    o = Oracle(LOGN, L, ALPHA)
    o.set_threads(8)
    toy = Toy(o, seed=4243)
    m = toy.rng.integers(-1000, 1000, o.N).astype(object) * (1 << 30)
    ct = toy.encrypt(m, ELL)
    op = host.Op("config_4_N15.cfg", "hrotate_hoisted", L, ELL, ALPHA, overrides={"N": 1 << LOGN, "rotations": R, "galois": g})
    op.write("ct1.c0", ct[0])
    op.write("ct1.c1", ct[1])
    for r in range(1, R + 1):
        evk = toy.evk_at_level(toy.gen_evk(toy.automorph(toy.s, pow(g, r, 2 * o.N))), ELL)
        for j in range(evk.shape[0]):
            for k in range(2):
                op.write(f"IP_Rot{r}_Key{k}_{j}", evk[j][k])
    op.execute(1)
    for r in range(1, R + 1):
        out = np.stack([op.read(f"out{r}.c0"), op.read(f"out{r}.c1")])
        got, _ = toy.decrypt(out, ELL)
        exp = toy.automorph(m, pow(g, r, 2 * o.N))
        assert max(abs(int(a) - int(b)) for a, b in zip(got, exp)) < 1 << 16, r   # hrotate's bound (tests/test_gpu_real_data.py)
    op.close()
