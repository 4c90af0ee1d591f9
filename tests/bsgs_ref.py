"""CPU reference of hbsgs composed from oracle primitives (test helper), following the op's definition literally:
    D_j       = ModUp(c1)                                      (ONCE, on the unrotated c1)
    acc_{r,k} = sum_j sigma_{g_r}(D_j) * evk_r[j][k]           (E limbs, once per baby rotation)
    S_{i,k}   = sum_r pt_{i,r} * acc_{r,k}                     (E limbs)
    U_i       = sum_r pt_{i,r}[Q limbs] * sigma_{g_r}(c0)      (l limbs)
    v_i       = (U_i + ModDown(S_{i,0}), ModDown(S_{i,1}))     (G intermediate ciphertexts)
    out       = rotsum(v_1 .. v_G) with elements h^i and the giant keys
with the element-wise chains the op's stages run.  Independent of the host layer's plan."""
from hoisted_ref import EWE_ADD, modup_digits
from lintrans_ref import key_product, moddown, weighted_sum
from rotsum_ref import rotsum


def baby_step(o, ell, ct, g, baby_keys, pts):
    """the G intermediate ciphertexts v_i; pts[i][r]: plaintext ([E][N]) of giant step i + 1 and baby rotation r + 1"""
    ids = o.ext_ids(ell)
    Q = ids[:ell]
    gs = [pow(g, r, 2 * o.N) for r in range(1, len(baby_keys) + 1)]
    D = modup_digits(o, ell, ct[1])
    acc = [key_product(o, ell, D, evk, gr) for evk, gr in zip(baby_keys, gs)]
    c0 = [o.automorph_eval(ct[0], gr) for gr in gs]
    v = []
    for p in pts:
        S = [weighted_sum(o, ids, [a[k] for a in acc], p) for k in range(2)]
        U = weighted_sum(o, Q, c0, [w[:ell] for w in p])
        v.append((o.ewe(EWE_ADD, Q, moddown(o, ell, S[0]), None, U), moddown(o, ell, S[1])))
    return v


def bsgs(o, ell, ct, g, h, baby_keys, giant_keys, pts):
    """(out.c0, out.c1): baby rotation r by g^r with baby_keys[r - 1], giant step i by h^i with giant_keys[i - 1] (keys [beta][2][E][N])"""
    return rotsum(o, ell, baby_step(o, ell, ct, g, baby_keys, pts), h, giant_keys)


def synthetic_inputs(o, ell, R, G, seed, copy=0, batch_seed_stride=100000):
    """the op's synthetic streams: ct1 from seed (c1: + 1000), op `copy` of a batch + copy * stride; baby key r (one for every op of a batch) from
    seed + 10000 + 100000 r, giant key i from seed + 10000 + 100000 (16 + i); plaintext pt<p>, p = (i - 1) R + r, from seed + 4000 + 100000 p.
    Returns (ct, baby_keys, giant_keys, pts[i][r])"""
    ids = o.ext_ids(ell)
    return (o.synth_ct(ell, seed + copy * batch_seed_stride),
            [o.synth_evk(ell, seed + 10000 + 100000 * r) for r in range(1, R + 1)],
            [o.synth_evk(ell, seed + 10000 + 100000 * (16 + i)) for i in range(1, G + 1)],
            [[o.fill_uniform(ids, seed + 4000 + 100000 * (i * R + r + 1) + copy * batch_seed_stride) for r in range(R)] for i in range(G)])
