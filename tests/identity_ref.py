"""CPU references of hlintrans and hbsgs with identity = 1 composed from oracle primitives (test helper), following DESIGN.md section 16 literally:
    S_k    = sum_{r=1..R} pt_r * acc_{r,k}                                  (E limbs, as tests/lintrans_ref.py)
    U      = pt_0[Q] * c0 + sum_{r=1..R} pt_r[Q] * sigma_{g_r}(c0)          (l limbs)
    W      = pt_0[Q] * c1                                                   (l limbs)
    out.c0 = U + ModDown(S_0),   out.c1 = W + ModDown(S_1)
with the element-wise chains the op's stages run (EWE_MUL, then EWE_MAC_ADD) and ONE ModDown.  The unrotated term meets no key.  Independent
of the host layer's plan.  hbsgs (bsgs_id): giant groups i = 0..G, baby steps r = 0..R, g_0 = h_0 = 1,
    S_{i,k} = sum_{r>=1} pt_{i,r} * acc_{r,k}    U_i = pt_{i,0}[Q] * c0 + sum_{r>=1} pt_{i,r}[Q] * sigma_{g_r}(c0)    W_i = pt_{i,0}[Q] * c1
    v_i     = (U_i + ModDown(S_{i,0}), W_i + ModDown(S_{i,1}))                                  i = 1..G only
    T_k     = S_{0,k} + sum_{i>=1} (key product of v_i through sigma_{h_i})_k                    V = U_0 + sum_{i>=1} sigma_{h_i}(v_i.c0)
    out     = (V + ModDown(T_0), W_0 + ModDown(T_1))
group 0 is never brought down on its own."""
from hoisted_ref import EWE_ADD, EWE_MUL, modup_digits
from lintrans_ref import key_product, moddown, weighted_sum
from rotsum_ref import add_chain

PT0_STREAM = 4300   # the identity plaintext's synthetic stream: seed + 4300 (pt<r>: seed + 4000 + 100000 r); hbsgs: pt0_<i> + 100000 i
PTG_STREAM = 4600   # hbsgs: group 0's rotations ptg<r>: seed + 4600 + 100000 r


def lintrans_id(o, ell, ct, galois, keys, pts, pt0):
    """(out.c0, out.c1): lintrans_ref.lintrans plus the unrotated term pt0 ([E][N], only its Q limbs are read) * ct"""
    ids = o.ext_ids(ell)
    Q = ids[:ell]
    gs = [pow(galois, r, 2 * o.N) for r in range(1, len(keys) + 1)]
    D = modup_digits(o, ell, ct[1])
    acc = [key_product(o, ell, D, evk, g) for evk, g in zip(keys, gs)]
    S = [weighted_sum(o, ids, [a[k] for a in acc], pts) for k in range(2)]
    U = weighted_sum(o, Q, [ct[0]] + [o.automorph_eval(ct[0], g) for g in gs], [pt0[:ell]] + [p[:ell] for p in pts])
    W = o.ewe(EWE_MUL, Q, ct[1], pt0[:ell])
    return o.ewe(EWE_ADD, Q, moddown(o, ell, S[0]), None, U), o.ewe(EWE_ADD, Q, moddown(o, ell, S[1]), None, W)


def bsgs_id(o, ell, ct, g, h, baby_keys, giant_keys, pts, pt0s, ptgs):
    """(out.c0, out.c1): pts[i - 1][r - 1] = pt_{i,r} for i, r >= 1 (as bsgs_ref.bsgs), pt0s[i] = pt_{i,0} for i = 0..G, ptgs[r - 1] = pt_{0,r};
    baby rotation r by g^r with baby_keys[r - 1], giant step i by h^i with giant_keys[i - 1]"""
    ids = o.ext_ids(ell)
    Q = ids[:ell]
    G, R = len(giant_keys), len(baby_keys)
    gs = [pow(g, r, 2 * o.N) for r in range(1, R + 1)]
    hs = [pow(h, i, 2 * o.N) for i in range(1, G + 1)]
    D = modup_digits(o, ell, ct[1])
    acc = [key_product(o, ell, D, evk, gr) for evk, gr in zip(baby_keys, gs)]
    rc0 = [o.automorph_eval(ct[0], gr) for gr in gs]
    S, U, W = [], [], []
    for i in range(G + 1):
        p = pts[i - 1] if i else ptgs
        S.append([weighted_sum(o, ids, [a[k] for a in acc], p) for k in range(2)])
        U.append(weighted_sum(o, Q, [ct[0]] + rc0, [pt0s[i][:ell]] + [w[:ell] for w in p]))
        W.append(o.ewe(EWE_MUL, Q, ct[1], pt0s[i][:ell]))
    v = [(o.ewe(EWE_ADD, Q, moddown(o, ell, S[i][0]), None, U[i]), o.ewe(EWE_ADD, Q, moddown(o, ell, S[i][1]), None, W[i])) for i in range(1, G + 1)]
    gacc = [key_product(o, ell, modup_digits(o, ell, vi[1]), evk, hi) for vi, evk, hi in zip(v, giant_keys, hs)]
    T = [add_chain(o, ids, [a[k] for a in gacc] + [S[0][k]]) for k in range(2)]   # the group-0 term last
    V = add_chain(o, Q, [o.automorph_eval(vi[0], hi) for vi, hi in zip(v, hs)] + [U[0]])
    return o.ewe(EWE_ADD, Q, moddown(o, ell, T[0]), None, V), o.ewe(EWE_ADD, Q, moddown(o, ell, T[1]), None, W[0])


def lintrans_id_inputs(o, ell, R, seed, copy=0, batch_seed_stride=100000):
    """hlintrans's synthetic streams for op `copy` of a batch: (the ciphertext, rotation r's key (one for every op of the batch), pt<r>, pt0)"""
    ids = o.ext_ids(ell)
    c = copy * batch_seed_stride
    return (o.synth_ct(ell, seed + c), [o.synth_evk(ell, seed + 10000 + 100000 * r) for r in range(1, R + 1)],
            [o.fill_uniform(ids, seed + 4000 + 100000 * r + c) for r in range(1, R + 1)], o.fill_uniform(ids, seed + PT0_STREAM + c))


def bsgs_id_inputs(o, ell, R, G, seed, copy=0, batch_seed_stride=100000):
    """the op's synthetic streams behind bsgs_ref.synthetic_inputs: (pt0s[i], i = 0..G; ptgs[r - 1], r = 1..R) of op `copy` of a batch"""
    ids = o.ext_ids(ell)
    c = copy * batch_seed_stride
    return ([o.fill_uniform(ids, seed + PT0_STREAM + 100000 * i + c) for i in range(G + 1)],
            [o.fill_uniform(ids, seed + PTG_STREAM + 100000 * r + c) for r in range(1, R + 1)])
