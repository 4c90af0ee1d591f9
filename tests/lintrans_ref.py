"""CPU reference of hlintrans composed from oracle primitives (test helper), following the op's definition literally:
    acc_{r,k} = sum_j sigma_r(D_j) * evk_r[j][k]     (E limbs; D_j = ModUp(c1), once, on the unrotated c1)
    S_k       = sum_r pt_r * acc_{r,k}               (E limbs)
    U         = sum_r pt_r[Q limbs] * sigma_r(c0)    (l limbs)
    out.c0    = U + ModDown(S_0),  out.c1 = ModDown(S_1)
with the element-wise chains the op's stages run (EWE_MUL, then EWE_MAC_ADD) and ONE ModDown.  Independent of the host layer's plan."""
from hoisted_ref import EWE_ADD, EWE_MAC_ADD, EWE_MUL, EWE_SUB_SCALE, modup_digits


def weighted_sum(o, ids, terms, weights):
    """sum_r terms[r] * weights[r] over the limbs `ids`: a MUL, then one MAC_ADD per further term"""
    acc = o.ewe(EWE_MUL, ids, terms[0], weights[0])
    for t, w in zip(terms[1:], weights[1:]):
        acc = o.ewe(EWE_MAC_ADD, ids, t, w, acc)
    return acc


def key_product(o, ell, digits, evk, galois):
    """acc_k = sum_j sigma_g(D_j) * evk[j][k], k = 0, 1 ([E][N] each): the key product of tests/hoisted_ref.py before its ModDown"""
    ids = o.ext_ids(ell)
    X = [o.automorph_eval(d, galois) for d in digits]
    return [weighted_sum(o, ids, X, [evk[j][k] for j in range(len(X))]) for k in range(2)]


def moddown(o, ell, acc):
    """ModDown of one extended polynomial ([E][N], evaluation form), as in hoisted_ref.key_product_moddown"""
    ids = o.ext_ids(ell)
    Q, P = ids[:ell], ids[ell:]
    pm = 1
    for p in P:
        pm *= o.moduli[p]
    pinv = [pow(pm % o.moduli[q], -1, o.moduli[q]) for q in Q]
    conv = o.bconv_matmul(P, Q, o.bconv_scale(P, o.ntt(P, acc[ell:], inverse=True)))
    return o.ewe(EWE_SUB_SCALE, Q, acc[:ell], None, o.ntt(Q, conv), k=pinv)


def lintrans(o, ell, ct, galois, keys, pts):
    """(out.c0, out.c1): rotation r = 1..len(keys) by galois^r mod 2N with keys[r - 1] ([beta][2][E][N]) and plaintext pts[r - 1] ([E][N])"""
    ids = o.ext_ids(ell)
    Q = ids[:ell]
    gs = [pow(galois, r, 2 * o.N) for r in range(1, len(keys) + 1)]
    D = modup_digits(o, ell, ct[1])
    acc = [key_product(o, ell, D, evk, g) for evk, g in zip(keys, gs)]
    S = [weighted_sum(o, ids, [a[k] for a in acc], pts) for k in range(2)]
    U = weighted_sum(o, Q, [o.automorph_eval(ct[0], g) for g in gs], [p[:ell] for p in pts])
    return o.ewe(EWE_ADD, Q, moddown(o, ell, S[0]), None, U), moddown(o, ell, S[1])
