"""CPU reference of hrotate_hoisted composed from oracle primitives (test helper): the ModUp digits of the UNROTATED c1 once
(Oracle.keyswitch(..., dump=True) "ext"), then per rotation the automorphism of every digit, the key product with that rotation's key and
the ModDown (INTT of the P limbs, base conversion P -> Q, NTT, SUB_SCALE by P^-1).  Independent of the host layer's plan."""
import numpy as np

EWE_MUL, EWE_MAC_ADD, EWE_ADD, EWE_SUB_SCALE = 0, 2, 3, 6


def modup_digits(o, ell, c1):
    """D_j, j < beta: the extended digits of c1 in evaluation form, [beta][ell + K][N]"""
    zero = np.zeros((o.beta(ell), 2, ell + o.K, o.N), dtype=np.uint64)
    return o.keyswitch(ell, c1, zero, dump=True)[2]["ext"]


def key_product_moddown(o, ell, digits, evk, galois=1):
    """(ks0, ks1) = ModDown(sum_j sigma_g(D_j) * evk[j]); galois = 1: the digits as they are"""
    ids = o.ext_ids(ell)
    Q, P = ids[:ell], ids[ell:]
    X = [d if galois == 1 else o.automorph_eval(d, galois) for d in digits]
    pm = 1
    for p in P:
        pm *= o.moduli[p]
    pinv = [pow(pm % o.moduli[q], -1, o.moduli[q]) for q in Q]
    out = []
    for k in range(2):
        acc = o.ewe(EWE_MUL, ids, X[0], evk[0][k])
        for j in range(1, len(X)):
            acc = o.ewe(EWE_MAC_ADD, ids, X[j], evk[j][k], acc)
        conv = o.bconv_matmul(P, Q, o.bconv_scale(P, o.ntt(P, acc[ell:], inverse=True)))
        out.append(o.ewe(EWE_SUB_SCALE, Q, acc[:ell], None, o.ntt(Q, conv), k=pinv))
    return out


def hoisted_rotations(o, ell, ct, galois, keys):
    """[(out_r.c0, out_r.c1)] for r = 1..len(keys): rotation r by galois^r mod 2N with keys[r - 1] ([beta][2][E][N])"""
    D = modup_digits(o, ell, ct[1])
    res = []
    for r, evk in enumerate(keys, start=1):
        g = pow(galois, r, 2 * o.N)
        ks0, ks1 = key_product_moddown(o, ell, D, evk, g)
        res.append((o.ewe(EWE_ADD, list(range(ell)), o.automorph_eval(ct[0], g), None, ks0), ks1))
    return res
