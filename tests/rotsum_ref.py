"""CPU reference of hrotsum composed from oracle primitives (test helper), following the op's definition literally:
    D_{i,j}   = ModUp(ct_i.c1)                          (per ciphertext, on the unrotated c1)
    acc_{i,k} = sum_j sigma_i(D_{i,j}) * evk_i[j][k]    (E limbs)
    S_k       = sum_i acc_{i,k}                          (E limbs)
    U         = sum_i sigma_i(ct_i.c0)                   (l limbs)
    out.c0    = U + ModDown(S_0),  out.c1 = ModDown(S_1)
with the EWE_ADD chains the op's stages run and ONE ModDown.  Independent of the host layer's plan."""
from hoisted_ref import EWE_ADD, modup_digits
from lintrans_ref import key_product, moddown


def add_chain(o, ids, terms):
    """sum of `terms` over the limbs `ids`: one ADD per further term onto the running sum"""
    acc = terms[0]
    for t in terms[1:]:
        acc = o.ewe(EWE_ADD, ids, acc, None, t)
    return acc


def rotsum(o, ell, cts, galois, keys):
    """(out.c0, out.c1): ciphertext i = 1..len(cts) rotated by galois^i mod 2N with keys[i - 1] ([beta][2][E][N])"""
    ids = o.ext_ids(ell)
    Q = ids[:ell]
    gs = [pow(galois, i, 2 * o.N) for i in range(1, len(cts) + 1)]
    acc = [key_product(o, ell, modup_digits(o, ell, ct[1]), evk, g) for ct, evk, g in zip(cts, keys, gs)]
    S = [add_chain(o, ids, [a[k] for a in acc]) for k in range(2)]
    U = add_chain(o, Q, [o.automorph_eval(ct[0], g) for ct, g in zip(cts, gs)])
    return o.ewe(EWE_ADD, Q, moddown(o, ell, S[0]), None, U), moddown(o, ell, S[1])


def synthetic_inputs(o, ell, G, seed, copy=0, batch_seed_stride=100000):
    """the op's synthetic streams: ct<i + 1> from seed + 2000 i (c1: + 1000), op `copy` of a batch + copy * stride; ciphertext i's key (one for
    every op of a batch) from seed + 10000 + 100000 i, i = 1..G"""
    return ([o.synth_ct(ell, seed + 2000 * i + copy * batch_seed_stride) for i in range(G)],
            [o.synth_evk(ell, seed + 10000 + 100000 * i) for i in range(1, G + 1)])
