"""CPU reference of hmodraise (test helper), following DESIGN.md section 18 literally, per component k and output limb j < T, with q_s = q_0:
    c      = INTT_{q_s}(ct.c_k limb 0)                      coefficient form, in [0, q_s)
    v_i    = c_i if c_i <= (q_s - 1) / 2 else c_i - q_s     the centred representative (q_s is odd)
    out_j  = NTT_{q_j}(v mod q_j)
Built from Oracle.ntt (inverse and forward) and Python integers for the centring.  Independent of the host layer's plan."""
import numpy as np


def centred(c, qs):
    """the centred representatives of the residues c mod qs, as Python integers (object array)"""
    half = (qs - 1) // 2
    return np.array([int(x) if int(x) <= half else int(x) - qs for x in c], dtype=object)


def lift(o, src_mod, mods, coeff):
    """coeff: [N] residues mod q_{src_mod} in coefficient form -> [len(mods)][N], row i = NTT_{mods[i]}(centre(coeff) mod q_{mods[i]})"""
    qs = o.moduli[src_mod]
    c = np.asarray(coeff, dtype=np.uint64).astype(np.int64)            # below 2^60: signed 64-bit integers hold c and c - q_s
    v = np.where(c <= (qs - 1) // 2, c, c - np.int64(qs))
    rows = np.stack([np.mod(v, np.int64(o.moduli[m])).astype(np.uint64) for m in mods])   # np.mod: the sign of the divisor, so in [0, q)
    return o.ntt(mods, rows)


def modraise_poly(o, T, limb0):
    """one component: limb0 = its one limb in evaluation form mod q_0 -> [T][N]"""
    c = o.ntt([0], np.asarray(limb0, dtype=np.uint64).reshape(1, o.N), inverse=True)[0]
    return lift(o, 0, list(range(T)), c)


def modraise_ct(o, T, ct):
    """(ModRaise(c0), ModRaise(c1)) of a ciphertext at level 1 (ct[k]: [1][N] or [N]): two [T][N] arrays"""
    return tuple(modraise_poly(o, T, np.asarray(ct[k]).reshape(-1, o.N)[0]) for k in range(2))
