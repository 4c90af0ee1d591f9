"""CPU references of the ops with rescale = 1 and of hrescale (test helper), following DESIGN.md section 17 literally: the op as it is with rescale = 0
(the existing helpers of tests/*_ref.py and the oracle's pmult), then Oracle.rescale on each component of its result:
    r      = INTT_{q_last}(x_last)
    out_i  = (x_i - NTT_{q_i}(r)) * [q_last^-1]_{q_i}        i < l - 1
Independent of the host layer's plan."""
from bsgs_ref import bsgs
from identity_ref import bsgs_id, lintrans_id
from lintrans_ref import lintrans
from rotsum_ref import rotsum


def rescale_ct(o, ell, ct):
    """(Rescale(c0), Rescale(c1)) of a ciphertext at level ell: two [ell - 1][N] arrays"""
    return o.rescale(ell, ct[0]), o.rescale(ell, ct[1])


def pmult_rescaled(o, ell, ct, pt):
    return rescale_ct(o, ell, o.pmult(ell, ct, pt))


def lintrans_rescaled(o, ell, ct, galois, keys, pts, pt0=None):
    """hlintrans with rescale = 1; pt0: the identity step's plaintext (identity = 1)"""
    out = lintrans(o, ell, ct, galois, keys, pts) if pt0 is None else lintrans_id(o, ell, ct, galois, keys, pts, pt0)
    return rescale_ct(o, ell, out)


def rotsum_rescaled(o, ell, cts, galois, keys):
    return rescale_ct(o, ell, rotsum(o, ell, cts, galois, keys))


def bsgs_rescaled(o, ell, ct, g, h, baby_keys, giant_keys, pts, pt0s=None, ptgs=None):
    """hbsgs with rescale = 1 (only the final result is rescaled); pt0s / ptgs: the identity steps' plaintexts (identity = 1)"""
    out = bsgs(o, ell, ct, g, h, baby_keys, giant_keys, pts) if pt0s is None else bsgs_id(o, ell, ct, g, h, baby_keys, giant_keys, pts, pt0s, ptgs)
    return rescale_ct(o, ell, out)
