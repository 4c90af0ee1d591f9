"""CPU reference of hmuladd from oracle primitives only, following the definition literally and independent of the host plan:
tensor ct1 with ct2 (MUL, MAC2, MUL), multiply the three polynomials by the per-limb scalars (MUL_CONST), per addend multiply both components by
the addend's per-limb scalars (MUL_CONST) and add them onto d0 and d1 (ADD), add the per-limb constants to every evaluation-form entry of d0 (numpy:
the oracle has no such opcode), then hmult's tail: key switch of d2, the two adds, the two rescales.

The real-data case (tests/toy_ckks.py; LOGN 13, L 6, alpha 2, Delta = 2^40) evaluates T_3 = 2 T_2 x - x on encrypted data:
  * x: a fresh encryption of X = m Delta (|m| < 50) at level 5, Dec = X + e_x with |e_x| <= FRESH_BOUND = 26 per coefficient (8 sigma of
    Toy.small_err);
  * T_2 = 2 x^2 - 1 by square_ref.square at level 5 (s = 2, k = -Delta^2): a ciphertext at level 4 with Dec = Y + e_Y, Y = E_2 / q_4,
    E_2 = 2 X X - Delta^2, which tests/test_square_ref.py holds to |e_Y| q_4 <= 2 (q_4 << 12), so |e_Y| <= 2^13;
  * hmuladd at level 4 with ct1 = T_2, ct2 = ct3 = x cut to its first four limbs, s = 2, u_1 = q_j - (D mod q_j) with D = round(Delta^2 / q_4) the
    (integer) scale of T_2: out at level 3 with Dec(out) q_3 = 2 Y X - D X + err.
The bound on |err|, term by term, from the bounds the square and real-data tests already use:
  * the op's own key switch and rescale, as one hmult (tests/test_gpu_real_data.py: q_last << 12 with q_last = q_3), times the scalar s = 2 as in
    square_ref.decryption_error:                                  2 (q_3 << 12)
  * the addend: its fresh error times |u| = D:                    D FRESH_BOUND
  * the error ct1 already carries, through the product with x: 2 e_Y X is a negacyclic product of N terms, each at most 2^13 times
    |X| <= 50 Delta:                                               2 N 2^13 50 Delta
(the products of e_x with Y and with D are inside the first and second term: |Y| is the size of a message there too).  With q_3 below 2^60,
N = 2^13 and D about 2^20 the sum is below 2^75; the signal 2 Y X is above 2^90.  Compared in integers, everything times q_4:
|Dec(out) q_3 q_4 - (2 E_2 X - D q_4 X)| <= bound q_4."""
import numpy as np

from oracle.homoracle import EWE_ADD, EWE_MAC2, EWE_MUL, EWE_MUL_CONST
from square_ref import add_const

SCALE_STREAM, ADD_SCALE_STRIDE, CONST_STREAM = 6400, 10, 6490
FRESH_BOUND = 26           # 8 sigma of tests/toy_ckks.py Toy.small_err (sigma 3.2), rounded up
DELTA = 1 << 40


def muladd_tensor(o, mods, ct1, ct2, addends=(), scale=None, add_scales=(), const=None):
    """(d0, d1, d2) = (s a b + sum_t u_t x_t + k, s (a d + c b) + sum_t u_t y_t, s c d) on the limbs `mods`; scale / const: per-limb lists or None;
    add_scales[t]: per-limb list"""
    a, c, b, d = ct1[0], ct1[1], ct2[0], ct2[1]
    d0, d1, d2 = o.ewe(EWE_MUL, mods, a, b), o.ewe(EWE_MAC2, mods, a, d, c, b), o.ewe(EWE_MUL, mods, c, d)
    if scale is not None:
        d0, d1, d2 = (o.ewe(EWE_MUL_CONST, mods, p, k=scale) for p in (d0, d1, d2))
    for ct, u in zip(addends, add_scales):
        d0 = o.ewe(EWE_ADD, mods, d0, None, o.ewe(EWE_MUL_CONST, mods, ct[0], k=u))
        d1 = o.ewe(EWE_ADD, mods, d1, None, o.ewe(EWE_MUL_CONST, mods, ct[1], k=u))
    if const is not None:
        d0 = add_const(d0, const, [o.moduli[m] for m in mods])
    return d0, d1, d2


def muladd(o, ell, ct1, ct2, evk, addends=(), scale=None, add_scales=(), const=None):
    """ct1, ct2, addends[t]: [2][ell][N] at level ell; evk: hmult's key.  Returns (out.c0, out.c1) at level ell - 1"""
    ids = list(range(ell))
    d0, d1, d2 = muladd_tensor(o, ids, ct1, ct2, addends, scale, add_scales, const)
    ks0, ks1 = o.keyswitch(ell, d2, evk)
    return (o.rescale(ell, o.ewe(EWE_ADD, ids, d0, None, ks0)), o.rescale(ell, o.ewe(EWE_ADD, ids, d1, None, ks1)))


def muladd_integers(o, ct1, ct2, addends, scale, add_scales, const, j, cols):
    """the definition of (d0, d1, d2) in Python integers: limb j, the entries `cols`"""
    q = o.moduli[j]
    s, k = (1 if scale is None else int(scale[j])), (0 if const is None else int(const[j]))
    v = lambda p, x: int(p[j][x])
    d0 = [(s * v(ct1[0], x) * v(ct2[0], x) + sum(int(u[j]) * v(ct[0], x) for ct, u in zip(addends, add_scales)) + k) % q for x in cols]
    d1 = [(s * (v(ct1[0], x) * v(ct2[1], x) + v(ct1[1], x) * v(ct2[0], x)) + sum(int(u[j]) * v(ct[1], x) for ct, u in zip(addends, add_scales))) % q for x in cols]
    d2 = [s * v(ct1[1], x) * v(ct2[1], x) % q for x in cols]
    return d0, d1, d2


def synthetic_constants(o, ell, seed, A, ma_scale, ma_const):
    """the op's synthetic constants: word 0 of limb j of the streams seed + 6400 (a 0 replaced by 1), seed + 6400 + 10 t (t = 1 .. A) and
    seed + 6490; scale / const None where the key is 0"""
    ids = list(range(ell))
    word0 = lambda stream: [int(v) for v in o.fill_uniform(ids, seed + stream)[:, 0]]
    scale = [v or 1 for v in word0(SCALE_STREAM)] if ma_scale else None
    add_scales = [word0(SCALE_STREAM + ADD_SCALE_STRIDE * t) for t in range(1, A + 1)]
    const = word0(CONST_STREAM) if ma_const else None
    return scale, add_scales, const


def synthetic_inputs(o, ell, seed, A, copy=0, batch_seed_stride=100000):
    """the op's synthetic streams: ct<i> from seed + 2000 (i - 1) (c1: + 1000), op `copy` of a batch + copy * stride; the key from seed + 10000.
    Returns (ct1, ct2, [ct3 ..], evk)"""
    cts = [o.synth_ct(ell, seed + copy * batch_seed_stride + 2000 * i) for i in range(2 + A)]
    return cts[0], cts[1], cts[2:], o.synth_evk(ell, seed + 10000)


def assert_ct(got, exp, what):
    assert np.array_equal(got[0], exp[0]), (what, "c0")
    assert np.array_equal(got[1], exp[1]), (what, "c1")


# ---- real data (tests/toy_ckks.py): T_3 = 2 T_2 x - x
def real_case(toy, ell):
    """ell: the level of x and of the square (5).  Returns what the two ops need and the exact result:
    x (fresh, level ell), the relinearisation key in full, the square's constants at level ell, hmuladd's constants at level ell - 1 (scale, u_1), and
    exact = (2 E_2 X - D q X) with q = q_{ell-1}: the value Dec(out) q_{ell-2} q_{ell-1} is held to"""
    from dot_ref import negacyclic_small
    s = np.array([int(x) for x in toy.s])
    evk_full = toy.gen_evk(negacyclic_small(s, s).astype(object))
    m = toy.rng.integers(-50, 50, toy.N)
    x = toy.encrypt(m.astype(object) * DELTA, ell)
    sq_scale = [2] * ell
    sq_const = [(-(DELTA * DELTA)) % toy.o.moduli[j] for j in range(ell)]
    q = toy.o.moduli[ell - 1]
    D = (DELTA * DELTA + q // 2) // q
    scale = [2] * (ell - 1)
    u1 = [toy.o.moduli[j] - D % toy.o.moduli[j] for j in range(ell - 1)]
    mmm = negacyclic_small(negacyclic_small(m, m), m).astype(object)      # below 50^3 N^2 < 2^43
    exact = 2 * (2 * mmm - m.astype(object)) * DELTA ** 3 - D * q * m.astype(object) * DELTA
    return x, evk_full, sq_scale, sq_const, scale, u1, D, exact


def error_bound(toy, ell, D):
    """the bound of the module docstring on |Dec(out) q_{ell-2} - (2 Y X - D X)| for hmuladd at level ell - 1"""
    ql = toy.o.moduli[ell - 2]
    return 2 * (ql << 12) + D * FRESH_BOUND + 2 * toy.N * (1 << 13) * 50 * DELTA


def decryption_error(toy, out, ell, D, exact):
    """max |Dec(out) q_{ell-2} q_{ell-1} - exact| over the coefficients, and the bound times q_{ell-1}; out at level ell - 2"""
    got, _ = toy.decrypt(np.stack(out), ell - 2)
    ql, q = toy.o.moduli[ell - 2], toy.o.moduli[ell - 1]
    assert max(abs(int(g)) for g in got) > 1 << 30   # a signal, not zeros
    return max(abs(int(g) * ql * q - int(e)) for g, e in zip(got, exact)), error_bound(toy, ell, D) * q
