"""CPU reference of hdotadd from oracle primitives only, following the definition literally and independent of the host plan:
tensor every pair (MUL, MAC2, MUL), multiply the pair's three polynomials by its per-limb scalars (MUL_CONST), add the pairs with EWE_ADD, per addend
multiply both components by the addend's per-limb scalars (MUL_CONST) and add them onto d0 and d1 (ADD), add the per-limb constants to every
evaluation-form entry of d0 (numpy: the oracle has no such opcode), then hmult's tail: key switch of d2, the two adds, the two rescales.

The real-data case (tests/toy_ckks.py; LOGN 13, L 6, level 5, alpha 2, Delta = 2^40): five fresh encryptions of m_i Delta (|m_i| < 50), T = 2 with
s = (3, -2) (the -2 stored as q_j - 2), A = 1 with u = 5 Delta mod q_j, k = 7 Delta^2 mod q_j (the constant polynomial: the same value on every
evaluation-form entry).  Dec(out) q_last = 3 m_1 m_2 Delta^2 - 2 m_3 m_4 Delta^2 + 5 Delta^2 m_5 + 7 Delta^2 + err.  The bound on |err| per coefficient,
from the bounds the tree already uses:
  * every product goes through the op's one key switch and rescale as one hmult does (tests/test_gpu_real_data.py: q_last << 12), times the
    scalar, as dot_ref.decryption_error (one per pair) and muladd_ref.error_bound (times s) take it:      (|s_1| + |s_2|) (q_last << 12)
  * the addend: its fresh error, 8 sigma of Toy.small_err, times |u| = 5 Delta:                          5 Delta FRESH_BOUND
  * the constant is exact.
With q_last below 2^60 the sum is about 2^74; the signal is above 2^90."""
import numpy as np

from dot_ref import negacyclic_small, tensor
from muladd_ref import DELTA, FRESH_BOUND
from oracle.homoracle import EWE_ADD, EWE_MUL_CONST
from square_ref import add_const

SCALE_STREAM, ADD_SCALE_STREAM, STREAM_STRIDE, CONST_STREAM = 6050, 7050, 50, 7900


def dotadd_tensor(o, mods, pairs, addends=(), scales=None, add_scales=(), const=None):
    """(d0, d1, d2) = (sum_t s_t a_t b_t + sum_r u_r x_r + k, sum_t s_t (a_t d_t + c_t b_t) + sum_r u_r y_r, sum_t s_t c_t d_t) on the limbs `mods`;
    pairs[t] = (ct, ct'), [2][.][N] each; scales: None or per pair a per-limb list; add_scales[r]: per-limb list; const: per-limb list or None"""
    d = None
    for t, (x, y) in enumerate(pairs):
        p = tensor(o, mods, x[0], x[1], y[0], y[1])
        if scales is not None:
            p = tuple(o.ewe(EWE_MUL_CONST, mods, v, k=scales[t]) for v in p)
        d = p if d is None else tuple(o.ewe(EWE_ADD, mods, v, None, w) for v, w in zip(d, p))
    d0, d1, d2 = d
    for ct, u in zip(addends, add_scales):
        d0 = o.ewe(EWE_ADD, mods, d0, None, o.ewe(EWE_MUL_CONST, mods, ct[0], k=u))
        d1 = o.ewe(EWE_ADD, mods, d1, None, o.ewe(EWE_MUL_CONST, mods, ct[1], k=u))
    if const is not None:
        d0 = add_const(d0, const, [o.moduli[m] for m in mods])
    return d0, d1, d2


def dotadd(o, ell, pairs, evk, addends=(), scales=None, add_scales=(), const=None):
    """pairs[t] = (ct<2t+1>, ct<2t+2>), addends[r]: [2][ell][N] at level ell; evk: hmult's key.  Returns (out.c0, out.c1) at level ell - 1"""
    ids = list(range(ell))
    d0, d1, d2 = dotadd_tensor(o, ids, pairs, addends, scales, add_scales, const)
    ks0, ks1 = o.keyswitch(ell, d2, evk)
    return (o.rescale(ell, o.ewe(EWE_ADD, ids, d0, None, ks0)), o.rescale(ell, o.ewe(EWE_ADD, ids, d1, None, ks1)))


def dotadd_integers(o, pairs, addends, scales, add_scales, const, j, cols):
    """the definition of (d0, d1, d2) in Python integers: limb j, the entries `cols`"""
    q = o.moduli[j]
    s = [1 if scales is None else int(scales[t][j]) for t in range(len(pairs))]
    k = 0 if const is None else int(const[j])
    v = lambda p, x: int(p[j][x])
    lin = lambda c, x: sum(int(u[j]) * v(ct[c], x) for ct, u in zip(addends, add_scales))
    d0 = [(sum(st * v(a[0], x) * v(b[0], x) for st, (a, b) in zip(s, pairs)) + lin(0, x) + k) % q for x in cols]
    d1 = [(sum(st * (v(a[0], x) * v(b[1], x) + v(a[1], x) * v(b[0], x)) for st, (a, b) in zip(s, pairs)) + lin(1, x)) % q for x in cols]
    d2 = [sum(st * v(a[1], x) * v(b[1], x) for st, (a, b) in zip(s, pairs)) % q for x in cols]
    return d0, d1, d2


def synthetic_constants(o, ell, seed, T, A, da_scale, da_const):
    """the op's synthetic constants: word 0 of limb j of the streams seed + 6050 + 50 t (t = 1 .. T, a 0 replaced by 1), seed + 7050 + 50 r
    (r = 1 .. A) and seed + 7900; scales / const None where the key is 0"""
    ids = list(range(ell))
    word0 = lambda stream: [int(v) for v in o.fill_uniform(ids, seed + stream)[:, 0]]
    scales = [[v or 1 for v in word0(SCALE_STREAM + STREAM_STRIDE * t)] for t in range(1, T + 1)] if da_scale else None
    add_scales = [word0(ADD_SCALE_STREAM + STREAM_STRIDE * r) for r in range(1, A + 1)]
    const = word0(CONST_STREAM) if da_const else None
    return scales, add_scales, const


def synthetic_inputs(o, ell, seed, T, A, copy=0, batch_seed_stride=100000):
    """the op's synthetic streams: ct<i> from seed + 2000 (i - 1) (c1: + 1000), op `copy` of a batch + copy * stride; the key from seed + 10000.
    Returns (pairs, addends, evk)"""
    cts = [o.synth_ct(ell, seed + copy * batch_seed_stride + 2000 * i) for i in range(2 * T + A)]
    return [(cts[2 * t], cts[2 * t + 1]) for t in range(T)], cts[2 * T:], o.synth_evk(ell, seed + 10000)


def input_streams(T, A, ell):
    """every stream offset (from seed) the op's inputs are filled from: ct<i + 1>.c<k> limb j = 2000 i + 1000 k + j"""
    return {2000 * i + 1000 * k + j for i in range(2 * T + A) for k in range(2) for j in range(ell)}


def constant_streams(T, A, ell):
    """by name, the stream offsets of the op's synthetic constants"""
    s = {f"scale{t}": [SCALE_STREAM + STREAM_STRIDE * t + j for j in range(ell)] for t in range(1, T + 1)}
    s.update({f"addscale{r}": [ADD_SCALE_STREAM + STREAM_STRIDE * r + j for j in range(ell)] for r in range(1, A + 1)})
    s["const"] = [CONST_STREAM + j for j in range(ell)]
    return s


def assert_ct(got, exp, what):
    assert np.array_equal(got[0], exp[0]), (what, "c0")
    assert np.array_equal(got[1], exp[1]), (what, "c1")


# ---- real data (tests/toy_ckks.py): 3 m1 m2 - 2 m3 m4 + 5 m5 + 7
REAL_S = (3, -2)


def real_case(toy, ell):
    """Returns the five fresh ciphertexts at level ell, the relinearisation key at level ell, the constants (scales, [u], const) and
    exact = 3 m1 m2 Delta^2 - 2 m3 m4 Delta^2 + 5 Delta^2 m5 + 7 Delta^2: the value Dec(out) q_{ell-1} is held to"""
    s = np.array([int(x) for x in toy.s])
    evk = toy.evk_at_level(toy.gen_evk(negacyclic_small(s, s).astype(object)), ell)
    ms = [toy.rng.integers(-50, 50, toy.N) for _ in range(5)]
    cts = [toy.encrypt(m.astype(object) * DELTA, ell) for m in ms]
    qs = [toy.o.moduli[j] for j in range(ell)]
    scales = [[sv % q for q in qs] for sv in REAL_S]
    u = [5 * DELTA % q for q in qs]
    const = [7 * DELTA * DELTA % q for q in qs]
    exact = (REAL_S[0] * negacyclic_small(ms[0], ms[1]).astype(object) + REAL_S[1] * negacyclic_small(ms[2], ms[3]).astype(object)
             + 5 * ms[4].astype(object)) * (DELTA * DELTA)
    exact[0] += 7 * DELTA * DELTA
    return cts, evk, scales, u, const, exact


def error_bound(toy, ell):
    """the bound of the module docstring on |Dec(out) q_{ell-1} - exact| per coefficient"""
    ql = toy.o.moduli[ell - 1]
    return (abs(REAL_S[0]) + abs(REAL_S[1])) * (ql << 12) + 5 * DELTA * FRESH_BOUND


def decryption_error(toy, out, ell, exact):
    """max |Dec(out) q_{ell-1} - exact| over the coefficients, and the bound; out at level ell - 1"""
    got, _ = toy.decrypt(np.stack(out), ell - 1)
    ql = toy.o.moduli[ell - 1]
    assert max(abs(int(g)) for g in got) > 1 << 30   # a signal, not zeros
    return max(abs(int(g) * ql - int(e)) for g, e in zip(got, exact)), error_bound(toy, ell)
