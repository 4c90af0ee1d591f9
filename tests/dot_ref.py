"""CPU reference of hdot from oracle primitives only, following the definition literally and independent of the host plan:
tensor every pair (MUL, MAC2, MUL), add the d's with EWE_ADD, then hmult's tail: key switch of d2, the two adds, the two rescales."""
import numpy as np

from oracle.homoracle import EWE_ADD, EWE_MAC2, EWE_MUL


def tensor(o, mods, c00, c01, c10, c11):
    """(d0, d1, d2) of one pair of ciphertexts (c00, c01), (c10, c11) on the limbs `mods`"""
    return o.ewe(EWE_MUL, mods, c00, c10), o.ewe(EWE_MAC2, mods, c00, c11, c01, c10), o.ewe(EWE_MUL, mods, c01, c11)


def tensor_sum(o, mods, pairs):
    """sum over the pairs [(c00, c01, c10, c11), ...] of their tensor products: the canonical residues of the exact integer sums"""
    d = None
    for p in pairs:
        t = tensor(o, mods, *p)
        d = t if d is None else tuple(o.ewe(EWE_ADD, mods, x, None, y) for x, y in zip(d, t))
    return d


def dot(o, ell, cts, evk):
    """cts: 2T ciphertexts [2][ell][N] at level ell, pair t = (cts[2t], cts[2t + 1]); evk: hmult's key.  Returns (out.c0, out.c1) at level ell - 1"""
    assert len(cts) >= 2 and len(cts) % 2 == 0
    ids = list(range(ell))
    d0, d1, d2 = tensor_sum(o, ids, [(cts[2 * t][0], cts[2 * t][1], cts[2 * t + 1][0], cts[2 * t + 1][1]) for t in range(len(cts) // 2)])
    ks0, ks1 = o.keyswitch(ell, d2, evk)
    return (o.rescale(ell, o.ewe(EWE_ADD, ids, d0, None, ks0)), o.rescale(ell, o.ewe(EWE_ADD, ids, d1, None, ks1)))


def synthetic_inputs(o, ell, T, seed, copy=0, batch_seed_stride=100000):
    """the op's synthetic streams: ct<i + 1> from seed + 2000 i (c1: + 1000), op `copy` of a batch + copy * stride; the key from seed + 10000"""
    return [o.synth_ct(ell, seed + 2000 * i + copy * batch_seed_stride) for i in range(2 * T)], o.synth_evk(ell, seed + 10000)


def assert_ct(got, exp, what):
    assert np.array_equal(got[0], exp[0]), (what, "c0")
    assert np.array_equal(got[1], exp[1]), (what, "c1")


# ---- real data (tests/toy_ckks.py)
def negacyclic_small(a, b):
    """exact product mod X^N + 1 of small integer polynomials (int64 convolution)"""
    n = len(a)
    full = np.convolve(np.asarray(a, dtype=np.int64), np.asarray(b, dtype=np.int64))
    res = full[:n].copy()
    res[: n - 1] -= full[n:]
    return res


def real_pairs(toy, T, ell):
    """T pairs of toy ciphertexts of small messages a 2^40, the relinearisation key, and the exact sum of the message products"""
    s = np.array([int(x) for x in toy.s])
    evk = toy.evk_at_level(toy.gen_evk(negacyclic_small(s, s).astype(object)), ell)
    cts, exact = [], np.zeros(toy.N, dtype=object)
    for _ in range(T):
        a1, a2 = toy.rng.integers(-50, 50, toy.N), toy.rng.integers(-50, 50, toy.N)
        cts += [toy.encrypt(a1.astype(object) * (1 << 40), ell), toy.encrypt(a2.astype(object) * (1 << 40), ell)]
        exact = exact + negacyclic_small(a1, a2).astype(object) * (1 << 80)
    return cts, evk, exact


def decryption_error(toy, out, ell, exact):
    """max |Dec(out) q_last - sum_t m_t m'_t|, and the bound: T x the one tests/test_gpu_real_data.py holds a single hmult to (q_last << 12)"""
    got, _ = toy.decrypt(np.stack(out), ell - 1)
    ql = toy.o.moduli[ell - 1]
    assert max(abs(int(g)) for g in got) > 1 << 30   # a signal, not zeros
    return max(abs(int(g) * ql - int(e)) for g, e in zip(got, exact)), ql << 12
