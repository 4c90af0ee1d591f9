"""The per-thread core of hm_inner_product_rotsum (homulator_amd/csrc/hm_ip_core.h: hm_ip_rotsum_thread) on the CPU against Python integers, no
GPU: tests/emu/hm_emu_rotsum.cpp compiles the device header with g++, once per arithmetic back-end (HM_GENERIC 0 and 1, as tests/emu/Makefile
defines them), and runs every thread of the first and the last workgroup of every record.  n_ct = 16 with TERMS = 4 and every operand q - 1
puts 64 (q - 1)^2 into each 128-bit accumulator and 16 (q - 1) into the addend's 64-bit one: the largest values the reductions ever see."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest
import sympy

from oracle.homoracle import Oracle, chain_below

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
LOGN = 13
N = 1 << LOGN
CHUNKS = [0, N // 512 - 1]
GUARD = 0x5A5A5A5A5A5A5A5A


@pytest.fixture(scope="module", params=[0, 1], ids=["mont32-build", "generic-build"])
def emu(request, tmp_path_factory):
    so = tmp_path_factory.mktemp("emu_rotsum") / f"libhm_emu_rotsum_{request.param}.so"
    subprocess.check_call(["g++"] + (["-DHM_GENERIC=1"] if request.param else []) +
                          ["-O2", "-std=c++17", "-fPIC", "-shared", "-Wall", "-Wno-unknown-pragmas", "-o", str(so),
                           os.path.join(HERE, "emu", "hm_emu_rotsum.cpp"), os.path.join(ROOT, "homulator_amd", "csrc", "hm_params.cpp")])
    lib = C.CDLL(str(so))
    assert lib.emu_rotsum_generic() == request.param
    lib.emu_ip_rotsum.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32] + [C.c_void_p] * 11 + [C.c_uint32] * 3 + [C.c_void_p, C.c_void_p, C.c_uint32]
    return lib


@pytest.fixture(scope="module")
def moduli():
    """the largest and the smallest modulus of the default chain (45 + 15 primes h 2^32 + 1) and of the 60-bit survey chain, and the largest
    31-bit prime = 1 mod 2N"""
    default = Oracle(LOGN, 45, 15).moduli
    survey = chain_below(LOGN, 60, 60)
    q31 = ((1 << 31) - 1) // (2 * N) * (2 * N) + 1
    while not sympy.isprime(q31):
        q31 -= 2 * N
    assert default[0] == max(default) and default[-1] == min(default) and survey[0] == max(survey) and survey[-1] == min(survey)
    assert (1 << 30) < q31 < (1 << 31)
    return [default[0], default[-1], survey[0], survey[-1], q31]


def p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def brev(i, bits):
    return int(format(i, f"0{bits}b")[::-1], 2)


def auto_src():
    """src(g)[i]: the stored (bit-reversed evaluation order) index sigma_g reads output i from — hm_automorph's index map, from its definition"""
    cache = {}

    def of(g):
        if g not in cache:
            cache[g] = np.array([brev(((g * (2 * brev(i, LOGN) + 1)) % (2 * N) - 1) >> 1, LOGN) for i in range(N)])
        return cache[g]
    return of


SRC = auto_src()


def elements(G, same=False):
    """3, 2N - 1, 2N - 3, then 5^c: both the in-order and the swapped source pair occur (checked below); same: ciphertexts 0 and 1 share one"""
    gs = ([3, 2 * N - 1, 2 * N - 3] + [pow(5, c, 2 * N) for c in range(3, 16)])[:G]
    if same and G > 1:
        gs[1] = gs[0]
    return gs


def run(emu, moduli, G, T, fill, addend_on, same=False):
    n = len(moduli)
    rng = np.random.default_rng(1000 * G + 10 * T + len(fill) + int(same))
    gs = elements(G, same)
    xl = rng.permutation(G * n * T).astype(np.uint32)            # [c][n][T]
    yl = rng.permutation(G * n * 2 * T).astype(np.uint32)        # [c][n][2][T]
    ol = rng.permutation(n * 2).astype(np.uint32)
    al = rng.permutation(G * n).astype(np.uint32)                # [c][n]
    aol = rng.permutation(n).astype(np.uint32)
    has = [addend_on == "all" or (addend_on == "some" and i % 2 == 0) for i in range(n)]
    for c in range(G):
        for i in range(n):
            if not has[i]:
                al[c * n + i] = 0xFFFFFFFF

    def filled(rows, mod_of_row):
        buf = np.zeros((rows, N), dtype=np.uint64)
        for r in range(rows):
            q = mod_of_row(r)
            if q is not None:
                buf[r] = q - 1 if fill == "q-1" else 0 if fill == "zero" else rng.integers(0, q, N, dtype=np.uint64)
        return buf
    mod_x, mod_y, mod_a = {}, {}, {}
    for c in range(G):
        for i in range(n):
            for j in range(T):
                mod_x[xl[(c * n + i) * T + j]] = moduli[i]
                for k in range(2):
                    mod_y[yl[((c * n + i) * 2 + k) * T + j]] = moduli[i]
            if has[i]:
                mod_a[al[c * n + i]] = moduli[i]
    X, Y, A = filled(G * n * T, mod_x.get), filled(G * n * 2 * T, mod_y.get), filled(G * n, mod_a.get)
    out, aout = np.full((n * 2, N), GUARD, dtype=np.uint64), np.full((n, N), GUARD, dtype=np.uint64)
    ml, mods, chunks, gl = np.array(moduli, dtype=np.uint64), np.arange(n, dtype=np.uint32), np.array(CHUNKS, dtype=np.uint32), np.array(gs, dtype=np.uint32)
    use_add = addend_on != "none"
    assert emu.emu_ip_rotsum(p(ml), n, LOGN, p(X), p(xl), p(Y), p(yl), p(A) if use_add else None, p(al) if use_add else None, p(out), p(ol),
                             p(aout) if use_add else None, p(aol) if use_add else None, p(mods), n, T, G, p(gl), p(chunks), len(chunks)) == 0
    cols = np.concatenate([np.arange(c * 512, (c + 1) * 512) for c in CHUNKS])
    rest = np.setdiff1d(np.arange(N), cols)
    for i, q in enumerate(moduli):
        for k in range(2):
            exp = [0] * len(cols)
            for c in range(G):
                src = SRC(gs[c])[cols]
                for j in range(T):
                    xs, ys = X[xl[(c * n + i) * T + j]][src], Y[yl[((c * n + i) * 2 + k) * T + j]][cols]
                    exp = [e + int(a) * int(b) for e, a, b in zip(exp, xs, ys)]
            got = out[ol[i * 2 + k]]
            assert [int(v) for v in got[cols]] == [e % q for e in exp], (G, T, fill, q, k)
            assert np.all(got[rest] == GUARD)
        if has[i]:
            exp = [0] * len(cols)
            for c in range(G):
                exp = [e + int(a) for e, a in zip(exp, A[al[c * n + i]][SRC(gs[c])[cols]])]
            assert [int(v) for v in aout[aol[i]][cols]] == [e % q for e in exp], (G, T, fill, q)
            assert np.all(aout[aol[i]][rest] == GUARD)
        else:
            assert np.all(aout[aol[i]] == GUARD)


def test_elements_cover_the_in_order_and_the_swapped_pair():
    """the source of the even output 2m is an even index (pair in order) for some elements and an odd one (pair swapped) for others"""
    parity = {g: int(SRC(g)[0] & 1) for g in elements(16)}
    assert set(parity.values()) == {0, 1}, parity
    for g in elements(16):
        s = SRC(g)
        assert np.all(s[1::2] == s[0::2] ^ 1)      # an aligned pair comes from one aligned pair


@pytest.mark.parametrize("fill", ["q-1", "zero", "random"])
@pytest.mark.parametrize("T", [1, 4])
@pytest.mark.parametrize("G", [1, 2, 16])
def test_core_against_python_integers(emu, moduli, G, T, fill):
    """one record per modulus, every limb list a random permutation of its buffer, every entry with addend sources"""
    run(emu, moduli, G, T, fill, "all")
    if fill == "q-1" and G == 16 and T == 4:   # the accumulator bounds the kernel's comment states
        assert 64 * (max(moduli) - 1) ** 2 < 1 << 126 and 16 * (max(moduli) - 1) < 1 << 64


def test_two_ciphertexts_under_the_same_element(emu, moduli):
    run(emu, moduli, 3, 3, "random", "all", same=True)


@pytest.mark.parametrize("addend_on", ["none", "some"])
def test_addend_is_optional_per_entry(emu, moduli, addend_on):
    run(emu, moduli, 3, 2, "random", addend_on)


def test_counts_out_of_range_are_refused(emu, moduli):
    z = np.zeros(8, dtype=np.uint64)
    l = np.zeros(8, dtype=np.uint32)
    ml = np.array(moduli, dtype=np.uint64)
    for T, G in ((0, 1), (5, 1), (1, 0), (1, 17)):
        assert emu.emu_ip_rotsum(p(ml), len(moduli), LOGN, p(z), p(l), p(z), p(l), None, None, p(z), p(l), None, None, p(l), 0, T, G, p(l), p(l), 0) == 2
