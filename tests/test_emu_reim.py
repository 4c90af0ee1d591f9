"""The per-thread core of hm_reim_split (homulator_amd/csrc/hm_rec_core.h: hm_reim_thread, the kernel of hreim) on the CPU, no GPU:
tests/emu/hm_emu_reim.cpp compiles the device header with g++, once per arithmetic back-end (HM_GENERIC 0 and 1), builds the records as the entry
point does, the constant w = -psi^(N/2) from the same root table, and runs every thread of the chosen workgroups.  Checked against Python integers:
re = x + y mod q, im = U (x - y) mod q with U = w on entries [0, N/2) and q - w on [N/2, N).
logN 13 to 17 with the first chunk, the chunks just below and just above N/2 and the last chunk (the choice between the two constants is made per
chunk and moves with N).  Fills: uniform, all 0, all q - 1, x = y.  Moduli: the smallest and the largest the back-end accepts (mont32: 18 2^32 + 1
and the largest prime h 2^32 + 1 below 2^60; generic: just above 2^20, or at N = 2^17 the first one there is, below 2^23, and just below 2^60) and the 36-bit chain's (generic)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from oracle.homoracle import Oracle, chain_below

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
u64, u32, vp = C.c_uint64, C.c_uint32, C.c_void_p
SOURCES = [os.path.join(HERE, "emu", "hm_emu_reim.cpp"), os.path.join(ROOT, "homulator_amd", "csrc", "hm_params.cpp")]
NARROW_MONT32 = 18 * 2**32 + 1      # the smallest prime h 2^32 + 1: 37 bits, 1 mod 2N for every ring
LOGNS = [13, 14, 15, 16, 17]
FILLS = ["uniform", "zero", "q-1", "x=y"]
GUARD = np.uint64(0xDEADBEEFDEADBEEF)


def narrowest(logN):
    """the largest prime = 1 mod 2N below the first power of two above 2^20 that has one (2^21 up to N = 2^16, 2^23 at N = 2^17)"""
    for bits in range(21, 30):
        try:
            q = chain_below(logN, bits, 1)[0]
        except Exception:
            continue
        if q >= 1 << 20:
            return q
    raise AssertionError("no narrow prime")


def chain_moduli(chain, logN):
    if chain == "mont32":
        m = Oracle(logN, 3, 1).moduli
        return [m[0], m[1], NARROW_MONT32, m[2]]
    wide, mid = chain_below(logN, 60, 1), chain_below(logN, 36, 2)
    return [wide[0], narrowest(logN), mid[0], mid[1]]


@pytest.fixture(scope="module", params=[(0, "mont32"), (1, "mont32"), (1, "mixed")], ids=["mont32-build", "generic-build", "generic-build-mixed-widths"])
def env(request, tmp_path_factory):
    """(library, chain name): the emulator of one arithmetic build, and the chain it runs"""
    generic, chain = request.param
    so = tmp_path_factory.mktemp("emu_reim") / f"libhm_emu_reim_{generic}.so"
    subprocess.check_call(["g++"] + (["-DHM_GENERIC=1"] if generic else []) + ["-O2", "-std=c++17", "-fPIC", "-shared", "-Wall", "-Wno-unknown-pragmas", "-o", str(so)] + SOURCES)
    lib = C.CDLL(str(so))
    assert lib.emu_reim_generic() == generic
    lib.emu_reim_rec_words.restype = u32
    lib.emu_reim.argtypes = [vp, u32, u32] + [vp] * 9 + [u32, vp, u32, vp]
    return lib, chain


def ptr(a):
    return None if a is None else a.ctypes.data_as(vp)


def u(v):
    return np.array(v, dtype=np.uint32)


def test_record_size_is_a_multiple_of_16_bytes(env):
    lib, _ = env
    assert lib.emu_reim_rec_words() * 4 % 16 == 0 and lib.emu_reim_rec_words() >= 5 + 4     # five ids, two 64-bit constants


@pytest.mark.parametrize("logN", LOGNS)
def test_the_constant_squares_to_minus_one_and_is_the_oracles(env, logN):
    """w as the entry point derives it: w^2 = -1 mod q, and on the default chain it is entry 0 of the oracle's transform of -X^(N/2)"""
    lib, chain = env
    mods = chain_moduli(chain, logN)
    m, w = np.array(mods, dtype=np.uint64), np.zeros(len(mods), dtype=np.uint64)
    z = np.zeros(1, dtype=np.uint64)
    keep = [u([0]), u([0])]
    assert lib.emu_reim(ptr(m), len(mods), logN, ptr(z), ptr(keep[0]), ptr(z), ptr(keep[0]), ptr(z), ptr(keep[0]), ptr(z), ptr(keep[0]), ptr(keep[1]),
                        0, ptr(keep[0]), 0, ptr(w)) == 0
    for q, wv in zip(mods, w):
        assert 0 < int(wv) < q and int(wv) ** 2 % q == q - 1
    if chain == "mont32":
        o = Oracle(logN, 3, 1)
        p = np.zeros((1, o.N), dtype=np.uint64)
        p[0][o.N // 2] = o.moduli[0] - 1
        assert int(o.ntt([0], p)[0][0]) == int(w[0])


@pytest.mark.parametrize("logN", LOGNS)
def test_records_with_permuted_and_repeated_limbs(env, logN):
    """the thread function over whole workgroups: one entry per modulus plus a fifth that reads entry 0's two input limbs again (repeated limbs)
    into output limbs of its own, the inputs and outputs at permuted limbs; the first chunk, the two chunks on either side of N/2 and the last chunk of every entry; the outputs
    of the chunks that did not run keep their guard value"""
    lib, chain = env
    mods = chain_moduli(chain, logN)
    N, M = 1 << logN, len(mods)
    half = N // 1024
    chunks = [0, half - 1, half, N // 512 - 1]
    rng = np.random.default_rng(300 + logN)
    m = np.array(mods, dtype=np.uint64)
    lx, ly = [2, 0, 3, 1, 2], [1, 3, 0, 2, 1]
    lre, lim, ids = [3, 2, 0, 1, 4], [0, 4, 2, 3, 1], [0, 1, 2, 3, 0]
    n = len(ids)
    w = np.zeros(M, dtype=np.uint64)
    for fill in FILLS:
        x, y = np.zeros((M, N), dtype=np.uint64), np.zeros((M, N), dtype=np.uint64)
        for i in range(M):
            q = mods[i]
            x[lx[i]] = {"uniform": rng.integers(0, q, N, dtype=np.uint64), "zero": 0, "q-1": q - 1, "x=y": rng.integers(0, q, N, dtype=np.uint64)}[fill]
            y[ly[i]] = x[lx[i]] if fill == "x=y" else {"uniform": rng.integers(0, q, N, dtype=np.uint64), "zero": 0, "q-1": q - 1}[fill]
        re, im = np.full((n, N), GUARD, dtype=np.uint64), np.full((n, N), GUARD, dtype=np.uint64)
        keep = [u(lx), u(ly), u(lre), u(lim), u(ids), u(chunks)]
        assert lib.emu_reim(ptr(m), M, logN, ptr(x), ptr(keep[0]), ptr(y), ptr(keep[1]), ptr(re), ptr(keep[2]), ptr(im), ptr(keep[3]), ptr(keep[4]), n,
                            ptr(keep[5]), len(chunks), ptr(w)) == 0
        ran = np.zeros(N, dtype=bool)
        for ch in chunks:
            ran[ch * 512:ch * 512 + 512] = True
        for i in range(n):
            q, wv = mods[ids[i]], int(w[ids[i]])
            for ch in chunks:
                sl = range(ch * 512, ch * 512 + 512)
                xs, ys = [int(x[lx[i]][e]) for e in sl], [int(y[ly[i]][e]) for e in sl]
                uu = wv if ch < half else q - wv
                assert [int(v) for v in re[lre[i]][ch * 512:ch * 512 + 512]] == [(a + b) % q for a, b in zip(xs, ys)], (fill, i, ch)
                assert [int(v) for v in im[lim[i]][ch * 512:ch * 512 + 512]] == [uu * (a - b) % q for a, b in zip(xs, ys)], (fill, i, ch)
            assert np.all(re[lre[i]][~ran] == GUARD) and np.all(im[lim[i]][~ran] == GUARD)
        if fill == "x=y":
            assert not im[:, ran].any()     # x - y = 0 everywhere


@pytest.mark.parametrize("generic,chain", [(0, "mont32"), (1, "mont32"), (1, "mixed")])
def test_stand_alone_program_under_the_sanitizers(tmp_path, generic, chain):
    """tests/emu/hm_emu_reim_main.cpp with its own main, compiled with the sanitizers and run as a process of its own (nothing is loaded into
    Python): every fill on every modulus, every chunk of every entry; every buffer is sized exactly"""
    exe = tmp_path / "hm_emu_reim_main"
    subprocess.check_call(["g++"] + (["-DHM_GENERIC=1"] if generic else []) + ["-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-Wall", "-Wno-unknown-pragmas", "-o", str(exe), os.path.join(HERE, "emu", "hm_emu_reim_main.cpp")] + SOURCES)
    r = subprocess.run([str(exe), "13"] + [str(q) for q in chain_moduli(chain, 13)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "bad=0" in r.stdout and "cases=4" in r.stdout, r.stdout + r.stderr
