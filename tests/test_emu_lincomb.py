"""The per-thread core of hm_lincomb (homulator_amd/csrc/hm_rec_core.h: hm_lincomb_thread, the kernel of hlincomb) on the CPU, no GPU:
tests/emu/hm_emu_lincomb.cpp compiles the device header with g++, once per arithmetic back-end (HM_GENERIC 0 and 1), builds the records as the entry
point does and runs every thread of the chosen workgroups.  Checked against Python integers: out = sum_t s_t x_t + k mod q.
T: 1, 2, 3, 16 (no round of the two-term loop, the tail behind it, one round, the most).  Fills: uniform, all 0, all q - 1.  Scalars: 0, 1, q - 1,
random.  Constants: none, 0, q - 1, random.  Moduli: the smallest and the largest the back-end accepts (mont32: 18 2^32 + 1 and the largest prime
h 2^32 + 1 below 2^60; generic: just above 2^20 and just below 2^60) and the 36-bit chain's (generic).  The worst case, T = 16 with every input,
scalar and the constant q - 1 at the largest modulus, puts 16 (q - 1)^2 + q - 1 < 2^125 into the accumulator."""
import ctypes as C
import itertools
import os
import subprocess

import numpy as np
import pytest

from oracle.homoracle import Oracle, chain_below

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
u64, u32, vp = C.c_uint64, C.c_uint32, C.c_void_p
SOURCES = [os.path.join(HERE, "emu", "hm_emu_lincomb.cpp"), os.path.join(ROOT, "homulator_amd", "csrc", "hm_params.cpp")]
NARROW_MONT32 = 18 * 2**32 + 1      # the smallest prime h 2^32 + 1: 37 bits, 1 mod 2N for every ring
LOGN = 13
TERMS = [1, 2, 3, 16]
FILLS = ["uniform", "zero", "q-1"]
SCALES = ["0", "1", "q-1", "random"]
CONSTS = [None, "0", "q-1", "random"]


def chain_moduli(chain, logN=LOGN):
    if chain == "mont32":
        m = Oracle(logN, 3, 1).moduli
        return [m[0], m[1], NARROW_MONT32, m[2]]
    wide, narrow, mid = chain_below(logN, 60, 1), chain_below(logN, 21, 1), chain_below(logN, 36, 2)
    return [wide[0], narrow[0], mid[0], mid[1]]


@pytest.fixture(scope="module", params=[(0, "mont32"), (1, "mont32"), (1, "mixed")], ids=["mont32-build", "generic-build", "generic-build-mixed-widths"])
def env(request, tmp_path_factory):
    """(library, moduli): the emulator of one arithmetic build, and the chain it runs"""
    generic, chain = request.param
    so = tmp_path_factory.mktemp("emu_lincomb") / f"libhm_emu_lincomb_{generic}.so"
    subprocess.check_call(["g++"] + (["-DHM_GENERIC=1"] if generic else []) + ["-O2", "-std=c++17", "-fPIC", "-shared", "-Wall", "-Wno-unknown-pragmas", "-o", str(so)] + SOURCES)
    lib = C.CDLL(str(so))
    assert lib.emu_lincomb_generic() == generic
    lib.emu_lincomb_rec_words.argtypes = [u32]
    lib.emu_lincomb_rec_words.restype = u32
    lib.emu_lincomb.argtypes = [vp, u32, u32, vp, vp, vp, vp, vp, u32, u32, vp, vp, vp, u32]
    return lib, chain_moduli(chain)


def ptr(a):
    return None if a is None else a.ctypes.data_as(vp)


def pick(kind, q, rng):
    return {"0": 0, "1": 1, "q-1": q - 1}[kind] if kind != "random" else int(rng.integers(0, q))


def test_record_size_is_a_multiple_of_16_bytes(env):
    lib, _ = env
    for T in range(1, 17):
        assert lib.emu_lincomb_rec_words(T) * 4 % 16 == 0 and lib.emu_lincomb_rec_words(T) >= 4 + 3 * T


@pytest.mark.parametrize("T", TERMS)
def test_records_with_permuted_and_repeated_limbs(env, T):
    """the thread function over whole workgroups: one entry per modulus, the inputs at permuted limbs, one limb read by two entries (and, at T >= 2,
    twice by one entry), the first and the last chunk of every entry; the outputs of the chunks that did not run keep their guard value"""
    lib, mods = env
    N, M = 1 << LOGN, len(mods)
    rng = np.random.default_rng(100 + T)
    m = np.array(mods, dtype=np.uint64)
    qmin = min(mods)          # a shared limb holds residues of every modulus that reads it
    n_in = M * T
    li = [(e * 7 + 3) % n_in for e in range(n_in)]
    li[n_in - 1] = li[0]      # entries 0 and M - 1 share a limb
    if T >= 2:
        li[1] = li[0]         # entry 0 reads one limb twice
    shared = {li[0]}
    lo, ids, chunks = [3, 2, 0, 1], [0, 1, 2, 3], [0, N // 512 - 1]
    u = lambda v: np.array(v, dtype=np.uint32)
    for fill in FILLS:
        x = np.zeros((n_in, N), dtype=np.uint64)
        for e in range(n_in):
            q = qmin if li[e] in shared else mods[e // T]
            x[li[e]] = {"uniform": rng.integers(0, q, N, dtype=np.uint64), "zero": 0, "q-1": q - 1}[fill]
        for sk, kk in itertools.product(SCALES, CONSTS):
            s = [pick(sk, mods[e // T], rng) for e in range(n_in)]
            k = None if kk is None else [pick(kk, q, rng) for q in mods]
            GUARD = np.uint64(0xDEADBEEFDEADBEEF)
            out = np.full((M, N), GUARD, dtype=np.uint64)
            sa = np.array(s, dtype=np.uint64)
            ka = None if k is None else np.array(k, dtype=np.uint64)
            keep = [u(li), u(lo), u(ids), u(chunks)]
            assert lib.emu_lincomb(ptr(m), M, LOGN, ptr(x), ptr(keep[0]), ptr(out), ptr(keep[1]), ptr(keep[2]), M, T, ptr(sa), ptr(ka), ptr(keep[3]),
                                   len(chunks)) == 0
            for i, q in enumerate(mods):
                for ch in chunks:
                    sl = slice(ch * 512, ch * 512 + 512)
                    cols = [[int(v) for v in x[li[i * T + t]][sl]] for t in range(T)]
                    exp = [(sum(s[i * T + t] * cols[t][j] for t in range(T)) + (0 if k is None else k[i])) % q for j in range(512)]
                    assert [int(v) for v in out[lo[i]][sl]] == exp, (T, fill, sk, kk, i, ch)
                assert np.all(out[lo[i]][512:N - 512] == GUARD)


def test_the_accumulator_at_its_fullest(env):
    """T = 16, every input, every scalar and the constant q - 1, at the largest modulus of the chain: 16 (q - 1)^2 + (q - 1), reduced once"""
    lib, mods = env
    N, T = 1 << LOGN, 16
    mod = max(range(len(mods)), key=lambda i: mods[i])
    q = mods[mod]
    assert 16 * (q - 1) ** 2 + q - 1 < 1 << 125
    m = np.array(mods, dtype=np.uint64)
    x = np.full((T, N), q - 1, dtype=np.uint64)
    out = np.zeros((1, N), dtype=np.uint64)
    u = lambda v: np.array(v, dtype=np.uint32)
    keep = [u(range(T)), u([0]), u([mod]), u(range(N // 512))]
    sa, ka = np.full(T, q - 1, dtype=np.uint64), np.array([q - 1], dtype=np.uint64)
    assert lib.emu_lincomb(ptr(m), len(mods), LOGN, ptr(x), ptr(keep[0]), ptr(out), ptr(keep[1]), ptr(keep[2]), 1, T, ptr(sa), ptr(ka), ptr(keep[3]),
                           N // 512) == 0
    assert np.all(out == np.uint64((16 * (q - 1) ** 2 + q - 1) % q))


@pytest.mark.parametrize("generic,chain", [(0, "mont32"), (1, "mont32"), (1, "mixed")])
def test_stand_alone_program_under_the_sanitizers(tmp_path, generic, chain):
    """tests/emu/hm_emu_lincomb_main.cpp with its own main, compiled with the sanitizers and run as a process of its own (nothing is loaded into
    Python): every T, fill, scalar and constant on every modulus, every chunk of every entry; every buffer is sized exactly"""
    exe = tmp_path / "hm_emu_lincomb_main"
    subprocess.check_call(["g++"] + (["-DHM_GENERIC=1"] if generic else []) + ["-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-Wall", "-Wno-unknown-pragmas", "-o", str(exe), os.path.join(HERE, "emu", "hm_emu_lincomb_main.cpp")] + SOURCES)
    r = subprocess.run([str(exe), str(LOGN)] + [str(q) for q in chain_moduli(chain)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "bad=0" in r.stdout and "cases=192" in r.stdout, r.stdout + r.stderr
