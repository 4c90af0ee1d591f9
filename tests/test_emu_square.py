"""The per-thread core of hm_tensor_square (homulator_amd/csrc/hm_rec_core.h: hm_tensor_square_one / hm_tensor_square_thread, the kernel of hsquare) and
the element-wise opcode ADD_CONST on the CPU, no GPU: tests/emu/hm_emu_square.cpp compiles the device header with g++, once per arithmetic back-end
(HM_GENERIC 0 and 1), builds the records as the entry point does and runs every thread of the chosen workgroups.  Checked against Python integers:
d0 = s a a + k, d1 = 2 s a c, d2 = s c c mod q.
Fills: uniform, all 0, all q - 1.  Scalars: 1, 2, q - 1, random, and no list.  Constants: 0, q - 1, random, and no list.
Moduli: the smallest and the largest the back-end accepts (mont32: 18 2^32 + 1 and the largest prime h 2^32 + 1 below 2^60; generic: just above 2^20
and just below 2^60) and the 36-bit chain's (generic)."""
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
SOURCES = [os.path.join(HERE, "emu", "hm_emu_square.cpp"), os.path.join(ROOT, "homulator_amd", "csrc", "hm_params.cpp")]
NARROW_MONT32 = 18 * 2**32 + 1      # the smallest prime h 2^32 + 1: 37 bits, 1 mod 2N for every ring
LOGN = 13
FILLS = ["uniform", "zero", "q-1"]
SCALES = ["1", "2", "q-1", "random", None]
CONSTS = ["0", "q-1", "random", None]


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
    so = tmp_path_factory.mktemp("emu_square") / f"libhm_emu_square_{generic}.so"
    subprocess.check_call(["g++"] + (["-DHM_GENERIC=1"] if generic else []) + ["-O2", "-std=c++17", "-fPIC", "-shared", "-Wall", "-Wno-unknown-pragmas", "-o", str(so)] + SOURCES)
    lib = C.CDLL(str(so))
    assert lib.emu_square_generic() == generic
    lib.emu_tensor_square.argtypes = [vp, u32, u32] + [vp] * 11 + [u32, vp, vp, vp, u32]
    lib.emu_square_words.argtypes = [vp, u32, u32, u32, u64, u64, vp, vp, u32, vp]
    lib.emu_add_const_words.argtypes = [vp, u32, u32, u32, u64, vp, u32, vp]
    return lib, chain_moduli(chain)


def ptr(a):
    return None if a is None else a.ctypes.data_as(vp)


def pick(kind, q, rng, lo):
    """a scalar (lo = 1) or a constant (lo = 0) of the named kind"""
    return {"0": 0, "1": 1, "2": 2, "q-1": q - 1}[kind] if kind != "random" else int(rng.integers(lo, q))


def expected(a, c, s, k, q):
    a, c = [int(v) for v in a], [int(v) for v in c]
    return ([(s * x * x + k) % q for x in a], [2 * s * x * y % q for x, y in zip(a, c)], [s * y * y % q for y in c])


def test_single_words_at_the_ends_of_the_range(env):
    """hm_tensor_square_one alone: every combination of a, c in {0, 1, 2, (q - 1) / 2, (q + 1) / 2, q - 2, q - 1, random} with every scalar and constant"""
    lib, mods = env
    rng = np.random.default_rng(5)
    m = np.array(mods, dtype=np.uint64)
    for mod, q in enumerate(mods):
        words = [0, 1, 2, (q - 1) // 2, (q + 1) // 2, q - 2, q - 1] + [int(v) for v in rng.integers(0, q, 9)]
        pairs = list(itertools.product(words, words))
        a = np.array([p[0] for p in pairs], dtype=np.uint64)
        c = np.array([p[1] for p in pairs], dtype=np.uint64)
        for sk, kk in itertools.product(SCALES[:4], CONSTS[:3]):
            s, k = pick(sk, q, rng, 1), pick(kk, q, rng, 0)
            out = np.empty(3 * len(pairs), dtype=np.uint64)
            assert lib.emu_square_words(ptr(m), len(mods), LOGN, mod, s, k, ptr(a), ptr(c), len(pairs), ptr(out)) == 0
            e0, e1, e2 = expected(a, c, s, k, q)
            got = out.reshape(-1, 3)
            assert [int(v) for v in got[:, 0]] == e0 and [int(v) for v in got[:, 1]] == e1 and [int(v) for v in got[:, 2]] == e2, (mod, sk, kk)
            assert int(got.max()) < q


@pytest.mark.parametrize("fill", FILLS)
def test_records_with_permuted_limbs(env, fill):
    """the thread function over whole workgroups: one entry per modulus, inputs and outputs at permuted (and, for the inputs, repeated) limbs, the
    first and the last chunk of every entry; the outputs of the chunks that did not run keep their guard value"""
    lib, mods = env
    N, M = 1 << LOGN, len(mods)
    rng = np.random.default_rng(17 + FILLS.index(fill))
    m = np.array(mods, dtype=np.uint64)
    la, lc = [2, 0, 2, 1], [1, 3, 0, 2]          # entries 0 and 2 share an a limb
    l0, l1, l2 = [3, 2, 1, 0], [0, 1, 2, 3], [1, 0, 3, 2]
    ids = [0, 1, 2, 3]
    chunks = [0, N // 512 - 1]
    a = np.zeros((M, N), dtype=np.uint64)
    c = np.zeros((M, N), dtype=np.uint64)
    qmin = min(mods)      # shared limbs hold residues of every modulus that reads them
    for buf in (a, c):
        buf[:] = {"uniform": rng.integers(0, qmin, (M, N), dtype=np.uint64), "zero": 0, "q-1": qmin - 1}[fill]
    if fill == "q-1":      # the exact top of each entry's own range where the limb is not shared
        a[la[1]] = mods[1] - 1
        c[lc[0]] = mods[0] - 1
    u = lambda v: np.array(v, dtype=np.uint32)
    for sk, kk in itertools.product(SCALES, CONSTS):
        s = None if sk is None else [pick(sk, q, rng, 1) for q in mods]
        k = None if kk is None else [pick(kk, q, rng, 0) for q in mods]
        GUARD = np.uint64(0xDEADBEEFDEADBEEF)
        o = [np.full((M, N), GUARD, dtype=np.uint64) for _ in range(3)]
        sa = None if s is None else np.array(s, dtype=np.uint64)
        ka = None if k is None else np.array(k, dtype=np.uint64)
        keep = [u(x) for x in (la, lc, l0, l1, l2, ids, chunks)]
        assert lib.emu_tensor_square(ptr(m), M, LOGN, ptr(a), ptr(keep[0]), ptr(c), ptr(keep[1]), ptr(o[0]), ptr(keep[2]), ptr(o[1]), ptr(keep[3]),
                                     ptr(o[2]), ptr(keep[4]), ptr(keep[5]), M, ptr(sa), ptr(ka), ptr(keep[6]), len(chunks)) == 0
        for i, q in enumerate(mods):
            for ch in chunks:
                sl = slice(ch * 512, ch * 512 + 512)
                av, cv = a[la[i]][sl] % np.uint64(q), c[lc[i]][sl] % np.uint64(q)
                # (the stored words are residues of the smallest modulus, so they are reduced for every entry already)
                assert np.array_equal(av, a[la[i]][sl]) and np.array_equal(cv, c[lc[i]][sl])
                e = expected(av, cv, 1 if s is None else s[i], 0 if k is None else k[i], q)
                for t, lt in enumerate((l0, l1, l2)):
                    assert [int(v) for v in o[t][lt[i]][sl]] == e[t], (fill, sk, kk, i, ch, t)
            for t, lt in enumerate((l0, l1, l2)):
                assert np.all(o[t][lt[i]][512:N - 512] == GUARD)


def test_add_const_words(env):
    lib, mods = env
    rng = np.random.default_rng(3)
    m = np.array(mods, dtype=np.uint64)
    for mod, q in enumerate(mods):
        a = np.array([0, 1, q - 2, q - 1] + [int(v) for v in rng.integers(0, q, 12)], dtype=np.uint64)
        for k in [0, 1, q - 1, int(rng.integers(0, q))]:
            out = np.empty(len(a), dtype=np.uint64)
            assert lib.emu_add_const_words(ptr(m), len(mods), LOGN, mod, k, ptr(a), len(a), ptr(out)) == 0
            assert [int(v) for v in out] == [(int(x) + k) % q for x in a], (mod, k)


@pytest.mark.parametrize("generic,chain", [(0, "mont32"), (1, "mont32"), (1, "mixed")])
def test_stand_alone_program_under_the_sanitizers(tmp_path, generic, chain):
    """tests/emu/hm_emu_square_main.cpp with its own main, compiled with the sanitizers and run as a process of its own (nothing is loaded into
    Python): every fill, scalar and constant on every modulus, every chunk of every entry; every buffer is sized exactly"""
    exe = tmp_path / "hm_emu_square_main"
    subprocess.check_call(["g++"] + (["-DHM_GENERIC=1"] if generic else []) + ["-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-Wall", "-Wno-unknown-pragmas", "-o", str(exe), os.path.join(HERE, "emu", "hm_emu_square_main.cpp")] + SOURCES)
    r = subprocess.run([str(exe), str(LOGN)] + [str(q) for q in chain_moduli(chain)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "bad=0" in r.stdout and "cases=60" in r.stdout, r.stdout + r.stderr
