"""The per-thread core of hm_tensor_muladd (homulator_amd/csrc/hm_rec_core.h: hm_tensor_muladd_thread, the kernel of hmuladd) on the CPU, no GPU:
tests/emu/hm_emu_muladd.cpp compiles the device header with g++, once per arithmetic back-end (HM_GENERIC 0 and 1), builds the records as the entry
point does and runs every thread of the chosen workgroups.  Checked against Python integers:
    d0 = s a b + sum_t u_t x_t + k,  d1 = s (a d + c b) + sum_t u_t y_t,  d2 = s c d   mod q.
A: 0, 1, 2, 3, 8 (no addend; one under the product and no round; the tail behind the rounds; one round; the most).  Fills: uniform, all 0, all q - 1.
Scalars: 1 (no list), 2, q - 1, random.  Addend scalars: 0, 1, q - 1, random.  Constants: none, 0, q - 1, random.  Moduli: the smallest and the
largest the back-end accepts (mont32: 18 2^32 + 1 and the largest prime h 2^32 + 1 below 2^60; generic: just above 2^20 and just below 2^60) and the
36-bit chain's (generic).  The worst case, A = 8 with every input, scalar and the constant q - 1 at the largest modulus, puts 10 (q - 1)^2 < 2^124
into d1's accumulator and 9 (q - 1)^2 + q - 1 into d0's."""
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
SOURCES = [os.path.join(HERE, "emu", "hm_emu_muladd.cpp"), os.path.join(ROOT, "homulator_amd", "csrc", "hm_params.cpp")]
NARROW_MONT32 = 18 * 2**32 + 1      # the smallest prime h 2^32 + 1: 37 bits, 1 mod 2N for every ring
LOGN = 13
ADDENDS = [0, 1, 2, 3, 8]
FILLS = ["uniform", "zero", "q-1"]
SCALES = [None, "2", "q-1", "random"]
ADD_SCALES = ["0", "1", "q-1", "random"]
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
    so = tmp_path_factory.mktemp("emu_muladd") / f"libhm_emu_muladd_{generic}.so"
    subprocess.check_call(["g++"] + (["-DHM_GENERIC=1"] if generic else []) + ["-O2", "-std=c++17", "-fPIC", "-shared", "-Wall", "-Wno-unknown-pragmas", "-o", str(so)] + SOURCES)
    lib = C.CDLL(str(so))
    assert lib.emu_muladd_generic() == generic
    lib.emu_muladd_rec_words.argtypes = [u32]
    lib.emu_muladd_rec_words.restype = u32
    lib.emu_muladd_max_addends.restype = u32
    lib.emu_muladd.argtypes = [vp, u32, u32] + [vp] * 12 + [u32, u32, vp, vp, vp, vp, u32]
    return lib, chain_moduli(chain)


def ptr(a):
    return None if a is None else a.ctypes.data_as(vp)


def pick(kind, q, rng, lowest=0):
    return {"0": 0, "1": 1, "2": 2, "q-1": q - 1}[kind] if kind != "random" else int(rng.integers(lowest, q))


def u32a(v):
    return np.array(list(v), dtype=np.uint32)


def u64a(v):
    return None if v is None else np.array([int(t) for t in v], dtype=np.uint64)


def run(lib, mods, x, la, lb, lc, ld, lx0, lx1, out, l0, l1, l2, ids, A, s, u, k, chunks):
    m = np.array(mods, dtype=np.uint64)
    keep = [u32a(v) for v in (la, lb, lc, ld)] + [u32a(lx0) if A else None, u32a(lx1) if A else None] + [u32a(v) for v in (l0, l1, l2, ids, chunks)]
    sa, ua, ka = u64a(s), u64a(u) if A else None, u64a(k)
    assert lib.emu_muladd(ptr(m), len(mods), LOGN, ptr(x), ptr(keep[0]), ptr(keep[1]), ptr(keep[2]), ptr(keep[3]), ptr(keep[4]), ptr(keep[5]), ptr(out),
                          ptr(keep[6]), ptr(keep[7]), ptr(keep[8]), ptr(keep[9]), len(ids), A, ptr(sa), ptr(ua), ptr(ka), ptr(keep[10]), len(chunks)) == 0


def test_record_size_is_a_multiple_of_16_bytes(env):
    lib, _ = env
    assert lib.emu_muladd_max_addends() == 8
    for A in range(0, 9):
        words = lib.emu_muladd_rec_words(A)
        assert words * 4 % 16 == 0 and words >= 16 + 4 * A


@pytest.mark.parametrize("A", ADDENDS)
def test_records_with_permuted_and_repeated_limbs(env, A):
    """the thread function over whole workgroups: one entry per modulus, the operands at permuted limbs, one limb read by two entries (the a of
    entry 0 is the d of the last entry) and, at A >= 1, twice by one entry (an addend component that is also the product's b: ct3 = ct2), the
    first and the last chunk of every entry; the outputs of the chunks that did not run keep their guard value"""
    lib, mods = env
    N, M, W = 1 << LOGN, len(mods), 4 + 2 * A
    rng = np.random.default_rng(200 + A)
    qmin = min(mods)          # a shared limb holds residues of every modulus that reads it
    n_in = M * W
    li = [(e * 7 + 3) % n_in for e in range(n_in)]
    li[(M - 1) * W + 3] = li[0]      # entries 0 and M - 1 share a limb
    if A >= 1:
        li[4] = li[1]                # entry 0: x_1 is b
    shared = {li[0], li[1]} if A >= 1 else {li[0]}
    la, lb, lc, ld = ([li[i * W + r] for i in range(M)] for r in range(4))
    lx0 = [li[i * W + 4 + 2 * t] for i in range(M) for t in range(A)]
    lx1 = [li[i * W + 5 + 2 * t] for i in range(M) for t in range(A)]
    l0, l1, l2, ids, chunks = [3, 2, 0, 1], [7, 4, 5, 6], [8, 11, 10, 9], [0, 1, 2, 3], [0, N // 512 - 1]
    for fill in FILLS:
        x = np.zeros((n_in, N), dtype=np.uint64)
        for e in range(n_in):
            q = qmin if li[e] in shared else mods[e // W]
            x[li[e]] = {"uniform": rng.integers(0, q, N, dtype=np.uint64), "zero": 0, "q-1": q - 1}[fill]
        for sk, uk, kk in itertools.product(SCALES, ADD_SCALES if A else ["0"], CONSTS):
            s = None if sk is None else [pick(sk, q, rng, 1) for q in mods]
            u = [pick(uk, mods[i], rng) for i in range(M) for _ in range(A)]
            k = None if kk is None else [pick(kk, q, rng) for q in mods]
            GUARD = np.uint64(0xDEADBEEFDEADBEEF)
            out = np.full((3 * M, N), GUARD, dtype=np.uint64)
            run(lib, mods, x, la, lb, lc, ld, lx0, lx1, out, l0, l1, l2, ids, A, s, u, k, chunks)
            for i, q in enumerate(mods):
                si, ki = (1 if s is None else s[i]), (0 if k is None else k[i])
                for ch in chunks:
                    sl = slice(ch * 512, ch * 512 + 512)
                    col = lambda limb: [int(v) for v in x[limb][sl]]
                    a, b, c, d = col(la[i]), col(lb[i]), col(lc[i]), col(ld[i])
                    xs, ys = [col(lx0[i * A + t]) for t in range(A)], [col(lx1[i * A + t]) for t in range(A)]
                    e0 = [(si * a[j] * b[j] + sum(u[i * A + t] * xs[t][j] for t in range(A)) + ki) % q for j in range(512)]
                    e1 = [(si * (a[j] * d[j] + c[j] * b[j]) + sum(u[i * A + t] * ys[t][j] for t in range(A))) % q for j in range(512)]
                    e2 = [si * c[j] * d[j] % q for j in range(512)]
                    what = (A, fill, sk, uk, kk, i, ch)
                    assert [int(v) for v in out[l0[i]][sl]] == e0, what
                    assert [int(v) for v in out[l1[i]][sl]] == e1, what
                    assert [int(v) for v in out[l2[i]][sl]] == e2, what
                for o in (l0[i], l1[i], l2[i]):
                    assert np.all(out[o][512:N - 512] == GUARD)


def test_the_accumulators_at_their_fullest(env):
    """A = 8, every input, the scalar, every addend scalar and the constant q - 1, at the largest modulus of the chain: d1's accumulator holds
    10 (q - 1)^2, d0's 9 (q - 1)^2 + (q - 1), each reduced once"""
    lib, mods = env
    N, A = 1 << LOGN, 8
    mod = max(range(len(mods)), key=lambda i: mods[i])
    q = mods[mod]
    assert 10 * (q - 1) ** 2 < 1 << 124 and 9 * (q - 1) ** 2 + q - 1 < 1 << 124
    x = np.full((4 + 2 * A, N), q - 1, dtype=np.uint64)
    out = np.zeros((3, N), dtype=np.uint64)
    run(lib, mods, x, [0], [1], [2], [3], range(4, 4 + 2 * A, 2), range(5, 4 + 2 * A, 2), out, [0], [1], [2], [mod], A, [q - 1], [q - 1] * A, [q - 1],
        range(N // 512))
    p = (q - 1) ** 2
    assert np.all(out[0] == np.uint64(((q - 1) * p + A * p + q - 1) % q))
    assert np.all(out[1] == np.uint64(((q - 1) * 2 * p + A * p) % q))
    assert np.all(out[2] == np.uint64((q - 1) * p % q))


@pytest.mark.parametrize("generic,chain", [(0, "mont32"), (1, "mont32"), (1, "mixed")])
def test_stand_alone_program_under_the_sanitizers(tmp_path, generic, chain):
    """tests/emu/hm_emu_muladd_main.cpp with its own main, compiled with the sanitizers and run as a process of its own (nothing is loaded into
    Python): every A, fill, scalar, addend scalar and constant on every modulus, every chunk of every entry; every buffer is sized exactly"""
    exe = tmp_path / "hm_emu_muladd_main"
    subprocess.check_call(["g++"] + (["-DHM_GENERIC=1"] if generic else []) + ["-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-Wall", "-Wno-unknown-pragmas", "-o", str(exe), os.path.join(HERE, "emu", "hm_emu_muladd_main.cpp")] + SOURCES)
    r = subprocess.run([str(exe), str(LOGN)] + [str(q) for q in chain_moduli(chain)], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0 and "bad=0" in r.stdout and "cases=816" in r.stdout, r.stdout + r.stderr
