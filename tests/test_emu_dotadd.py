"""The per-thread core of hm_tensor_dotadd (homulator_amd/csrc/hm_rec_core.h: hm_tensor_dotadd_thread, the kernel of hdotadd) on the CPU, no GPU:
tests/emu/hm_emu_dotadd.cpp compiles the device header with g++, once per arithmetic back-end (HM_GENERIC 0 and 1), builds the records as the entry
point does and runs every thread of the chosen workgroups.  Checked against Python integers:
    d0 = sum_t s_t a_t b_t + sum_r u_r x_r + k,  d1 = sum_t s_t (a_t d_t + c_t b_t) + sum_r u_r y_r,  d2 = sum_t s_t c_t d_t   mod q.
(T, A): (1,0), (1,1), (2,1), (2,2), (3,3), (16,8): no round of either term loop; addend 0 under the pairs and no round; one tail of the pair loop;
one tail of both; one round of both; the most.  Fills: uniform, all 0, all q - 1, independently for the operands of the pairs and the addends.
Pair scalars: 1 (no list), 2, q - 1, random, and mixed within one record (1, 2, q - 1, random by pair: the uniform branch taken and skipped).
Addend scalars: 0, 1, q - 1, random.  Constants: none, 0, q - 1, random.  Moduli: the smallest and the largest the back-end accepts (mont32:
18 2^32 + 1 and the largest prime h 2^32 + 1 below 2^60; generic: just above 2^20 and just below 2^60) and the 36-bit chain's (generic).  The worst
case, (16, 8) with every input, scalar and the constant q - 1 at the largest modulus, puts 40 (q - 1)^2 < 2^126 into d1's accumulator and
24 (q - 1)^2 + q - 1 into d0's.  The Python tests take every value of every dimension, the full product of the constants on uniform fills and every
pair of fills on mixed / random constants; the stand-alone program takes the full product of all five dimensions under the sanitizers."""
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
SOURCES = [os.path.join(HERE, "emu", "hm_emu_dotadd.cpp"), os.path.join(ROOT, "homulator_amd", "csrc", "hm_params.cpp")]
NARROW_MONT32 = 18 * 2**32 + 1      # the smallest prime h 2^32 + 1: 37 bits, 1 mod 2N for every ring
LOGN = 13
SHAPES = [(1, 0), (1, 1), (2, 1), (2, 2), (3, 3), (16, 8)]
FILLS = ["uniform", "zero", "q-1"]
SCALES = [None, "2", "q-1", "random", "mixed"]
MIXED = ["1", "2", "q-1", "random"]      # by pair, within one record
ADD_SCALES = ["0", "1", "q-1", "random"]
CONSTS = [None, "0", "q-1", "random"]
GUARD = np.uint64(0xDEADBEEFDEADBEEF)


def chain_moduli(chain, logN=LOGN):
    if chain == "mont32":
        m = Oracle(logN, 3, 1).moduli
        return [m[0], m[1], NARROW_MONT32, m[2]]
    wide, narrow, mid = chain_below(logN, 60, 1), chain_below(logN, 21 if logN == LOGN else logN + 8, 1), chain_below(logN, 36, 2)
    return [wide[0], narrow[0], mid[0], mid[1]]


BUILDS = [(0, "mont32"), (1, "mont32"), (1, "mixed")]


@pytest.fixture(scope="module", params=BUILDS, ids=["mont32-build", "generic-build", "generic-build-mixed-widths"])
def env(request, tmp_path_factory):
    """(library, chain): the emulator of one arithmetic build, and the chain it runs"""
    generic, chain = request.param
    so = tmp_path_factory.mktemp("emu_dotadd") / f"libhm_emu_dotadd_{generic}.so"
    subprocess.check_call(["g++"] + (["-DHM_GENERIC=1"] if generic else []) + ["-O2", "-std=c++17", "-fPIC", "-shared", "-Wall", "-Wno-unknown-pragmas", "-o", str(so)] + SOURCES)
    lib = C.CDLL(str(so))
    assert lib.emu_dotadd_generic() == generic
    lib.emu_dotadd_rec_words.argtypes = [u32, u32]
    lib.emu_dotadd_rec_words.restype = u32
    lib.emu_dotadd_max_terms.restype = u32
    lib.emu_dotadd_max_addends.restype = u32
    lib.emu_dotadd.argtypes = [vp, u32, u32] + [vp] * 12 + [u32, u32, u32, vp, vp, vp, vp, u32]
    return lib, chain


def ptr(a):
    return None if a is None else a.ctypes.data_as(vp)


def pick(kind, q, rng, lowest=0):
    return {"0": 0, "1": 1, "2": 2, "q-1": q - 1}[kind] if kind != "random" else int(rng.integers(lowest, q))


def u32a(v):
    return np.array(list(v), dtype=np.uint32)


def u64a(v):
    return None if v is None else np.array([int(t) for t in v], dtype=np.uint64)


def run(lib, mods, logN, x, la, lb, lc, ld, lx0, lx1, out, l0, l1, l2, ids, T, A, s, u, k, chunks):
    m = np.array(mods, dtype=np.uint64)
    keep = [u32a(v) for v in (la, lb, lc, ld)] + [u32a(lx0) if A else None, u32a(lx1) if A else None] + [u32a(v) for v in (l0, l1, l2, ids, chunks)]
    sa, ua, ka = u64a(s), u64a(u) if A else None, u64a(k)
    assert lib.emu_dotadd(ptr(m), len(mods), logN, ptr(x), ptr(keep[0]), ptr(keep[1]), ptr(keep[2]), ptr(keep[3]), ptr(keep[4]), ptr(keep[5]), ptr(out),
                          ptr(keep[6]), ptr(keep[7]), ptr(keep[8]), ptr(keep[9]), len(ids), T, A, ptr(sa), ptr(ua), ptr(ka), ptr(keep[10]), len(chunks)) == 0


def test_record_size_is_the_issues(env):
    lib, _ = env
    assert lib.emu_dotadd_max_terms() == 16 and lib.emu_dotadd_max_addends() == 8
    for T in range(1, 17):
        for A in range(0, 9):
            assert lib.emu_dotadd_rec_words(T, A) * 4 == 32 + 32 * T + 16 * A


def layout(M, T, A):
    """operand r of entry i at a permuted limb of a buffer of exactly M W limbs; one limb read by two entries (the a of pair 0 of entry 0 is the d of
    the last pair of the last entry) and, at A >= 1, twice by one entry (x_0 of entry 0 is the b of its pair 0); at T >= 2 the c of pair 1 of entry 0
    is the a of its pair 0 (a limb repeated across the pairs of one record)"""
    W = 4 * T + 2 * A
    n_in = M * W
    li = [(e * 7 + 3) % n_in for e in range(n_in)]
    li[(M - 1) * W + 4 * (T - 1) + 3] = li[0]
    shared = {li[0]}
    if A >= 1:
        li[4 * T] = li[1]
        shared.add(li[1])
    if T >= 2:
        li[6] = li[0]
    la, lb, lc, ld = ([li[i * W + 4 * t + r] for i in range(M) for t in range(T)] for r in range(4))
    lx0 = [li[i * W + 4 * T + 2 * r] for i in range(M) for r in range(A)]
    lx1 = [li[i * W + 4 * T + 2 * r + 1] for i in range(M) for r in range(A)]
    return W, n_in, li, shared, la, lb, lc, ld, lx0, lx1


L0, L1, L2, IDS = [3, 2, 0, 1], [7, 4, 5, 6], [8, 11, 10, 9], [0, 1, 2, 3]


def check(lib, mods, logN, T, A, fill_p, fill_a, sk, uk, kk, rng, chunks):
    N, M = 1 << logN, len(mods)
    W, n_in, li, shared, la, lb, lc, ld, lx0, lx1 = layout(M, T, A)
    qmin = min(mods)          # a shared limb holds residues of every modulus that reads it
    x = np.zeros((n_in, N), dtype=np.uint64)
    for e in range(n_in):
        q = qmin if li[e] in shared else mods[e // W]
        fill = fill_p if e % W < 4 * T else fill_a
        for ch in chunks:
            sl = slice(ch * 512, ch * 512 + 512)
            x[li[e]][sl] = {"uniform": rng.integers(0, q, 512, dtype=np.uint64), "zero": 0, "q-1": q - 1}[fill]
    kind = lambda t: MIXED[t % 4] if sk == "mixed" else sk
    s = None if sk is None else [pick(kind(t), q, rng, 1) for q in mods for t in range(T)]
    u = [pick(uk, mods[i], rng) for i in range(M) for _ in range(A)]
    k = None if kk is None else [pick(kk, q, rng) for q in mods]
    out = np.full((3 * M, N), GUARD, dtype=np.uint64)
    run(lib, mods, logN, x, la, lb, lc, ld, lx0, lx1, out, L0, L1, L2, IDS, T, A, s, u, k, chunks)
    for i, q in enumerate(mods):
        ki = 0 if k is None else k[i]
        for ch in chunks:
            sl = slice(ch * 512, ch * 512 + 512)
            col = lambda limb: x[limb][sl].astype(object)
            e0, e1, e2 = ki, 0, 0
            for t in range(T):
                st = 1 if s is None else s[i * T + t]
                a, b, c, d = col(la[i * T + t]), col(lb[i * T + t]), col(lc[i * T + t]), col(ld[i * T + t])
                e0, e1, e2 = e0 + st * a * b, e1 + st * (a * d + c * b), e2 + st * c * d
            for r in range(A):
                e0, e1 = e0 + u[i * A + r] * col(lx0[i * A + r]), e1 + u[i * A + r] * col(lx1[i * A + r])
            what = (T, A, fill_p, fill_a, sk, uk, kk, i, ch)
            for limb, e in ((L0[i], e0), (L1[i], e1), (L2[i], e2)):
                assert np.array_equal(out[limb][sl].astype(object), e % q), what
        ran = np.zeros(N, dtype=bool)
        for ch in chunks:
            ran[ch * 512:ch * 512 + 512] = True
        for limb in (L0[i], L1[i], L2[i]):
            assert np.all(out[limb][~ran] == GUARD)       # the chunks that did not run keep their guard value


@pytest.mark.parametrize("T,A", SHAPES)
def test_records_with_permuted_and_repeated_limbs(env, T, A):
    """the thread function over whole workgroups: one entry per modulus, the first and the last chunk of every entry; the full product of the
    constants on uniform fills, every pair of fills on mixed scalars and random constants"""
    lib, chain = env
    mods = chain_moduli(chain)
    rng = np.random.default_rng(300 + 17 * T + A)
    chunks = [0, (1 << LOGN) // 512 - 1]
    for sk, uk, kk in itertools.product(SCALES, ADD_SCALES if A else ["0"], CONSTS):
        check(lib, mods, LOGN, T, A, "uniform", "uniform", sk, uk, kk, rng, chunks)
    for fp, fa in itertools.product(FILLS, FILLS if A else ["uniform"]):
        check(lib, mods, LOGN, T, A, fp, fa, "mixed", "random", "random", rng, chunks)
        check(lib, mods, LOGN, T, A, fp, fa, "q-1", "q-1", "q-1", rng, chunks)


@pytest.mark.parametrize("T,A", [(1, 0), (2, 1), (3, 3)])
def test_the_large_ring(env, T, A):
    """logN = 17: the first and the last of 256 chunks"""
    lib, chain = env
    mods = chain_moduli(chain, 17)
    check(lib, mods, 17, T, A, "uniform", "uniform", "mixed", "random", "random", np.random.default_rng(17), [0, (1 << 17) // 512 - 1])


def test_the_accumulators_at_their_fullest(env):
    """(16, 8), every input, every scalar and the constant q - 1, at the largest modulus of the chain: d1's accumulator holds 40 (q - 1)^2, d0's
    24 (q - 1)^2 + (q - 1), each reduced once"""
    lib, chain = env
    mods = chain_moduli(chain)
    N, T, A = 1 << LOGN, 16, 8
    mod = max(range(len(mods)), key=lambda i: mods[i])
    q = mods[mod]
    assert 40 * (q - 1) ** 2 < 1 << 126 and 24 * (q - 1) ** 2 + q - 1 < 1 << 126
    W = 4 * T + 2 * A
    x = np.full((W, N), q - 1, dtype=np.uint64)
    out = np.zeros((3, N), dtype=np.uint64)
    run(lib, mods, LOGN, x, range(0, 4 * T, 4), range(1, 4 * T, 4), range(2, 4 * T, 4), range(3, 4 * T, 4), range(4 * T, W, 2), range(4 * T + 1, W, 2), out,
        [0], [1], [2], [mod], T, A, [q - 1] * T, [q - 1] * A, [q - 1], range(N // 512))
    p = (q - 1) ** 2
    assert np.all(out[0] == np.uint64((T * (q - 1) * p + A * p + q - 1) % q))
    assert np.all(out[1] == np.uint64((T * (q - 1) * 2 * p + A * p) % q))
    assert np.all(out[2] == np.uint64(T * (q - 1) * p % q))


@pytest.fixture(scope="module", params=BUILDS, ids=["mont32-build", "generic-build", "generic-build-mixed-widths"])
def program(request, tmp_path_factory):
    """tests/emu/hm_emu_dotadd_main.cpp with its own main, compiled with the sanitizers: a CPU build that loads nothing into Python"""
    generic, chain = request.param
    exe = tmp_path_factory.mktemp("emu_dotadd_main") / "hm_emu_dotadd_main"
    subprocess.check_call(["g++"] + (["-DHM_GENERIC=1"] if generic else []) + ["-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-Wall", "-Wno-unknown-pragmas", "-o", str(exe), os.path.join(HERE, "emu", "hm_emu_dotadd_main.cpp")] + SOURCES)
    return exe, chain


def test_stand_alone_program_under_the_sanitizers(program):
    """run as a process of its own: every shape, pair of fills, scalar, addend scalar and constant on every modulus, the first, a middle and the last
    chunk of every entry; every buffer is sized exactly"""
    exe, chain = program
    r = subprocess.run([str(exe), str(LOGN)] + [str(q) for q in chain_moduli(chain)] + ["all"], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0 and "bad=0" in r.stdout and "cases=3660" in r.stdout, r.stdout + r.stderr


def test_stand_alone_program_on_the_large_ring(program):
    exe, chain = program
    r = subprocess.run([str(exe), "17"] + [str(q) for q in chain_moduli(chain, 17)] + ["few"], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0 and "bad=0" in r.stdout and "cases=160" in r.stdout, r.stdout + r.stderr
