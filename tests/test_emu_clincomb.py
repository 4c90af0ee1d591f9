"""The per-thread core of hm_clincomb (homulator_amd/csrc/hm_rec_core.h: hm_clincomb_thread, the kernel of hclincomb) on the CPU, no GPU:
tests/emu/hm_emu_clincomb.cpp compiles the device header with g++, once per arithmetic back-end (HM_GENERIC 0 and 1), builds the records as the
entry point does and runs every thread of the chosen workgroups.  Checked against Python integers: out = sum_t (a_t + b_t m) x_t + k_re + k_im m
mod q with m = v = psi^(N/2) on the entries below N/2 and q - v behind.
Rings: logN 13 to 17, with the first chunk, the chunks just below and just above N/2 and the last one.  T: 1, 2, 3, 16 (no round of the two-term
loop, the tail behind it, one round, the most).  Fills: uniform, all 0, all q - 1.  Scalars 0, 1, q - 1, random and constants none, 0, q - 1,
random, in both parts.  Moduli: the smallest and the largest the back-end accepts (mont32: 18 2^32 + 1 and the largest prime h 2^32 + 1 below
2^60; generic: just above 2^20 and just below 2^60) and the 36-bit chain's (generic).  The worst case, T = 16 with every input q - 1 and the
scalar and the constant of the half q - 1 at the largest modulus, puts 16 (q - 1)^2 + q - 1 < 2^125 into the accumulator."""
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
SOURCES = [os.path.join(HERE, "emu", "hm_emu_clincomb.cpp"), os.path.join(ROOT, "homulator_amd", "csrc", "hm_params.cpp")]
NARROW_MONT32 = 18 * 2**32 + 1      # the smallest prime h 2^32 + 1: 37 bits, 1 mod 2N for every ring
LOGN = 13
TERMS = [1, 2, 3, 16]
FILLS = ["uniform", "zero", "q-1"]
KINDS = ["0", "1", "q-1", "random"]
GUARD = np.uint64(0xDEADBEEFDEADBEEF)


def chain_moduli(chain, logN=LOGN):
    if chain == "mont32":
        m = Oracle(logN, 3, 1).moduli
        return [int(m[0]), int(m[1]), NARROW_MONT32, int(m[2])]
    wide, mid = chain_below(logN, 60, 1), chain_below(logN, 36, 2)
    narrow = next(c for c in (chain_below(logN, bits, 1) for bits in (21, 22, 23)) if c[0] > 1 << 20)      # the back-end takes primes above 2^20
    return [int(wide[0]), int(narrow[0]), int(mid[0]), int(mid[1])]


@pytest.fixture(scope="module", params=[(0, "mont32"), (1, "mont32"), (1, "mixed")], ids=["mont32-build", "generic-build", "generic-build-mixed-widths"])
def env(request, tmp_path_factory):
    """(library, chain): the emulator of one arithmetic build, and the name of the chain it runs"""
    generic, chain = request.param
    so = tmp_path_factory.mktemp("emu_clincomb") / f"libhm_emu_clincomb_{generic}.so"
    subprocess.check_call(["g++"] + (["-DHM_GENERIC=1"] if generic else []) + ["-O2", "-std=c++17", "-fPIC", "-shared", "-Wall", "-Wno-unknown-pragmas", "-o", str(so)] + SOURCES)
    lib = C.CDLL(str(so))
    assert lib.emu_clincomb_generic() == generic
    lib.emu_clincomb_rec_words.argtypes = [u32]
    lib.emu_clincomb_rec_words.restype = u32
    lib.emu_clincomb.argtypes = [vp, u32, u32, vp, vp, vp, vp, vp, u32, u32, vp, vp, vp, vp, vp, u32, vp]
    return lib, chain


def ptr(a):
    return None if a is None else a.ctypes.data_as(vp)


def u(v):
    return np.array(list(v), dtype=np.uint32)


def w(v):
    return None if v is None else np.array([int(a) for a in v], dtype=np.uint64)


def pick(kind, q, rng):
    return {"0": 0, "1": 1, "q-1": q - 1}[kind] if kind != "random" else int(rng.integers(0, q))


def run(lib, mods, logN, x, li, out, lo, ids, T, re, im, kre, kim, chunks):
    """runs the emulator; returns v = psi^(N/2) per modulus, from the roots the records were built with, checked to be 2N-th roots"""
    N = 1 << logN
    m, psi = w(mods), np.zeros(len(mods), dtype=np.uint64)
    keep = [u(li), u(lo), u(ids), u(chunks), w(re), w(im), w(kre), w(kim)]
    assert lib.emu_clincomb(ptr(m), len(mods), logN, ptr(x), ptr(keep[0]), ptr(out), ptr(keep[1]), ptr(keep[2]), len(ids), T, ptr(keep[4]), ptr(keep[5]),
                            ptr(keep[6]), ptr(keep[7]), ptr(keep[3]), len(chunks), ptr(psi)) == 0
    vs = []
    for p, q in zip(psi, mods):
        assert pow(int(p), N, q) == q - 1
        vs.append(pow(int(p), N // 2, q))
        assert vs[-1] * vs[-1] % q == q - 1
    return vs


def expected(x, li, i, T, q, v, N, ch, re, im, kre, kim):
    """entry i under modulus q, chunk ch, in Python integers"""
    mono = v if ch * 512 < N // 2 else q - v
    sl = slice(ch * 512, ch * 512 + 512)
    acc = np.full(512, (0 if kre is None else kre[i]) + (0 if kim is None else kim[i]) * mono, dtype=object)
    for t in range(T):
        e = i * T + t
        acc = acc + x[li[e]][sl].astype(object) * (re[e] + (0 if im is None else im[e]) * mono)
    return [int(a) % q for a in acc]


def test_record_size_is_32_bytes_and_32_per_term(env):
    lib, _ = env
    for T in range(1, 17):
        assert lib.emu_clincomb_rec_words(T) * 4 == 32 + 32 * T


@pytest.mark.parametrize("T", TERMS)
def test_records_with_permuted_and_repeated_limbs(env, T):
    """the thread function over whole workgroups: one entry per modulus, the inputs at permuted limbs, one limb read by two entries (and, at T >= 2,
    twice by one entry), the first chunk, the two chunks around N/2 and the last chunk of every entry; the outputs of the chunks that did not run
    keep their guard value.  Every pair of scalar kinds (real, monomial) runs, each with one pair of constant kinds, so that every pair of those
    runs too"""
    lib, chain = env
    mods = chain_moduli(chain)
    N, M = 1 << LOGN, len(mods)
    rng = np.random.default_rng(200 + T)
    qmin = min(mods)          # a shared limb holds residues of every modulus that reads it
    n_in = M * T
    li = [(e * 7 + 3) % n_in for e in range(n_in)]
    li[n_in - 1] = li[0]      # entries 0 and M - 1 share a limb
    if T >= 2:
        li[1] = li[0]         # entry 0 reads one limb twice
    shared = {li[0]}
    lo, ids = [3, 2, 0, 1], [0, 1, 2, 3]
    half = N // 1024
    chunks = [0, half - 1, half, N // 512 - 1]
    ran = np.zeros(N, dtype=bool)
    for ch in chunks:
        ran[ch * 512:ch * 512 + 512] = True
    pairs = list(itertools.product(KINDS, KINDS))
    combos = list(zip(pairs, pairs)) + [(("random", "random"), (None, None))]      # (scalar kinds, constant kinds); the last: no constant lists
    for fill in FILLS:
        x = np.zeros((n_in, N), dtype=np.uint64)
        for e in range(n_in):
            q = qmin if li[e] in shared else mods[e // T]
            x[li[e]] = {"uniform": rng.integers(0, q, N, dtype=np.uint64), "zero": 0, "q-1": q - 1}[fill]
        for c, ((ka, kb), (kr, ki)) in enumerate(combos):
            re = [pick(ka, mods[e // T], rng) for e in range(n_in)]
            im = None if (kb == "0" and c % 8 == 0) else [pick(kb, mods[e // T], rng) for e in range(n_in)]      # a null list is all zeros
            kre = None if kr is None else [pick(kr, q, rng) for q in mods]
            kim = None if ki is None else [pick(ki, q, rng) for q in mods]
            out = np.full((M, N), GUARD, dtype=np.uint64)
            vs = run(lib, mods, LOGN, x, li, out, lo, ids, T, re, im, kre, kim, chunks)
            for i, q in enumerate(mods):
                for ch in chunks:
                    got = [int(a) for a in out[lo[i]][ch * 512:ch * 512 + 512]]
                    assert got == expected(x, li, i, T, q, vs[i], N, ch, re, im, kre, kim), (T, fill, ka, kb, kr, ki, i, ch)
                assert np.all(out[lo[i]][~ran] == GUARD)


@pytest.mark.parametrize("logN", [13, 14, 15, 16, 17])
def test_the_half_is_chosen_per_workgroup_in_every_ring(env, logN):
    """T = 3 with random scalars and constants in both parts at every ring size: chunk N/1024 - 1 is the last that meets v, chunk N/1024 the first
    that meets q - v"""
    lib, chain = env
    mods = chain_moduli(chain, logN)
    N, M, T = 1 << logN, len(mods), 3
    rng = np.random.default_rng(300 + logN)
    li = [(e * 5 + 1) % (M * T) for e in range(M * T)]
    x = np.stack([rng.integers(0, mods[li.index(r) // T], N, dtype=np.uint64) for r in range(M * T)])
    re = [pick("random", mods[e // T], rng) for e in range(M * T)]
    im = [pick("random", mods[e // T], rng) for e in range(M * T)]
    kre, kim = [pick("random", q, rng) for q in mods], [pick("random", q, rng) for q in mods]
    half = N // 1024
    chunks = [0, half - 1, half, N // 512 - 1]
    lo, ids = [1, 0, 3, 2], [0, 1, 2, 3]
    out = np.full((M, N), GUARD, dtype=np.uint64)
    vs = run(lib, mods, logN, x, li, out, lo, ids, T, re, im, kre, kim, chunks)
    ran = np.zeros(N, dtype=bool)
    for i, q in enumerate(mods):
        for ch in chunks:
            ran[ch * 512:ch * 512 + 512] = True
            got = [int(a) for a in out[lo[i]][ch * 512:ch * 512 + 512]]
            assert got == expected(x, li, i, T, q, vs[i], N, ch, re, im, kre, kim), (logN, i, ch)
        assert np.all(out[lo[i]][~ran] == GUARD)
        # the two middle chunks differ by the sign of the monomial, nothing else: with the halves swapped they do not match
        assert [int(a) for a in out[lo[i]][half * 512:half * 512 + 512]] != expected(x, li, i, T, q, q - vs[i], N, half, re, im, kre, kim)


def test_the_accumulator_at_its_fullest(env):
    """T = 16, every input q - 1 and (a, b) = (q - 1, 0), the constant q - 1, at the largest modulus of the chain: both halves' scalars are q - 1,
    16 (q - 1)^2 + (q - 1), reduced once; and with (a, b) chosen so that the scalar of the FIRST half is q - 1 where a alone is not"""
    lib, chain = env
    mods = chain_moduli(chain)
    N, T = 1 << LOGN, 16
    mod = max(range(len(mods)), key=lambda i: mods[i])
    q = mods[mod]
    assert 16 * (q - 1) ** 2 + q - 1 < 1 << 125
    x = np.full((T, N), q - 1, dtype=np.uint64)
    out = np.zeros((1, N), dtype=np.uint64)
    allc = range(N // 512)
    vs = run(lib, mods, LOGN, x, range(T), out, [0], [mod], T, [q - 1] * T, [0] * T, [q - 1], None, allc)
    assert np.all(out == np.uint64((16 * (q - 1) ** 2 + q - 1) % q))
    v = vs[mod]
    b = 5
    a = (q - 1 - b * v) % q                       # a + b v = q - 1 on the first half; a - b v on the second
    out[:] = 0
    run(lib, mods, LOGN, x, range(T), out, [0], [mod], T, [a] * T, [b] * T, [q - 1], [0], allc)
    assert np.all(out[0][:N // 2] == np.uint64((16 * (q - 1) ** 2 + q - 1) % q))
    assert np.all(out[0][N // 2:] == np.uint64((16 * ((a - b * v) % q) * (q - 1) + q - 1) % q))


@pytest.mark.parametrize("generic,chain", [(0, "mont32"), (1, "mont32"), (1, "mixed")])
def test_stand_alone_program_under_the_sanitizers(tmp_path, generic, chain):
    """tests/emu/hm_emu_clincomb_main.cpp with its own main, compiled with the sanitizers and run as a process of its own (nothing is loaded into
    Python): every T, fill, pair of scalars and constants on every modulus, every chunk of every entry; every buffer is sized exactly"""
    exe = tmp_path / "hm_emu_clincomb_main"
    subprocess.check_call(["g++"] + (["-DHM_GENERIC=1"] if generic else []) + ["-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-Wall", "-Wno-unknown-pragmas", "-o", str(exe), os.path.join(HERE, "emu", "hm_emu_clincomb_main.cpp")] + SOURCES)
    r = subprocess.run([str(exe), str(LOGN)] + [str(q) for q in chain_moduli(chain)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "bad=0" in r.stdout and "cases=768" in r.stdout, r.stdout + r.stderr
