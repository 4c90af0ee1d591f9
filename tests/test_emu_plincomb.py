"""The per-thread core of hm_plincomb (homulator_amd/csrc/hm_rec_core.h: hm_plincomb_thread, the kernel of hplincomb) on the CPU, no GPU:
tests/emu/hm_emu_plincomb.cpp compiles the device header with g++, once per arithmetic back-end (HM_GENERIC 0 and 1), builds the records as the
entry point does and runs every thread of the chosen workgroups.  Checked against Python integers: o0 = sum_t p_t x_t + p_0, o1 = sum_t p_t y_t
mod q, entry by entry.
Rings: logN 13 and 17, the first and the last chunk.  T: 1, 2, 3, 16 (no round of the two-term loop, the tail behind it, one round, the most).
Fills: uniform, all 0, all q - 1, for the plaintexts and the ciphertexts independently.  Addend: none, all 0, all q - 1, uniform.  Moduli: the
smallest and the largest the back-end accepts (mont32: 18 2^32 + 1 and the largest prime h 2^32 + 1 below 2^60; generic: just above 2^20 and just
below 2^60) and the 36-bit chain's (generic).  The worst case, T = 16 with every plaintext, ciphertext and addend entry q - 1 at the largest
modulus, puts 16 (q - 1)^2 + q - 1 < 2^125 into c0's accumulator and 16 (q - 1)^2 into c1's."""
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
SOURCES = [os.path.join(HERE, "emu", "hm_emu_plincomb.cpp"), os.path.join(ROOT, "homulator_amd", "csrc", "hm_params.cpp")]
NARROW_MONT32 = 18 * 2**32 + 1      # the smallest prime h 2^32 + 1: 37 bits, 1 mod 2N for every ring
LOGN = 13
TERMS = [1, 2, 3, 16]
FILLS = ["uniform", "zero", "q-1"]
ADDENDS = [None, "zero", "q-1", "uniform"]
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
    so = tmp_path_factory.mktemp("emu_plincomb") / f"libhm_emu_plincomb_{generic}.so"
    subprocess.check_call(["g++"] + (["-DHM_GENERIC=1"] if generic else []) + ["-O2", "-std=c++17", "-fPIC", "-shared", "-Wall", "-Wno-unknown-pragmas", "-o", str(so)] + SOURCES)
    lib = C.CDLL(str(so))
    assert lib.emu_plincomb_generic() == generic
    lib.emu_plincomb_rec_words.argtypes = [u32]
    lib.emu_plincomb_rec_words.restype = u32
    lib.emu_plincomb.argtypes = [vp, u32, u32] + [vp] * 11 + [u32, u32, vp, u32]
    return lib, chain


def ptr(a):
    return None if a is None else a.ctypes.data_as(vp)


def u(v):
    return None if v is None else np.array(list(v), dtype=np.uint32)


def run(lib, mods, logN, p, lp, x, lx0, lx1, addend, la, out, l0, l1, ids, T, chunks):
    m = np.array([int(q) for q in mods], dtype=np.uint64)
    keep = [u(lp), u(lx0), u(lx1), u(la), u(l0), u(l1), u(ids), u(chunks)]
    assert lib.emu_plincomb(ptr(m), len(mods), logN, ptr(p), ptr(keep[0]), ptr(x), ptr(keep[1]), ptr(keep[2]), ptr(addend), ptr(keep[3]), ptr(out),
                            ptr(keep[4]), ptr(keep[5]), ptr(keep[6]), len(ids), T, ptr(keep[7]), len(chunks)) == 0


def expected(p, lp, x, lx, addend, la, i, T, q, ch):
    """one output of entry i under modulus q, chunk ch, in Python integers; addend None: nothing is added"""
    sl = slice(ch * 512, ch * 512 + 512)
    acc = np.zeros(512, dtype=object) if addend is None else addend[la[i]][sl].astype(object)
    for t in range(T):
        e = i * T + t
        acc = acc + p[lp[e]][sl].astype(object) * x[lx[e]][sl].astype(object)
    return [int(a) % q for a in acc]


def filled(kind, q, N, rng):
    return {"uniform": rng.integers(0, q, N, dtype=np.uint64), "zero": np.zeros(N, dtype=np.uint64), "q-1": np.full(N, q - 1, dtype=np.uint64)}[kind]


def test_record_size_is_32_bytes_and_16_per_term(env):
    lib, _ = env
    for T in range(1, 17):
        assert lib.emu_plincomb_rec_words(T) * 4 == 32 + 16 * T


@pytest.mark.parametrize("T", TERMS)
def test_records_with_permuted_repeated_and_shared_limbs(env, T):
    """the thread function over whole workgroups: one entry per modulus, the ciphertext limbs permuted, one ciphertext limb read by two entries
    (and, at T >= 2, twice by one entry, as x and as y), one plaintext limb shared by two entries and, at T >= 2, by two terms of one entry; the
    first and the last chunk of every entry; the outputs of the chunks that did not run, and the guard limb between the outputs, keep their guard
    value.  Every pair of fills (plaintexts, ciphertexts) runs with every kind of addend"""
    lib, chain = env
    mods = chain_moduli(chain)
    N, M = 1 << LOGN, len(mods)
    rng = np.random.default_rng(400 + T)
    qmin = min(mods)          # a shared limb holds residues of every modulus that reads it
    n_x = 2 * M * T
    lx0 = [(2 * e * 7 + 3) % n_x for e in range(M * T)]
    lx1 = [((2 * e + 1) * 7 + 3) % n_x for e in range(M * T)]
    lp = [M * T - 1 - e for e in range(M * T)]
    lx0[M * T - 1] = lx0[0]   # entries 0 and M - 1 share a ciphertext limb
    lp[M * T - 1] = lp[0]     # ... and a plaintext limb
    if T >= 2:
        lx1[1] = lx0[0]       # entry 0 reads one limb as x of term 0 and as y of term 1
        lp[1] = lp[0]         # ... and one plaintext limb in two terms
    shared_x, shared_p = {lx0[0]}, {lp[0]}
    l0, l1, la, ids = [3, 6, 0, 5], [8, 2, 4, 1], [2, 0, 3, 1], [0, 1, 2, 3]      # limb 7 of the output buffer is nobody's: a guard
    chunks = [0, N // 512 - 1]
    ran = np.zeros(N, dtype=bool)
    for ch in chunks:
        ran[ch * 512:ch * 512 + 512] = True
    for fp, fx in itertools.product(FILLS, FILLS):
        p, x = np.zeros((M * T, N), dtype=np.uint64), np.zeros((n_x, N), dtype=np.uint64)
        for e in range(M * T):
            q = mods[e // T]
            p[lp[e]] = filled(fp, qmin if lp[e] in shared_p else q, N, rng)
            for lx in (lx0, lx1):
                x[lx[e]] = filled(fx, qmin if lx[e] in shared_x else q, N, rng)
        for ka in ADDENDS:
            addend = None if ka is None else np.stack([filled(ka, mods[la.index(r)], N, rng) for r in range(M)])
            out = np.full((9, N), GUARD, dtype=np.uint64)
            run(lib, mods, LOGN, p, lp, x, lx0, lx1, addend, None if ka is None else la, out, l0, l1, ids, T, chunks)
            for i, q in enumerate(mods):
                for ch in chunks:
                    sl = slice(ch * 512, ch * 512 + 512)
                    assert [int(a) for a in out[l0[i]][sl]] == expected(p, lp, x, lx0, addend, la, i, T, q, ch), (T, fp, fx, ka, i, ch, "c0")
                    assert [int(a) for a in out[l1[i]][sl]] == expected(p, lp, x, lx1, None, la, i, T, q, ch), (T, fp, fx, ka, i, ch, "c1")
                assert np.all(out[l0[i]][~ran] == GUARD) and np.all(out[l1[i]][~ran] == GUARD)
            assert np.all(out[7] == GUARD)


@pytest.mark.parametrize("logN", [13, 17])
def test_the_first_and_the_last_chunk_of_both_rings(env, logN):
    """T = 3 with uniform fills and an addend: chunk 0 and chunk N / 512 - 1, whose last thread touches the last 16 bytes of every limb-poly; the
    neighbouring chunks keep their guard value"""
    lib, chain = env
    mods = chain_moduli(chain, logN)
    N, M, T = 1 << logN, len(mods), 3
    rng = np.random.default_rng(500 + logN)
    lp = [(e * 5 + 1) % (M * T) for e in range(M * T)]
    lx0 = [(e * 5 + 2) % (M * T) for e in range(M * T)]
    lx1 = [M * T + (e * 7 + 4) % (M * T) for e in range(M * T)]
    p = np.stack([rng.integers(0, mods[lp.index(r) // T], N, dtype=np.uint64) for r in range(M * T)])
    x = np.stack([rng.integers(0, mods[(lx0.index(r) if r < M * T else lx1.index(r)) // T], N, dtype=np.uint64) for r in range(2 * M * T)])
    la, l0, l1, ids = [1, 0, 3, 2], [1, 0, 3, 2], [5, 7, 4, 6], [0, 1, 2, 3]
    addend = np.stack([rng.integers(0, mods[la.index(r)], N, dtype=np.uint64) for r in range(M)])
    out = np.full((2 * M, N), GUARD, dtype=np.uint64)
    chunks = [0, N // 512 - 1]
    run(lib, mods, logN, p, lp, x, lx0, lx1, addend, la, out, l0, l1, ids, T, chunks)
    for i, q in enumerate(mods):
        for ch in chunks:
            sl = slice(ch * 512, ch * 512 + 512)
            assert [int(a) for a in out[l0[i]][sl]] == expected(p, lp, x, lx0, addend, la, i, T, q, ch), (logN, i, ch, "c0")
            assert [int(a) for a in out[l1[i]][sl]] == expected(p, lp, x, lx1, None, la, i, T, q, ch), (logN, i, ch, "c1")
        assert np.all(out[l0[i]][512:N - 512] == GUARD) and np.all(out[l1[i]][512:N - 512] == GUARD)


def test_the_accumulators_at_their_fullest(env):
    """T = 16, every plaintext, ciphertext and addend entry q - 1, at the largest modulus of the chain: 16 (q - 1)^2 + (q - 1) in c0's
    accumulator, 16 (q - 1)^2 in c1's, each reduced once"""
    lib, chain = env
    mods = chain_moduli(chain)
    N, T = 1 << LOGN, 16
    mod = max(range(len(mods)), key=lambda i: mods[i])
    q = mods[mod]
    assert 16 * (q - 1) ** 2 + q - 1 < 1 << 125
    p = np.full((T, N), q - 1, dtype=np.uint64)
    x = np.full((2 * T, N), q - 1, dtype=np.uint64)
    addend = np.full((1, N), q - 1, dtype=np.uint64)
    out = np.zeros((2, N), dtype=np.uint64)
    run(lib, mods, LOGN, p, range(T), x, range(T), range(T, 2 * T), addend, [0], out, [0], [1], [mod], T, range(N // 512))
    assert np.all(out[0] == np.uint64((16 * (q - 1) ** 2 + q - 1) % q))
    assert np.all(out[1] == np.uint64((16 * (q - 1) ** 2) % q))


@pytest.mark.parametrize("generic,chain", [(0, "mont32"), (1, "mont32"), (1, "mixed")])
def test_stand_alone_program_under_the_sanitizers(tmp_path, generic, chain):
    """tests/emu/hm_emu_plincomb_main.cpp with its own main, compiled with the sanitizers and run as a process of its own (nothing is loaded into
    Python): every T, pair of fills and addend on every modulus, every chunk of every entry; every buffer is sized exactly"""
    exe = tmp_path / "hm_emu_plincomb_main"
    subprocess.check_call(["g++"] + (["-DHM_GENERIC=1"] if generic else []) + ["-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-Wall", "-Wno-unknown-pragmas", "-o", str(exe), os.path.join(HERE, "emu", "hm_emu_plincomb_main.cpp")] + SOURCES)
    r = subprocess.run([str(exe), str(LOGN)] + [str(q) for q in chain_moduli(chain)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "bad=0" in r.stdout and "cases=144" in r.stdout, r.stdout + r.stderr
