"""The per-thread core of hm_lincomb_multi (homulator_amd/csrc/hm_rec_core.h: hm_lincomb_multi_thread, the kernel of hmlincomb) on the CPU, no
GPU: tests/emu/hm_emu_mlincomb.cpp compiles the device header with g++, once per arithmetic back-end (HM_GENERIC 0 and 1), builds the records as
the entry point does and runs every thread of the chosen workgroups, for both built tiles.  Checked against Python integers:
out_m = sum_t s_{m,t} x_t + k_m mod q.
T: 1, 2, 3, 16 (no round of the two-term loop, the tail behind it, one round, the most).  M: 1, TILE - 1, TILE, TILE + 1, 16 (one short tile, a
full one, a full one and a tile of one output, the most).  Fills: uniform, all 0, all q - 1.  Scalars: 0, 1, q - 1, random.  Constants: none, 0,
q - 1, random.  Moduli: the smallest and the largest the back-end accepts (mont32: 18 2^32 + 1 and the largest prime h 2^32 + 1 below 2^60;
generic: just above 2^20 and just below 2^60) and the 36-bit chain's (generic).  The worst case, T = 16 with every input, scalar and constant
q - 1 at the largest modulus, puts 16 (q - 1)^2 + q - 1 < 2^125 into every accumulator.
Every (tile, T, M) runs six combinations that hold every fill, scalar and constant kind; (T, M) = (3, TILE + 1) runs all 48."""
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
SOURCES = [os.path.join(HERE, "emu", "hm_emu_mlincomb.cpp"), os.path.join(ROOT, "homulator_amd", "csrc", "hm_params.cpp")]
NARROW_MONT32 = 18 * 2**32 + 1      # the smallest prime h 2^32 + 1: 37 bits, 1 mod 2N for every ring
LOGN = 13
TILES = [4, 8]
TERMS = [1, 2, 3, 16]
FILLS = ["uniform", "zero", "q-1"]
SCALES = ["0", "1", "q-1", "random"]
CONSTS = [None, "0", "q-1", "random"]
# every fill, every scalar kind and every constant kind at least once
COVER = [("uniform", "random", "random"), ("zero", "random", None), ("q-1", "q-1", "q-1"), ("uniform", "0", "0"), ("uniform", "1", "random"),
         ("q-1", "random", "q-1")]
GUARD = np.uint64(0xDEADBEEFDEADBEEF)


def outputs(tile):
    return [1, tile - 1, tile, tile + 1, 16]


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
    so = tmp_path_factory.mktemp("emu_mlincomb") / f"libhm_emu_mlincomb_{generic}.so"
    subprocess.check_call(["g++"] + (["-DHM_GENERIC=1"] if generic else []) + ["-O2", "-std=c++17", "-fPIC", "-shared", "-Wall", "-Wno-unknown-pragmas", "-o", str(so)] + SOURCES)
    lib = C.CDLL(str(so))
    assert lib.emu_mlincomb_generic() == generic
    for f in (lib.emu_mlincomb_rec_words, lib.emu_mlincomb_records):
        f.argtypes = [u32, u32]
        f.restype = u32
    lib.emu_mlincomb_default_tile.restype = u32
    lib.emu_mlincomb.argtypes = [vp, u32, u32, vp, vp, vp, vp, vp, u32, u32, u32, u32, vp, vp, vp, u32]
    return lib, chain_moduli(chain)


def ptr(a):
    return None if a is None else a.ctypes.data_as(vp)


def pick(kind, q, rng):
    return {"0": 0, "1": 1, "q-1": q - 1}[kind] if kind != "random" else int(rng.integers(0, q))


def test_record_size_and_count(env):
    """a record is a multiple of 16 bytes that holds its header, T limbs and per slot a limb, a constant and T scalars; an entry takes
    ceil(M / tile) of them; the default tile is the one the Python binding names"""
    from homulator_amd import hip
    lib, _ = env
    assert lib.emu_mlincomb_default_tile() == hip.LINCOMB_MULTI_TILE and hip.LINCOMB_MULTI_TILE in TILES and hip.LINCOMB_MULTI_MAX_OUT == 16
    for tile in TILES:
        for T in range(1, 17):
            w = lib.emu_mlincomb_rec_words(T, tile)
            assert w * 4 % 16 == 0 and 3 + T + tile * (3 + 2 * T) <= w < 3 + T + tile * (3 + 2 * T) + 4 + tile + 4
        for M in range(1, 17):
            assert lib.emu_mlincomb_records(M, tile) == -(-M // tile)
    assert lib.emu_mlincomb_rec_words(16, 8) * 4 == 1232   # the largest record: about 1.2 KB


def run(lib, mods, tile, T, M, combos, rng):
    """one entry per modulus, the inputs at permuted limbs, one limb read by two entries (and, at T >= 2, twice by one entry), the outputs at
    permuted limbs, the first and the last chunk of every record; the outputs of the chunks that did not run keep their guard value"""
    N, E = 1 << LOGN, len(mods)
    m = np.array(mods, dtype=np.uint64)
    qmin = min(mods)          # a shared limb holds residues of every modulus that reads it
    n_in, n_out = E * T, E * M
    li = [(e * 7 + 3) % n_in for e in range(n_in)]
    li[n_in - 1] = li[0]      # entries 0 and E - 1 share a limb
    if T >= 2:
        li[1] = li[0]         # entry 0 reads one limb twice
    shared = {li[0]}
    lo = [(e * 11 + 1) % n_out for e in range(n_out)]   # 11 is coprime to every E M
    ids, chunks = list(range(E)), [0, N // 512 - 1]
    cols = np.r_[0:512, N - 512:N]
    u = lambda v: np.array(v, dtype=np.uint32)
    x = None
    last_fill = None
    for fill, sk, kk in combos:
        if fill != last_fill:
            x = np.zeros((n_in, N), dtype=np.uint64)
            for e in range(n_in):
                q = qmin if li[e] in shared else mods[e // T]
                x[li[e]] = {"uniform": rng.integers(0, q, N, dtype=np.uint64), "zero": 0, "q-1": q - 1}[fill]
            last_fill = fill
        s = [pick(sk, mods[e // (M * T)], rng) for e in range(n_out * T)]
        k = None if kk is None else [pick(kk, mods[e // M], rng) for e in range(n_out)]
        out = np.full((n_out, N), GUARD, dtype=np.uint64)
        sa = np.array(s, dtype=np.uint64)
        ka = None if k is None else np.array(k, dtype=np.uint64)
        keep = [u(li), u(lo), u(ids), u(chunks)]
        assert lib.emu_mlincomb(ptr(m), E, LOGN, ptr(x), ptr(keep[0]), ptr(out), ptr(keep[1]), ptr(keep[2]), E, T, M, tile, ptr(sa), ptr(ka),
                                ptr(keep[3]), len(chunks)) == 0
        for i, q in enumerate(mods):
            xs = x[[li[i * T + t] for t in range(T)]][:, cols].astype(object)                      # (T, 1024) Python integers
            S = np.array(s[i * M * T:(i + 1) * M * T], dtype=object).reshape(M, T)
            K = np.array([0] * M if k is None else k[i * M:(i + 1) * M], dtype=object).reshape(M, 1)
            exp = (S.dot(xs) + K) % q
            for o in range(M):
                row = out[lo[i * M + o]]
                assert [int(v) for v in row[cols]] == list(exp[o]), (tile, T, M, fill, sk, kk, i, o)
                assert np.all(row[512:N - 512] == GUARD)


@pytest.mark.parametrize("tile", TILES)
@pytest.mark.parametrize("T", TERMS)
def test_records_with_permuted_and_repeated_limbs(env, tile, T):
    lib, mods = env
    rng = np.random.default_rng(1000 * tile + T)
    for M in outputs(tile):
        run(lib, mods, tile, T, M, COVER, rng)


@pytest.mark.parametrize("tile", TILES)
def test_every_fill_scalar_and_constant(env, tile):
    lib, mods = env
    run(lib, mods, tile, 3, tile + 1, list(itertools.product(FILLS, SCALES, CONSTS)), np.random.default_rng(77 + tile))


@pytest.mark.parametrize("tile", TILES)
def test_the_accumulators_at_their_fullest(env, tile):
    """T = 16, M = 16, every input, every scalar and every constant q - 1, at the largest modulus of the chain: 16 (q - 1)^2 + (q - 1) in every
    accumulator, reduced once"""
    lib, mods = env
    N, T, M = 1 << LOGN, 16, 16
    mod = max(range(len(mods)), key=lambda i: mods[i])
    q = mods[mod]
    assert 16 * (q - 1) ** 2 + q - 1 < 1 << 125
    m = np.array(mods, dtype=np.uint64)
    x = np.full((T, N), q - 1, dtype=np.uint64)
    out = np.zeros((M, N), dtype=np.uint64)
    u = lambda v: np.array(v, dtype=np.uint32)
    keep = [u(range(T)), u(range(M)), u([mod]), u(range(N // 512))]
    sa, ka = np.full(M * T, q - 1, dtype=np.uint64), np.full(M, q - 1, dtype=np.uint64)
    assert lib.emu_mlincomb(ptr(m), len(mods), LOGN, ptr(x), ptr(keep[0]), ptr(out), ptr(keep[1]), ptr(keep[2]), 1, T, M, tile, ptr(sa), ptr(ka),
                            ptr(keep[3]), N // 512) == 0
    assert np.all(out == np.uint64((16 * (q - 1) ** 2 + q - 1) % q))


def test_a_tile_that_is_not_built_is_refused(env):
    lib, mods = env
    m = np.array(mods, dtype=np.uint64)
    assert lib.emu_mlincomb(ptr(m), len(mods), LOGN, None, None, None, None, None, 0, 1, 1, 2, None, None, None, 0) == 2


@pytest.mark.parametrize("generic,chain", [(0, "mont32"), (1, "mont32"), (1, "mixed")])
def test_stand_alone_program_under_the_sanitizers(tmp_path, generic, chain):
    """tests/emu/hm_emu_mlincomb_main.cpp with its own main, compiled with the sanitizers and run as a process of its own (nothing is loaded into
    Python): both tiles, every T, M, fill, scalar and constant on every modulus; every buffer is sized exactly"""
    exe = tmp_path / "hm_emu_mlincomb_main"
    subprocess.check_call(["g++"] + (["-DHM_GENERIC=1"] if generic else []) + ["-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-Wall", "-Wno-unknown-pragmas", "-o", str(exe), os.path.join(HERE, "emu", "hm_emu_mlincomb_main.cpp")] + SOURCES)
    r = subprocess.run([str(exe), str(LOGN)] + [str(q) for q in chain_moduli(chain)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "bad=0" in r.stdout and "cases=1920" in r.stdout, r.stdout + r.stderr
