"""The lifted forward first pass (homulator_amd/csrc/hm_ntt_passes.inl: MODE 10, hm_ph_load_global_lift over hm_lift: the kernel of hm_ntt_lift, ModRaise)
on the CPU, no GPU: tests/emu/hm_emu_lift.cpp compiles the device headers with g++, once per arithmetic back-end (HM_GENERIC 0 and 1), and runs every
thread of every workgroup, phase by phase, in both geometries.  Checked against Python integers: the input is centred against the source modulus and
reduced into the target modulus with integers, then transformed by the oracle.
Modulus pairs: target above, below and equal to the source; a 60-bit source into a 21-bit target and the reverse; the pairs of the 36-bit chain; on
the mont32 build (moduli h 2^32 + 1) the widest and the narrowest such primes the test uses, 60 and 37 bits.
Fills: uniform, 0, q_s - 1, and (q_s - 1) / 2 and (q_s + 1) / 2, the two sides of the centring boundary."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from oracle.homoracle import Oracle, chain_below

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
L, K = 3, 1
u64, u32, vp = C.c_uint64, C.c_uint32, C.c_void_p
SOURCES = [os.path.join(HERE, "emu", "hm_emu_lift.cpp"), os.path.join(ROOT, "homulator_amd", "csrc", "hm_params.cpp")]
FILLS = ["uniform", "zero", "qs-1", "half", "half+1"]
NARROW_MONT32 = 18 * 2**32 + 1      # the smallest prime h 2^32 + 1: 37 bits, 1 mod 2N for every ring


def chain_moduli(chain, logN):
    """the L + K = 4 moduli of a named chain and the (source, target) pairs worth running on it"""
    if chain == "mont32":     # 60-bit primes h 2^32 + 1, descending, and the 37-bit one
        m = Oracle(logN, L, K).moduli
        return [m[0], m[1], NARROW_MONT32, m[2]], [(0, 1), (1, 0), (0, 0), (0, 2), (2, 0), (2, 2), (3, 2)]
    wide, narrow, mid = chain_below(logN, 60, 1), chain_below(logN, 21, 1), chain_below(logN, 36, 2)
    # 60 -> 21 bits and back, the 36-bit chain's pairs in both orders, equal, 36 -> 21
    return [wide[0], narrow[0], mid[0], mid[1]], [(0, 1), (1, 0), (2, 3), (3, 2), (2, 2), (1, 1), (2, 1), (0, 2)]


@pytest.fixture(scope="module", params=[(0, "mont32"), (1, "mont32"), (1, "mixed")], ids=["mont32-build", "generic-build", "generic-build-mixed-widths"])
def env(request, tmp_path_factory):
    """(library, chain): the emulator of one arithmetic build, and the chain it runs"""
    generic, chain = request.param
    so = tmp_path_factory.mktemp("emu_lift") / f"libhm_emu_lift_{generic}.so"
    subprocess.check_call(["g++"] + (["-DHM_GENERIC=1"] if generic else []) + ["-O2", "-std=c++17", "-fPIC", "-shared", "-Wall", "-Wno-unknown-pragmas", "-o", str(so)] + SOURCES)
    lib = C.CDLL(str(so))
    assert lib.emu_lift_generic() == generic
    lib.emu_lift_create.restype = vp
    lib.emu_lift_create.argtypes = [u32, u32, u32, vp, vp]
    lib.emu_lift_destroy.argtypes = [vp]
    lib.emu_lift_modulus.restype = u64
    lib.emu_lift_modulus.argtypes = [vp, u32]
    lib.emu_ntt_lift.argtypes = [vp, C.c_int, u32, u32, vp, vp]
    lib.emu_lift_word.restype = u64
    lib.emu_lift_word.argtypes = [vp, u32, u32, u64]
    return lib, chain


_made = {}


def context(env, logN):
    """(emulator handle, oracle, pairs) on the same moduli"""
    lib, chain = env
    key = (id(lib), chain, logN)
    if key not in _made:
        mods, pairs = chain_moduli(chain, logN)
        o = Oracle(logN, L, K, chain=mods)
        o.set_threads(8)
        arr = np.array(mods, dtype=np.uint64)
        h = lib.emu_lift_create(logN, L, K, arr[:L].ctypes.data_as(vp), arr[L:].ctypes.data_as(vp))
        assert h and [lib.emu_lift_modulus(h, m) for m in range(L + K)] == o.moduli == mods
        _made[key] = (h, o, pairs)
    return _made[key]


def centred_mod(c, qs, q):
    return (c if c <= (qs - 1) // 2 else c - qs) % q


def filled(rng, qs, N, fill):
    if fill == "uniform":
        return rng.integers(0, qs, N, dtype=np.uint64)
    return np.full(N, {"zero": 0, "qs-1": qs - 1, "half": (qs - 1) // 2, "half+1": (qs + 1) // 2}[fill], dtype=np.uint64)


def lift_case(env, logN, ept, src, dst, fill):
    lib, _ = env
    h, o, _ = context(env, logN)
    qs, q = o.moduli[src], o.moduli[dst]
    x = filled(np.random.default_rng(logN * 100 + ept + 7 * src + dst), qs, o.N, fill)
    out = np.empty(o.N, dtype=np.uint64)
    assert lib.emu_ntt_lift(h, ept, src, dst, x.ctypes.data_as(vp), out.ctypes.data_as(vp)) == 0
    red = np.array([centred_mod(int(v), qs, q) for v in x], dtype=np.uint64)
    exp = o.ntt([dst], red[None, :])[0]
    assert np.array_equal(out, exp), (logN, ept, src, dst, fill)
    if src == dst:   # the identity lift is the plain forward transform of the input
        assert np.array_equal(out, o.ntt([dst], x[None, :])[0])


GEOMETRIES = [(13, 16), (15, 16), (15, 8), (16, 8)]   # (logN, coefficients per thread): the smallest ring, both geometries where both exist, both COL lengths of the small one


@pytest.mark.parametrize("logN,ept", GEOMETRIES)
def test_uniform_input_on_every_modulus_pair(env, logN, ept):
    for src, dst in context(env, logN)[2]:
        lift_case(env, logN, ept, src, dst, "uniform")


@pytest.mark.parametrize("fill", FILLS[1:])
def test_constant_fills_at_the_ends_and_the_centring_boundary(env, fill):
    for logN, ept in ((13, 16), (15, 8)):
        for src, dst in context(env, logN)[2]:
            lift_case(env, logN, ept, src, dst, fill)


def test_the_load_routine_word_by_word(env):
    """hm_lift alone: the boundary words of every pair, and ANY word below 2^60 (the stated range, wider than the residues of the source) against the
    target modulus alone (source = target: both halves reduce to c mod q)"""
    lib, _ = env
    h, o, pairs = context(env, 13)
    rng = np.random.default_rng(11)
    for src, dst in pairs:
        qs, q = o.moduli[src], o.moduli[dst]
        words = [0, 1, (qs - 1) // 2 - 1, (qs - 1) // 2, (qs + 1) // 2, (qs + 1) // 2 + 1, qs - 2, qs - 1, min(q, qs - 1), min(q - 1, qs - 1)]
        words += [k * q + d for k in (1, 2, qs // q) for d in (-1, 0, 1) if 0 <= k * q + d < qs]
        words += [int(v) for v in rng.integers(0, qs, 200, dtype=np.uint64)]
        for c in words:
            got = lib.emu_lift_word(h, src, dst, c)
            assert got == centred_mod(c, qs, q) and got < q, (src, dst, c)
    top = 2**60 - 1
    for dst in range(L + K):
        q = o.moduli[dst]
        for c in [top, top - 1, q, q + 1, 2 * q - 1, (top // q) * q - 1, (top // q) * q, (top // q) * q + 1] + [int(v) for v in rng.integers(0, 2**60, 200, dtype=np.uint64)]:
            if c <= top:
                assert lib.emu_lift_word(h, dst, dst, c) == c % q, (dst, c)


@pytest.mark.parametrize("generic,chain,logN", [(0, "mont32", 13), (1, "mixed", 13), (1, "mixed", 15)])
def test_stand_alone_program_under_the_sanitizers(tmp_path, generic, chain, logN):
    """tests/emu/hm_emu_lift_main.cpp with its own main, compiled with the sanitizers and run as a process of its own (nothing is loaded into
    Python): every ordered pair of the chain's moduli, the five fills, both geometries where the ring has both; every buffer is sized exactly"""
    exe = tmp_path / "hm_emu_lift_main"
    subprocess.check_call(["g++"] + (["-DHM_GENERIC=1"] if generic else []) + ["-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-Wall", "-Wno-unknown-pragmas", "-o", str(exe), os.path.join(HERE, "emu", "hm_emu_lift_main.cpp")] + SOURCES)
    mods, _ = chain_moduli(chain, logN)
    r = subprocess.run([str(exe), str(logN)] + [str(m) for m in mods], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "bad=0" in r.stdout, r.stdout + r.stderr
