"""The product operands of the transforms (homulator_amd/csrc/hm_ntt_passes.inl: MODE 8, the fused forward epilogue whose minuend is a (.) a2, and
MODE 9, the inverse first pass whose input is src (.) a2: the kernels of hm_ntt_mix_sub_scale_mul and hm_ntt_mul) on the CPU, no GPU:
tests/emu/hm_emu_rescale.cpp compiles the device headers with g++, once per arithmetic back-end (HM_GENERIC 0 and 1), and runs every thread of
every workgroup, phase by phase, in both geometries.  Checked against Python integers (the oracle's transform, then the formula with integers) and
against the existing MODE 3 / plain inverse passes fed a separately computed product: the two must agree word for word."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from oracle.homoracle import Oracle

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
L, K = 3, 1
u64, u32, vp = C.c_uint64, C.c_uint32, C.c_void_p
SOURCES = [os.path.join(HERE, "emu", "hm_emu_rescale.cpp"), os.path.join(ROOT, "homulator_amd", "csrc", "hm_params.cpp")]


@pytest.fixture(scope="module", params=[(0, "mont32"), (1, "mont32"), (1, "survey")], ids=["mont32-build", "generic-build", "generic-build-60-bit-chain"])
def env(request, tmp_path_factory):
    """(library, chain): the emulator of one arithmetic build, and the chain it runs"""
    generic, chain = request.param
    so = tmp_path_factory.mktemp("emu_rescale") / f"libhm_emu_rescale_{generic}.so"
    subprocess.check_call(["g++"] + (["-DHM_GENERIC=1"] if generic else []) + ["-O2", "-std=c++17", "-fPIC", "-shared", "-Wall", "-Wno-unknown-pragmas", "-o", str(so)] + SOURCES)
    lib = C.CDLL(str(so))
    assert lib.emu_rescale_generic() == generic
    lib.emu_rescale_create.restype = vp
    lib.emu_rescale_create.argtypes = [u32, u32, u32, vp, vp]
    lib.emu_rescale_destroy.argtypes = [vp]
    lib.emu_rescale_modulus.restype = u64
    lib.emu_rescale_modulus.argtypes = [vp, u32]
    lib.emu_ntt_sub_scale_mul.argtypes = [vp, C.c_int, u32, vp, vp, vp, vp, vp, u64, vp, u64, u64]
    lib.emu_intt_mul.argtypes = [vp, C.c_int, u32, vp, vp, vp, u64, C.c_int]
    lib.emu_epi_mul.restype = u64
    lib.emu_epi_mul.argtypes = [vp, u32, u64, u64]
    lib.emu_epilogue8.restype = u64
    lib.emu_epilogue8.argtypes = [vp, u32, u64, u64, u64, C.c_int, u64, u64]
    return lib, chain


_made = {}


def context(env, logN):
    """(emulator handle, oracle) on the same moduli"""
    lib, chain = env
    key = (id(lib), chain, logN)
    if key not in _made:
        o = Oracle(logN, L, K, chain=chain)
        o.set_threads(8)
        mods = np.array(o.moduli, dtype=np.uint64)
        h = lib.emu_rescale_create(logN, L, K, mods[:L].ctypes.data_as(vp), mods[L:].ctypes.data_as(vp))
        assert h and [lib.emu_rescale_modulus(h, m) for m in range(L + K)] == o.moduli
        _made[key] = (h, o)
    return _made[key]


def p(a):
    return None if a is None else a.ctypes.data_as(vp)


def filled(rng, q, N, fill):
    return np.full(N, q - 1 if fill == "q-1" else 0, dtype=np.uint64) if fill != "uniform" else rng.integers(0, q, N, dtype=np.uint64)


def obj(a):
    return np.array([int(x) for x in a], dtype=object)


def forward_case(env, logN, ept, mod, fill, with_mix, with_addend, addend_k):
    lib, _ = env
    h, o = context(env, logN)
    N, q = o.N, o.moduli[mod]
    rng = np.random.default_rng(logN * 1000 + ept * 10 + mod + len(fill))
    x, a, b, d, mix = (filled(rng, q, N, fill) for _ in range(5))
    k, mk = int(rng.integers(1, q)), int(rng.integers(1, q))
    out, out3 = np.empty(N, dtype=np.uint64), np.empty(N, dtype=np.uint64)
    args = lambda minuend, fac, dst: (h, ept, mod, p(x), p(minuend), p(fac), p(d) if with_addend else None, p(dst), k, p(mix) if with_mix else None,
                                      mk if with_mix else 0, addend_k if with_addend else 0)
    assert lib.emu_ntt_sub_scale_mul(*args(a, b, out)) == 0
    # Python integers: the oracle's transform of the prologue's result, then the formula
    xin = (obj(x) + mk * obj(mix)) % q if with_mix else obj(x)
    t = obj(o.ntt([mod], np.array([[int(v) for v in xin]], dtype=np.uint64))[0])
    exp = (obj(a) * obj(b) - t) * k
    if with_addend:
        exp = exp + obj(d) * (addend_k or 1)
    assert np.array_equal(obj(out), exp % q), (logN, ept, mod, fill, with_mix, with_addend, addend_k)
    # the existing MODE 3 epilogue fed the separately computed product
    ab = np.array([int(v) for v in obj(a) * obj(b) % q], dtype=np.uint64)
    assert lib.emu_ntt_sub_scale_mul(*args(ab, None, out3)) == 0
    assert np.array_equal(out, out3)


def inverse_case(env, logN, ept, mod, fill, scale):
    lib, _ = env
    h, o = context(env, logN)
    N, q = o.N, o.moduli[mod]
    rng = np.random.default_rng(logN * 1000 + ept * 10 + mod + len(fill) + 5)
    a, b = filled(rng, q, N, fill), filled(rng, q, N, fill)
    out, out0 = np.empty(N, dtype=np.uint64), np.empty(N, dtype=np.uint64)
    assert lib.emu_intt_mul(h, ept, mod, p(a), p(b), p(out), scale or 0, 1 if scale else 0) == 0
    ab = np.array([int(v) for v in obj(a) * obj(b) % q], dtype=np.uint64)
    exp = obj(o.ntt([mod], ab[None, :], inverse=True)[0]) * (scale or 1) % q
    assert np.array_equal(obj(out), exp), (logN, ept, mod, fill, scale)
    assert lib.emu_intt_mul(h, ept, mod, p(ab), None, p(out0), scale or 0, 1 if scale else 0) == 0   # the existing inverse passes on the product
    assert np.array_equal(out, out0)


GEOMETRIES = [(13, 16), (15, 16), (15, 8), (16, 8)]   # (logN, coefficients per thread): the smallest ring, both geometries where both exist, both COL lengths of the small one


@pytest.mark.parametrize("logN,ept", GEOMETRIES)
def test_forward_product_minuend(env, logN, ept):
    """uniform operands on every modulus; with and without the mix prologue, the addend and its constant"""
    for mod in range(L + K):
        forward_case(env, logN, ept, mod, "uniform", with_mix=mod % 2 == 0, with_addend=mod != 1, addend_k=12345 if mod == 2 else 0)
    forward_case(env, logN, ept, 0, "uniform", with_mix=True, with_addend=True, addend_k=777)
    forward_case(env, logN, ept, L, "uniform", with_mix=False, with_addend=False, addend_k=0)


@pytest.mark.parametrize("fill", ["q-1", "zero"])
def test_forward_worst_case_operands(env, fill):
    """every operand q - 1: the product's operands are the largest a stored limb holds; and all zeros"""
    for logN, ept in ((13, 16), (15, 8)):
        forward_case(env, logN, ept, 0, fill, with_mix=True, with_addend=True, addend_k=3)
        forward_case(env, logN, ept, L + K - 1, fill, with_mix=False, with_addend=False, addend_k=0)


@pytest.mark.parametrize("logN,ept", GEOMETRIES)
def test_inverse_product_input(env, logN, ept):
    for mod in range(L + K):
        inverse_case(env, logN, ept, mod, "uniform", scale=98765 if mod % 2 else None)


@pytest.mark.parametrize("fill", ["q-1", "zero"])
def test_inverse_worst_case_operands(env, fill):
    for logN, ept in ((13, 16), (15, 8)):
        inverse_case(env, logN, ept, 0, fill, scale=None)
        inverse_case(env, logN, ept, L, fill, scale=5)


def test_product_step_range_and_the_epilogue_at_its_upper_end(env):
    """hm_epi_mul leaves [0, q): exact on the extremes of its operands, and va = q - 1 (x = q - 1, y = 1: the upper end of the stated range) goes through
    the MODE 8 epilogue with the transform's lazy value at both ends of ITS range [0, 2 HM_LAZY_Q q): (va + 2 HM_LAZY_Q q - x) stays below
    (1 + 2 HM_LAZY_Q) q, inside the constant product's operand range, and the result is exact"""
    lib, _ = env
    h, o = context(env, 13)
    lazy = lib.emu_lazy_q()
    for mod in range(L + K):
        q = o.moduli[mod]
        for x, y in ((q - 1, q - 1), (q - 1, 1), (1, q - 1), (0, q - 1), (q - 1, 2), ((q + 1) // 2, 2), (q // 2, q // 2), (12345678901234567 % q, q - 2)):
            got = lib.emu_epi_mul(h, mod, x, y)
            assert got == x * y % q and got < q, (mod, x, y)
        va = lib.emu_epi_mul(h, mod, q - 1, 1)
        assert va == q - 1
        k, ak, vd = 0x123456789ABCDEF % q, q - 5, q - 1
        for xt in (0, 1, q - 1, q, 2 * lazy * q - 1):
            assert lib.emu_epilogue8(h, mod, xt, va, 0, 0, k, 0) == (va - xt) * k % q, (mod, xt)
            assert lib.emu_epilogue8(h, mod, xt, va, vd, 1, k, ak) == ((va - xt) * k + vd * ak) % q, (mod, xt)
            assert lib.emu_epilogue8(h, mod, xt, va, vd, 1, k, 0) == ((va - xt) * k + vd) % q, (mod, xt)


def test_stand_alone_program_under_the_sanitizers(tmp_path):
    """tests/emu/hm_emu_rescale_main.cpp with its own main, compiled with the sanitizers and run as a process of its own (nothing is loaded into
    Python): every buffer is sized exactly"""
    exe = tmp_path / "hm_emu_rescale_main"
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall", "-Wno-unknown-pragmas",
                           "-o", str(exe), os.path.join(HERE, "emu", "hm_emu_rescale_main.cpp")] + SOURCES)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "bad=0" in r.stdout, r.stdout + r.stderr
