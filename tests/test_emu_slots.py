"""The slot transform (homulator_amd/csrc/hm_slot_core.h: the per-thread code of k_slot_fft, the kernel of hm_encode / hm_decode) on the CPU, no GPU:
tests/emu/hm_emu_slots.cpp compiles the header with g++ (contraction off: every fused operation of the header is an explicit fma) and runs every
thread of every workgroup of both launches, phase by phase.  Checked against tests/slots_ref.py, the definition in longdouble.

Encode: |c_emu - Delta m_exact| <= 1/2 + 8 B.  B = 0.0046049 is the largest |c_emu - Delta m_exact| - 1/2 measured over the inputs of this file
(every fill at Delta = 2^30, 2^40, 2^50 and N = 2^13, the uniform fill at Delta = 2^50 and N = 2^16, 2^17; the largest is the uniform fill at
Delta = 2^50 and N = 2^13, whose coefficients reach 2^45, where a double resolves 2^-8; 2^16: 0.0023, 2^17: 0.0011; every other fill and scale
is below 5e-5); the factor 8 covers inputs other than the seeded ones, and 8 B = 0.0368 is far from the 1/4 at which the transform, not the
margin, would be wrong.  Decode: F = 7.45e-16 is the largest |z_emu - z_exact| measured the same way over the same inputs (slots of modulus at
most 1; the uniform fill at N = 2^17; 5.8e-16 at 2^13), on the exactly rounded coefficients; the test asserts 8 F.  Each test prints its
figure before it asserts.  tests/test_gpu_slots.py takes both constants from here."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import slots_ref as R
from oracle.homoracle import Oracle, chain_below

HERE = os.path.dirname(os.path.abspath(__file__))
SOURCE = os.path.join(HERE, "emu", "hm_emu_slots.cpp")
u32, u64, vp = C.c_uint32, C.c_uint64, C.c_void_p
B_MEASURED = 0.0046049
F_MEASURED = 7.45e-16
FILLS = ["uniform", "slot0", "slot1", "slot_last", "ones", "zero"]
SCALES = [2.0 ** 30, 2.0 ** 40, 2.0 ** 50]
_lib = None


def emu():
    """the emulator, built once per process into a temporary directory (tests/test_gpu_slots.py uses it too)"""
    global _lib
    if _lib is None:
        import tempfile
        so = os.path.join(tempfile.mkdtemp(prefix="emu_slots_"), "libhm_emu_slots.so")
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-Wall", "-Wno-unknown-pragmas", "-ffp-contract=off", "-o", so, SOURCE])
        lib = C.CDLL(so)
        lib.emu_slots_encode.argtypes = [u32, vp, u32, C.c_double, u64, vp, vp]
        lib.emu_slots_decode.argtypes = [u32, vp, u32, C.c_double, u64, vp]
        _lib = lib
    return _lib


def emu_encode(logN, z, scale, q):
    """(coefficients [n_vec][N] uint64 modulo q, the overflow flag)"""
    z = np.ascontiguousarray(z, dtype=np.complex128).reshape(-1, 1 << (logN - 1))
    coef = np.empty((z.shape[0], 1 << logN), dtype=np.uint64)
    ovf = u32(0)
    assert emu().emu_slots_encode(logN, z.ctypes.data_as(vp), z.shape[0], float(scale), q, coef.ctypes.data_as(vp), C.byref(ovf)) == 0
    return coef, ovf.value


def emu_decode(logN, coef, scale, q):
    coef = np.ascontiguousarray(coef, dtype=np.uint64).reshape(-1, 1 << logN)
    z = np.empty((coef.shape[0], 1 << (logN - 1)), dtype=np.complex128)
    assert emu().emu_slots_decode(logN, coef.ctypes.data_as(vp), coef.shape[0], float(scale), q, z.ctypes.data_as(vp)) == 0
    return z


def fill(logN, name, seed=1):
    n = 1 << (logN - 1)
    z = np.zeros(n, dtype=np.complex128)
    if name == "uniform":     # |z_j| <= 1
        rng = np.random.default_rng(seed + logN)
        z = np.sqrt(rng.uniform(0, 1, n)) * np.exp(2j * np.pi * rng.uniform(0, 1, n))
    elif name == "ones":
        z[:] = 1
    elif name != "zero":
        z[{"slot0": 0, "slot1": 1, "slot_last": n - 1}[name]] = 0.6 - 0.8j
    return z


Q = Oracle(13, 3, 1).moduli[0]   # a 60-bit prime: every coefficient of this file fits half of it
_exact = {}


def exact(logN, name):
    """m_exact of a fill, longdouble, computed once: the definition at N = 2^13, the longdouble transform above it"""
    if (logN, name) not in _exact:
        _exact[(logN, name)] = (R.exact_coeffs if logN == 13 else R.fft_coeffs)(fill(logN, name), logN)
    return _exact[(logN, name)]


def encode_error(logN, name, scale):
    """max |c_emu - Delta m_exact| - 1/2"""
    coef, ovf = emu_encode(logN, fill(logN, name), scale, Q)
    assert ovf == 0
    c = np.array([R.LD(int(v)) for v in R.centre(coef[0], Q)], dtype=R.LD)
    return float(np.abs(c - exact(logN, name) * R.LD(scale)).max()) - 0.5


def decode_error(logN, name, scale):
    """max |z_emu - z_exact| on the exactly rounded coefficients"""
    c = R.round_exact(exact(logN, name) * R.LD(scale))
    got = emu_decode(logN, R.residues(c, Q), scale, Q)[0]
    want = R.decode_int(c, logN, scale, R.exact_slots if logN == 13 else R.fft_slots)
    return float(np.abs(got - want).max())


CASES = [(13, f, s) for f in FILLS for s in SCALES] + [(14, "uniform", SCALES[1]), (14, "uniform", SCALES[2]), (16, "uniform", SCALES[2]),
                                                      (17, "uniform", SCALES[2])]
IDS = [f"N2^{l}-{f}-scale2^{int(np.log2(s))}" for l, f, s in CASES]


@pytest.mark.parametrize("logN,name,scale", CASES, ids=IDS)
def test_encode_is_the_exact_rounding_within_half_plus_the_transform_error(logN, name, scale):
    err = encode_error(logN, name, scale)
    print(f"encode {logN} {name} {scale:g}: max |c - Delta m| - 1/2 = {err:.6g}")
    assert 8 * B_MEASURED < 0.25
    assert err <= 8 * B_MEASURED


@pytest.mark.parametrize("logN,name,scale", CASES, ids=IDS)
def test_decode_is_the_exact_evaluation_within_the_transform_error(logN, name, scale):
    err = decode_error(logN, name, scale)
    print(f"decode {logN} {name} {scale:g}: max |z - z_exact| = {err:.6g}")
    assert err <= 8 * F_MEASURED


def test_zero_encodes_to_zero_and_decodes_to_zero():
    coef, ovf = emu_encode(13, fill(13, "zero"), 2.0 ** 40, Q)
    assert ovf == 0 and not coef.any()
    assert not emu_decode(13, coef, 2.0 ** 40, Q).any()


def test_several_vectors_are_independent():
    zs = np.stack([fill(13, "uniform", seed=s) for s in (1, 2, 3)])
    both, _ = emu_encode(13, zs, 2.0 ** 40, Q)
    for v in range(3):
        assert np.array_equal(both[v], emu_encode(13, zs[v], 2.0 ** 40, Q)[0][0])
    back = emu_decode(13, both, 2.0 ** 40, Q)
    for v in range(3):
        assert np.array_equal(back[v], emu_decode(13, both[v], 2.0 ** 40, Q)[0])


@pytest.mark.parametrize("sign", [1, -1])
def test_the_overflow_flag_on_both_sides_of_half_the_modulus(sign):
    """the constant slot vector v encodes to the constant polynomial rint(Delta v), exactly (sums of equal doubles, differences that are 0): with a
    36-bit prime, Delta = 2^20, Delta v = (q - 1) / 2 is kept and (q - 1) / 2 + 1 is refused: stored as 0, never wrapped"""
    q = chain_below(13, 36, 1)[0]
    half, scale = (q - 1) // 2, 2.0 ** 20
    n = 1 << 12
    coef, ovf = emu_encode(13, np.full(n, sign * half / scale), scale, q)
    assert ovf == 0 and int(coef[0, 0]) == (sign * half) % q and not coef[0, 1:].any()
    coef, ovf = emu_encode(13, np.full(n, sign * (half + 1) / scale), scale, q)
    assert ovf == 1 and not coef.any()
    # the flag is the vector's, a NaN or an infinity raises it too
    z = fill(13, "uniform")
    z[5] = np.inf
    assert emu_encode(13, z, scale, q)[1] == 1


@pytest.mark.parametrize("logN,logscale", [(13, 30), (14, 40), (16, 50), (17, 40)])
def test_stand_alone_program_under_the_sanitizers(tmp_path, logN, logscale):
    """tests/emu/hm_emu_slots_main.cpp with its own main, compiled with the sanitizers and run as a process of its own (nothing is loaded into
    Python): every fill, two vectors, every buffer sized exactly; both pass splits (log n even and odd)"""
    exe = tmp_path / "hm_emu_slots_main"
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall", "-Wno-unknown-pragmas",
                           "-ffp-contract=off", "-o", str(exe), os.path.join(HERE, "emu", "hm_emu_slots_main.cpp"), SOURCE])
    r = subprocess.run([str(exe), str(logN), str(logscale), str(Q)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "bad=0" in r.stdout, r.stdout + r.stderr
