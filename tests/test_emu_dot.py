"""The per-thread core of hm_tensor_dot (homulator_amd/csrc/hm_rec_core.h: hm_tensor_dot_thread) on the CPU against Python integers, no GPU:
tests/emu/hm_emu_dot.cpp compiles the device header with g++, once per arithmetic back-end (HM_GENERIC 0 and 1, as tests/emu/Makefile defines
them), and runs every thread of the first and the last workgroup of every record.  T = 16 with every operand q - 1 puts 32 (q - 1)^2 into d1's
128-bit accumulator: the largest value the wide reduction ever sees."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest
import sympy

from oracle.homoracle import Oracle, chain_below

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
LOGN = 13
N = 1 << LOGN
CHUNKS = [0, N // 512 - 1]


@pytest.fixture(scope="module", params=[0, 1], ids=["mont32-build", "generic-build"])
def emu(request, tmp_path_factory):
    so = tmp_path_factory.mktemp("emu_dot") / f"libhm_emu_dot_{request.param}.so"
    subprocess.check_call(["g++"] + (["-DHM_GENERIC=1"] if request.param else []) +
                          ["-O2", "-std=c++17", "-fPIC", "-shared", "-Wall", "-Wno-unknown-pragmas", "-o", str(so),
                           os.path.join(HERE, "emu", "hm_emu_dot.cpp"), os.path.join(ROOT, "homulator_amd", "csrc", "hm_params.cpp")])
    lib = C.CDLL(str(so))
    assert lib.emu_dot_generic() == request.param
    lib.emu_tensor_dot.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32] + [C.c_void_p] * 15 + [C.c_uint32, C.c_uint32, C.c_void_p, C.c_uint32]
    return lib


@pytest.fixture(scope="module")
def moduli():
    """the largest and the smallest modulus of the default chain (45 + 15 primes h 2^32 + 1) and of the 60-bit survey chain, and the largest
    31-bit prime = 1 mod 2N"""
    default = Oracle(LOGN, 45, 15).moduli
    survey = chain_below(LOGN, 60, 60)
    q31 = ((1 << 31) - 1) // (2 * N) * (2 * N) + 1
    while not sympy.isprime(q31):
        q31 -= 2 * N
    assert default[0] == max(default) and default[-1] == min(default) and survey[0] == max(survey) and survey[-1] == min(survey)
    assert (1 << 30) < q31 < (1 << 31)
    return [default[0], default[-1], survey[0], survey[-1], q31]


def p(a):
    return a.ctypes.data_as(C.c_void_p)


@pytest.mark.parametrize("fill", ["q-1", "zero", "random"])
@pytest.mark.parametrize("T", [1, 2, 3, 4, 16])
def test_core_against_python_integers(emu, moduli, T, fill):
    """one record per modulus, every limb list a random permutation of its buffer.  The four ways out of the term loop (hm_term_rounds): T = 1 no
    round and no tail, 2 the tail alone, 3 one round and no tail, 4 one round and the tail; 16 the largest sum"""
    n = len(moduli)
    rng = np.random.default_rng(100 * T + len(fill))
    lists = [rng.permutation(n * T).astype(np.uint32) for _ in range(4)] + [rng.permutation(n).astype(np.uint32) for _ in range(3)]
    mods = np.arange(n, dtype=np.uint32)
    ins = [np.zeros((n * T, N), dtype=np.uint64) for _ in range(4)]
    for buf, ls in zip(ins, lists):
        for i in range(n):
            q = moduli[i]
            for t in range(T):
                buf[ls[i * T + t]] = q - 1 if fill == "q-1" else 0 if fill == "zero" else rng.integers(0, q, N, dtype=np.uint64)
    GUARD = 0x5A5A5A5A5A5A5A5A
    outs = [np.full((n, N), GUARD, dtype=np.uint64) for _ in range(3)]
    chunks = np.array(CHUNKS, dtype=np.uint32)
    ml = np.array(moduli, dtype=np.uint64)
    assert emu.emu_tensor_dot(p(ml), n, LOGN, p(ins[0]), p(lists[0]), p(ins[1]), p(lists[1]), p(ins[2]), p(lists[2]), p(ins[3]), p(lists[3]),
                              p(outs[0]), p(lists[4]), p(outs[1]), p(lists[5]), p(outs[2]), p(lists[6]), p(mods), n, T, p(chunks), len(chunks)) == 0
    cols = np.concatenate([np.arange(c * 512, (c + 1) * 512) for c in CHUNKS])
    rest = np.setdiff1d(np.arange(N), cols)
    for i, q in enumerate(moduli):
        a, b, c, d = ([[int(x) for x in buf[ls[i * T + t]][cols]] for t in range(T)] for buf, ls in zip(ins, lists))
        exp = [[sum(a[t][x] * b[t][x] for t in range(T)) % q for x in range(len(cols))],
               [sum(a[t][x] * d[t][x] + c[t][x] * b[t][x] for t in range(T)) % q for x in range(len(cols))],
               [sum(c[t][x] * d[t][x] for t in range(T)) % q for x in range(len(cols))]]
        for k in range(3):
            got = outs[k][lists[4 + k][i]]
            assert [int(x) for x in got[cols]] == exp[k], (T, fill, q, k)
            assert np.all(got[rest] == GUARD)
    if fill == "q-1" and T == 16:   # the accumulator bound the kernel's comment states: 2T products below 2^120
        assert 32 * (max(moduli) - 1) ** 2 < 1 << 125
