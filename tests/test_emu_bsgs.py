"""The per-thread core of hm_inner_product_lintrans_multi (homulator_amd/csrc/hm_ip_core.h: hm_ip_lintrans_multi_thread) on the CPU against Python
integers, no GPU: tests/emu/hm_emu_bsgs.cpp compiles the device header with g++, once per arithmetic back-end (HM_GENERIC 0 and 1, as
tests/emu/Makefile defines them), and runs every thread of the first and the last workgroup of every record and tile, with both built tile sizes;
the same buffers go through the single-sum core hm_ip_lintrans_thread once per output, and the two must agree word for word.  n_rot = 16 with every
operand q - 1 puts 16 (q - 1)^2 into each 128-bit accumulator: the largest value the wide reduction ever sees."""
import ctypes as C
import os
import re
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
GUARD = 0x5A5A5A5A5A5A5A5A
TILE = int(re.search(r"#define HM_IP_LINTRANS_MULTI_TILE (\d+)", open(os.path.join(ROOT, "include", "homulator_hip.h")).read()).group(1))


@pytest.fixture(scope="module", params=[0, 1], ids=["mont32-build", "generic-build"])
def emu(request, tmp_path_factory):
    so = tmp_path_factory.mktemp("emu_bsgs") / f"libhm_emu_bsgs_{request.param}.so"
    subprocess.check_call(["g++"] + (["-DHM_GENERIC=1"] if request.param else []) +
                          ["-O2", "-std=c++17", "-fPIC", "-shared", "-Wall", "-Wno-unknown-pragmas", "-o", str(so),
                           os.path.join(HERE, "emu", "hm_emu_bsgs.cpp"), os.path.join(ROOT, "homulator_amd", "csrc", "hm_params.cpp")])
    lib = C.CDLL(str(so))
    assert lib.emu_bsgs_generic() == request.param and lib.emu_bsgs_default_tile() == TILE
    lib.emu_ip_lintrans_multi.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32] + [C.c_void_p] * 15 + [C.c_uint32] * 5 + [C.c_void_p, C.c_void_p, C.c_uint32]
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
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def brev(i, bits):
    return int(format(i, f"0{bits}b")[::-1], 2)


def auto_src():
    """src(g)[i]: the stored (bit-reversed evaluation order) index sigma_g reads output i from — hm_automorph's index map, from its definition"""
    cache = {}

    def of(g):
        if g not in cache:
            cache[g] = np.array([brev(((g * (2 * brev(i, LOGN) + 1)) % (2 * N) - 1) >> 1, LOGN) for i in range(N)])
        return cache[g]
    return of


SRC = auto_src()


def elements(R):
    """3, 2N - 1, 2N - 3, then 5^r: both the in-order and the swapped source pair occur (checked below)"""
    return ([3, 2 * N - 1, 2 * N - 3] + [pow(5, r, 2 * N) for r in range(3, 16)])[:R]


def test_the_python_binding_names_the_header_s_tile():
    from homulator_amd import hip
    assert hip.LINTRANS_MULTI_TILE == TILE


def test_elements_cover_the_in_order_and_the_swapped_pair():
    parity = {g: int(SRC(g)[0] & 1) for g in elements(16)}
    assert set(parity.values()) == {0, 1}, parity


def run(emu, moduli, T, R, G, fill, addend_on, tile=TILE):
    n = len(moduli)
    rng = np.random.default_rng(10000 * G + 100 * R + 10 * T + len(fill) + tile)
    gs = elements(R)
    xl = rng.permutation(n * T).astype(np.uint32)                # [n][T]
    yl = rng.permutation(R * n * 2 * T).astype(np.uint32)        # [r][n][2][T]
    pl = rng.permutation(G * R * n).astype(np.uint32)            # [m][r][n]
    ol = rng.permutation(G * n * 2).astype(np.uint32)            # [m][n][2]
    al = rng.permutation(n).astype(np.uint32)                    # [n]
    aol = rng.permutation(G * n).astype(np.uint32)               # [m][n]
    has = [addend_on == "all" or (addend_on == "some" and i % 2 == 0) for i in range(n)]
    for i in range(n):
        if not has[i]:
            al[i] = 0xFFFFFFFF

    def filled(rows, mod_of_row):
        buf = np.zeros((rows, N), dtype=np.uint64)
        for r in range(rows):
            q = mod_of_row(r)
            if q is not None:
                buf[r] = q - 1 if fill == "q-1" else 0 if fill == "zero" else rng.integers(0, q, N, dtype=np.uint64)
        return buf
    mod_x, mod_y, mod_p, mod_a = {}, {}, {}, {}
    for i in range(n):
        for j in range(T):
            mod_x[xl[i * T + j]] = moduli[i]
            for r in range(R):
                for k in range(2):
                    mod_y[yl[((r * n + i) * 2 + k) * T + j]] = moduli[i]
        for m in range(G):
            for r in range(R):
                mod_p[pl[(m * R + r) * n + i]] = moduli[i]
        if has[i]:
            mod_a[al[i]] = moduli[i]
    X, Y, P, A = filled(n * T, mod_x.get), filled(R * n * 2 * T, mod_y.get), filled(G * R * n, mod_p.get), filled(n, mod_a.get)
    out, out1 = (np.full((G * n * 2, N), GUARD, dtype=np.uint64) for _ in range(2))
    aout, aout1 = (np.full((G * n, N), GUARD, dtype=np.uint64) for _ in range(2))
    ml, mods, chunks, gl = np.array(moduli, dtype=np.uint64), np.arange(n, dtype=np.uint32), np.array(CHUNKS, dtype=np.uint32), np.array(gs, dtype=np.uint32)
    use_add = addend_on != "none"
    opt = lambda v: p(v) if use_add else None
    assert emu.emu_ip_lintrans_multi(p(ml), n, LOGN, p(X), p(xl), p(Y), p(yl), p(P), p(pl), opt(A), opt(al), p(out), p(out1), p(ol), opt(aout),
                                     opt(aout1), opt(aol), p(mods), n, T, R, G, tile, p(gl), p(chunks), len(chunks)) == 0
    what = (T, R, G, fill, addend_on, tile)
    assert np.array_equal(out, out1) and np.array_equal(aout, aout1), (what, "differs from hm_ip_lintrans_thread run n_out times")
    cols = np.concatenate([np.arange(c * 512, (c + 1) * 512) for c in CHUNKS])
    rest = np.setdiff1d(np.arange(N), cols)
    for i, q in enumerate(moduli):
        t = [[None, None] for _ in range(R)]                      # t[r][k]: the reduced key product of rotation r, once
        for r in range(R):
            src = SRC(gs[r])[cols]
            for k in range(2):
                acc = [0] * len(cols)
                for j in range(T):
                    xs, ys = X[xl[i * T + j]][src], Y[yl[((r * n + i) * 2 + k) * T + j]][cols]
                    acc = [e + int(a) * int(b) for e, a, b in zip(acc, xs, ys)]
                t[r][k] = [e % q for e in acc]
        for m in range(G):
            w = [[int(v) for v in P[pl[(m * R + r) * n + i]][cols]] for r in range(R)]
            for k in range(2):
                exp = [sum(w[r][c] * t[r][k][c] for r in range(R)) % q for c in range(len(cols))]
                got = out[ol[(m * n + i) * 2 + k]]
                assert [int(v) for v in got[cols]] == exp, (what, q, m, k)
                assert np.all(got[rest] == GUARD)
            got = aout[aol[m * n + i]]
            if has[i]:
                c0 = [[int(v) for v in A[al[i]][SRC(gs[r])[cols]]] for r in range(R)]
                exp = [sum(w[r][c] * c0[r][c] for r in range(R)) % q for c in range(len(cols))]
                assert [int(v) for v in got[cols]] == exp, (what, q, m, "addend")
                assert np.all(got[rest] == GUARD)
            else:
                assert np.all(got == GUARD)


@pytest.mark.parametrize("fill", ["q-1", "zero", "random"])
@pytest.mark.parametrize("T", [1, 4])
@pytest.mark.parametrize("R", [1, 2, 16])
def test_core_against_python_integers(emu, moduli, T, R, fill):
    """one record per modulus, every limb list a random permutation of its buffer, every entry with an addend source; outputs 1, TILE, TILE + 1
    and 16: the tile boundary is where it can go wrong"""
    for G in (1, TILE, TILE + 1, 16):
        run(emu, moduli, T, R, G, fill, "all")
    if fill == "q-1" and R == 16:   # the accumulator bound the kernel's comment states
        assert 16 * (max(moduli) - 1) ** 2 < 1 << 124


@pytest.mark.parametrize("tile", [2, 4])
def test_both_tile_sizes_at_their_boundaries(emu, moduli, tile):
    for G in (tile - 1, tile, tile + 1, 2 * tile + 1):
        run(emu, moduli, 3, 3, G, "random", "all", tile=tile)


@pytest.mark.parametrize("addend_on", ["none", "some"])
def test_addend_is_optional_per_entry(emu, moduli, addend_on):
    run(emu, moduli, 2, 3, TILE + 1, "random", addend_on)


def test_counts_out_of_range_are_refused(emu, moduli):
    z = np.zeros(8, dtype=np.uint64)
    l = np.zeros(8, dtype=np.uint32)
    ml = np.array(moduli, dtype=np.uint64)
    for T, R, G, tile in ((0, 1, 1, 4), (5, 1, 1, 4), (1, 0, 1, 4), (1, 17, 1, 4), (1, 1, 0, 4), (1, 1, 17, 4), (1, 1, 1, 3)):
        assert emu.emu_ip_lintrans_multi(p(ml), len(moduli), LOGN, p(z), p(l), p(z), p(l), p(z), p(l), None, None, p(z), p(z), p(l), None, None, None,
                                         p(l), 0, T, R, G, tile, p(l), p(l), 0) == 2


def test_table_builder_and_core_as_a_stand_alone_program_under_asan_and_ubsan(tmp_path):
    """tests/emu/hm_emu_bsgs_main.cpp with its own main, compiled with the sanitizers and run as a process of its own (nothing is loaded into
    Python): exact-size tables and buffers, every count at which the tile loop takes another path"""
    exe = tmp_path / "hm_emu_bsgs_main"
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall", "-Wno-unknown-pragmas",
                           "-o", str(exe), os.path.join(HERE, "emu", "hm_emu_bsgs_main.cpp"), os.path.join(HERE, "emu", "hm_emu_bsgs.cpp"),
                           os.path.join(ROOT, "homulator_amd", "csrc", "hm_params.cpp")])
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0 and "bad=0" in r.stdout, (r.stdout[-2000:], r.stderr[-4000:])
