"""The identity forms of the weighted sums' per-thread cores (homulator_amd/csrc/hm_ip_core.h: hm_ip_lintrans_multi_thread<TERMS, TILE, true> and, for
one sum, hm_ip_lintrans_thread<TERMS, true>: the kernels of hm_inner_product_lintrans_id) on the CPU against Python integers, no GPU:
tests/emu/hm_emu_identity.cpp compiles the device header with g++, once per arithmetic back-end (HM_GENERIC 0 and 1), and runs every thread of
the first and the last workgroup of every record and tile.  The same buffers go through the core WITHOUT the identity step followed by the
element-wise MAC_ADD / MUL, which is what the entry point promises to equal: the two must agree word for word.  n_rot = 15 with every operand
q - 1 puts 16 (q - 1)^2 into the addend accumulator: the bound the wide reduction is stated for."""
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
NO_LIMB = 0xFFFFFFFF
TILE = int(re.search(r"#define HM_IP_LINTRANS_MULTI_TILE (\d+)", open(os.path.join(ROOT, "include", "homulator_hip.h")).read()).group(1))
MAX_ROT = int(re.search(r"#define HM_IP_LINTRANS_ID_MAX_ROT (\d+)", open(os.path.join(ROOT, "include", "homulator_hip.h")).read()).group(1))


@pytest.fixture(scope="module", params=[0, 1], ids=["mont32-build", "generic-build"])
def emu(request, tmp_path_factory):
    so = tmp_path_factory.mktemp("emu_identity") / f"libhm_emu_identity_{request.param}.so"
    subprocess.check_call(["g++"] + (["-DHM_GENERIC=1"] if request.param else []) +
                          ["-O2", "-std=c++17", "-fPIC", "-shared", "-Wall", "-Wno-unknown-pragmas", "-o", str(so),
                           os.path.join(HERE, "emu", "hm_emu_identity.cpp"), os.path.join(ROOT, "homulator_amd", "csrc", "hm_params.cpp")])
    lib = C.CDLL(str(so))
    assert lib.emu_identity_generic() == request.param
    lib.emu_ip_rotsum_init.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32] + [C.c_void_p] * 16 + [C.c_uint32] * 3 + [C.c_void_p, C.c_void_p, C.c_uint32]
    lib.emu_ip_lintrans_id.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32] + [C.c_void_p] * 21 + [C.c_uint32] * 5 + [C.c_void_p, C.c_void_p, C.c_uint32]
    return lib


@pytest.fixture(scope="module")
def moduli():
    """the largest and the smallest modulus of the default chain and of the 60-bit survey chain, and the largest 31-bit prime = 1 mod 2N"""
    default = Oracle(LOGN, 45, 15).moduli
    survey = chain_below(LOGN, 60, 60)
    q31 = ((1 << 31) - 1) // (2 * N) * (2 * N) + 1
    while not sympy.isprime(q31):
        q31 -= 2 * N
    assert default[0] == max(default) and default[-1] == min(default) and survey[0] == max(survey) and survey[-1] == min(survey)
    return [default[0], default[-1], survey[0], survey[-1], q31]


def p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def brev(i, bits):
    return int(format(i, f"0{bits}b")[::-1], 2)


_src = {}


def SRC(g):
    """the stored (bit-reversed evaluation order) index sigma_g reads output i from — hm_automorph's index map, from its definition"""
    if g not in _src:
        _src[g] = np.array([brev(((g * (2 * brev(i, LOGN) + 1)) % (2 * N) - 1) >> 1, LOGN) for i in range(N)])
    return _src[g]


def elements(R):
    """3, 2N - 1, 2N - 3, then 5^r: both the in-order and the swapped source pair occur (checked below)"""
    return ([3, 2 * N - 1, 2 * N - 3] + [pow(5, r, 2 * N) for r in range(3, 16)])[:R]


def test_the_header_bounds_the_rotations_at_15():
    assert MAX_ROT == 15


def test_elements_cover_the_in_order_and_the_swapped_pair():
    assert {int(SRC(g)[0] & 1) for g in elements(MAX_ROT)} == {0, 1} and {int(SRC(g)[0] & 1) for g in elements(3)} == {0, 1}


def run(emu, moduli, T, R, G, fill, addend_on, tile=TILE):
    n = len(moduli)
    rng = np.random.default_rng(10000 * G + 100 * R + 10 * T + len(fill) + tile)
    gs = elements(R)
    has = [addend_on == "all" or i % 2 == 0 for i in range(n)]
    na = sum(has)
    xl = rng.permutation(n * T).astype(np.uint32)                # [n][T]
    yl = rng.permutation(R * n * 2 * T).astype(np.uint32)        # [r][n][2][T]
    ppool = rng.permutation(G * R * n + G * n).astype(np.uint32)
    pl, idl = ppool[:G * R * n].copy(), ppool[G * R * n:].copy()  # [m][r][n] and the identity plaintexts [m][n], limbs of one buffer
    ol = rng.permutation(G * n * 2).astype(np.uint32)            # [m][n][2]
    al, a1l = rng.permutation(n).astype(np.uint32), rng.permutation(n).astype(np.uint32)   # [n]
    aol, a1ol = rng.permutation(G * n).astype(np.uint32), rng.permutation(G * n).astype(np.uint32)   # [m][n]
    for i in range(n):
        if not has[i]:
            al[i] = a1l[i] = NO_LIMB
            for m in range(G):   # ignored there: anything may stand in the lists
                idl[m * n + i] = aol[m * n + i] = a1ol[m * n + i] = NO_LIMB

    def filled(rows, mod_of_row):
        buf = np.zeros((rows, N), dtype=np.uint64)
        for r in range(rows):
            q = mod_of_row(r)
            if q is not None:
                buf[r] = q - 1 if fill == "q-1" else 0 if fill == "zero" else rng.integers(0, q, N, dtype=np.uint64)
        return buf
    mod_x, mod_y, mod_p, mod_a, mod_a1 = {}, {}, {}, {}, {}
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
                mod_p[idl[m * n + i]] = moduli[i]
        if has[i]:
            mod_a[al[i]], mod_a1[a1l[i]] = moduli[i], moduli[i]
    X, Y, P = filled(n * T, mod_x.get), filled(R * n * 2 * T, mod_y.get), filled(G * R * n + G * n, mod_p.get)
    A, A1 = filled(n, mod_a.get), filled(n, mod_a1.get)
    out, out1 = (np.full((G * n * 2, N), GUARD, dtype=np.uint64) for _ in range(2))
    aout, aout1, wout, wout1 = (np.full((G * n, N), GUARD, dtype=np.uint64) for _ in range(4))
    ml, mods, chunks, gl = np.array(moduli, dtype=np.uint64), np.arange(n, dtype=np.uint32), np.array(CHUNKS, dtype=np.uint32), np.array(gs, dtype=np.uint32)
    assert emu.emu_ip_lintrans_id(p(ml), n, LOGN, p(X), p(xl), p(Y), p(yl), p(P), p(pl), p(idl), p(A), p(al), p(A1), p(a1l), p(out), p(out1), p(ol),
                                  p(aout), p(aout1), p(aol), p(wout), p(wout1), p(a1ol), p(mods), n, T, R, G, tile, p(gl), p(chunks), len(chunks)) == 0
    what = (T, R, G, fill, addend_on, tile)
    assert np.array_equal(out, out1) and np.array_equal(aout, aout1) and np.array_equal(wout, wout1), (what, "differs from the core without the identity step + MAC_ADD / MUL")
    cols = np.concatenate([np.arange(c * 512, (c + 1) * 512) for c in CHUNKS])
    rest = np.setdiff1d(np.arange(N), cols)
    written_a, written_w = set(), set()
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
            for k in range(2):   # the sums over the rotations take no identity term
                exp = [sum(w[r][c] * t[r][k][c] for r in range(R)) % q for c in range(len(cols))]
                got = out[ol[(m * n + i) * 2 + k]]
                assert [int(v) for v in got[cols]] == exp, (what, q, m, k)
                assert np.all(got[rest] == GUARD)
            if has[i]:
                w0 = [int(v) for v in P[idl[m * n + i]][cols]]
                c0r = [[int(v) for v in A[al[i]][SRC(gs[r])[cols]]] for r in range(R)]
                c0, c1 = [int(v) for v in A[al[i]][cols]], [int(v) for v in A1[a1l[i]][cols]]          # unrotated: read where they are stored
                expU = [(w0[c] * c0[c] + sum(w[r][c] * c0r[r][c] for r in range(R))) % q for c in range(len(cols))]
                expW = [w0[c] * c1[c] % q for c in range(len(cols))]
                gotU, gotW = aout[aol[m * n + i]], wout[a1ol[m * n + i]]
                assert [int(v) for v in gotU[cols]] == expU, (what, q, m, "addend")
                assert [int(v) for v in gotW[cols]] == expW, (what, q, m, "second addend")
                assert np.all(gotU[rest] == GUARD) and np.all(gotW[rest] == GUARD)
                written_a.add(int(aol[m * n + i]))
                written_w.add(int(a1ol[m * n + i]))
    for row in range(G * n):   # entries without an addend write neither addend output
        assert row in written_a or np.all(aout[row] == GUARD)
        assert row in written_w or np.all(wout[row] == GUARD)


@pytest.mark.parametrize("fill", ["q-1", "zero", "random"])
@pytest.mark.parametrize("T", [1, 4])
@pytest.mark.parametrize("R", [1, 15])
def test_core_against_python_integers(emu, moduli, T, R, fill):
    """one record per modulus, every limb list a random permutation of its buffer, every entry with both addend sources; outputs 1, TILE,
    TILE + 1 and 16: the tile boundary is where it can go wrong"""
    for G in (1, TILE, TILE + 1, 16):
        run(emu, moduli, T, R, G, fill, "all")
    run(emu, moduli, T, R, 1, fill, "all", tile=1)   # one sum: the single-sum core with the identity step (hm_ip_lintrans_thread<TERMS, true>)
    if fill == "q-1" and R == 15:   # the accumulator bound the kernel's comment states: 16 products
        assert (MAX_ROT + 1) * (max(moduli) - 1) ** 2 < 1 << 124


@pytest.mark.parametrize("tile", [2, 4])
def test_both_tile_sizes_at_their_boundaries(emu, moduli, tile):
    for G in (tile - 1, tile, tile + 1, 2 * tile + 1):
        run(emu, moduli, 3, 3, G, "random", "all", tile=tile)


def test_entries_without_an_addend_take_no_identity_step(emu, moduli):
    run(emu, moduli, 2, 3, TILE + 1, "random", "some")
    run(emu, moduli, 2, 3, 1, "random", "some", tile=1)


def test_counts_out_of_range_are_refused(emu, moduli):
    z = np.zeros(8, dtype=np.uint64)
    l = np.zeros(8, dtype=np.uint32)
    ml = np.array(moduli, dtype=np.uint64)
    for T, R, G, tile in ((0, 1, 1, 4), (5, 1, 1, 4), (1, 0, 1, 4), (1, 16, 1, 4), (1, 1, 0, 4), (1, 1, 17, 4), (1, 1, 1, 3), (1, 1, 2, 1)):
        assert emu.emu_ip_lintrans_id(p(ml), len(moduli), LOGN, p(z), p(l), p(z), p(l), p(z), p(l), p(l), p(z), p(l), p(z), p(l), p(z), p(z), p(l),
                                      p(z), p(z), p(l), p(z), p(z), p(l), p(l), 0, T, R, G, tile, p(l), p(l), 0) == 2


def test_table_builder_and_core_as_a_stand_alone_program_under_asan_and_ubsan(tmp_path):
    """tests/emu/hm_emu_identity_main.cpp with its own main, compiled with the sanitizers and run as a process of its own (nothing is loaded
    into Python): exact-size tables and buffers, every count at which the tile loop takes another path"""
    exe = tmp_path / "hm_emu_identity_main"
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall", "-Wno-unknown-pragmas",
                           "-o", str(exe), os.path.join(HERE, "emu", "hm_emu_identity_main.cpp"), os.path.join(HERE, "emu", "hm_emu_identity.cpp"),
                           os.path.join(ROOT, "homulator_amd", "csrc", "hm_params.cpp")])
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0 and "bad=0" in r.stdout, (r.stdout[-2000:], r.stderr[-4000:])


# ---- the sum over ciphertexts with initial sums (hm_ip_rotsum_thread<TERMS, true>, the kernel of hm_inner_product_rotsum_init)
def run_init(emu, moduli, T, G, fill, addend_on):
    n = len(moduli)
    rng = np.random.default_rng(1000 * G + 10 * T + len(fill))
    gs = elements(G)
    has = [addend_on == "all" or i % 2 == 0 for i in range(n)]
    xl = rng.permutation(G * n * T).astype(np.uint32)            # [c][n][T]
    yl = rng.permutation(G * n * 2 * T).astype(np.uint32)        # [c][n][2][T]
    apool = rng.permutation(G * n + n).astype(np.uint32)
    al, ail = apool[:G * n].copy(), apool[G * n:].copy()         # addend sources [c][n] and the initial addend sums [n], limbs of one buffer
    il = rng.permutation(n * 2).astype(np.uint32)                # [n][2]
    ol, aol = rng.permutation(n * 2).astype(np.uint32), rng.permutation(n).astype(np.uint32)
    for i in range(n):
        if not has[i]:
            ail[i] = NO_LIMB
            for c in range(G):
                al[c * n + i] = NO_LIMB

    def filled(rows, mod_of_row):
        buf = np.zeros((rows, N), dtype=np.uint64)
        for r in range(rows):
            q = mod_of_row(r)
            if q is not None:
                buf[r] = q - 1 if fill == "q-1" else 0 if fill == "zero" else rng.integers(0, q, N, dtype=np.uint64)
        return buf
    mod_x, mod_y, mod_a, mod_i = {}, {}, {}, {}
    for i in range(n):
        for c in range(G):
            for j in range(T):
                mod_x[xl[(c * n + i) * T + j]] = moduli[i]
                for k in range(2):
                    mod_y[yl[((c * n + i) * 2 + k) * T + j]] = moduli[i]
            if has[i]:
                mod_a[al[c * n + i]] = moduli[i]
        if has[i]:
            mod_a[ail[i]] = moduli[i]
        for k in range(2):
            mod_i[il[i * 2 + k]] = moduli[i]
    X, Y, A, I = filled(G * n * T, mod_x.get), filled(G * n * 2 * T, mod_y.get), filled(G * n + n, mod_a.get), filled(n * 2, mod_i.get)
    out, out1 = (np.full((n * 2, N), GUARD, dtype=np.uint64) for _ in range(2))
    aout, aout1 = (np.full((n, N), GUARD, dtype=np.uint64) for _ in range(2))
    ml, mods, chunks, gl = np.array(moduli, dtype=np.uint64), np.arange(n, dtype=np.uint32), np.array(CHUNKS, dtype=np.uint32), np.array(gs, dtype=np.uint32)
    assert emu.emu_ip_rotsum_init(p(ml), n, LOGN, p(X), p(xl), p(Y), p(yl), p(A), p(al), p(I), p(il), p(ail), p(out), p(out1), p(ol), p(aout),
                                  p(aout1), p(aol), p(mods), n, T, G, p(gl), p(chunks), len(chunks)) == 0
    what = (T, G, fill, addend_on)
    assert np.array_equal(out, out1) and np.array_equal(aout, aout1), (what, "differs from the core without initial sums + ADD")
    cols = np.concatenate([np.arange(c * 512, (c + 1) * 512) for c in CHUNKS])
    rest = np.setdiff1d(np.arange(N), cols)
    for i, q in enumerate(moduli):
        for k in range(2):
            acc = [int(v) for v in I[il[i * 2 + k]][cols]]
            for c in range(G):
                src = SRC(gs[c])[cols]
                for j in range(T):
                    xs, ys = X[xl[(c * n + i) * T + j]][src], Y[yl[((c * n + i) * 2 + k) * T + j]][cols]
                    acc = [e + int(a) * int(b) for e, a, b in zip(acc, xs, ys)]
            got = out[ol[i * 2 + k]]
            assert [int(v) for v in got[cols]] == [e % q for e in acc], (what, q, k)
            assert np.all(got[rest] == GUARD)
        got = aout[aol[i]]
        if has[i]:
            acc = [int(v) for v in A[ail[i]][cols]]
            for c in range(G):
                acc = [e + int(a) for e, a in zip(acc, A[al[c * n + i]][SRC(gs[c])[cols]])]
            assert [int(v) for v in got[cols]] == [e % q for e in acc], (what, q, "addend")
            assert np.all(got[rest] == GUARD)
        else:
            assert np.all(got == GUARD)


@pytest.mark.parametrize("fill", ["q-1", "zero", "random"])
@pytest.mark.parametrize("T", [1, 4])
@pytest.mark.parametrize("G", [1, 15])
def test_rotsum_init_core_against_python_integers(emu, moduli, T, G, fill):
    run_init(emu, moduli, T, G, fill, "all")
    if fill == "q-1" and G == 15:   # the bounds the kernel's comments state: 60 products and a residue in 128 bits, 16 residues in 64
        assert 60 * (max(moduli) - 1) ** 2 + max(moduli) < 1 << 126 and 16 * (max(moduli) - 1) < 1 << 64


def test_rotsum_init_entries_without_addends(emu, moduli):
    run_init(emu, moduli, 2, 3, "random", "some")


def test_rotsum_init_counts_out_of_range_are_refused(emu, moduli):
    z = np.zeros(8, dtype=np.uint64)
    l = np.zeros(8, dtype=np.uint32)
    ml = np.array(moduli, dtype=np.uint64)
    for T, G in ((0, 1), (5, 1), (1, 0), (1, 16)):
        assert emu.emu_ip_rotsum_init(p(ml), len(moduli), LOGN, p(z), p(l), p(z), p(l), p(z), p(l), p(z), p(l), p(l), p(z), p(z), p(l), p(z), p(z),
                                      p(l), p(l), 0, T, G, p(l), p(l), 0) == 2
