"""tests/exchange_ref.py checked on its own, without a GPU: its row rule against the library's host-only hm_slice_rows, the partition
property of both slice domains, and forward followed by reverse."""
import numpy as np
import pytest

import exchange_ref as ref

# (world, N, owners): the reference's limb % world rule, one owner, a middle rank that owns nothing, n = 1, n < world
CASES = [
    (1, 1 << 10, [0, 0, 0]),
    (2, 1 << 10, [i % 2 for i in range(5)]),
    (4, 1 << 12, [i % 4 for i in range(10)]),
    (4, 1 << 12, [2] * 5),
    (4, 1 << 12, [0, 3, 0, 3, 3, 1]),
    (16, 1 << 13, [7]),
    (16, 1 << 13, [3, 9, 15]),
    (8, 1 << 11, [(5 * i + 1) % 8 for i in range(19)]),
]


def pools(world, N, limbs, owners, pool, salt):
    """word k of pool limb l on rank r names (r, l, k)"""
    k = np.arange(N, dtype=np.uint64)
    return [np.stack([(np.uint64(salt) << np.uint64(56)) | (np.uint64(r) << np.uint64(48)) | (np.uint64(l) << np.uint64(32)) | k for l in range(pool)])
            for r in range(world)]


def shuffled_limbs(n, pool, seed):
    return [int(x) for x in np.random.default_rng(seed).permutation(pool)[:n]]


@pytest.mark.parametrize("world,N,owners", CASES)
def test_rows_equal_the_librarys(world, N, owners):
    import ctypes as C
    from homulator_amd import hip
    lib = hip.load()   # host-only entry point: no context, no GPU
    lib.hm_slice_rows.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p]
    o = np.asarray(owners, dtype=np.uint32)
    rows = np.empty_like(o)
    assert lib.hm_slice_rows(o.ctypes.data, len(o), world, rows.ctypes.data) == 0
    assert rows.tolist() == ref.slice_rows(owners, world)
    assert sorted(rows.tolist()) == list(range(len(owners)))


@pytest.mark.parametrize("world,N,owners", CASES)
def test_every_coefficient_is_in_exactly_one_ranks_slice(world, N, owners):
    n, pool = len(owners), len(owners) + 3
    limbs = shuffled_limbs(n, pool, 5)
    bufs = pools(world, N, limbs, owners, pool, 1)
    rows = ref.slice_rows(owners, world)
    want = sorted(int(w) for l, o in zip(limbs, owners) for w in bufs[o][l])   # every word is unique: a multiset comparison is a bijection
    sl = ref.limbs_to_slices(world, N, limbs, owners, bufs)
    assert sorted(int(w) for s in sl for w in s.ravel()) == want
    for i, (l, o) in enumerate(zip(limbs, owners)):    # ... and in coefficient order, rank after rank
        assert np.array_equal(np.concatenate([sl[r][rows[i]] for r in range(world)]), bufs[o][l])
    if ref.ROW % world == 0:
        cs = ref.limbs_to_colslices(world, N, limbs, owners, bufs)
        assert np.array_equal(sum(m.astype(int) for _, m in cs), np.ones(N, dtype=int))   # the column blocks partition a limb-poly
        assert sorted(int(w) for v, m in cs for w in v[:, m].ravel()) == want
        for r, (v, m) in enumerate(cs):
            assert not v[:, ~m].any()                  # nothing outside a rank's own columns
            x2 = np.nonzero(m)[0] % ref.ROW
            assert x2.min() == r * (ref.ROW // world) and x2.max() == (r + 1) * (ref.ROW // world) - 1


@pytest.mark.parametrize("world,N,owners", CASES)
def test_forward_then_reverse_is_the_identity(world, N, owners):
    n, pool = len(owners), len(owners) + 2
    limbs = shuffled_limbs(n, pool, 9)
    bufs = pools(world, N, limbs, owners, pool, 2)
    blank = [np.full_like(b, 0xAA) for b in bufs]
    back = ref.slices_to_limbs(world, N, limbs, owners, ref.limbs_to_slices(world, N, limbs, owners, bufs), blank)
    listed = {(o, l) for l, o in zip(limbs, owners)}
    for r in range(world):
        for l in range(pool):
            assert np.array_equal(back[r][l], bufs[r][l] if (r, l) in listed else blank[r][l]), (r, l)
    if ref.ROW % world == 0:
        cs = [v for v, _ in ref.limbs_to_colslices(world, N, limbs, owners, bufs)]
        back = ref.colslices_to_limbs(world, N, limbs, owners, cs, blank)
        for r in range(world):
            for l in range(pool):
                assert np.array_equal(back[r][l], bufs[r][l] if (r, l) in listed else blank[r][l]), (r, l)
    rep = ref.replicate_limbs(world, N, limbs, owners, bufs)
    for r in range(world):
        for l in range(pool):
            src = [o for ll, o in zip(limbs, owners) if ll == l]
            assert np.array_equal(rep[r][l], bufs[src[0]][l] if src else bufs[r][l])
