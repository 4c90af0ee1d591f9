"""The five exchange calls of include/homulator_hip.h restated in plain numpy, from their documented contracts alone (no staging buffers,
no chunks, no peers: every function sees all ranks at once).

Arguments everywhere: world, N, the lists limbs / owners (one entry per limb-poly: owners[i] holds it at index limbs[i] of ITS pool) and the
ranks' buffers as a list of [pool][N] uint64 arrays (bufs[r] = rank r's pool).  Nothing is modified in place.

  slice_rows(owners, world)                       the row of limb i in every rank's slice array: grouped by owner, list order inside an owner
  limbs_to_slices(world, N, limbs, owners, bufs)  -> per rank [n][N / world]: row rows[i] = coefficients [rank * N / world, ...) of limb i
  limbs_to_colslices(...)                         -> per rank ([n][N] values, [N] bool mask): row rows[i] in the limb-poly layout, index
                                                     x1 * 256 + x2 valid (mask) for x2 in [rank * 256 / world, (rank + 1) * 256 / world)
  slices_to_limbs(world, N, limbs, owners, slices, bufs)     -> the ranks' pools afterwards: the owner of limb i holds the whole limb at limbs[i]
  colslices_to_limbs(world, N, limbs, owners, slices, bufs)  -> the same from column slices (slices[r]: [n][N], rank r's columns are read)
  replicate_limbs(world, N, limbs, owners, bufs)  -> the ranks' pools afterwards: every rank holds every limb of the list at limbs[i]
"""
import numpy as np

ROW = 256   # i = x1 * 256 + x2: the contiguous sub-transform length (HM_ROW_LOG = 8)


def slice_rows(owners, world):
    owners = [int(o) for o in owners]
    assert all(0 <= o < world for o in owners)
    order = sorted(range(len(owners)), key=lambda i: (owners[i], i))   # stable: list order inside an owner
    rows = [0] * len(owners)
    for row, i in enumerate(order):
        rows[i] = row
    return rows


def column_mask(world, N, rank):
    """the words of a limb-poly that belong to rank's column slice"""
    assert ROW % world == 0 and N % ROW == 0
    cw = ROW // world
    x2 = np.arange(N) % ROW
    return (x2 >= rank * cw) & (x2 < (rank + 1) * cw)


def limbs_to_slices(world, N, limbs, owners, bufs):
    assert N % world == 0
    ln, rows = N // world, slice_rows(owners, world)
    out = [np.zeros((len(limbs), ln), dtype=np.uint64) for _ in range(world)]
    for r in range(world):
        for i, (l, o) in enumerate(zip(limbs, owners)):
            out[r][rows[i]] = bufs[o][l, r * ln:(r + 1) * ln]
    return out


def limbs_to_colslices(world, N, limbs, owners, bufs):
    rows = slice_rows(owners, world)
    out = []
    for r in range(world):
        m = column_mask(world, N, r)
        v = np.zeros((len(limbs), N), dtype=np.uint64)
        for i, (l, o) in enumerate(zip(limbs, owners)):
            v[rows[i], m] = bufs[o][l, m]
        out.append((v, m))
    return out


def slices_to_limbs(world, N, limbs, owners, slices, bufs):
    ln, rows = N // world, slice_rows(owners, world)
    out = [np.array(b, dtype=np.uint64, copy=True) for b in bufs]
    for i, (l, o) in enumerate(zip(limbs, owners)):
        for r in range(world):
            out[o][l, r * ln:(r + 1) * ln] = slices[r][rows[i]]
    return out


def colslices_to_limbs(world, N, limbs, owners, slices, bufs):
    rows = slice_rows(owners, world)
    out = [np.array(b, dtype=np.uint64, copy=True) for b in bufs]
    for r in range(world):
        m = column_mask(world, N, r)
        for i, (l, o) in enumerate(zip(limbs, owners)):
            out[o][l, m] = np.asarray(slices[r])[rows[i], m]
    return out


def replicate_limbs(world, N, limbs, owners, bufs):
    out = [np.array(b, dtype=np.uint64, copy=True) for b in bufs]
    for l, o in zip(limbs, owners):
        for r in range(world):
            out[r][l] = bufs[o][l]
    return out
