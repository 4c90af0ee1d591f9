"""The five exchange calls of the C ABI, called directly: hm_limbs_to_slices / hm_slices_to_limbs, hm_limbs_to_colslices /
hm_colslices_to_limbs and hm_replicate_limbs against tests/exchange_ref.py (their documented contracts in numpy), bit for bit.

Several ranks are several hip.Contexts of this process on the one GPU, each driven by a thread of its own, exchanging through
homulator_amd.dist.InProcessGroup.  The contexts of one (logN, world, replicate threshold) are built once per module and shared by every
case (small chain: L = 6, K = 3; the exchanges never look at a modulus).

Data: word k of pool limb l on rank r is salt << 56 | r << 48 | l << 32 | k, so a misplaced word names the place it came from; every
destination is pre-filled (slice arrays with GUARD, pools with their own traceable pattern) and compared WHOLE: the valid positions against
the reference, every other word against what was there before.  Every case runs twice on the same contexts with different salts (the staging
buffers are reused, and grow from case to case).  Every thread is joined with a time limit; after a failure on any rank the group refuses
further work."""
import os
import re
import threading
import time

import numpy as np
import pytest

import exchange_ref as ref

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GUARD = np.uint64(0xC0DEC0DEC0DEC0DE)
JOIN_SECONDS = 60


def launch_cut():
    """chunks per launch of chunk_copy / col_copy (hm_exchange.inl): HM_MAX_CHUNKS / 2, read from hm_backend.hip"""
    with open(os.path.join(ROOT, "homulator_amd", "csrc", "hm_backend.hip")) as f:
        return int(re.search(r"^#define HM_MAX_CHUNKS (\d+)", f.read(), re.M).group(1)) // 2


class Ranks:
    """`world` contexts at N = 2^logN with one communicator over an InProcessGroup"""

    def __init__(self, logN, world, split=None, L=6, K=3):
        from homulator_amd import hip
        from homulator_amd.dist import InProcessGroup
        self.world, self.N, self.broken = world, 1 << logN, None
        self.grp = InProcessGroup(world)
        self.ctxs = [hip.Context(logN, L, K) for _ in range(world)]
        if split is not None:
            for c in self.ctxs:   # before the communicator exists, the same on every rank
                c.set_option("replicate_split_bytes", split)
        self.run(lambda r: self.ctxs[r].comm_init_external(r, world, self.grp.transport(r)))

    def run(self, fn):
        """fn(rank) on a thread per rank, then that rank's hm_sync; raises the first rank's exception"""
        if self.broken:
            pytest.fail(f"no further GPU work on this group: {self.broken}")
        errs = [None] * self.world

        def work(r):
            try:
                fn(r)
                self.ctxs[r].sync()
            except BaseException as e:  # noqa: BLE001 - reported below
                errs[r] = e
                self.grp.barrier.abort()   # the peers must not wait for this rank
        th = [threading.Thread(target=work, args=(r,), daemon=True) for r in range(self.world)]
        for t in th:
            t.start()
        deadline = time.monotonic() + JOIN_SECONDS
        for t in th:
            t.join(max(0.0, deadline - time.monotonic()))
        if any(t.is_alive() for t in th):
            self.broken = "a rank did not return in time"
            pytest.fail(self.broken)
        bad = [(r, e) for r, e in enumerate(errs) if e is not None]
        if bad or self.grp.failed:
            self.broken = f"ranks failed: {bad!r}"
            if bad:
                raise bad[0][1]
            pytest.fail(self.broken)

    def close(self):
        for c in self.ctxs:
            c.close()


@pytest.fixture(scope="module")
def groups():
    made = {}

    def get(logN, world, split=None):
        key = (logN, world, split)
        if key not in made:
            made[key] = Ranks(logN, world, split)
        return made[key]
    yield get
    for g in made.values():
        g.close()


# ---- data
def pattern(salt, rank, n_rows, N, kind=0):
    k = np.arange(N, dtype=np.uint64)
    head = (int(salt) << 56) | (int(kind) << 55) | (int(rank) << 48)
    return np.stack([np.uint64(head | (l << 32)) | k for l in range(n_rows)])


def guard_rows(n_rows, N):
    return np.full((n_rows, N), GUARD, dtype=np.uint64)


def shuffled_limbs(n, pool, seed):
    """n distinct pool indices, not monotonic, with gaps"""
    return [int(x) for x in np.random.default_rng(seed).permutation(pool)[:n]]


def owner_patterns(world, big):
    """(name, owners): limb % world, every limb on one rank (first, a middle one, last), a middle rank that owns nothing, n = 1, n < world"""
    n = world + 3 if big else 2 * world + 3
    mid = world // 2
    out = [("mod", [i % world for i in range(n)])]
    for o in sorted({0, mid, world - 1}):
        out.append((f"all-on-{o}", [o] * 4))
    if world >= 3:
        others = [r for r in range(world) if r != mid]
        out.append((f"none-on-{mid}", [others[(2 * i + 1) % len(others)] for i in range(n)]))
        out.append(("fewer-than-ranks", [(3 * i + 1) % world for i in range(world - 1)]))
    out.append(("one-limb", [world - 1]))
    return out


def most_chunks(owners, world):
    """the largest number of pack / unpack chunks one launch sequence of a rank handles: its own limbs x its peers"""
    return max(owners.count(r) for r in range(world)) * (world - 1)


CONTIG = [(13, w, name, ow) for w in (1, 2, 4, 16) for name, ow in owner_patterns(w, False)]
CONTIG.append((13, 16, "cut-18-on-5", [5, 0] + [5] * 8 + [15] + [5] * 9))        # 18 x 15 = 270 pack chunks on rank 5
COLUMN = [(logN, w, name, ow) for logN, ws in ((15, (1, 2, 4, 8)), (16, (2, 16))) for w in ws for name, ow in owner_patterns(w, True)]
COLUMN.append((15, 8, "cut-37-on-3", [3] * 20 + [6] + [3] * 17))                  # 37 x 7 = 259 pack chunks on rank 3
ids = lambda cases: [f"N{c[0]}-w{c[1]}-{c[2]}" for c in cases]


def check_cut(name, owners, world):
    if name.startswith("cut"):
        assert most_chunks(owners, world) > launch_cut(), "the case must cross the launch cut of chunk_copy / col_copy"


# ---- the four slice exchanges
def forward(g, owners, col, salt):
    W, N, n = g.world, g.N, len(owners)
    pool = n + 5
    limbs = shuffled_limbs(n, pool, salt)
    host = [pattern(salt, r, pool, N) for r in range(W)]
    words = n * N if col else n * (N // W)
    S = words // N + 1                                  # at least one guard word behind the last row
    bufs = [c.from_host(h) for c, h in zip(g.ctxs, host)]
    sl = [c.from_host(guard_rows(S, N)) for c in g.ctxs]
    try:
        if col:
            g.run(lambda r: g.ctxs[r].limbs_to_colslices(bufs[r], limbs, owners, sl[r]))
            exp = ref.limbs_to_colslices(W, N, limbs, owners, host)
        else:
            g.run(lambda r: g.ctxs[r].limbs_to_slices(bufs[r], limbs, owners, sl[r]))
            exp = ref.limbs_to_slices(W, N, limbs, owners, host)
        for r in range(W):
            got = sl[r].download().ravel()
            assert (got[words:] == GUARD).all(), f"rank {r}: words behind the last row"
            if col:
                v, m = exp[r]
                rows = got[:words].reshape(n, N)
                assert np.array_equal(rows[:, m], v[:, m]), f"rank {r}: its columns"
                assert (rows[:, ~m] == GUARD).all(), f"rank {r}: the other ranks' columns of its rows"
            else:
                assert np.array_equal(got[:words].reshape(n, N // W), exp[r]), f"rank {r}"
            assert np.array_equal(bufs[r].download(), host[r]), f"rank {r}: source pool"
    finally:
        for b in bufs + sl:
            b.free()


def reverse(g, owners, col, salt):
    W, N, n = g.world, g.N, len(owners)
    pool = n + 5
    limbs = shuffled_limbs(n, pool, salt)
    host = [pattern(salt, r, pool, N) for r in range(W)]
    if col:   # whole rows hold the rank's pattern: the other ranks' columns are junk that must not travel
        hsl = [pattern(salt, r, n, N, kind=1) for r in range(W)]
    else:
        hsl = [pattern(salt, r, n, N, kind=1)[:, :N // W].copy() for r in range(W)]
    S = hsl[0].size // N + 1
    flat = []
    for h in hsl:
        f = guard_rows(S, N).ravel()
        f[:h.size] = h.ravel()
        flat.append(f)
    bufs = [c.from_host(h) for c, h in zip(g.ctxs, host)]
    sl = [c.from_host(f) for c, f in zip(g.ctxs, flat)]
    try:
        if col:
            g.run(lambda r: g.ctxs[r].colslices_to_limbs(sl[r], bufs[r], limbs, owners))
            exp = ref.colslices_to_limbs(W, N, limbs, owners, hsl, host)
        else:
            g.run(lambda r: g.ctxs[r].slices_to_limbs(sl[r], bufs[r], limbs, owners))
            exp = ref.slices_to_limbs(W, N, limbs, owners, hsl, host)
        for r in range(W):
            # the whole pool: the owner's limbs hold every rank's part, limbs outside the list and the pools of non-owners are as before
            got = bufs[r].download()
            for l in range(pool):
                assert np.array_equal(got[l], exp[r][l]), f"rank {r}, pool limb {l} (listed: {l in limbs})"
            assert np.array_equal(sl[r].download().ravel(), flat[r]), f"rank {r}: source slices"
    finally:
        for b in bufs + sl:
            b.free()


@pytest.mark.parametrize("logN,world,name,owners", CONTIG, ids=ids(CONTIG))
def test_limbs_to_slices(groups, logN, world, name, owners):
    """slices[rows[i]][k] = limb_i[rank * N / world + k] for all n limbs on every rank; world = 1 is a local copy; world = 16 at N = 2^13 is
    len = 512, one block per chunk; the `cut` case runs chunk_copy's second launch"""
    check_cut(name, owners, world)
    g = groups(logN, world)
    for salt in (1, 2):
        forward(g, owners, False, salt)


@pytest.mark.parametrize("logN,world,name,owners", CONTIG, ids=ids(CONTIG))
def test_slices_to_limbs(groups, logN, world, name, owners):
    """the owner of limb i holds the whole limb at limbs[i]; nothing else changes in any pool"""
    check_cut(name, owners, world)
    g = groups(logN, world)
    for salt in (3, 4):
        reverse(g, owners, False, salt)


@pytest.mark.parametrize("logN,world,name,owners", COLUMN, ids=ids(COLUMN))
def test_limbs_to_colslices(groups, logN, world, name, owners):
    """row rows[i] in the limb-poly layout, the rank's column block x2 in [rank * 256 / world, ...) of every row x1 valid, the rest of the
    row untouched; the `cut` case runs col_copy's second launch"""
    check_cut(name, owners, world)
    g = groups(logN, world)
    for salt in (5, 6):
        forward(g, owners, True, salt)


@pytest.mark.parametrize("logN,world,name,owners", COLUMN, ids=ids(COLUMN))
def test_colslices_to_limbs(groups, logN, world, name, owners):
    check_cut(name, owners, world)
    g = groups(logN, world)
    for salt in (7, 8):
        reverse(g, owners, True, salt)


# ---- replicate
def replicate(g, owners, salt, calls):
    W, N, n = g.world, g.N, len(owners)
    pool = n + 5
    limbs = shuffled_limbs(n, pool, salt)
    host = [pattern(salt, r, pool, N) for r in range(W)]
    bufs = [c.from_host(h) for c, h in zip(g.ctxs, host)]
    try:
        before = list(g.grp.calls)
        g.run(lambda r: g.ctxs[r].replicate_limbs(bufs[r], limbs, owners))
        exp = ref.replicate_limbs(W, N, limbs, owners, host)
        for r in range(W):
            got = bufs[r].download()
            for l in range(pool):
                assert np.array_equal(got[l], exp[r][l]), f"rank {r}, pool limb {l} (listed: {l in limbs})"
        assert [a - b for a, b in zip(g.grp.calls, before)] == [calls] * W, "exchanges per rank: 1 = one exchange, 2 = scatter + exchange of chunks"
    finally:
        for b in bufs:
            b.free()


def three_owners(world):
    return sorted({0, world // 2, world - 1})


SINGLE = [(w, name, ow) for w in (2, 4, 16) for name, ow in owner_patterns(w, False) if not name.startswith("all-on")]
SINGLE += [(w, f"one-owner-{o}", [o] * 3) for w in (2, 4, 16) for o in three_owners(w)]


@pytest.mark.parametrize("world,name,owners", SINGLE, ids=[f"w{c[0]}-{c[1]}" for c in SINGLE])
def test_replicate_single_exchange(groups, world, name, owners):
    """every rank ends up with every limb of the list; lists below the default threshold (2 MiB) take ONE exchange whatever their owners"""
    g = groups(13, world)
    for salt in (9, 10):
        replicate(g, owners, salt, 1)


# (world, n): 4 KiB blocks against peers: 16 for 15 and 48 for 15 (runs of 2 and 4 blocks: 7 and 3 peers have nothing to send), 48 for 3 (even),
# 80 for 3 (a short last run), 16 for 3
SPLIT = [(16, 1), (16, 3), (4, 3), (4, 5), (4, 1)]
SPLIT = [(w, n, o) for w, n in SPLIT for o in three_owners(w)]


@pytest.mark.parametrize("world,n,owner", SPLIT, ids=[f"w{w}-n{n}-owner{o}" for w, n, o in SPLIT])
def test_replicate_split(groups, world, n, owner):
    """replicate_split_bytes = 1: a list with ONE owner on >= 4 ranks runs as scatter + exchange of chunks (two exchanges per rank), with
    fewer blocks than peers, an even division and a short last run; the owner first, in the middle (peers on both sides of it: the index
    shift of the runs) and last"""
    g = groups(13, world, 1)
    for salt in (11, 12):
        replicate(g, [owner] * n, salt, 2)


@pytest.mark.parametrize("world,owners", [(4, [1, 1, 2]), (4, [0, 3]), (2, [1, 1]), (2, [0])], ids=["w4-two-owners", "w4-two-owners-ends", "w2-one-owner", "w2-one-limb"])
def test_replicate_split_boundary(groups, world, owners):
    """with the threshold at 1: two owners, or a world of 2, still take the single exchange"""
    g = groups(13, world, 1)
    for salt in (13, 14):
        replicate(g, owners, salt, 1)


# ---- refusals: each returns before anything is launched or exchanged (hm_exchange.inl: the null test, col_geometry and hm_slice_rows /
# the owner loop of hm_replicate_limbs come before ensure_stage, the first kernel and the first exchange), so one rank may call alone
def five_calls(c, pool, sl, limbs, owners):
    return [("hm_limbs_to_slices", lambda: c.limbs_to_slices(pool, limbs, owners, sl)),
            ("hm_slices_to_limbs", lambda: c.slices_to_limbs(sl, pool, limbs, owners)),
            ("hm_limbs_to_colslices", lambda: c.limbs_to_colslices(pool, limbs, owners, sl)),
            ("hm_colslices_to_limbs", lambda: c.colslices_to_limbs(sl, pool, limbs, owners)),
            ("hm_replicate_limbs", lambda: c.replicate_limbs(pool, limbs, owners))]


def test_refusals(groups):
    from homulator_amd import hip
    g = groups(15, 2)           # column slices are served here, so the column calls reach their owner test
    c = g.ctxs[0]
    pool, sl = c.from_host(pattern(15, 0, 3, g.N)), c.from_host(guard_rows(3, g.N))
    try:
        for name, call in five_calls(c, pool, sl, [0, 1, 2], [0, 2, 1]):      # owner 2 in a world of 2
            with pytest.raises(hip.HmError, match=rf"hm error 1: {name}: owner out of range"):
                call()
        for name, call in five_calls(c, pool, sl, None, [0, 1, 0]):           # no limb list
            with pytest.raises(hip.HmError, match=rf"hm error 1: {name}: null argument"):
                call()
        c.sync()
        assert np.array_equal(pool.download(), pattern(15, 0, 3, g.N)) and (sl.download() == GUARD).all()
    finally:
        pool.free(); sl.free()
    g = groups(13, 4)           # N / 4096 = 2 first-pass tiles cannot be dealt to 4 ranks
    c = g.ctxs[0]
    pool, sl = c.from_host(pattern(15, 0, 3, g.N)), c.from_host(guard_rows(3, g.N))
    try:
        for name, call in five_calls(c, pool, sl, [0, 1, 2], [0, 3, 1])[2:4]:
            with pytest.raises(hip.HmError, match=rf"hm error 3: {name}: column slices need world"):
                call()
        c.sync()
        assert np.array_equal(pool.download(), pattern(15, 0, 3, g.N)) and (sl.download() == GUARD).all()
    finally:
        pool.free(); sl.free()
