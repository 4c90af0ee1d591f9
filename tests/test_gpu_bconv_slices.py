"""The base conversion as the sharded plans call it, at kernel level and against the oracle, bit for bit:

 1. hm_bconv_col on ranges of column tiles (one context): a range writes its own columns of every output limb and nothing else, the ranges of
    a partition add up to the full call, and the second pass on the union is the oracle's ntt(bconv_matmul(...));
 2. the sharded ModUp of one digit as the header documents it: hm_limbs_to_colslices -> hm_bconv_col on the rank's tiles ->
    hm_colslices_to_limbs -> hm_ntt_second_pass, several ranks as threads over homulator_amd.dist.InProcessGroup;
 3. hm_bconv_batch on coefficient slices (log_len from 8 to logN, limb stride 2^log_len in both buffers).

Destinations are pre-filled with GUARD (above 2^63: no residue and no lazy value of a transform can equal it), so "written" is "differs from
GUARD"."""
import numpy as np
import pytest

import exchange_ref as ref
from oracle.homoracle import Oracle
from test_gpu_exchange import GUARD, Ranks

pytestmark = pytest.mark.gpu


def make_env(logN, L, K, chain):
    from homulator_amd import hip
    o = Oracle(logN, L, K, chain=chain)
    ctx = hip.Context(logN, L, K) if chain == "mont32" else hip.Context(logN, L, K, q=o.moduli[:L], p=o.moduli[L:])
    assert ctx.moduli == o.moduli
    return ctx, o, hip


def pack30(a):
    """the split-30 packed form hm_ntt_ex(out_packed) stores and hm_bconv_desc.in_packed takes"""
    return (a & np.uint64(0x3FFFFFFF)) | ((a >> np.uint64(30)) << np.uint64(32))


def guard_rows(n_rows, N):
    return np.full((n_rows, N), GUARD, dtype=np.uint64)


def digit_inputs(o, ins, seed, ends=()):
    """uniform residues with q_i - 1, 0 and 1 on the first coefficients (every input at q_i - 1 at once: the sums at their largest) and q_i - 1
    on the last coefficient of every length in `ends`"""
    y = o.fill_uniform(ins, seed)
    for r, m in enumerate(ins):
        y[r, :4] = o.moduli[m] - 1
        y[r, 4:6] = [0, 1]
        y[r, -1] = o.moduli[m] - 1
        for e in ends:
            y[r, e - 1] = o.moduli[m] - 1
    return y


# ------------------------------------------------------------------------------------------------------------------------------------------
# 1. hm_bconv_col on tile ranges
# ------------------------------------------------------------------------------------------------------------------------------------------
N_OUT = 9                                             # odd: the last workgroup of the two-output form has one output
HAND_LIMBS = [11, 2, 7, 0, 9, 4, 12, 5, 3]            # where the hand-off limbs go: shuffled, with gaps (1, 6, 8, 10 stay free)
HAND_POOL = 13


@pytest.fixture(scope="module", params=[(15, "mont32"), (16, "mont32"), (15, "survey")], ids=lambda p: f"N{p[0]}-{p[1]}")
def colenv(request):
    logN, chain = request.param
    ctx, o, hip = make_env(logN, 32, N_OUT, chain)
    yield ctx, o, hip
    ctx.close()


@pytest.mark.parametrize("packed", [0, 1], ids=["plain", "packed"])
@pytest.mark.parametrize("n_in", [1, 5, 15, 17, 32])
def test_bconv_col_tile_ranges(colenv, n_in, packed):
    """hm_bconv_col(tile0, n_tiles) with T = N / 4096 tiles, on every range (r T / w, T / w) of the partitions w = 2, 4, T and on the full
    call, one and two outputs per workgroup, digits of one input group (1, 5, 15) and of two (17, 32).

    The hand-off layout (hm_ntt_passes.inl, gidx of the strided pass): word x1 * 256 + (tile << log2(256 / T)) + c, so tile t of the first
    pass IS the column block x2 in [t * 256 / T, (t + 1) * 256 / T) of every row x1, before and after the pass (a column transform stays in
    its column).  Hence (c): a range writes exactly the words whose index i has i % 256 in its column block, which is what
    hm_colslices_to_limbs carries back; (a) disjoint ranges that cover every output word once, (b) their union equals the full call, (d)
    nothing outside the output limbs, (e) hm_ntt_second_pass on the union equals the oracle."""
    ctx, o, hip = colenv
    N = ctx.N
    T = N // 4096
    ins, outs = list(range(n_in)), list(range(32, 32 + N_OUT))
    y = digit_inputs(o, ins, 300 + n_in)
    want = o.ntt(outs, o.bconv_matmul(ins, outs, y))
    in_pool = n_in + 3
    in_limbs = [int(x) for x in np.random.default_rng(n_in).permutation(in_pool)[:n_in]]
    hsrc = guard_rows(in_pool, N)
    hsrc[in_limbs] = pack30(y) if packed else y
    src, hand = ctx.from_host(hsrc), ctx.alloc(HAND_POOL)
    free = [l for l in range(HAND_POOL) if l not in HAND_LIMBS]
    x2 = np.arange(N) % 256

    def run(tile0, n_tiles):
        hand.upload(guard_rows(HAND_POOL, N))
        ctx.bconv_col([(src, in_limbs, ins, hand, HAND_LIMBS, outs, packed)], tile0, n_tiles)
        return hand.download()
    try:
        for outs_per_wg in (1, 2):
            ctx.set_option("bconv_col_outs", outs_per_wg)
            full = run(0, 0)
            assert (full[free] == GUARD).all() and (full[HAND_LIMBS] != GUARD).all(), outs_per_wg       # (d) and a complete hand-off
            for w in (2, 4, T):
                count = np.zeros((HAND_POOL, N), dtype=np.int32)
                union = guard_rows(HAND_POOL, N)
                for r in range(w):
                    got = run(r * T // w, T // w)
                    written = got != GUARD
                    assert not written[free].any(), (outs_per_wg, w, r)                                  # (d)
                    block = (x2 // (256 // w)) == r
                    assert np.array_equal(written[HAND_LIMBS], np.broadcast_to(block, (N_OUT, N))), (outs_per_wg, w, r)   # (c), 1 / w of each limb
                    count += written
                    union[written] = got[written]
                assert (count[HAND_LIMBS] == 1).all(), (outs_per_wg, w)                                  # (a)
                assert np.array_equal(union, full), (outs_per_wg, w)                                     # (b)
            hand.upload(full)                                                                            # (e)
            ctx.ntt_second_pass(hand, outs, limbs=HAND_LIMBS)
            done = hand.download()
            assert np.array_equal(done[HAND_LIMBS], want), outs_per_wg
            assert (done[free] == GUARD).all(), outs_per_wg
    finally:
        ctx.set_option("bconv_col_outs", 0)
        src.free(); hand.free()


def test_bconv_col_refuses_bad_tile_ranges(colenv):
    """hm_tile_range_ok is enforced before anything is launched (bconv_col_launch: its first check): a power of two of tiles, aligned, inside
    the limb-poly"""
    ctx, o, hip = colenv
    N, T = ctx.N, ctx.N // 4096
    ins, outs = [0, 1, 2], list(range(32, 32 + N_OUT))
    src, hand = ctx.from_host(digit_inputs(o, ins, 7)), ctx.from_host(guard_rows(HAND_POOL, N))
    try:
        for tile0, n_tiles in ((0, 3), (1, 2), (T // 2, T), (T, T), (T, 1)):
            with pytest.raises(hip.HmError, match=r"hm error 1: fused conversion: tile range"):
                ctx.bconv_col([(src, None, ins, hand, HAND_LIMBS, outs)], tile0, n_tiles)
        ctx.sync()
        assert (hand.download() == GUARD).all()
    finally:
        src.free(); hand.free()


# ------------------------------------------------------------------------------------------------------------------------------------------
# 2. the sharded ModUp of one digit, call by call
# ------------------------------------------------------------------------------------------------------------------------------------------
MODUP_OUT = 7


@pytest.fixture(scope="module")
def modup_groups():
    made = {}

    def get(logN, world):
        if (logN, world) not in made:
            made[logN, world] = Ranks(logN, world, L=20, K=4), Oracle(logN, 20, 4)
        return made[logN, world]
    yield get
    for g, _ in made.values():
        g.close()


@pytest.mark.parametrize("n_in", [5, 17])
@pytest.mark.parametrize("logN,world", [(15, 2), (15, 8), (16, 16)])
def test_sharded_modup_digit(modup_groups, logN, world, n_in):
    """limb-polys of the digit on their owners (i % world) -> column slices -> conversion + first pass on the rank's tiles (tile0 = rank T /
    world, n_tiles = T / world) -> the hand-off's column slices back to the owners of the output limbs (i % world) -> second pass there:
    every owner's limbs equal the oracle's ntt(bconv_matmul(...)); nothing else is written in the output pools"""
    g, o = modup_groups(logN, world)
    assert g.ctxs[0].moduli == o.moduli
    W, N = world, g.N
    T = N // 4096
    ins, outs = list(range(n_in)), list(range(17, 17 + MODUP_OUT))
    y = digit_inputs(o, ins, 500 + n_in)
    want = o.ntt(outs, o.bconv_matmul(ins, outs, y))
    in_owners, out_owners = [i % W for i in range(n_in)], [i % W for i in range(MODUP_OUT)]
    in_rows, out_rows = ref.slice_rows(in_owners, W), ref.slice_rows(out_owners, W)
    rng = np.random.default_rng(n_in * 100 + world)
    in_pool, out_pool = n_in + 3, MODUP_OUT + 4
    in_limbs = [int(x) for x in rng.permutation(in_pool)[:n_in]]
    out_limbs = [int(x) for x in rng.permutation(out_pool)[:MODUP_OUT]]
    pools, sls, hands, dsts = [], [], [], []
    for r, c in enumerate(g.ctxs):
        h = guard_rows(in_pool, N)                       # a limb is present on its owner only: anything read elsewhere is GUARD
        for i in range(n_in):
            if in_owners[i] == r:
                h[in_limbs[i]] = y[i]
        pools.append(c.from_host(h))
        sls.append(c.from_host(guard_rows(n_in, N)))
        hands.append(c.from_host(guard_rows(MODUP_OUT, N)))
        dsts.append(c.from_host(guard_rows(out_pool, N)))

    def body(r):
        c = g.ctxs[r]
        c.limbs_to_colslices(pools[r], in_limbs, in_owners, sls[r])
        c.bconv_col([(sls[r], in_rows, ins, hands[r], out_rows, outs)], r * T // W, T // W)
        c.colslices_to_limbs(hands[r], dsts[r], out_limbs, out_owners)
        mine = [t for t in range(MODUP_OUT) if out_owners[t] == r]
        if mine:
            c.ntt_second_pass(dsts[r], [outs[t] for t in mine], limbs=[out_limbs[t] for t in mine])
    try:
        g.run(body)
        for r in range(W):
            got = dsts[r].download()
            mine = {out_limbs[t]: t for t in range(MODUP_OUT) if out_owners[t] == r}
            for l in range(out_pool):
                if l in mine:
                    assert np.array_equal(got[l], want[mine[l]]), f"rank {r}: output {mine[l]}"
                else:
                    assert (got[l] == GUARD).all(), f"rank {r}: pool limb {l} is not its output"
    finally:
        for b in pools + sls + hands + dsts:
            b.free()


# ------------------------------------------------------------------------------------------------------------------------------------------
# 3. hm_bconv_batch on coefficient slices
# ------------------------------------------------------------------------------------------------------------------------------------------
# (n_in, n_out) of the problems of the two calls: every width of {1, 2, 15, 16, 17, 32} and every output count of {1, 7, 33}; each call has three
# widths (three launches) and call A a second problem of one width (two records of one launch, ragged output counts)
CALLS = {"A": [(1, 33), (15, 7), (32, 1), (15, 1)], "B": [(2, 1), (16, 33), (17, 7)]}
LOG_LENS = [8, 9, 10, 12]
BLOCKS = [3072, 1, 1 << 20]    # option bconv_blocks (hm_bconv_grid): the default; one chunk (every output of a problem in one block); chunks of 4 outputs


@pytest.fixture(scope="module", params=[(13, "mont32"), (16, "mont32"), (13, "survey")], ids=lambda p: f"N{p[0]}-{p[1]}")
def lenenv(request):
    """context, oracle and — computed once — the inputs and the oracle's conversion of every problem on all N coefficients: the conversion is
    coefficient-wise, a call on slices of 2^log_len coefficients must give the first 2^log_len columns"""
    logN, chain = request.param
    ctx, o, hip = make_env(logN, 46, 3, chain)
    data = {}
    for name, shapes in CALLS.items():
        for j, (n_in, n_out) in enumerate(shapes):
            ins, outs = list(range(n_in)), list(range(n_in, n_in + n_out))
            x = digit_inputs(o, ins, 700 + 10 * j + ord(name), ends=[1 << k for k in range(8, logN + 1)])
            data[name, j] = ins, outs, x, o.bconv_matmul(ins, outs, x)
    yield ctx, o, hip, data
    ctx.close()


def slots(total, pool, rng, last=False):
    """`total` distinct slots of a pool, shuffled (gaps: pool > total); last: the pool's last slot is one of them"""
    s = [int(x) for x in rng.permutation(pool - 1 if last else pool)[:total - 1 if last else total]] + ([pool - 1] if last else [])
    rng.shuffle(s)
    return [int(v) for v in s]


@pytest.mark.parametrize("packed", [0, 1], ids=["plain", "packed"])
@pytest.mark.parametrize("call", ["A", "B"])
@pytest.mark.parametrize("log_len", LOG_LENS + ["logN-1", "logN"])
def test_bconv_batch_on_slices(lenenv, log_len, call, packed):
    """limb stride 2^log_len in both buffers, limbs at shuffled slots with gaps; every word of the output buffer that is not an output limb keeps
    its guard (the words behind the pool's last slot, which is an output, included).  log_len = 8: half a block's threads leave at the
    bounds check; "logN": the full length given explicitly."""
    ctx, o, hip, data = lenenv
    ll = ctx.logN - 1 if log_len == "logN-1" else ctx.logN if log_len == "logN" else log_len
    if ll in LOG_LENS and log_len == "logN-1":
        ll = 11            # N = 2^13: 12 is in the list already; one more length instead of a repeat
    N, ln = ctx.N, 1 << ll
    shapes = CALLS[call]
    rng = np.random.default_rng(ll * 4 + packed)
    n_ins, n_outs = sum(s[0] for s in shapes), sum(s[1] for s in shapes)
    in_pool, out_pool = n_ins + 7, n_outs + 6
    in_slots, out_slots = slots(n_ins, in_pool, rng), slots(n_outs, out_pool, rng, last=True)
    rows = lambda words: -(-words // N)
    hin = guard_rows(rows(in_pool * ln), N).ravel()
    hout = guard_rows(rows((out_pool + 1) * ln), N).ravel()           # at least 2^log_len guard words behind the last slot
    expect = hout.copy()
    probs, a, b = [], 0, 0
    src, dst = ctx.alloc(hin.size // N), ctx.alloc(hout.size // N)
    for j, (n_in, n_out) in enumerate(shapes):
        ins, outs, x, want = data[call, j]
        il, ol = in_slots[a:a + n_in], out_slots[b:b + n_out]
        a, b = a + n_in, b + n_out
        for i, s in enumerate(il):
            hin[s * ln:(s + 1) * ln] = pack30(x[i, :ln]) if packed else x[i, :ln]
        for t, s in enumerate(ol):
            expect[s * ln:(s + 1) * ln] = want[t, :ln]
        probs.append((src, il, ins, dst, ol, outs, packed))
    src.upload(hin)
    try:
        for blocks in BLOCKS:
            ctx.set_option("bconv_blocks", blocks)
            dst.upload(hout)
            ctx.bconv_batch(probs, log_len=ll)
            got = dst.download().ravel()
            bad = np.nonzero(got != expect)[0]
            assert bad.size == 0, (blocks, f"{bad.size} words differ, first at slot {bad[0] // ln} + {bad[0] % ln} (output slots {out_slots})")
        assert np.array_equal(src.download().ravel(), hin)
    finally:
        ctx.set_option("bconv_blocks", 3072)
        src.free(); dst.free()


def test_bconv_batch_refuses_bad_lengths(lenenv):
    """each refusal comes from hm_bconv_batch's argument loop, before the first table is built or kernel launched"""
    import ctypes as C
    ctx, o, hip, data = lenenv
    N = ctx.N
    ins, outs, x, _ = data["B", 0]
    src, dst, other = ctx.from_host(x), ctx.from_host(guard_rows(2, N)), ctx.from_host(guard_rows(1, N))
    prob = (src, None, ins, dst, None, outs)
    try:
        with pytest.raises(hip.HmError, match=r"hm error 1: hm_bconv: log_len 7"):
            ctx.bconv_batch([prob], log_len=7)
        with pytest.raises(hip.HmError, match=rf"hm error 1: hm_bconv: log_len {ctx.logN + 1}"):
            ctx.bconv_batch([prob], log_len=ctx.logN + 1)
        keep, descs = ctx._bconv_descs([prob, prob], 8)
        descs[1].log_len = 9
        assert ctx.L.hm_bconv_batch(ctx.h, descs, 2) == 1 and b"mixed log_len" in ctx.L.hm_last_error(ctx.h)
        keep, descs = ctx._bconv_descs([prob], 8)          # the sub_from epilogue works on whole limb-polys
        ks = np.ones(len(outs), dtype=np.uint64)
        descs[0].sub_from, descs[0].sub_k = other.ptr, ks.ctypes.data_as(C.c_void_p)
        assert ctx.L.hm_bconv_batch(ctx.h, descs, 1) == 3 and b"epilogue works on whole limb-polys" in ctx.L.hm_last_error(ctx.h)
        ctx.sync()
        assert (dst.download() == GUARD).all()
    finally:
        src.free(); dst.free(); other.free()
