"""The launch-table cache of a context (homulator_amd/csrc/hm_table_cache.h, device_table in hm_backend.hip) on the GPU, bit for bit against the
oracle: every call that obtains more than one table before it launches, with the cache at its limit at every position within the call; eviction
behind kernels still in flight; the pins (a live graph, a capture in progress), the refused miss under capture, and graphs that outlive their context.

The contract: no table handed out since the entry of an ABI call is freed before that call returns.  The cache starts over at the entry of a call
when it holds `launch_table_limit` tables or more and nothing pins it, so between two evictions it holds at most limit - 1 tables plus one call's.

A "position sweep" of a call that makes T tables: with the limit M = T + 2, the cache is emptied, filled with M - j cheap filler tables (an inverse
hm_ntt of one limb-poly with a scale nobody used before), and the call runs twice, each time onto a cleared output; for every j in 0 .. T.  At j = 0
the first run's entry evicts; at every other j the first run carries the cache over the limit and the second run's entry frees the tables the first
run's kernels may still be reading.  The counters are read, never assumed."""
import ctypes as C

import numpy as np
import pytest

from oracle.homoracle import Oracle

pytestmark = pytest.mark.gpu
CHAINS = ["mont32", "survey"]
DEFAULT_LIMIT = 1024
GUARD = 0x5A5A5A5A5A5A5A5A
ADD, MUL_CONST, SUB_SCALE = 3, 5, 6   # hm_ewe / ho_ewe opcodes
_oracles = {}


def oracle(logN, L, K, chain):
    key = (logN, L, K, chain)
    if key not in _oracles:
        _oracles[key] = Oracle(logN, L, K, chain=chain)
        _oracles[key].set_threads(16)
    return _oracles[key]


class Env:
    """a context of its own (the limit option changes it), the oracle on the same moduli, and the filler"""

    def __init__(self, logN, L, K, chain="mont32"):
        from homulator_amd import hip
        self.hip, self.o = hip, oracle(logN, L, K, chain)
        self.ctx = hip.Context(logN, L, K) if chain == "mont32" else hip.Context(logN, L, K, q=self.o.moduli[:L], p=self.o.moduli[L:])
        assert self.ctx.moduli == self.o.moduli
        assert self.ctx.counter("launch_table_limit") == DEFAULT_LIMIT and self.tables() == 0 and self.evictions() == 0
        self.fsrc, self.fdst, self.fscale = self.ctx.alloc(1), self.ctx.alloc(1), 1
        self.ctx.fill_uniform(self.fsrc, [0], 1)

    def tables(self):
        return self.ctx.counter("launch_tables")

    def evictions(self):
        return self.ctx.counter("launch_table_evictions")

    def limit(self, v):
        self.ctx.set_option("launch_table_limit", v)
        assert self.ctx.counter("launch_table_limit") == v

    def filler(self):
        """one new table: an inverse transform of one limb-poly with a scale of its own (not synchronised)"""
        self.fscale += 1
        self.ctx.ntt(self.fsrc, self.fdst, [0], inverse=True, scale=[self.fscale])

    def empty_then_fill(self, limit, count):
        """the cache holds exactly `count` >= 1 filler tables and nothing else; the limit is `limit`"""
        self.limit(1)
        self.filler()               # at limit 1 every call with a table in the cache starts over at its entry
        assert self.tables() == 1
        self.limit(limit)
        while self.tables() < count:
            self.filler()
        assert self.tables() == count

    def close(self):
        self.ctx.close()


def sweep(env, run, clear, check, what):
    """the position sweep of `run` (see the module's docstring); returns (tables the call makes, evictions seen during the runs under test)"""
    env.empty_then_fill(DEFAULT_LIMIT, 1)
    clear(); run(); check((what, "cold"))
    made = env.tables() - 1
    assert made >= 1, what
    M, seen = made + 2, 0
    for j in range(made + 1):
        env.empty_then_fill(M, M - j)
        ev = env.evictions()
        for rep in range(2):
            clear(); run()
            assert env.tables() <= M - 1 + made, (what, j, rep, env.tables())
            check((what, f"limit {M}, {M - j} tables at the entry", rep))
        seen += env.evictions() - ev
    print(f"{what}: {made} tables per call, {seen} evictions during the sweep")
    assert seen > 0, what
    return made, seen


def guard(buf):
    buf.upload(np.full((buf.n_limbs, buf.ctx.N), GUARD, dtype=np.uint64))


# ============================================================================================================================
# a. hm_bconv_batch with the sub_from epilogue: the constants of every problem are a table whose address sits in the launch's records
# ============================================================================================================================
class EpilogueCase:
    """four conversions with out = (sub_from - conv) * sub_k [+ add], two input-basis sizes (two launches), constants of their own"""

    def __init__(self, env):
        ctx, o = env.ctx, env.o
        L = o.L
        shapes = [([L, L + 1, L + 2], [0, 1, 2, 3, 4, 5], True), ([L, L + 1, L + 2], [0, 1, 2, 3], False),
                  ([4, 5], [0, 1, 2, L], True), ([0, 1], [2, 3, L + 1], False)]
        self.ctx, self.bufs, self.keep, self.exp, self.outs = ctx, [], [], [], []
        self.descs = (env.hip.hm_bconv_desc * len(shapes))()
        for i, (ins, outs, with_add) in enumerate(shapes):
            x = o.fill_uniform(ins, 400 + i)
            for r, m in enumerate(ins):
                x[r, :3] = [o.moduli[m] - 1, 0, 1]
            if i == 0:
                x[0, :] = o.moduli[ins[0]] - 1
            a, b = o.fill_uniform(outs, 500 + i), o.fill_uniform(outs, 600 + i)
            a[0, :2] = [0, o.moduli[outs[0]] - 1]
            k = [o.moduli[m] - 2 - 7 * i - t for t, m in enumerate(outs)]
            e = o.ewe(SUB_SCALE, outs, a, None, o.bconv_matmul(ins, outs, x), k=k)
            self.exp.append(o.ewe(ADD, outs, e, None, b) if with_add else e)
            dx, da, db, out = ctx.from_host(x), ctx.from_host(a), ctx.from_host(b), ctx.alloc(len(outs))
            arrs = [np.asarray(ins, dtype=np.uint32), np.asarray(outs, dtype=np.uint32), np.asarray(k, dtype=np.uint64)]
            d = self.descs[i]
            d.in_, d.in_ids, d.n_in, d.out, d.out_ids, d.n_out = dx.ptr, arrs[0].ctypes.data, len(ins), out.ptr, arrs[1].ctypes.data, len(outs)
            d.sub_from, d.sub_k, d.add = da.ptr, arrs[2].ctypes.data, db.ptr if with_add else None
            self.bufs += [dx, da, db, out]; self.keep.append(arrs); self.outs.append(out)

    def run(self):
        self.ctx._ck(self.ctx.L.hm_bconv_batch(self.ctx.h, self.descs, len(self.descs)))

    def clear(self):
        for out in self.outs:
            guard(out)

    def check(self, what):
        for i, (out, e) in enumerate(zip(self.outs, self.exp)):
            assert np.array_equal(out.download(), e), (what, "problem", i)


@pytest.mark.parametrize("chain", CHAINS)
def test_bconv_batch_epilogue_constants_survive_an_eviction_inside_the_call(chain):
    env = Env(13, 6, 3, chain)
    try:
        case = EpilogueCase(env)
        made, _ = sweep(env, case.run, case.clear, case.check, f"hm_bconv_batch epilogue {chain}")
        assert made == 6   # four constants tables and the records of two launches
    finally:
        env.close()


# ============================================================================================================================
# b. hm_ntt_mix_sub_scale with conversions inside and the mix prologue; hm_bconv_col alone
# ============================================================================================================================
class MixCase:
    """the shape and the expected chain of test_gpu_kernels.py::test_mix_sub_scale_with_conversion_inside: two keys of K special limbs converted to
    ell = 7 limbs inside the first pass, with the mix operand, plus two limb-polys with an ordinary input"""

    def __init__(self, env, ell, K):
        ctx, o = env.ctx, env.o
        N = ctx.N
        qs, ps, nkeys = list(range(ell)), list(range(ell, ell + K)), 2
        y = o.fill_uniform(ps * nkeys, 21).reshape(nkeys, K, N)
        y[0, 0, :] = o.moduli[ps[0]] - 1
        y[1, :, :3] = [[o.moduli[m] - 1, 0, 1] for m in ps]
        extra_ids = [1, 4]
        extra = o.fill_uniform(extra_ids, 22)
        self.ids = ids = qs * nkeys + extra_ids
        mn, ad, mx = (o.fill_uniform(ids, s) for s in (23, 24, 25))
        self.k = k = [o.moduli[m] - 2 - r for r, m in enumerate(ids)]
        self.mk = mk = [(kk * 3 + 1) % o.moduli[m] for kk, m in zip(k, ids)]
        self.ak = ak = [(kk * 5 + 1) % o.moduli[m] for kk, m in zip(k, ids)]
        self.ctx = ctx
        self.ysrc, self.xsrc = ctx.from_host(y.reshape(-1, N)), ctx.from_host(extra)
        self.dmn, self.dad, self.dmx, self.out = ctx.from_host(mn), ctx.from_host(ad), ctx.from_host(mx), ctx.alloc(len(ids))
        self.conv = [(self.ysrc, [kk_ * K + i for i in range(K)], ps, [kk_ * ell + t for t in range(ell)], qs) for kk_ in range(nkeys)]
        self.in_limbs = [0] * (nkeys * ell) + [0, 1]
        conv_out = np.concatenate([o.bconv_matmul(ps, qs, y[kk_]) for kk_ in range(nkeys)])
        xin = np.concatenate([conv_out, extra])
        x = o.ewe(ADD, ids, xin, None, o.ewe(MUL_CONST, ids, mx, k=mk))
        self.exp = o.ewe(ADD, ids, o.ewe(SUB_SCALE, ids, mn, None, o.ntt(ids, x), k=k), None, o.ewe(MUL_CONST, ids, ad, k=ak))
        # hm_bconv_col alone: the hand-off of the two conversions, finished by hm_ntt_second_pass
        self.hand = ctx.alloc(nkeys * ell)
        self.col_probs = [(self.ysrc, c[1], c[2], self.hand, c[3], c[4]) for c in self.conv]
        self.col_ids = qs * nkeys
        self.col_exp = o.ntt(self.col_ids, conv_out)

    def run(self):
        self.ctx.ntt_mix_sub_scale(self.xsrc, self.dmn, self.out, self.ids, self.k, addend=self.dad, addend_k=self.ak, mix=self.dmx, mix_k=self.mk,
                                   in_limbs=self.in_limbs, conv=self.conv)

    def clear(self):
        guard(self.out)

    def check(self, what):
        assert np.array_equal(self.out.download(), self.exp), what

    def run_col(self):
        self.ctx.bconv_col(self.col_probs)
        self.ctx.ntt_second_pass(self.hand, self.col_ids)

    def clear_col(self):
        guard(self.hand)

    def check_col(self, what):
        assert np.array_equal(self.hand.download(), self.col_exp), what


@pytest.mark.parametrize("chain", CHAINS)
@pytest.mark.parametrize("outs_per_wg", [1, 2])
@pytest.mark.parametrize("K", [2, 5])
def test_mix_constants_survive_an_eviction_inside_the_fused_conversion(chain, K, outs_per_wg):
    env = Env(15, 7, K, chain)
    try:
        env.ctx.set_option("bconv_col_outs", outs_per_wg)
        case = MixCase(env, 7, K)
        made, _ = sweep(env, case.run, case.clear, case.check, f"hm_ntt_mix_sub_scale conv + mix K={K} outs={outs_per_wg} {chain}")
        assert made >= 3   # a constants table per conversion and the records of at least one launch
        if outs_per_wg == 2:
            sweep(env, case.run_col, case.clear_col, case.check_col, f"hm_bconv_col + hm_ntt_second_pass K={K} {chain}")
    finally:
        env.close()


# ============================================================================================================================
# c. hm_ntt_inner_product with conversions inside
# ============================================================================================================================
@pytest.mark.parametrize("nip_small", [0, 4096], ids=["wide", "small-launch"])
def test_ntt_inner_product_with_conversions_at_every_position(nip_small):
    """the shape of test_gpu_kernels.py::test_ntt_inner_product_with_conversion_inside at N = 2^15: two digits of two limbs, two ops sharing the key"""
    n_in, K, N = 2, 3, 1 << 15
    env = Env(15, 2 * n_in, K)
    try:
        ctx, o = env.ctx, env.o
        ell, beta, nops = 2 * n_in, 2, 2
        ext = o.ext_ids(ell); E = len(ext)
        digits = [list(range(0, n_in)), list(range(n_in, 2 * n_in))]
        own = o.fill_uniform(list(range(ell)) * nops, 5).reshape(nops, ell, -1)
        scaled = o.fill_uniform(list(range(ell)) * nops, 6).reshape(nops, ell, -1)
        scaled[0, 0, :] = o.moduli[0] - 1
        scaled[1, :, :3] = [[o.moduli[m] - 1, 0, 1] for m in range(ell)]
        evk = np.stack([o.fill_uniform(ext, 100 + 10 * k + j) for k in range(2) for j in range(beta)])
        src, ownb, evkb = ctx.from_host(scaled.reshape(-1, N)), ctx.from_host(own.reshape(-1, N)), ctx.from_host(evk.reshape(-1, N))
        hand, out = ctx.alloc(nops * beta * E), ctx.alloc(nops * 2 * E)
        conv, xl, flags, hl, yl, ol, mods = [], [], [], [], [], [], []
        for b in range(nops):
            for j, dj in enumerate(digits):
                outs = [t for t in range(E) if t not in dj]
                conv.append((src, [b * ell + i for i in dj], dj, [(b * beta + j) * E + t for t in outs], [ext[t] for t in outs]))
            for t in range(E):
                for j, dj in enumerate(digits):
                    isown = t in dj
                    xl.append(b * ell + t if isown else 0); hl.append((b * beta + j) * E + t); flags.append(0 if isown else 1)
                for k in range(2):
                    yl += [(k * beta + j) * E + t for j in range(beta)]
                    ol.append((b * 2 + k) * E + t)
                mods.append(ext[t])
        exp = np.empty((nops, 2, E, N), dtype=np.uint64)
        for b in range(nops):
            X = []
            for j, dj in enumerate(digits):
                outs = [t for t in range(E) if t not in dj]
                full = np.zeros((E, N), dtype=np.uint64)
                full[outs] = o.ntt([ext[t] for t in outs], o.bconv_matmul(dj, [ext[t] for t in outs], scaled[b, dj]))
                full[dj] = own[b, dj]
                X.append(full)
            for k in range(2):
                exp[b, k] = o.ewe(1, ext, X[0], evk[k * beta + 0], X[1], evk[k * beta + 1])
        ctx.set_option("nip_small_limbs", nip_small)

        def check(what):
            assert np.array_equal(out.download().reshape(nops, 2, E, N), exp), what
        sweep(env, lambda: ctx.ntt_inner_product(ownb, xl, flags, hand, hl, evkb, yl, out, ol, mods, beta, 2, conv=conv), lambda: guard(out), check,
              f"hm_ntt_inner_product conv nip_small_limbs={nip_small}")
    finally:
        env.close()


# ============================================================================================================================
# d. a transform cut into many launches, behind an un-synchronised launch of the same size
# ============================================================================================================================
def test_chunked_inverse_transform_behind_kernels_in_flight():
    """140 limb-polys with a scale at ntt_launch_entries = 8 (the smallest launches): many launches, each with a table of its own.  The second call follows the first
    without a synchronisation, with limits at which its entry (or the next call's) frees the tables the first call's kernels read: the free waits"""
    n = 140
    env = Env(13, 6, 3)
    try:
        ctx, o = env.ctx, env.o
        mods = [i % 9 for i in range(n)]
        x = o.fill_uniform(mods, 77)
        x[0, :] = o.moduli[0] - 1
        x[1, :] = 0
        s1, s2 = [o.moduli[m] - 1 - i for i, m in enumerate(mods)], [3 + i for i in range(n)]
        inv = o.ntt(mods, x, inverse=True)
        exp1, exp2 = o.ewe(MUL_CONST, mods, inv, k=s1), o.ewe(MUL_CONST, mods, inv, k=s2)
        dx, out1, out2 = ctx.from_host(x), ctx.alloc(n), ctx.alloc(n)
        ctx.set_option("ntt_launch_entries", 8)
        env.empty_then_fill(DEFAULT_LIMIT, 1)
        ctx.ntt(dx, out1, mods, inverse=True, scale=s1)
        made = env.tables() - 1
        # (a launch holds at least eight same-modulus groups, hm_launch_split: 140 limb-polys in groups of two are nine launches)
        assert made > 2 and np.array_equal(out1.download(), exp1)
        print(f"chunked inverse transform: {made} tables per call")
        ev0 = env.evictions()
        for lim in (1, 2, made - 1, made, made + 1, 2 * made, 2 * made + 1):
            env.empty_then_fill(lim, 1)
            guard(out1); guard(out2)
            ev = env.evictions()
            ctx.ntt(dx, out1, mods, inverse=True, scale=s1)
            ctx.ntt(dx, out2, mods, inverse=True, scale=s2)     # no synchronisation in between
            env.filler()
            assert env.evictions() > ev, lim   # at the second call's entry, or at the filler's
            assert np.array_equal(out1.download(), exp1) and np.array_equal(out2.download(), exp2), lim
        assert env.evictions() > ev0
    finally:
        env.close()


# ============================================================================================================================
# e. single-table calls at limit 1; more than the default limit of tables in one context
# ============================================================================================================================
def test_single_table_calls_at_limit_one():
    """every call evicts the table of the call before it: hm_inner_product_lintrans_id, hm_inner_product_rotsum_init, hm_tensor_dot,
    hm_ntt_mix_sub_scale_mul, each against the reference of its own test module, three times"""
    import test_gpu_dot, test_gpu_identity, test_gpu_rescale
    env = Env(13, 6, 3)
    try:
        ctx, o = env.ctx, env.o
        env.limit(1)
        mods = [0, 7, 3]
        for rep in range(3):
            ev = env.evictions()
            test_gpu_identity.run_kernel_case(ctx, o, mods, 2, test_gpu_identity.elements(3), 1, 11 + rep, add_mask=[True, False, True])
            test_gpu_identity.run_init_case(ctx, mods, 2, test_gpu_identity.elements(3), 21 + rep, add_mask=[True, False, True])
            test_gpu_dot.run_kernel_case(ctx, o, mods, 2, 31 + rep)
            test_gpu_rescale.forward_case(ctx, o, mods, 41 + rep, mix=True, addend=True, addend_k=True, plain=(1,))
            assert env.evictions() >= ev + 4 and env.tables() <= 2, rep
    finally:
        env.close()


def test_more_than_the_default_limit_of_tables():
    env = Env(13, 6, 3)
    try:
        case = EpilogueCase(env)
        count = DEFAULT_LIMIT + 40
        top = 0
        for i in range(count):
            env.filler()
            if i >= DEFAULT_LIMIT - 2:
                top = max(top, env.tables())
        assert top == DEFAULT_LIMIT and env.evictions() == 1 and env.tables() == count - DEFAULT_LIMIT
        env.empty_then_fill(DEFAULT_LIMIT, 1)
        while env.tables() < DEFAULT_LIMIT - 3:
            env.filler()
        ev = env.evictions()
        case.clear(); case.run(); case.check("over the default limit inside the call")   # six tables: the call passes the limit
        assert env.tables() == DEFAULT_LIMIT + 3 and env.evictions() == ev
        case.clear(); case.run(); case.check("the default limit at the entry")
        assert env.tables() == 6 and env.evictions() == ev + 1
    finally:
        env.close()


# ============================================================================================================================
# f. g. h. graphs
# ============================================================================================================================
def capture(ctx, run):
    g = C.c_void_p()
    ctx._ck(ctx.L.hm_capture_begin(ctx.h))
    run()
    ctx._ck(ctx.L.hm_capture_end(ctx.h, C.byref(g)))
    return g


@pytest.mark.parametrize("chain", CHAINS)
def test_a_live_graph_pins_the_cache(chain):
    env = Env(15, 7, 2, chain)
    try:
        ctx = env.ctx
        ctx.L.hm_graph_launch.argtypes = [C.c_void_p, C.c_void_p]
        ctx.L.hm_graph_destroy.argtypes = [C.c_void_p]
        case = MixCase(env, 7, 2)
        case.clear(); case.run(); case.check("warm")
        g = capture(ctx, case.run)
        count, ev = env.tables(), env.evictions()
        env.limit(2)
        assert count > 2
        for _ in range(5):
            env.filler()
        assert env.evictions() == ev and env.tables() == count + 5      # over the limit, nothing freed
        case.clear()
        ctx._ck(ctx.L.hm_graph_launch(ctx.h, g))
        case.check("replay with the cache over its limit")
        print(f"pinned {chain}: {env.tables()} tables at limit 2, {env.evictions() - ev} evictions while pinned")
        ctx.L.hm_graph_destroy(g)
        env.filler()                                                      # the pin is gone: this call starts over
        assert env.evictions() == ev + 1 and env.tables() == 1
        case.clear(); case.run(); case.check("after the graph")
    finally:
        env.close()


def test_a_miss_under_capture_is_refused_and_the_context_goes_on():
    env = Env(13, 6, 3)
    try:
        ctx, o, hip = env.ctx, env.o, env.hip
        ctx.L.hm_graph_launch.argtypes = [C.c_void_p, C.c_void_p]
        ctx.L.hm_graph_destroy.argtypes = [C.c_void_p]
        mods = [0, 7, 3]
        x = o.fill_uniform(mods, 5)
        x[0, :3] = [o.moduli[0] - 1, 0, 1]
        scale = [o.moduli[m] - 9 for m in mods]
        exp = o.ewe(MUL_CONST, mods, o.ntt(mods, x, inverse=True), k=scale)
        dx, out = ctx.from_host(x), ctx.alloc(3)
        run = lambda: ctx.ntt(dx, out, mods, inverse=True, scale=scale)
        env.filler()
        count, ev = env.tables(), env.evictions()
        guard(out)
        ctx._ck(ctx.L.hm_capture_begin(ctx.h))
        with pytest.raises(hip.HmError, match="run the plan once"):
            run()                                        # its table was never built
        assert env.tables() == count and env.evictions() == ev
        g = C.c_void_p()
        st = ctx.L.hm_capture_end(ctx.h, C.byref(g))     # either status: the capture holds no call
        print(f"hm_capture_end after a refused call: status {st}" + ("" if st == 0 else f" ({ctx.L.hm_last_error(ctx.h).decode()})"))
        if st == 0 and g.value:
            ctx.L.hm_graph_destroy(g)
        run()
        assert np.array_equal(out.download(), exp), "directly, after the refused capture"
        guard(out)
        g = capture(ctx, run)                            # warm now
        assert np.all(out.download() == GUARD)
        ctx._ck(ctx.L.hm_graph_launch(ctx.h, g))
        assert np.array_equal(out.download(), exp), "replay"
        ctx.L.hm_graph_destroy(g)
    finally:
        env.close()


def test_a_graph_outlives_its_context():
    env, other = Env(13, 6, 3), Env(13, 6, 3)
    try:
        ctx = env.ctx
        ctx.L.hm_graph_launch.argtypes = [C.c_void_p, C.c_void_p]
        ctx.L.hm_graph_destroy.argtypes = [C.c_void_p]
        case = EpilogueCase(env)
        case.run(); case.check("warm")
        g = capture(ctx, case.run)
        env.close()
        st = other.ctx.L.hm_graph_launch(other.ctx.h, g)
        assert st != 0 and b"captured from another (or a destroyed) context" in other.ctx.L.hm_last_error(other.ctx.h)
        other.ctx.L.hm_graph_destroy(g)                  # the orphan: returns normally
        other.filler(); other.ctx.sync()
    finally:
        env.close(); other.close()
