"""hrotate_hoisted at the shapes it is used at, on both arithmetic back-ends (mont32 and chain_bits = 60), bit for bit:
 A. hm_inner_product_hoisted against the ORACLE (tests/test_gpu_hoisted.py compares it with its sibling kernel only): out[r][i][k] =
    sum_j sigma_{g_r}(x[i][j]) * y[r][i][k][j] mod q_i, across the 64- and 128-entry boundaries, with worst-case operands, repeated
    moduli, shared digits, every kind of Galois element and every ring size; one output per case is recomputed with Python integers
    and a permutation written out here, so the check does not rest on the oracle's C arithmetic alone;
 B. the op at every digit shape of a 13-limb chain (N = 2^13): the hoisted route (beta <= 4) and the fallback route (beta >= 5: an
    automorphism launch per rotation and plain element-wise key products), the test asserting which one it ran;
 C. rotation counts 1 and 16, a Galois element that is not 5, the conjugation;
 D. the measured shape (config_4.cfg 45/35/15, batch 10, 4 rotations) and HIP-graph capture + replay of the hoisted launch;
 E. the op as the last link of a chain, on the bound output of the link before it."""
import numpy as np
import pytest

from homulator_amd import host
from oracle.homoracle import EWE_MAC_ADD, EWE_MUL, Oracle, chain_below

pytestmark = pytest.mark.gpu
CHAINS = ["mont32", "survey"]
SEED = host.SEED
BATCH_SEED_STRIDE = 100000   # host/src/Arch.cpp kBatchSeedStride
NQ, NP = 6, 3                # the kernel tests' chain: 6 + 3 moduli
_oracles = {}


def oracle(logN, L, K, chain="mont32", threads=8):
    key = (logN, L, K, chain)
    if key not in _oracles:
        _oracles[key] = Oracle(logN, L, K, chain=chain)
    _oracles[key].set_threads(threads)
    return _oracles[key]


def chain_ov(chain, base):
    return dict(base, chain_bits=60) if chain != "mont32" else dict(base)


# ============================================================================================================================
# A. the kernel against the oracle
# ============================================================================================================================
@pytest.fixture(scope="module")
def envs():
    """(hip context, oracle on the same moduli) per (logN, chain), made on first use"""
    from homulator_amd import hip
    made = {}

    def get(logN, chain):
        if (logN, chain) not in made:
            if chain == "mont32":
                ctx = hip.Context(logN, NQ, NP)
            else:
                mods = chain_below(logN, 60, NQ + NP)
                ctx = hip.Context(logN, NQ, NP, q=mods[:NQ], p=mods[NQ:])
            o = oracle(logN, NQ, NP, chain)
            assert ctx.moduli == o.moduli
            made[(logN, chain)] = (ctx, o)
        return made[(logN, chain)]
    yield get
    for ctx, _ in made.values():
        ctx.close()


def brev(x, bits):
    r = np.zeros_like(x)
    for _ in range(bits):
        r, x = (r << 1) | (x & 1), x >> 1
    return r


def sigma_index(logN, g):
    """sigma_g in evaluation form is a permutation: slot i of the bit-reversed layout holds a(psi^e), e = 2 brev(i) + 1, and
    sigma_g(a)(psi^e) = a(psi^(g e)): out[i] = in[brev((g e mod 2N - 1) / 2)]"""
    i = np.arange(1 << logN, dtype=np.int64)
    e = g * (2 * brev(i, logN) + 1) % (2 << logN)
    return brev((e - 1) >> 1, logN)


class Case:
    """one hm_inner_product_hoisted call on device-filled operands.  Every limb list is a random permutation (the output's leaves two
    GUARD limb-polys out, which must come back untouched); y_cap bounds the key pool: rotation r's keys are rotation (r mod cap)'s,
    same entry, same modulus.  shared = [(i, i2)]: entry i2 names the digit limb-polys of entry i."""
    GUARD = 0x5A5A5A5A5A5A5A5A

    def __init__(self, ctx, o, mods, terms, galois, seed, shared=(), y_rot_cap=None):
        self.ctx, self.o, self.mods, self.T, self.galois = ctx, o, list(mods), terms, list(galois)
        n, T, R = len(mods), terms, len(galois)
        self.n, self.R = n, R
        rng = np.random.default_rng(seed)
        Ry = min(R, y_rot_cap or R)
        nx, ny, no = n * T, Ry * n * 2 * T, R * n * 2
        self.xb, self.yb, self.ob = ctx.alloc(nx), ctx.alloc(ny), ctx.alloc(no + 2)
        xp, yp, op_ = (rng.permutation(k) for k in (nx, ny, no + 2))
        self.xl = [int(v) for v in xp]
        for i, i2 in shared:
            assert self.mods[i] == self.mods[i2]
            self.xl[i2 * T:(i2 + 1) * T] = self.xl[i * T:(i + 1) * T]
        self.yl = [int(yp[e % ny]) for e in range(R * n * 2 * T)]
        self.ol, self.guards = [int(v) for v in op_[:no]], [int(v) for v in op_[no:]]
        ctx.fill_uniform(self.xb, [self.mods[e // T] for e in range(nx)], seed * 7 + 1, out_limbs=[int(v) for v in xp])
        ctx.fill_uniform(self.yb, [self.mods[e // (2 * T) % n] for e in range(ny)], seed * 7 + 2, out_limbs=[int(v) for v in yp])
        for gl in self.guards:
            self.ob.upload(np.full((1, ctx.N), self.GUARD, dtype=np.uint64), gl)
        self._rows = {}

    def x_limb(self, i, j):
        return self.xl[i * self.T + j]

    def y_limb(self, r, i, k, j):
        return self.yl[((r * self.n + i) * 2 + k) * self.T + j]

    def out_limb(self, r, i, k):
        return self.ol[(r * self.n + i) * 2 + k]

    def set_entry(self, i, x=None, y=None):
        """every coefficient of entry i's digits (x) / keys of every rotation (y): `q - 1` or 0"""
        val = lambda v: np.full((1, self.ctx.N), self.ctx.moduli[self.mods[i]] - 1 if v == "q-1" else 0, dtype=np.uint64)
        if x is not None:
            for j in range(self.T):
                self.xb.upload(val(x), self.x_limb(i, j))
        if y is not None:
            for r in range(self.R):
                for k in range(2):
                    for j in range(self.T):
                        self.yb.upload(val(y), self.y_limb(r, i, k, j))

    def run(self):
        self.ctx.inner_product_hoisted(self.xb, self.xl, self.yb, self.yl, self.ob, self.ol, self.mods, self.T, self.galois)
        return self

    def row(self, buf, limb):
        if (id(buf), limb) not in self._rows:
            self._rows[(id(buf), limb)] = buf.download(limb, 1)[0]
        return self._rows[(id(buf), limb)]

    def check(self, entries=None, rots=None):
        """the oracle's automorphism and MUL / MAC_ADD chain on the downloaded operands of `entries` x `rots` (default: all)"""
        o, T = self.o, self.T
        entries = list(range(self.n)) if entries is None else sorted(set(entries))
        rots = list(range(self.R)) if rots is None else sorted(set(rots))
        ids = [self.mods[i] for i in entries]
        X = [np.stack([self.row(self.xb, self.x_limb(i, j)) for i in entries]) for j in range(T)]
        for r in rots:
            XR = [o.automorph_eval(X[j], self.galois[r]) for j in range(T)]
            for k in range(2):
                Y = [np.stack([self.row(self.yb, self.y_limb(r, i, k, j)) for i in entries]) for j in range(T)]
                exp = o.ewe(EWE_MUL, ids, XR[0], Y[0])
                for j in range(1, T):
                    exp = o.ewe(EWE_MAC_ADD, ids, XR[j], Y[j], exp)
                got = np.stack([self.row(self.ob, self.out_limb(r, i, k)) for i in entries])
                for e, i in enumerate(entries):
                    assert np.array_equal(got[e], exp[e]), f"rotation {r} (g = {self.galois[r]}) entry {i} of {self.n} key {k}"
        for gl in self.guards:
            assert (self.ob.download(gl, 1) == np.uint64(self.GUARD)).all(), "a limb-poly outside out_limbs was written"
        return self

    def check_plain(self, r, i, k):
        """one output limb-poly with Python integers and the permutation above"""
        q = self.ctx.moduli[self.mods[i]]
        idx = sigma_index(self.ctx.logN, self.galois[r])
        acc = 0
        for j in range(self.T):
            acc = acc + self.row(self.xb, self.x_limb(i, j))[idx].astype(object) * self.row(self.yb, self.y_limb(r, i, k, j)).astype(object)
        got = self.row(self.ob, self.out_limb(r, i, k))
        assert np.array_equal(got.astype(object), acc % q), f"plain integers: rotation {r} entry {i} key {k}"
        return self

    def free(self):
        for b in (self.xb, self.yb, self.ob):
            b.free()


def rotations_of(logN, n_rot):
    """g^r as the op uses them, the conjugation in third place where there is one"""
    g = [pow(5, r + 1, 2 << logN) for r in range(n_rot)]
    if n_rot >= 3:
        g[2] = (2 << logN) - 1
    return g


def runs_of_moduli(rng, n):
    """n modulus ids in runs of 1 .. 5 equal ids (the launches of a batch carry every modulus batch times in a row)"""
    out = []
    while len(out) < n:
        out += [int(rng.integers(0, NQ + NP))] * int(rng.integers(1, 6))
    return out[:n]


@pytest.mark.parametrize("chain", CHAINS)
@pytest.mark.parametrize("n,terms,n_rot", [(1, 1, 3), (1, 4, 3), (65, 1, 3), (65, 4, 3), (130, 1, 3), (130, 4, 3), (65, 1, 16), (65, 4, 16)])
def test_entry_counts_across_the_64_and_128_boundaries(envs, chain, n, terms, n_rot):
    """hm_inner_product_ex splits its launches at 64 entries; the hoisted kernel runs ONE grid of n N / 512 workgroups over ONE table of
    [n_rot][n] records.  Compared: the first and the last entry and both sides of 64 and 128, rotations 0, 1 and the last.  The largest
    case (65 entries, 4 terms, 16 rotations) keeps 8 rotations of keys (rotation r reads rotation r mod 8's): 6500 limb-polys of 64 KiB,
    0.4 GiB."""
    ctx, o = envs(13, chain)
    rng = np.random.default_rng(1000 * n + 10 * terms + n_rot)
    c = Case(ctx, o, runs_of_moduli(rng, n), terms, rotations_of(13, n_rot), seed=n + terms + n_rot, y_rot_cap=8).run()
    sel = [i for i in (0, 1, 62, 63, 64, 126, 127, 128, 129, n - 1) if i < n]
    c.check(sel, (0, 1, n_rot - 1)).check_plain(n_rot - 1, n - 1, 1).check_plain(1 % n_rot, min(64, n - 1), 0)
    c.free()


@pytest.mark.parametrize("chain", CHAINS)
def test_worst_case_operands(envs, chain):
    """four terms of (q - 1)^2: the largest 128-bit sum the kernel's Barrett reduction sees (4 (q - 1)^2 < 2^122 for q < 2^60), on the
    largest modulus of the chain and on a special modulus; entries of zeros; the rest random"""
    ctx, o = envs(13, chain)
    big = ctx.moduli.index(max(ctx.moduli))
    mods = [big, big, NQ + NP - 1, 3, 3, 5, NQ, 1]
    c = Case(ctx, o, mods, 4, rotations_of(13, 3), seed=77)
    c.set_entry(0, x="q-1", y="q-1")
    c.set_entry(2, x="q-1", y="q-1")
    c.set_entry(3, x="q-1")            # (q - 1) x random
    c.set_entry(4, y="q-1")            # random x (q - 1)
    c.set_entry(5, x="0")
    c.set_entry(6, y="0")
    c.set_entry(7, x="0", y="0")
    c.run().check().check_plain(2, 0, 1).check_plain(0, 2, 0)
    q0 = ctx.moduli[big]                # 4 (q - 1)^2 = 4 mod q, whatever the rotation
    assert (c.row(c.ob, c.out_limb(1, 0, 0)) == np.uint64(4 % q0)).all()
    assert not c.row(c.ob, c.out_limb(1, 5, 1)).any() and not c.row(c.ob, c.out_limb(2, 7, 0)).any()
    c.free()


@pytest.mark.parametrize("chain", CHAINS)
@pytest.mark.parametrize("terms", [2, 3])
def test_repeated_moduli_and_shared_digits(envs, chain, terms):
    """runs of equal modulus ids, and entries that name the SAME digit limb-polys with their own keys and outputs (what batching an
    operand shared by the ops of a batch produces)"""
    ctx, o = envs(13, chain)
    mods = [2, 2, 2, 5, 5, 0, 0, 0, 0, 8, 2]
    c = Case(ctx, o, mods, terms, rotations_of(13, 3), seed=31 + terms, shared=[(0, 1), (5, 8), (0, 10)]).run()
    c.check().check_plain(1, 1, 0).check_plain(2, 10, 1)
    assert not np.array_equal(c.row(c.ob, c.out_limb(0, 0, 0)), c.row(c.ob, c.out_limb(0, 1, 0)))   # same digits, own keys
    c.free()


@pytest.mark.parametrize("chain", CHAINS)
@pytest.mark.parametrize("which", ["mixed", "sixteen"])
def test_galois_elements(envs, chain, which):
    """one call whose rotations are the identity (every output lands where its digit pair was read), the conjugation 2N - 1, 3, 2N - 3
    (elements outside the powers of 5) and 5^k for a large k; and sixteen distinct elements in one call"""
    ctx, o = envs(13, chain)
    twoN = 2 << 13
    if which == "mixed":
        galois = [1, twoN - 1, 3, twoN - 3, pow(5, 2001, twoN)]
    else:
        galois = [pow(5, 3 * r + 1, twoN) for r in range(8)] + [twoN - pow(5, 7 * r + 2, twoN) for r in range(7)] + [twoN - 1]
        assert len(set(galois)) == 16
    rng = np.random.default_rng(len(galois))
    c = Case(ctx, o, runs_of_moduli(rng, 6), 3, galois, seed=5 + len(galois)).run()
    c.check().check_plain(0, 0, 0).check_plain(1, 3, 1).check_plain(len(galois) - 1, 5, 0)
    c.free()


@pytest.mark.parametrize("chain", CHAINS)
@pytest.mark.parametrize("logN", [14, 15, 17])
def test_other_ring_sizes(envs, chain, logN):
    """hm_auto_src and the inverse element the kernel scatters by depend on logN: 5 entries, 3 terms, rotations 5, 25 and the conjugation"""
    ctx, o = envs(logN, chain)
    c = Case(ctx, o, [0, 4, 4, NQ + 1, 2], 3, rotations_of(logN, 3), seed=logN).run()
    c.check().check_plain(2, 1, 1).check_plain(0, 4, 0)
    c.free()


# ============================================================================================================================
# B. the op at every digit shape
# ============================================================================================================================
def hoisted_keys(o, ell, R, seed=SEED):
    """rotation r's key is the synthetic stream seed + 10000 + 100000 r (Operation.cpp, HROTATE_HOISTED)"""
    return [o.synth_evk(ell, seed + 10000 + 100000 * r) for r in range(1, R + 1)]


def read_rotations(op, R, copy=0):
    return [(op.read(f"out{r}.c0", copy=copy), op.read(f"out{r}.c1", copy=copy)) for r in range(1, R + 1)]


def assert_rotations(got, exp, what):
    assert len(got) == len(exp)
    for r, (g, e) in enumerate(zip(got, exp), start=1):
        for k in range(2):
            assert np.array_equal(g[k], e[k]), (what, f"out{r}.c{k}")


def route_of(kinds):
    return "hoisted" if "IP_HOISTED" in kinds else "fallback"


@pytest.mark.parametrize("alpha,chain", [(a, "mont32") for a in (1, 2, 3, 5, 13)] + [(1, "survey"), (3, "survey")])
def test_every_level_small_ring_hoisted(alpha, chain):
    """hrotate_hoisted (2 rotations) at EVERY level of a 13-limb chain on N = 2^13, as test_every_level_small_ring runs hmult and hrotate:
    beta = 1 .. 13, short and one-limb last digits.  The planner builds key-product records of at most 4 terms, so only beta <= 4 takes the
    hoisted launch; deeper decompositions run an automorphism launch per rotation and element-wise key products (the fallback route).
    Every point asserts the route it took.  The unfused plan runs at the highest level of each route."""
    from hoisted_ref import hoisted_rotations
    L, logN, R = 13, 13, 2
    o = oracle(logN, L, alpha, chain, threads=4)
    beta = lambda ell: -(-ell // alpha)
    unfused_at = {max(e for e in range(1, L + 1) if beta(e) <= 4)} | ({L} if beta(L) > 4 else set())
    for ell in range(1, L + 1):
        exp = hoisted_rotations(o, ell, o.synth_ct(ell, SEED), 5, hoisted_keys(o, ell, R))
        for fuse in (True, False) if ell in unfused_at else (True,):
            op = host.Op("config_4_N15.cfg", "hrotate_hoisted", L, ell, alpha, fuse=fuse, overrides=chain_ov(chain, {"N": 1 << logN, "rotations": R}))
            kinds = [ln.split()[0] for ln in op.plan()]
            if not fuse:
                assert "IP_HOISTED" not in kinds
            elif beta(ell) <= 4:
                assert kinds.count("IP_HOISTED") == 1 and "AUTO" not in kinds, (alpha, ell, kinds)
            else:
                assert "IP_HOISTED" not in kinds and kinds.count("AUTO") >= 1, (alpha, ell, kinds)
            op.execute(1)
            assert_rotations(read_rotations(op, R), exp, (alpha, ell, route_of(kinds) if fuse else "unfused"))
            op.close()


# ============================================================================================================================
# C. rotation counts and elements
# ============================================================================================================================
N15 = ("config_4_N15.cfg", 15, 16, 10, 4)


@pytest.mark.parametrize("chain", CHAINS)
@pytest.mark.parametrize("R,galois", [(1, 5), (16, 5), (3, 3), (1, 2 * 32768 - 1)])
def test_rotation_counts_and_elements(chain, R, galois):
    """config_4_N15.cfg 16/10/4: one rotation, the sixteen a launch takes at most, a Galois element outside the powers of 5, and the
    conjugation (its square is 1: only rotations = 1 is valid)"""
    from hoisted_ref import hoisted_rotations
    cfg, logN, L, ell, alpha = N15
    o = oracle(logN, L, alpha, chain)
    op = host.Op(cfg, "hrotate_hoisted", L, ell, alpha, overrides=chain_ov(chain, {"rotations": R, "galois": galois}))
    hoisted = [ln for ln in op.plan() if ln.startswith("IP_HOISTED")]
    assert len(hoisted) == 1 and f" rot={R} " in hoisted[0] + " "
    op.execute(1)
    exp = hoisted_rotations(o, ell, o.synth_ct(ell, SEED), galois, hoisted_keys(o, ell, R))
    assert_rotations(read_rotations(op, R), exp, (R, galois))
    op.close()


# ============================================================================================================================
# D. the measured shape, and graph replay
# ============================================================================================================================
def test_bench_shape_batch_10_graph_replay():
    """what tools/hoist_bench.py times: config_4.cfg 45/35/15 (N = 2^16), 10 ops per launch, 4 rotations: a hoisted launch of 500 entries, the
    plan captured into a HIP graph (run 1 direct, run 2 captures, runs 3 and 4 replay).  After the last run copies 0, 5 and 9 of the batch,
    all four rotations, equal the reference; the launch count is the single op's and the stage bytes scale by the batch."""
    from hoisted_ref import hoisted_rotations
    cfg, logN, L, ell, alpha, R, B = "config_4.cfg", 16, 45, 35, 15, 4, 10
    o = oracle(logN, L, alpha, threads=16)
    single = host.Op(cfg, "hrotate_hoisted", L, ell, alpha, backend=host.BACKEND_COUNT, overrides={"rotations": R})
    op = host.Op(cfg, "hrotate_hoisted", L, ell, alpha, overrides={"rotations": R, "batch": B, "graph": 1})
    assert op.batch == B
    hoisted = [ln for ln in op.plan() if ln.startswith("IP_HOISTED")]
    assert len(hoisted) == 1 and f" n={B * (ell + alpha)} " in hoisted[0] + " "
    for _ in range(4):
        op.execute(1)
    assert op.launch_count() == single.launch_count()
    assert op.stage_bytes() == B * single.stage_bytes()
    keys = hoisted_keys(o, ell, R)
    for c in (0, 5, 9):
        ct = o.synth_ct(ell, SEED + c * BATCH_SEED_STRIDE)
        assert np.array_equal(op.read("ct1.c1", copy=c), ct[1])
        assert_rotations(read_rotations(op, R, copy=c), hoisted_rotations(o, ell, ct, 5, keys), f"copy {c}")
    op.close()
    single.close()


@pytest.mark.parametrize("chain", CHAINS)
def test_graph_replay_sixteen_rotations_batch_3(chain):
    """config_4_N15.cfg 16/10/4, 3 ops per launch, 16 rotations, graph = 1: every copy and rotation after the first (direct) execution and
    after the fourth (second replay).  Repeated execution does not consume its inputs, and the replayed hoisted launch reads the record
    table the direct run made."""
    from hoisted_ref import hoisted_rotations
    cfg, logN, L, ell, alpha = N15
    R, B = 16, 3
    o = oracle(logN, L, alpha, chain)
    keys = hoisted_keys(o, ell, R)
    exp = [hoisted_rotations(o, ell, o.synth_ct(ell, SEED + c * BATCH_SEED_STRIDE), 5, keys) for c in range(B)]
    op = host.Op(cfg, "hrotate_hoisted", L, ell, alpha, overrides=chain_ov(chain, {"rotations": R, "batch": B, "graph": 1}))
    for run in range(4):
        op.execute(1)
        if run in (0, 3):
            for c in range(B):
                assert_rotations(read_rotations(op, R, copy=c), exp[c], f"run {run} copy {c}")
    op.close()


# ============================================================================================================================
# E. in a chain
# ============================================================================================================================
@pytest.mark.parametrize("ops,batch", [("hmult,hrotate_hoisted", 1), ("hadd,hrotate_hoisted", 2)])
def test_last_link_of_a_chain(ops, batch):
    """the hoisted op on the bound output of the link before it (after an hmult: one level down).  Seeds: link k runs under seed + 31 k
    (OpChain), so the hoisted link's rotation r has the key of stream seed + 31 k + 10000 + 100000 r, ONE key for every op of a batch; op c of
    a batch starts from the chain input of seed + 100000 c."""
    from hoisted_ref import hoisted_rotations
    from test_gpu_chain import expected_chain
    L, ell, alpha, R = 6, 5, 2, 2
    o = oracle(15, L, alpha)
    prefix = ops.split(",")[:-1]
    chain = host.Chain("config_4_N15.cfg", ops, L, ell, alpha, overrides={"rotations": R, "batch": batch})
    assert len(chain) == len(prefix) + 1
    chain.execute(1)
    ell_h = ell - prefix.count("hmult")
    keys = hoisted_keys(o, ell_h, R, SEED + 31 * len(prefix))
    for c in range(batch):
        mid = expected_chain(o, prefix, ell, SEED + c * BATCH_SEED_STRIDE)[-1]
        assert np.array_equal(chain[-1].read("ct1.c0", copy=c), mid[0]) and np.array_equal(chain[-1].read("ct1.c1", copy=c), mid[1])
        assert_rotations(read_rotations(chain[-1], R, copy=c), hoisted_rotations(o, ell_h, mid, 5, keys), f"copy {c}")
    chain.close()
