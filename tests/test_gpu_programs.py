"""Whole encrypted programs on the MI355X against their slot statements, on both arithmetic back-ends (mont32 and the 36-bit generic chain).

The step lists of tests/program_ref.py (P: a degree-7 polynomial in Paterson-Stockmeyer form; M: a six-diagonal matrix-vector product through hbsgs
and through hrotate + 2 x hlintrans + hrotsum, then hplincomb; C: hreim, hclincomb, conjugation) run through host.Op objects chained with
bind_input(name, producer, output=...), each op built at the level the interpreter tracks for its inputs.  Per step: the op's output_level() is the
interpreter's level and every output ciphertext read back is the interpreter's bit for bit; where the op encodes plaintexts on the device, the
reference is fed the buffers read back from the op, each held to the longdouble encoding: equal, or one apart where the exact coefficient lies
within the transform's error of a half-integer (the check of tests/test_gpu_slots.py at this file's scales).  The final outputs decrypt and decode to the statement within 4 x REF_ERR[program, chain], the error the CPU pipeline
makes (tests/test_program_ref.py holds it to the table); each test prints its figure before it asserts.

The diagonal contract (DESIGN.md sections 12, 15, 16): hbsgs computes sum_i rot_{h^i}(sum_r pt_{i,r} (.) rot_{g^r}(ct)) over giant groups i = 0..G
and baby steps r = 0..R (identity = 1: g^0 = h^0 = 1; buffers pt0_<i> for r = 0, ptg<r> for i = 0, pt<(i-1)R+r> otherwise), and g = 5^k rotates the
slots left by k.  For y_j = sum_d diag_d[j] z[(j + d) mod n] with d = (R + 1) i + r, g = 5 and h = 5^(R+1), the plaintext of (i, r) is the diagonal
rotated right by the giant rotation: pt_{i,r}[m] = diag_d[m - (R + 1) i]; the baby rotation needs no pre-rotation.  hlintrans is one group
(pt<r>, r = 0..R, no pre-rotation by itself); hrotsum rotates input i = 1..G by h^i and has no unrotated input, so the second route starts from
rot_-3(z) and pre-rotates group i by 3 i."""
import numpy as np
import pytest

import program_ref as P
import slots_ref as R
from test_emu_slots import B_MEASURED

pytestmark = pytest.mark.gpu
CHAINS = ["mont32", "generic"]


def read_ct(op, name, copy=0):
    return np.stack([op.read(name + ".c0", copy), op.read(name + ".c1", copy)])


def assert_encoding(o, got, z, scale, mods, what):
    """a plaintext buffer the op encoded on the device against the longdouble encoding: the same integers, but for coefficients whose exact value
    lies within the double transform's error of a half-integer, where the two round apart by one.  That error is at most 8 B
    (tests/test_emu_slots.py, where B is measured at these scales and this N and 8 B is asserted): every coefficient that differs differs by
    one and its exact value is that close to a half-integer"""
    exact = R.fft_coeffs(z, P.LOGN) * R.LD(scale)
    ref = np.array([int(v) for v in np.rint(exact)], dtype=np.int64)
    near_half = np.abs(np.abs(exact - np.rint(exact)) - R.LD(0.5)) <= 8 * B_MEASURED
    coef = o.ntt(list(mods), got, inverse=True).astype(np.int64)
    for r, m in enumerate(mods):
        q = o.moduli[m]
        diff = np.where(coef[r] > (q - 1) // 2, coef[r] - q, coef[r]) - ref
        assert np.abs(diff).max() <= 1 and np.all(near_half[diff != 0]), (what, m, np.count_nonzero(diff))
        assert np.count_nonzero(diff) <= np.count_nonzero(near_half)


class Runner:
    """the programs of `machines` (one per copy of a batch, the same step list and keys) op by op on the GPU"""

    def __init__(self, chain, machines, extra=None):
        self.chain, self.ms, self.extra = chain, machines, dict(extra or {})
        self.ops, self.by_rec, self.fresh = [], {}, []

    def overrides(self, rec):
        return dict({"N": P.N, "batch": len(self.ms)}, **P.CHAINS[self.chain]["ov"], **rec.ov, **self.extra)

    def step(self, sts, refusals=True):
        """one step: sts[c] is the step of copy c.  Builds the op, binds, writes, encodes, runs the reference on what the op holds; the op is not
        executed here.  Returns (op, recs)"""
        from homulator_amd import host
        recs = [m.prepare(st) for m, st in zip(self.ms, sts)]
        rec = recs[0]
        op = host.Op(P.CFG, rec.op, P.L, rec.level, P.ALPHA, overrides=self.overrides(rec))
        for name, values in rec.consts.items():      # the constants first: writing a buffer prepares the op; one set for the whole batch
            assert all(r.consts[name] == values for r in recs)
            op.set_constants(name, values)
        bound = [(inp, self.by_rec[id(prod[0])], prod[1]) for inp, _, prod in rec.inputs if prod is not None]
        for inp, producer, output in bound:
            op.bind_input(inp, producer, output=output)
        if refusals and bound and rec.level > 2:
            wrong = host.Op(P.CFG, rec.op, P.L, rec.level - 1, P.ALPHA, overrides=self.overrides(rec))
            for inp, producer, output in bound:
                with pytest.raises(host.HostError, match="levels differ"):
                    wrong.bind_input(inp, producer, output=output)
            wrong.close()
        for stem, evk in rec.keys.items():
            for j in range(evk.shape[0]):
                for k in range(2):
                    op.write(f"{stem}Key{k}_{j}", evk[j][k])
        for c, (m, r) in enumerate(zip(self.ms, recs)):
            for inp, name, prod in r.inputs:
                if prod is None:
                    op.write(inp + ".c0", m.cts[name].limbs[0], copy=c)
                    op.write(inp + ".c1", m.cts[name].limbs[1], copy=c)
                    self.fresh.append((op, inp, name, c))
            for name, limbs in r.raw.items():
                op.write(name, limbs, copy=c)
            given = {}
            for name, (z, scale, ids) in r.encode.items():
                op.encode_plaintext(name, z, scale, copy=c)
                given[name] = op.read(name, c)
                assert_encoding(m.o, given[name], z, scale, ids, (rec.op, name))
            m.finish(r, given)
        self.ops.append(op)
        for r in recs:
            self.by_rec[id(r)] = op
        return op, recs

    def check(self, op, recs):
        for c, r in enumerate(recs):
            for out, ct in r.outs.items():
                assert op.output_level() == r.outs[next(iter(r.outs))].level
                assert op.read(out + ".c0", c).shape[0] == ct.level, (r.op, out, "level")
                got = read_ct(op, out, c)
                assert np.array_equal(got[0], ct.limbs[0]) and np.array_equal(got[1], ct.limbs[1]), (r.op, out, f"copy {c}")

    def run(self, programs):
        for sts in zip(*programs):
            op, recs = self.step(list(sts))
            op.execute(1)
            self.check(op, recs)
        return self

    def close(self):
        for op in reversed(self.ops):
            op.close()


def check_slots(name, chain, m, wants, what=""):
    for n, want in wants.items():
        err = P.slot_error(m, n, want)      # the interpreter's ciphertext is the GPU's bit for bit (checked above)
        print(f"{name} {chain} {what}{n}: max |slots - statement| = {err:.4g} on the GPU (recorded through the CPU reference {P.REF_ERR[(name, chain)]:.4g})")
        assert err <= 4 * P.REF_ERR[(name, chain)]


def polynomial_steps(m):
    """program P's steps for machine m; the one scale that is a function of the data in flight is resolved when its step comes"""
    for st in P.program_P(m.env.name):
        yield dict(st, target=m.cts[st["ins"][0]].scale ** 2) if st.get("target") == "square" else st


def machine(name, chain, seed_name=None):
    m = P.Machine(chain)
    seed = P.Z_SEED[seed_name or name]
    m.put("z", P.uniform_disc(seed), seed, P.CHAINS[chain]["M_scale"] if name == "M" else None)
    return m


def gpu_ciphertext(run, m, name, copy=0):
    """the Ct of the interpreter with the limbs read from the GPU op that produced it"""
    rec, out = m.producer[name]
    ct = m.cts[name]
    return P.Ct(read_ct(run.by_rec[id(rec)], out, copy), ct.level, ct.scale, ct.value, ct.sym)


@pytest.mark.parametrize("chain", CHAINS)
def test_polynomial(chain):
    m = machine("P", chain)
    run = Runner(chain, [m]).run([polynomial_steps(m)])
    try:
        assert [op.output_level() for op in run.ops] == [6, 6, 5, 5, 5, 5, 4]
        m.cts["out"] = gpu_ciphertext(run, m, "out")
        check_slots("P", chain, m, {"out": P.statement_P(m)})
    finally:
        run.close()


@pytest.mark.parametrize("chain", CHAINS)
def test_matrix_both_routes_and_the_plaintext_combination(chain):
    m = machine("M", chain)
    run = Runner(chain, [m]).run([P.program_M(chain)])
    try:
        assert [op.output_level() for op in run.ops] == [7, 6, 7, 7, 7, 7, 6, 6, 6]
        y, out = P.statement_M(P.uniform_disc(P.Z_SEED["M"]))
        for n in ("yA_r", "yB_r", "out"):
            m.cts[n] = gpu_ciphertext(run, m, n)
        check_slots("M", chain, m, {"yA_r": y, "yB_r": y, "out": out})
        a, b = (m.env.slots_of(m.cts[n].limbs, 6, m.cts[n].scale) for n in ("yA_r", "yB_r"))
        diff = float(np.abs(a - b).max())
        print(f"M {chain}: max |route 1 - route 2| = {diff:.4g}")
        assert diff <= 2 * 4 * P.REF_ERR[("M", chain)]
    finally:
        run.close()


@pytest.mark.parametrize("chain", CHAINS)
@pytest.mark.parametrize("name", ["C_identity", "C_generic"])
def test_complex_weights(name, chain):
    m = machine(name, chain)
    run = Runner(chain, [m]).run([P.program_C(name, chain)])
    try:
        assert [op.output_level() for op in run.ops] == [7, 6, 6]
        m.cts["out"] = gpu_ciphertext(run, m, "out")
        check_slots(name, chain, m, {"out": P.statement_C(name, P.uniform_disc(P.Z_SEED[name]))})
    finally:
        run.close()


@pytest.mark.parametrize("chain", CHAINS)
def test_polynomial_with_a_batch_of_two(chain):
    """copy 1 carries a different z under the same keys and constants: each copy meets its own statement"""
    ms = [machine("P", chain), machine("P", chain, "P_copy1")]
    run = Runner(chain, ms).run([polynomial_steps(m) for m in ms])
    try:
        assert not np.array_equal(ms[0].cts["out"].limbs, ms[1].cts["out"].limbs)
        for c, m in enumerate(ms):
            m.cts["out"] = gpu_ciphertext(run, m, "out", c)
            check_slots(["P", "P_copy1"][c], chain, m, {"out": P.statement_P(m)}, f"copy {c} ")
    finally:
        run.close()


@pytest.mark.parametrize("chain", CHAINS)
def test_polynomial_replayed_from_graphs_follows_a_rewritten_input(chain):
    """graph = 1 on every op: pass 1 runs direct, pass 2 captures, pass 3 replays.  The input ciphertext is rewritten between the second and the
    third pass: the third result is the new input's, bit for bit and by its statement"""
    m = machine("P", chain)
    run = Runner(chain, [m], extra={"graph": 1})
    try:
        run.run([polynomial_steps(m)])      # pass 1, op by op: a consumer binds to a producer that has run
        pairs = list(zip(run.ops, [[r] for r in m.recs]))
        for op, _ in pairs:
            op.execute(1)
        for op, recs in pairs:
            run.check(op, recs)
        new = machine("P", chain, "P_rewritten")
        for op, inp, name, c in run.fresh:
            op.write(inp + ".c0", new.cts[name].limbs[0], copy=c)
            op.write(inp + ".c1", new.cts[name].limbs[1], copy=c)
        for st in polynomial_steps(new):
            new.finish(new.prepare(st))
        for op, _ in pairs:
            op.execute(1)
        for (op, _), rec in zip(pairs, new.recs):
            run.check(op, [rec])
        assert not np.array_equal(new.cts["out"].limbs, m.cts["out"].limbs)
        new.cts["out"] = P.Ct(read_ct(pairs[-1][0], "out"), 4, new.cts["out"].scale, new.cts["out"].value, new.cts["out"].sym)   # what the GPU holds now
        check_slots("P_rewritten", chain, new, {"out": P.statement_P(new)})
    finally:
        run.close()
