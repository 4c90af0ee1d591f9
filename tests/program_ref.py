"""Whole CKKS programs through the CPU references (test helper only): a small interpreter for a program given as a list of steps, each an op name, its
outputs, its inputs and its parameters.  Every step runs through the op's reference (tests/*_ref.py, the oracle's hmult / hrotate / pmult) and never
through the GPU; encoding and decoding are tests/slots_ref.py's, encryption, keys and decryption tests/toy_ckks.py's.

For every ciphertext in flight the interpreter tracks
    level   the number of limbs,
    scale   a fractions.Fraction: Delta' = Delta_a Delta_b / q_dropped is exact,
    value   the slot vector the statement says it holds, complex longdouble,
    sym     where the value is a polynomial in the input z with rational coefficients, those coefficients as Fractions (program P).

A weight c of a scaling op is never a residue in the step list.  The step names the scale S_pre the sum has before a rescale (`target`), the op's
integer scalar is s = rint(c S_pre / Delta_in), and the statement uses the rational s Delta_in / S_pre, not c: rounding a scalar is not part of the
error, and every term of a sum has the scale S_pre exactly.  Constants are k = rint(c S_pre): a constant carries the scale BEFORE the rescale.
A plaintext encoded at the double scale f where the sum wants the Fraction S is weighted Fraction(f) / S in the same way.

Two conditions are asserted at every step (conditions, not measurements): the terms of an addition have equal levels and equal scales as Fractions,
and max |value| scale < Q_level / 4 before and after a rescale.

The programs (N = 2^13, L = 8, alpha = 2, the input at level 7; |z_j| <= 1; chains "mont32" and "generic", the 36-bit chain):
  P   a degree-7 polynomial in Paterson-Stockmeyer form, p = q_lo(z) + z^4 q_hi(z) + c: hsquare, hlincomb (rescale), hmult, hsquare, hmlincomb
      (rescale), hmlincomb (M = 2, constants), hdotadd (scale, addend, constant).
  M   y = A z for six diagonals d = 0..5, once through hbsgs (identity = 1: baby steps 0..2, giant groups 0..1) and once through hrotate by -3,
      2 x hlintrans (identity = 1) and hrotsum; hrescale; then w (.) y + v (.) z + c through hlincomb (z to y's level and scale) and hplincomb.
      hrotsum rotates every one of its inputs, so route 2 starts from rot_-3(z): its groups are rotated by 3 and 6 where hbsgs rotates by 0 and 3.
  C   hreim, hclincomb with the weights (a + b i) / 2 and (c + d i) / 2 and a constant, hrotate by 2N - 1: conj((a + b i) Re z + (c + d i) Im z + k);
      "C_identity" has the weights (1, i) and k = 0 and returns conj(z), "C_generic" a generic pair.

The diagonal contract of hbsgs / hlintrans (DESIGN.md sections 12, 15, 16): the op computes sum_i rot_{h^i}(sum_r pt_{i,r} (.) rot_{g^r}(ct)), and
g = 5^k rotates the slots left by k (slot j receives slot j + k).  With g = 5 and h = 5^3, slot j of the result is sum_{i,r} pt_{i,r}[j + 3 i]
z[j + 3 i + r]: for y_j = sum_d diag_d[j] z[j + d] the plaintext of (i, r) is diagonal d = 3 i + r rotated RIGHT by the giant rotation,
pt_{i,r}[m] = diag_d[m - 3 i] (numpy.roll(diag_d, 3 i)); the baby rotation needs no pre-rotation.

REF_ERR: max |slots(dec(out)) - statement| of the reference pipeline per (program, chain), measured on the CPU with the seeds below
(print_reference_errors()).  The CPU test holds the pipeline to them within a factor 2 (the runs are deterministic; the factor absorbs a libm
difference), the GPU tests assert 4 x these, the margin of tests/test_gpu_slots.py."""
from fractions import Fraction

import numpy as np

import slots_ref as R
from oracle.homoracle import Oracle

LD, CLD = np.longdouble, np.clongdouble
LOGN, L, ALPHA, ELL = 13, 8, 2, 7
N, NSLOT = 1 << LOGN, 1 << (LOGN - 1)
CFG = "config_4_N15.cfg"
# per chain: the oracle's chain, the op overrides that select it, the scale of a fresh ciphertext (about one modulus, so it stays stable through
# rescales), the input scale of program M (times the plaintext scale over one modulus it is y's scale: 2^50 and 2^36), the scale of a device-encoded
# plaintext (|coefficient| <= (q_src - 1) / 2) and the integer S the weights of a sum without a rescale are scaled by
CHAINS = {
    "mont32": dict(chain="mont32", ov={}, ct_scale=1 << 60, M_scale=1 << 60, pt_scale=2.0 ** 50, S=1 << 30),
    "generic": dict(chain=36, ov={"chain_bits": 36}, ct_scale=1 << 36, M_scale=1 << 48, pt_scale=2.0 ** 24, S=1 << 20),
}
SECRET_SEED, KEY_SEED, ENC_SEED = 4273, 52000, 61000      # the secret; key of Galois element g: KEY_SEED + g (relinearisation: KEY_SEED); inputs
Z_SEED = {"P": 81, "P_copy1": 82, "P_rewritten": 83, "M": 84, "C_identity": 85, "C_generic": 86}
REF_ERR = {
    ("P", "mont32"): 4.96e-14,
    ("P", "generic"): 8.09e-07,
    ("P_copy1", "mont32"): 1.79e-13,
    ("P_copy1", "generic"): 3e-06,
    ("P_rewritten", "mont32"): 1.12e-13,
    ("P_rewritten", "generic"): 1.9e-06,
    ("M", "mont32"): 1.41e-10,
    ("M", "generic"): 1.44e-05,
    ("C_identity", "mont32"): 3.31e-12,
    ("C_identity", "generic"): 5.54e-05,
    ("C_generic", "mont32"): 2.71e-12,
    ("C_generic", "generic"): 4.51e-05,
}


class Ct:
    def __init__(self, limbs, level, scale, value, sym=None):
        self.limbs, self.level, self.scale, self.value, self.sym = np.stack(limbs), level, Fraction(scale), np.asarray(value, dtype=CLD), sym


class Env:
    """one chain: the oracle, the toy scheme under one secret, and the keys, each made once from a seed of its own (so no result depends on the
    order in which the tests ask for them)"""

    def __init__(self, chain):
        from toy_ckks import Toy
        self.name, self.par = chain, CHAINS[chain]
        self.o = Oracle(LOGN, L, ALPHA, chain=self.par["chain"])
        self.o.set_threads(8)
        self.toy = Toy(self.o, seed=SECRET_SEED)
        self._keys = {}

    def Q(self, level):
        q = 1
        for j in range(level):
            q *= self.o.moduli[j]
        return q

    def _full_key(self, g):
        if g not in self._keys:
            from dot_ref import negacyclic_small
            toy = self.toy
            toy.rng = np.random.default_rng(KEY_SEED + g)
            if g == 0:
                s = np.array([int(x) for x in toy.s])
                self._keys[g] = toy.gen_evk(negacyclic_small(s, s).astype(object))
            else:
                self._keys[g] = toy.gen_evk(toy.automorph(toy.s, g))
        return self._keys[g]

    def relin_key(self, level):
        return self.toy.evk_at_level(self._full_key(0), level)

    def rot_key(self, g, level):
        return self.toy.evk_at_level(self._full_key(g), level)

    def encrypt(self, z, seed, level=ELL, scale=None):
        """a fresh encryption of the exact encoding of z at the chain's ciphertext scale: value z, sym the polynomial z"""
        self.toy.rng = np.random.default_rng(ENC_SEED + seed)
        scale = self.par["ct_scale"] if scale is None else scale
        return Ct(self.toy.encrypt(R.encode_int(z, LOGN, scale, R.fft_coeffs), level), level, scale, z, [Fraction(0), Fraction(1)])

    def slots_of(self, limbs, level, scale):
        """decrypt with Python integers, decode with the longdouble reference at the Fraction scale"""
        dec, _ = self.toy.decrypt(np.stack(limbs), level)
        m = np.array([LD(int(v)) for v in dec], dtype=LD) / (LD(scale.numerator) / LD(scale.denominator))
        re, im = R.fft_slots(m, LOGN)
        return re + 1j * im.astype(CLD)


_envs = {}


def env(chain):
    if chain not in _envs:
        _envs[chain] = Env(chain)
    return _envs[chain]


def rint_frac(x):
    """the integer nearest to a Fraction, ties to even"""
    return round(Fraction(x))


def as_frac(c):
    return c if isinstance(c, Fraction) else Fraction(c)      # a float is a dyadic rational: exact


def to_ld(x):
    x = Fraction(x)
    return LD(x.numerator) / LD(x.denominator)


def poly_mul(a, b):
    out = [Fraction(0)] * (len(a) + len(b) - 1)
    for i, x in enumerate(a):
        for j, y in enumerate(b):
            out[i + j] += x * y
    return out


def poly_sum(terms, const=Fraction(0)):
    """sum_t w_t p_t + const for (weight, coefficient list) pairs; None if any term has no polynomial"""
    if any(p is None for _, p in terms):
        return None
    out = [Fraction(const)] + [Fraction(0)] * (max(len(p) for _, p in terms) - 1)
    for w, p in terms:
        for i, x in enumerate(p):
            out[i] += w * x
    return out


def rotation(k):
    """the Galois element that rotates the slots left by k (k may be negative)"""
    return pow(5, k % NSLOT, 2 * N)


def rot(v, k):
    """slot j receives slot j + k"""
    return np.roll(v, -k)


class Rec:
    """one step as the GPU side needs it: the op and its overrides, the level it is built at, what its inputs are bound to, its integer constants,
    its keys, the plaintexts to encode on the device and the buffers to write as they are; after finish() the outputs by output name"""

    def __init__(self, op, ov, level):
        self.op, self.ov, self.level = op, dict(ov), level
        self.inputs, self.consts, self.keys, self.encode, self.raw = [], {}, {}, {}, {}
        self.outs, self.out_names, self.compute = {}, {}, None


class Machine:
    """the interpreter.  `broken` names one deliberate break of the pipeline's input (the statement is never touched): "unrotated" feeds hbsgs and
    hlintrans the diagonals without their pre-rotation, "swap_ab" swaps a_t and b_t of hclincomb, "post_rescale_const" scales the constant of
    hdotadd by the scale after the rescale"""

    def __init__(self, chain, broken=None):
        self.env, self.o, self.par, self.broken = env(chain), env(chain).o, CHAINS[chain], broken
        self.cts, self.producer, self.recs = {}, {}, []

    # ---- the two conditions
    def headroom(self, value, scale, level, what):
        assert float(np.abs(value).max()) * scale < Fraction(self.env.Q(level), 4), (what, "headroom")

    def same(self, xs, what):
        assert len({x.level for x in xs}) == 1, (what, "levels differ", [x.level for x in xs])
        return xs[0].level

    def residues(self, s, level):
        return [int(s) % self.o.moduli[j] for j in range(level)]

    def scalar(self, c, x, target, what):
        """(the integer scalar of weight c on ciphertext x for a sum at scale `target`, the rational weight it stands for)"""
        s = rint_frac(as_frac(c) * target / x.scale)
        assert x.scale * (target / x.scale) == target      # the term's scale is the sum's, as Fractions
        return s, Fraction(s) * x.scale / target

    def put(self, name, ct_or_z, seed=None, scale=None):
        """a program input: a slot vector (encrypted here) or a Ct"""
        self.cts[name] = ct_or_z if isinstance(ct_or_z, Ct) else self.env.encrypt(ct_or_z, seed, scale=scale)
        self.producer[name] = None
        self.headroom(self.cts[name].value, self.cts[name].scale, self.cts[name].level, name)

    def bind(self, rec, input_name, name):
        rec.inputs.append((input_name, name, self.producer[name]))
        return self.cts[name]

    def target(self, st, xs):
        """the scale of the sum before a rescale: st["target"] as it is, or the first term's scale times st["S"]"""
        return Fraction(st["target"]) if "target" in st else xs[0].scale * st.get("S", self.par["S"])

    def close(self, rec, limbs, level, scale, value, sym, rescaled, out="out"):
        """the result of a step: the conditions before and after the rescale, the Ct"""
        self.headroom(value, scale, level, (rec.op, "before the rescale"))
        if rescaled:
            scale, level = scale / self.o.moduli[level - 1], level - 1
            self.headroom(value, scale, level, (rec.op, "after the rescale"))
        assert np.stack(limbs).shape == (2, level, N), (rec.op, np.stack(limbs).shape, level)
        return Ct(limbs, level, scale, value, sym)

    # ---- the steps: each returns the Rec with rec.compute(plaintext limbs by name) -> {output name: Ct}
    def op_hsquare(self, st):
        x = self.cts[st["ins"][0]]
        rec = Rec("hsquare", {}, x.level)
        self.bind(rec, "ct1", st["ins"][0])
        rec.keys["IP_"] = self.env.relin_key(x.level)

        def compute(_):
            import square_ref
            out = square_ref.square(self.o, x.level, x.limbs, rec.keys["IP_"])
            return {"out": self.close(rec, out, x.level, x.scale * x.scale, x.value * x.value, None if x.sym is None else poly_mul(x.sym, x.sym), True)}
        rec.compute = compute
        return rec

    def op_hmult(self, st):
        x, y = (self.cts[n] for n in st["ins"])
        level = self.same([x, y], "hmult")
        rec = Rec("hmult", {}, level)
        self.bind(rec, "ct1", st["ins"][0])
        self.bind(rec, "ct2", st["ins"][1])
        rec.keys["IP_"] = self.env.relin_key(level)

        def compute(_):
            out = self.o.hmult(level, x.limbs, y.limbs, rec.keys["IP_"])
            sym = None if x.sym is None or y.sym is None else poly_mul(x.sym, y.sym)
            return {"out": self.close(rec, out, level, x.scale * y.scale, x.value * y.value, sym, True)}
        rec.compute = compute
        return rec

    def op_hrescale(self, st):
        x = self.cts[st["ins"][0]]
        rec = Rec("hrescale", {}, x.level)
        self.bind(rec, "ct1", st["ins"][0])

        def compute(_):
            import rescale_ref
            return {"out": self.close(rec, rescale_ref.rescale_ct(self.o, x.level, x.limbs), x.level, x.scale, x.value, x.sym, True)}
        rec.compute = compute
        return rec

    def op_hrotate(self, st):
        """st["rot"] = k: slots left by k; st["conj"]: the conjugation, g = 2N - 1"""
        x = self.cts[st["ins"][0]]
        g = 2 * N - 1 if st.get("conj") else rotation(st["rot"])
        rec = Rec("hrotate", {"galois": g}, x.level)
        self.bind(rec, "ct1", st["ins"][0])
        rec.keys["IP_"] = self.env.rot_key(g, x.level)

        def compute(_):
            out = self.o.hrotate(x.level, x.limbs, g, rec.keys["IP_"])
            value = np.conj(x.value) if st.get("conj") else rot(x.value, st["rot"])
            return {"out": self.close(rec, out, x.level, x.scale, value, None, False)}
        rec.compute = compute
        return rec

    def op_hreim(self, st):
        x = self.cts[st["ins"][0]]
        rec = Rec("hreim", {}, x.level)
        self.bind(rec, "ct1", st["ins"][0])
        rec.keys["IP_"] = self.env.rot_key(2 * N - 1, x.level)

        def compute(_):
            import reim_ref
            re, im, _ = reim_ref.reim(self.o, x.level, x.limbs, rec.keys["IP_"])
            return {"out": self.close(rec, re, x.level, x.scale, 2 * x.value.real + 0j, None, False),
                    "out_im": self.close(rec, im, x.level, x.scale, 2 * x.value.imag + 0j, None, False, "out_im")}
        rec.compute = compute
        return rec

    def _rows(self, st, xs, target, names):
        """M rows of T weights -> (integer scalars [m][t] as residues under names(m, t), rational weights [m][t])"""
        level = xs[0].level
        res, wts = {}, []
        for m, row in enumerate(st["rows"]):
            wts.append([])
            for t, (c, x) in enumerate(zip(row, xs)):
                s, w = self.scalar(c, x, target, st["op"])
                res[names(m, t)] = self.residues(s, level)
                wts[-1].append(w)
        return res, wts

    def _consts(self, cs, target):
        ks = [rint_frac(as_frac(c) * target) for c in cs]
        return ks, [Fraction(k) / target for k in ks]

    def op_hlincomb(self, st):
        """rows = [[c_1 .. c_T]], const = c or None"""
        return self._lincombs(st, "hlincomb")

    def op_hmlincomb(self, st):
        """rows = M rows of T weights, consts = M constants or None"""
        return self._lincombs(st, "hmlincomb")

    def _lincombs(self, st, op):
        xs = [self.cts[n] for n in st["ins"]]
        level, target, multi = self.same(xs, op), self.target(st, xs), op == "hmlincomb"
        st = dict(st, op=op)
        cs = st.get("consts") if multi else (None if st.get("const") is None else [st["const"]])
        M, T, rs = len(st["rows"]), len(xs), int(st.get("rescale", 0))
        ov = {"terms": T, "rescale": rs}
        ov.update({"outputs": M, "ml_const": int(cs is not None)} if multi else {"lc_const": int(cs is not None)})
        rec = Rec(op, ov, level)
        for t, n in enumerate(st["ins"]):
            self.bind(rec, f"ct{t + 1}", n)
        res, wts = self._rows(st, xs, target, (lambda m, t: f"scale{m + 1}_{t + 1}") if multi else (lambda m, t: f"scale{t + 1}"))
        rec.consts.update(res)
        ks, kvals = self._consts(cs, target) if cs is not None else (None, [Fraction(0)] * M)
        if ks is not None:
            for m, k in enumerate(ks):
                rec.consts[f"const{m + 1}" if multi else "const"] = self.residues(k, level)

        def compute(_):
            from lincomb_ref import lincomb
            outs = {}
            for m in range(M):
                scales = [rec.consts[f"scale{m + 1}_{t + 1}" if multi else f"scale{t + 1}"] for t in range(T)]
                const = None if ks is None else rec.consts[f"const{m + 1}" if multi else "const"]
                out = lincomb(self.o, level, [x.limbs for x in xs], scales, const, bool(rs))
                value = sum(to_ld(w) * x.value for w, x in zip(wts[m], xs)) + to_ld(kvals[m])
                sym = poly_sum([(w, x.sym) for w, x in zip(wts[m], xs)], kvals[m])
                name = f"out{m + 1}" if multi else "out"
                outs[name] = self.close(rec, out, level, target, value, sym, bool(rs), name)
            return outs
        rec.compute = compute
        return rec

    def op_hclincomb(self, st):
        """weights = T complex weights, const = real c or None"""
        xs = [self.cts[n] for n in st["ins"]]
        level, target, rs = self.same(xs, "hclincomb"), self.target(st, xs), int(st.get("rescale", 0))
        rec = Rec("hclincomb", {"terms": len(xs), "cl_const": int(st.get("const") is not None), "rescale": rs}, level)
        wts = []
        for t, (n, x, c) in enumerate(zip(st["ins"], xs, st["weights"])):
            self.bind(rec, f"ct{t + 1}", n)
            (a, wa), (b, wb) = self.scalar(complex(c).real, x, target, "hclincomb"), self.scalar(complex(c).imag, x, target, "hclincomb")
            wts.append(CLD(to_ld(wa)) + CLD(1j) * CLD(to_ld(wb)))
            if self.broken == "swap_ab":
                a, b = b, a
            rec.consts[f"scale{t + 1}"], rec.consts[f"scale_im{t + 1}"] = self.residues(a, level), self.residues(b, level)
        kval = Fraction(0)
        if st.get("const") is not None:
            (k,), (kval,) = self._consts([st["const"]], target)
            rec.consts["const"] = self.residues(k, level)

        def compute(_):
            from clincomb_ref import clincomb
            T = len(xs)
            out = clincomb(self.o, level, [x.limbs for x in xs], [rec.consts[f"scale{t + 1}"] for t in range(T)],
                           [rec.consts[f"scale_im{t + 1}"] for t in range(T)], rec.consts.get("const"), bool(rs))
            value = sum(w * x.value for w, x in zip(wts, xs)) + to_ld(kval)
            return {"out": self.close(rec, out, level, target, value, None, bool(rs))}
        rec.compute = compute
        return rec

    def op_hdotadd(self, st):
        """pairs = [(name, name, c)], addends = [(name, c)], const = c or None; the sum's scale before the rescale is the first pair's product
        scale times S0"""
        pairs = [(self.cts[a], self.cts[b], c) for a, b, c in st["pairs"]]
        adds = [(self.cts[a], c) for a, c in st.get("addends", [])]
        level = self.same([x for a, b, _ in pairs for x in (a, b)] + [a for a, _ in adds], "hdotadd")
        target = pairs[0][0].scale * pairs[0][1].scale * st.get("S0", 1)
        rec = Rec("hdotadd", {"terms": len(pairs), "addends": len(adds), "da_scale": 1, "da_const": int(st.get("const") is not None)}, level)
        wts, uts = [], []
        for t, (a, b, c) in enumerate(st["pairs"]):
            self.bind(rec, f"ct{2 * t + 1}", a)
            self.bind(rec, f"ct{2 * t + 2}", b)
            x, y = pairs[t][0], pairs[t][1]
            s = rint_frac(as_frac(c) * target / (x.scale * y.scale))
            wts.append(Fraction(s) * x.scale * y.scale / target)
            rec.consts[f"scale{t + 1}"] = self.residues(s, level)
        for r, (a, c) in enumerate(st.get("addends", [])):
            self.bind(rec, f"ct{2 * len(pairs) + r + 1}", a)
            u, w = self.scalar(c, adds[r][0], target, "hdotadd")
            uts.append(w)
            rec.consts[f"addscale{r + 1}"] = self.residues(u, level)
        kval = Fraction(0)
        if st.get("const") is not None:
            (k,), (kval,) = self._consts([st["const"]], target)
            if self.broken == "post_rescale_const":
                k = rint_frac(as_frac(st["const"]) * target / self.o.moduli[level - 1])
            rec.consts["const"] = self.residues(k, level)
        rec.keys["IP_"] = self.env.relin_key(level)

        def compute(_):
            from dotadd_ref import dotadd
            out = dotadd(self.o, level, [(x.limbs, y.limbs) for x, y, _ in pairs], rec.keys["IP_"], [a.limbs for a, _ in adds],
                         [rec.consts[f"scale{t + 1}"] for t in range(len(pairs))], [rec.consts[f"addscale{r + 1}"] for r in range(len(adds))],
                         rec.consts.get("const"))
            value = sum(to_ld(w) * x.value * y.value for w, (x, y, _) in zip(wts, pairs)) + sum(to_ld(w) * a.value for w, (a, _) in zip(uts, adds))
            sym = poly_sum([(w, None if x.sym is None or y.sym is None else poly_mul(x.sym, y.sym)) for w, (x, y, _) in zip(wts, pairs)]
                           + [(w, a.sym) for w, (a, _) in zip(uts, adds)], kval)
            return {"out": self.close(rec, out, level, target, value + to_ld(kval), sym, True)}
        rec.compute = compute
        return rec

    def _plain(self, rec, name, slots, scale, ids):
        """a plaintext the op encodes on the device at the double `scale`; on the CPU the longdouble encoding of the same slots"""
        rec.encode[name] = (np.asarray(slots, dtype=np.complex128), float(scale), list(ids))

    def _limbs_of(self, rec, name, given):
        if given is not None and name in given:
            return given[name]
        if name in rec.raw:
            return rec.raw[name]
        slots, scale, ids = rec.encode[name]
        return R.encode_limbs(self.o, slots, scale, ids, R.fft_coeffs)

    def op_hplincomb(self, st):
        """weights = T slot vectors, addend = a slot vector or None, pt_scale: the scale of the weights (default: the chain's).  The addend sits at
        the sum's scale, which no device encoding holds: it is encoded on the CPU at the double nearest to it and written as it is"""
        xs = [self.cts[n] for n in st["ins"]]
        level, rs = self.same(xs, "hplincomb"), int(st.get("rescale", 0))
        ps = float(st.get("pt_scale", self.par["pt_scale"]))
        target = xs[0].scale * as_frac(ps)
        for x in xs:
            assert x.scale * as_frac(ps) == target, ("hplincomb", "scales differ")
        rec = Rec("hplincomb", {"terms": len(xs), "pl_addend": int(st.get("addend") is not None), "rescale": rs}, level)
        for t, (n, w) in enumerate(zip(st["ins"], st["weights"])):
            self.bind(rec, f"ct{t + 1}", n)
            self._plain(rec, f"pt{t + 1}", w, ps, range(level))
        aw = Fraction(0)
        if st.get("addend") is not None:
            f = float(target)
            aw = as_frac(f) / target
            rec.raw["pt0"] = R.encode_limbs(self.o, st["addend"], f, range(level), R.fft_coeffs)

        def compute(given):
            from plincomb_ref import plincomb
            pts = [self._limbs_of(rec, f"pt{t + 1}", given) for t in range(len(xs))]
            out = plincomb(self.o, level, [x.limbs for x in xs], pts, rec.raw.get("pt0"), bool(rs))
            value = sum(np.asarray(w, dtype=CLD) * x.value for w, x in zip(st["weights"], xs))
            if st.get("addend") is not None:
                value = value + to_ld(aw) * np.asarray(st["addend"], dtype=CLD)
            return {"out": self.close(rec, out, level, target, value, None, bool(rs))}
        rec.compute = compute
        return rec

    def op_hlintrans(self, st):
        """identity = 1: diags = [w_0 .. w_R], the plaintext of baby step r (rotation by r * baby) as the op is to receive it"""
        x = self.cts[st["ins"][0]]
        level, kb, ws = x.level, st.get("baby", 1), st["diags"]
        Rn, ps = len(ws) - 1, float(st.get("pt_scale", self.par["pt_scale"]))
        rec = Rec("hlintrans", {"rotations": Rn, "galois": rotation(kb), "identity": 1, "rescale": 0}, level)
        self.bind(rec, "ct1", st["ins"][0])
        keys = [self.env.rot_key(rotation(kb * r), level) for r in range(1, Rn + 1)]
        for r in range(Rn + 1):
            self._plain(rec, f"pt{r}", ws[r], ps, self.o.ext_ids(level))
            if r:
                rec.keys[f"IP_Rot{r}_"] = keys[r - 1]

        def compute(given):
            from identity_ref import lintrans_id
            pts = [self._limbs_of(rec, f"pt{r}", given) for r in range(Rn + 1)]
            out = lintrans_id(self.o, level, x.limbs, rotation(kb), keys, pts[1:], pts[0])
            value = sum(np.asarray(ws[r], dtype=CLD) * rot(x.value, kb * r) for r in range(Rn + 1))
            return {"out": self.close(rec, out, level, x.scale * as_frac(ps), value, None, False)}
        rec.compute = compute
        return rec

    def op_hrotsum(self, st):
        """input i = 1..G rotated left by i * giant"""
        xs = [self.cts[n] for n in st["ins"]]
        level, kg = self.same(xs, "hrotsum"), st["giant"]
        assert len({x.scale for x in xs}) == 1, ("hrotsum", "scales differ")
        rec = Rec("hrotsum", {"rotations": len(xs), "galois": rotation(kg)}, level)
        keys = [self.env.rot_key(rotation(kg * i), level) for i in range(1, len(xs) + 1)]
        for i, n in enumerate(st["ins"], 1):
            self.bind(rec, f"ct{i}", n)
            rec.keys[f"IP_Rot{i}_"] = keys[i - 1]

        def compute(_):
            from rotsum_ref import rotsum
            out = rotsum(self.o, level, [x.limbs for x in xs], rotation(kg), keys)
            value = sum(rot(x.value, kg * i) for i, x in enumerate(xs, 1))
            return {"out": self.close(rec, out, level, xs[0].scale, value, None, False)}
        rec.compute = compute
        return rec

    def op_hbsgs(self, st):
        """identity = 1: diags[i][r], i = 0..G, r = 0..R: the plaintext of giant group i (rotation by i * giant) and baby step r (rotation by
        r * baby) as the op is to receive it"""
        x = self.cts[st["ins"][0]]
        level, kb, kg, ws = x.level, st.get("baby", 1), st["giant"], st["diags"]
        G, Rn, ps = len(ws) - 1, len(ws[0]) - 1, float(st.get("pt_scale", self.par["pt_scale"]))
        rec = Rec("hbsgs", {"rotations": Rn, "giants": G, "galois": rotation(kb), "galois_giant": rotation(kg), "identity": 1, "rescale": 0}, level)
        self.bind(rec, "ct1", st["ins"][0])
        baby = [self.env.rot_key(rotation(kb * r), level) for r in range(1, Rn + 1)]
        giant = [self.env.rot_key(rotation(kg * i), level) for i in range(1, G + 1)]
        ids = self.o.ext_ids(level)
        name = lambda i, r: f"pt0_{i}" if r == 0 else f"ptg{r}" if i == 0 else f"pt{(i - 1) * Rn + r}"
        for i in range(G + 1):
            for r in range(Rn + 1):
                self._plain(rec, name(i, r), ws[i][r], ps, ids)
        for r in range(1, Rn + 1):
            rec.keys[f"IP_Rot{r}_"] = baby[r - 1]
        for i in range(1, G + 1):
            rec.keys[f"IP_Giant{i}_"] = giant[i - 1]

        def compute(given):
            from identity_ref import bsgs_id
            pt = lambda i, r: self._limbs_of(rec, name(i, r), given)
            out = bsgs_id(self.o, level, x.limbs, rotation(kb), rotation(kg), baby, giant,
                          [[pt(i, r) for r in range(1, Rn + 1)] for i in range(1, G + 1)], [pt(i, 0) for i in range(G + 1)],
                          [pt(0, r) for r in range(1, Rn + 1)])
            value = sum(rot(sum(np.asarray(ws[i][r], dtype=CLD) * rot(x.value, kb * r) for r in range(Rn + 1)), kg * i) for i in range(G + 1))
            return {"out": self.close(rec, out, level, x.scale * as_frac(ps), value, None, False)}
        rec.compute = compute
        return rec

    # ---- running
    def prepare(self, st):
        rec = getattr(self, "op_" + st["op"])(st)
        rec.out_names = st["outs"] if isinstance(st["outs"], dict) else {"out": st["outs"]}      # {the op's output name: the program's name}
        return rec

    def finish(self, rec, plaintexts=None):
        """run the step through its reference; plaintexts: {buffer name: limbs} read back from the device, where the op encoded them"""
        got = rec.compute(plaintexts)
        for out, name in rec.out_names.items():
            rec.outs[out] = self.cts[name] = got[out]
            self.producer[name] = (rec, out)
        self.recs.append(rec)
        return rec

    def run(self, steps):
        for st in steps:
            self.finish(self.prepare(st))
        return self


# ============================================================================================================================
# the programs
# ============================================================================================================================
def uniform_disc(seed, count=1):
    """`count` slot vectors with |z_j| <= 1"""
    rng = np.random.default_rng(seed)
    out = [np.sqrt(rng.uniform(0, 1, NSLOT)) * np.exp(2j * np.pi * rng.uniform(0, 1, NSLOT)) for _ in range(count)]
    return out[0] if count == 1 else out


P_COEFFS = [0.3125, -0.71, 0.44, 0.93, -0.58, 0.27, -0.86, 0.65]      # a_0 .. a_7, real, |a_k| <= 1; a_0 is split below
P_EXTRA = 0.25                                                        # the part of the constant term that hdotadd's constant adds


def program_P(chain):
    """p(z) = sum_k a_k z^k + P_EXTRA as q_lo(z) + z^4 q_hi(z) + P_EXTRA.  z at (7, D): z2 at (6, D^2 / q_6); hlincomb with the integer scalar D
    and rescale = 1 brings z to exactly that level and scale; z3 = z1 z2 and z4 = z2^2 at (5, D1^2 / q_5); hmlincomb with the scalars rint(D1)
    and rescale = 1 carries z1 and z2 beside them (the weights rint(D1) / D1 are part of the statement); q_lo and q_hi at scale D2 S, no rescale;
    hdotadd: q_hi z4 at D2 S D2, q_lo times rint(D2) beside it, the constant at that scale, one rescale: level 4"""
    a = P_COEFFS
    D = CHAINS[chain]["ct_scale"]
    return [
        dict(op="hsquare", ins=["z"], outs="z2"),
        dict(op="hlincomb", ins=["z"], outs="z1", rows=[[1]], target=Fraction(D) * D, rescale=1),
        dict(op="hmult", ins=["z1", "z2"], outs="z3"),
        dict(op="hsquare", ins=["z2"], outs="z4"),
        dict(op="hmlincomb", ins=["z1", "z2"], outs={"out1": "y1", "out2": "y2"}, rows=[[1, 0], [0, 1]], target="square", rescale=1),
        dict(op="hmlincomb", ins=["y1", "y2", "z3"], outs={"out1": "q_lo", "out2": "q_hi"}, rows=[a[1:4], a[5:8]], consts=[a[0], a[4]]),
        dict(op="hdotadd", pairs=[("q_hi", "z4", 1)], addends=[("q_lo", 1)], const=P_EXTRA, S0=1, outs="out"),
    ]


def run_P(chain, z, seed, broken=None):
    m = Machine(chain, broken)
    m.put("z", z, seed)
    for st in program_P(chain):
        if st.get("target") == "square":      # the scale of the products beside it: the input scale squared
            st = dict(st, target=m.cts[st["ins"][0]].scale ** 2)
        m.finish(m.prepare(st))
    return m


def statement_P(m):
    """p evaluated by numpy.polynomial in longdouble at the input's slots, with the rational coefficients the integer scalars stand for"""
    from numpy.polynomial import polynomial as npoly
    sym = m.cts["out"].sym
    assert len(sym) == 8
    coeffs = np.array([to_ld(c) for c in sym], dtype=LD)
    want = np.array(P_COEFFS, dtype=LD)
    want[0] += LD(P_EXTRA)
    assert float(np.abs(coeffs - want).max()) < 2.0 ** -15      # the rounded coefficients are the chosen ones to the precision of S
    return npoly.polyval(m.cts["z"].value, coeffs)


M_DIAGS, M_GIANT, M_BABY = 6, 3, 3      # six diagonals as baby steps 0..2 and giant groups 0..1: d = 3 i + r


def inputs_M():
    """(the six diagonals, w, v, c), all of modulus at most 1"""
    vs = uniform_disc(303, M_DIAGS + 3)
    return vs[:M_DIAGS], vs[M_DIAGS], vs[M_DIAGS + 1], vs[M_DIAGS + 2]


def program_M(chain, broken=None):
    """both routes to y = A z, a rescale of each, then w (.) y + v (.) z + c on route 1's y"""
    d, w, v, c = inputs_M()
    G = M_DIAGS // M_BABY
    pre = (lambda x, k: x) if broken == "unrotated" else (lambda x, k: np.roll(x, k))
    ps = int(CHAINS[chain]["pt_scale"])
    steps = [dict(op="hbsgs", ins=["z"], outs="yA", giant=M_GIANT,
                  diags=[[pre(d[M_BABY * i + r], M_GIANT * i) for r in range(M_BABY)] for i in range(G)]),
             dict(op="hrescale", ins=["yA"], outs="yA_r"),
             dict(op="hrotate", ins=["z"], outs="z_back", rot=-M_GIANT)]
    for i in range(1, G + 1):      # route 2: group i rotated by 3 i holds the diagonals 3 (i - 1) + r of the vector rotated back by 3
        steps.append(dict(op="hlintrans", ins=["z_back"], outs=f"u{i}", diags=[pre(d[M_BABY * (i - 1) + r], M_GIANT * i) for r in range(M_BABY)]))
    steps += [dict(op="hrotsum", ins=[f"u{i}" for i in range(1, G + 1)], outs="yB", giant=M_GIANT),
              dict(op="hrescale", ins=["yB"], outs="yB_r"),
              dict(op="hlincomb", ins=["z"], outs="z_down", rows=[[1]], S=ps, rescale=1),      # z at y's level and scale: the scalar is the plaintext scale
              dict(op="hplincomb", ins=["yA_r", "z_down"], outs="out", weights=[w, v], addend=c)]
    return steps


def statement_M(z):
    """(y, w (.) y + v (.) z + c) with y_j = sum_d diag_d[j] z[(j + d) mod n], in longdouble"""
    d, w, v, c = inputs_M()
    z = np.asarray(z, dtype=CLD)
    j = np.arange(NSLOT)
    y = sum(np.asarray(d[k], dtype=CLD) * z[(j + k) % NSLOT] for k in range(M_DIAGS))
    return y, np.asarray(w, dtype=CLD) * y + np.asarray(v, dtype=CLD) * z + np.asarray(c, dtype=CLD)


C_WEIGHTS = {"C_identity": ((1, 1j), 0.0), "C_generic": ((0.61 - 0.37j, -0.28 + 0.83j), 0.4375)}


def program_C(name, chain):
    """the sum is scaled by S = the ciphertext scale, so the rescale brings the scale back to about one modulus"""
    (c1, c2), k = C_WEIGHTS[name]
    return [dict(op="hreim", ins=["z"], outs={"out": "re", "out_im": "im"}),
            dict(op="hclincomb", ins=["re", "im"], outs="lin", weights=[c1 / 2, c2 / 2], const=k, S=CHAINS[chain]["ct_scale"], rescale=1),
            dict(op="hrotate", ins=["lin"], outs="out", conj=True)]


def statement_C(name, z):
    """conj((a + b i) Re z + (c + d i) Im z + k); the weights are dyadic to the precision of S or rounded: the rational weights differ from these
    by at most 2^-S's bits, which the test holds the tracked value to"""
    (c1, c2), k = C_WEIGHTS[name]
    z = np.asarray(z, dtype=CLD)
    return np.conj(CLD(c1) * z.real + CLD(c2) * z.imag + LD(k))


def run_program(name, chain, broken=None, z=None, seed=None):
    """the program through the interpreter: (machine, {what: (name of the ciphertext, statement)})"""
    z = uniform_disc(Z_SEED[name]) if z is None else z
    seed = Z_SEED[name] if seed is None else seed
    if name.startswith("P"):      # "P_copy1", "P_rewritten": the same program on another input (the batch and graph tests of the GPU side)
        m = run_P(chain, z, seed, broken)
        return m, {"out": statement_P(m)}
    m = Machine(chain, broken)
    m.put("z", z, seed, CHAINS[chain]["M_scale"] if name == "M" else None)
    if name == "M":
        m.run(program_M(chain, broken))
        y, out = statement_M(z)
        return m, {"yA_r": y, "yB_r": y, "out": out}
    m.run(program_C(name, chain))
    return m, {"out": statement_C(name, z)}


def slot_error(m, name, want):
    ct = m.cts[name]
    return float(np.abs(m.env.slots_of(ct.limbs, ct.level, ct.scale) - want).max())


def program_error(name, chain, broken=None):
    """max over the program's statements of max |slots(dec) - statement|"""
    m, wants = run_program(name, chain, broken)
    return max(slot_error(m, n, w) for n, w in wants.items())


def print_reference_errors():
    for name, chain in REF_ERR:
        print(f'    ("{name}", "{chain}"): {program_error(name, chain):.3g},')
