"""Every op that switches keys, at EVERY level, at the ring sizes where the capability table (homulator_amd/csrc/hm_caps.h) gives the fused forms:
the base conversion inside the transform's first pass, the key product handing over the first inverse pass, the 8-coefficient geometry and the
one-launch transform exist at N = 2^15 and 2^16 only, so the level grids at N = 2^13 (test_every_level_small_ring and the 13-limb grids of the ops'
own files) never reach them.  Bit for bit against the references the ops' own files use (tests/*_ref.py), on the ops' synthetic inputs:
 A. N = 2^15, L = 13, alpha in {2, 3, 5, 13} on the default chain, {3, 13} on chain_bits = 60 and 5 on chain_bits = 36 (the generic back-end),
    every level: beta = 1 .. 7, short and one-limb last digits, l <= alpha, the switch to the fallback route between beta = 4 and 5; fuse = False
    as well at l = 2, alpha, alpha + 1 and 13, so that a mismatch says which plan is wrong; at alpha = 3, l = 2, 4, 7, 13 a batch of three as well
    (an odd number of outputs under two outputs per workgroup, one evaluation key for the batch), copies 0 and 2;
 B. N = 2^15, L = alpha = 28, l = 15, 16, 17, 28: the last one-group digit, one full input group, two groups, the top; and N = 2^16 at l = 17,
    where a digit above 15 limbs keeps a conversion launch of its own;
 E. the element-wise ops with rescale = 1 and their constant on, pmult with the product transforms, hrescale and hmodraise at every level.
Every fused run's plan is the route recorded in tests/golden/level_sweep_routes.json (launch kinds, ModUp conversion launches, second_pass_only
transforms, output level), which tests/test_host_level_sweep_plan.py holds to the planner and to the rules of the routes: the sweep cannot pass by
running the plain plan."""
import importlib.util
import json
import os

import numpy as np
import pytest

from homulator_amd import host
from oracle.homoracle import Oracle

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
_spec = importlib.util.spec_from_file_location("make_level_sweep_routes", os.path.join(HERE, "golden", "make_level_sweep_routes.py"))
gen = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(gen)

GOLDEN = json.load(open(gen.PATH))["routes"]
SEED = host.SEED
CHAIN_OF = {0: "mont32", 60: "survey", 36: 36}      # chain_bits -> the oracle's chain
REFUSAL = "Rescale needs at least two limbs"
_oracles = {}


def oracle(logN, L, alpha, bits):
    key = (logN, L, alpha, bits)
    if key not in _oracles:
        _oracles[key] = Oracle(logN, L, alpha, chain=CHAIN_OF[bits])
        _oracles[key].set_threads(16)
    return _oracles[key]


# ============================================================================================================================
# the references: name -> f(o, l, copy) = [(c0, c1) per output], on the synthetic streams of op `copy` of a batch
# ============================================================================================================================
def _hoisted(o, ell, c):
    from hoisted_ref import hoisted_rotations
    from identity_ref import lintrans_id_inputs
    ct, keys, _, _ = lintrans_id_inputs(o, ell, gen.R_HOIST, SEED, copy=c)      # rotation r's key is hlintrans's
    return hoisted_rotations(o, ell, ct, 5, keys)


def _lintrans(identity, rescale):
    def ref(o, ell, c):
        from identity_ref import lintrans_id, lintrans_id_inputs
        from lintrans_ref import lintrans
        from rescale_ref import lintrans_rescaled
        ct, keys, pts, pt0 = lintrans_id_inputs(o, ell, 3, SEED, copy=c)
        if rescale:
            return [lintrans_rescaled(o, ell, ct, 5, keys, pts)]
        return [lintrans_id(o, ell, ct, 5, keys, pts, pt0) if identity else lintrans(o, ell, ct, 5, keys, pts)]
    return ref


def _dot(o, ell, c):
    from dot_ref import dot, synthetic_inputs
    return [dot(o, ell, *synthetic_inputs(o, ell, 3, SEED, copy=c))]


def _rotsum(rescale):
    def ref(o, ell, c):
        from rescale_ref import rotsum_rescaled
        from rotsum_ref import rotsum, synthetic_inputs
        cts, keys = synthetic_inputs(o, ell, 3, SEED, copy=c)
        return [(rotsum_rescaled if rescale else rotsum)(o, ell, cts, 5, keys)]
    return ref


def _bsgs(identity, rescale):
    def ref(o, ell, c):
        from bsgs_ref import bsgs, synthetic_inputs
        from identity_ref import bsgs_id, bsgs_id_inputs
        from rescale_ref import bsgs_rescaled
        R, G = 2, 2
        ct, baby, giant, pts = synthetic_inputs(o, ell, R, G, SEED, copy=c)
        if identity:      # the giant element behind an identity step is g^(R + 1)
            return [bsgs_id(o, ell, ct, 5, pow(5, R + 1, 2 * o.N), baby, giant, pts, *bsgs_id_inputs(o, ell, R, G, SEED, copy=c))]
        return [(bsgs_rescaled if rescale else bsgs)(o, ell, ct, 5, pow(5, R, 2 * o.N), baby, giant, pts)]
    return ref


def _square(o, ell, c):
    from square_ref import square, synthetic_constants, synthetic_inputs
    return [square(o, ell, *synthetic_inputs(o, ell, SEED, copy=c), *synthetic_constants(o, ell, SEED, 1, 1))]


def _muladd(o, ell, c):
    from muladd_ref import muladd, synthetic_constants, synthetic_inputs
    ct1, ct2, addends, evk = synthetic_inputs(o, ell, SEED, 2, copy=c)
    return [muladd(o, ell, ct1, ct2, evk, addends, *synthetic_constants(o, ell, SEED, 2, 1, 1))]


def _dotadd(o, ell, c):
    from dotadd_ref import dotadd, synthetic_constants, synthetic_inputs
    pairs, addends, evk = synthetic_inputs(o, ell, SEED, 3, 2, copy=c)
    return [dotadd(o, ell, pairs, evk, addends, *synthetic_constants(o, ell, SEED, 3, 2, 1, 1))]


def _reim(o, ell, c):
    from reim_ref import reim, synthetic_input
    re, im, _ = reim(o, ell, *synthetic_input(o, ell, SEED, copy=c))
    return [re, im]


def _lincomb(o, ell, c):
    from lincomb_ref import lincomb, synthetic_constants, synthetic_inputs
    return [lincomb(o, ell, synthetic_inputs(o, ell, SEED, 3, copy=c), *synthetic_constants(o, ell, SEED, 3, 1), rescale=True)]


def _clincomb(o, ell, c):
    from clincomb_ref import clincomb, synthetic_constants
    from lincomb_ref import synthetic_inputs
    return [clincomb(o, ell, synthetic_inputs(o, ell, SEED, 3, copy=c), *synthetic_constants(o, ell, SEED, 3, 1), rescale=True)]


def _plincomb(o, ell, c):
    from lincomb_ref import synthetic_inputs
    from plincomb_ref import plincomb, synthetic_plaintexts
    return [plincomb(o, ell, synthetic_inputs(o, ell, SEED, 3, copy=c), *synthetic_plaintexts(o, ell, SEED, 3, 1, copy=c), rescale=True)]


def _mlincomb(o, ell, c):
    from mlincomb_ref import mlincomb, synthetic_constants, synthetic_inputs
    return mlincomb(o, ell, synthetic_inputs(o, ell, SEED, 3, copy=c), *synthetic_constants(o, ell, SEED, 3, 5, 1), rescale=True)


def _pmult(o, ell, c):
    from rescale_ref import pmult_rescaled
    return [pmult_rescaled(o, ell, o.synth_ct(ell, SEED), o.fill_uniform(list(range(ell)), SEED + 4000))]


def _rescale(o, ell, c):
    from rescale_ref import rescale_ct
    return [rescale_ct(o, ell, o.synth_ct(ell, SEED))]


def _modraise(o, T, c):
    from modraise_ref import modraise_ct
    return [modraise_ct(o, T, o.synth_ct(1, SEED))]


REFERENCE = {
    "hrotate_hoisted": _hoisted, "hlintrans": _lintrans(False, False), "hlintrans_id": _lintrans(True, False), "hdot": _dot, "hrotsum": _rotsum(False),
    "hbsgs": _bsgs(False, False), "hbsgs_id": _bsgs(True, False), "hsquare": _square, "hmuladd": _muladd, "hdotadd": _dotadd, "hreim": _reim,
    "hlintrans_rescale": _lintrans(False, True), "hrotsum_rescale": _rotsum(True), "hbsgs_rescale": _bsgs(False, True),
    "hlincomb": _lincomb, "hclincomb": _clincomb, "hplincomb": _plincomb, "hmlincomb": _mlincomb, "pmult": _pmult, "hrescale": _rescale,
    "hmodraise": _modraise,
}


# ============================================================================================================================
# one point
# ============================================================================================================================
def run(pt, bits, fuse=True, batch=1, copies=(0,)):
    """the point on the GPU: ({copy: [(c0, c1) per output]}, the plan's route)"""
    extra = dict({"chain_bits": bits} if bits else {}, **({"batch": batch} if batch > 1 else {}))
    op = gen.make_op(pt, backend=host.BACKEND_HIP, fuse=fuse, **extra)
    try:
        if bits:
            assert op.backend_counter("arith") == 1
        op.execute(1)
        outs = {c: [(op.read(f"{n}.c0", copy=c), op.read(f"{n}.c1", copy=c)) for n in gen.row_of(pt[1]).outputs] for c in copies}
        return outs, gen.route(op, pt[1])
    finally:
        op.close()


def assert_outputs(got, exp, level, what):
    """every output, both components, every limb"""
    assert len(got) == len(exp), what
    for i, (g, e) in enumerate(zip(got, exp)):
        for k in range(2):
            assert g[k].shape == e[k].shape and g[k].shape[0] == level, (what, i, k, g[k].shape, e[k].shape)
            if not np.array_equal(g[k], e[k]):
                raise AssertionError((what, f"output {i} c{k} differs in limbs", [j for j in range(level) if not np.array_equal(g[k][j], e[k][j])]))


def check_point(pt, bits):
    """the fused run against the reference and the recorded route; the unfused run and the batch of three where the grid has them"""
    grid, name, _, logN, L, alpha, ell = pt
    row, what = gen.row_of(name), (gen.key(pt), f"chain_bits={bits}")
    if row.rescales and ell == 1:
        with pytest.raises(host.HostError, match=REFUSAL):
            gen.make_op(pt, backend=host.BACKEND_HIP, **({"chain_bits": bits} if bits else {}))
        return
    level = ell - row.rescales
    o = oracle(logN, L, alpha, bits)
    exp = REFERENCE[name](o, ell, 0)
    outs, route = run(pt, bits)
    assert route == GOLDEN[gen.key(pt)], (what, route)
    if "level" in route:
        assert route["level"] == level, what
    assert_outputs(outs[0], exp, level, (what, "fused"))
    if grid == "A" and ell in gen.unfused_levels(alpha):
        outs, route = run(pt, bits, fuse=False)
        assert not set(route["kinds"]) & set(gen.MERGED_KINDS) and "NTT_IP" not in route["kinds"], (what, route)
        assert_outputs(outs[0], exp, level, (what, "unfused"))
    if grid == "A" and (alpha, bits) == (gen.BATCH_ALPHA, 0) and ell in gen.BATCH_LEVELS:
        outs, route = run(pt, bits, batch=gen.BATCH, copies=(0, gen.BATCH - 1))
        assert route == GOLDEN[gen.key(pt)], (what, "batch", route)
        assert_outputs(outs[0], exp, level, (what, "batch of 3, copy 0"))
        assert_outputs(outs[gen.BATCH - 1], REFERENCE[name](o, ell, gen.BATCH - 1), level, (what, "batch of 3, copy 2"))
    if grid == "B" and name in gen.OWN_MODUP:
        assert route["modup_bconv"] == 0, (what, "the wide digit goes inside the first pass")
    if grid == "B16":
        assert route["modup_bconv"] >= 1, (what, "N = 2^16: a digit above 15 limbs keeps its conversion launch")


# ============================================================================================================================
# the grids.  hbsgs's reference takes seconds at the higher levels: its variants are parametrized over the level too
# ============================================================================================================================
BY_LEVEL = [n for n, r in gen.ROWS.items() if r.op == "hbsgs"]
A_LEVELS = list(range(1, gen.A_L + 1))
A_LOOPED = [(n, a, b) for n in gen.ROWS if n not in BY_LEVEL for a, b in gen.A_RUNS]
A_SINGLE = [(n, a, b, ell) for n in BY_LEVEL for a, b in gen.A_RUNS for ell in A_LEVELS]
B_LOOPED = [(n, b) for n in gen.ROWS if n not in BY_LEVEL for b in gen.B_CHAINS]
B_SINGLE = [(n, b, ell) for n in BY_LEVEL for b in gen.B_CHAINS for ell in gen.B_LEVELS]
E_RUNS = [(n, b) for n in list(gen.ELEMENTWISE) + ["hmodraise"] for b in (0, 60)]


def point_a(name, alpha, ell):
    return ("A", name, gen.CFG15, 15, gen.A_L, alpha, ell)


def point_b(name, ell):
    return ("B", name, gen.CFG15, 15, gen.B_L, gen.B_ALPHA, ell)


def test_the_parametrization_covers_every_point_of_the_grids():
    a = {(n, al, b, ell) for n, al, b in A_LOOPED for ell in A_LEVELS} | set(A_SINGLE)
    assert a == {(n, al, b, ell) for n in gen.ROWS for al, b in gen.A_RUNS for ell in A_LEVELS} and len(a) == 14 * 7 * 13
    b = {(n, c, ell) for n, c in B_LOOPED for ell in gen.B_LEVELS} | set(B_SINGLE)
    assert b == {(n, c, ell) for n in gen.ROWS for c in gen.B_CHAINS for ell in gen.B_LEVELS} and len(b) == 14 * 2 * 4
    assert len(A_LOOPED) == 77 and len(A_SINGLE) == 273 and len(B_LOOPED) == 22 and len(B_SINGLE) == 24 and len(E_RUNS) == 14
    assert {p for p in gen.points() if p[0] == "A"} == {point_a(n, al, ell) for n, al, _, ell in a}
    assert {p for p in gen.points() if p[0] == "B"} == {point_b(n, ell) for n, _, ell in b}
    assert set(REFERENCE) == {p[1] for p in gen.points()}


@pytest.mark.parametrize("name,alpha,bits", A_LOOPED)
def test_every_level_fused_ring(name, alpha, bits):
    for ell in A_LEVELS:
        check_point(point_a(name, alpha, ell), bits)


@pytest.mark.parametrize("name,alpha,bits,ell", A_SINGLE)
def test_every_level_fused_ring_bsgs(name, alpha, bits, ell):
    check_point(point_a(name, alpha, ell), bits)


@pytest.mark.parametrize("name,bits", B_LOOPED)
def test_wide_digits(name, bits):
    for ell in gen.B_LEVELS:
        check_point(point_b(name, ell), bits)


@pytest.mark.parametrize("name,bits,ell", B_SINGLE)
def test_wide_digits_bsgs(name, bits, ell):
    check_point(point_b(name, ell), bits)


@pytest.mark.parametrize("name", gen.B16_ROWS)
def test_wide_digit_at_the_larger_ring(name):
    check_point(("B16", name, gen.CFG16, 16, gen.B_L, gen.B_ALPHA, gen.B16_LEVEL), 0)


@pytest.mark.parametrize("name,bits", E_RUNS)
def test_elementwise_ops_and_level_changes_at_every_level(name, bits):
    """l = 1 .. 13 (hmodraise: raise_to = 2 .. 13 from level 1); the ops that rescale refuse l = 1"""
    for pt in gen.points():
        if pt[1] == name:
            check_point(pt, bits)
