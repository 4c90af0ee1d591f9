"""The composed programs of tests/program_ref.py through the CPU references alone (no GPU): every program on both chains meets its slot statement
within the recorded error, the interpreter's two conditions (equal levels and scales under every addition, headroom under Q_level / 4) hold at every
step (they are assertions inside the interpreter: a run that returns has met them), and one negative test per convention shows that the statement
can fail: each breaks what the pipeline is fed, never the statement, and must move the error by at least 10^3 x the recorded one."""
from fractions import Fraction

import numpy as np
import pytest

import program_ref as P

PROGRAMS = ["P", "P_copy1", "P_rewritten", "M", "C_identity", "C_generic"]
CHAINS = ["mont32", "generic"]
_runs = {}


def run(name, chain):
    """each program once per process"""
    if (name, chain) not in _runs:
        _runs[(name, chain)] = P.run_program(name, chain)
    return _runs[(name, chain)]


@pytest.mark.parametrize("chain", CHAINS)
@pytest.mark.parametrize("name", PROGRAMS)
def test_the_program_meets_its_statement_within_the_recorded_error(name, chain):
    m, wants = run(name, chain)
    err = max(P.slot_error(m, n, w) for n, w in wants.items())
    rec = P.REF_ERR[(name, chain)]
    print(f"{name} {chain}: max |slots - statement| = {err:.4g} (recorded {rec:.4g})")
    assert rec > 0 and rec / 2 <= err <= 2 * rec
    for n, w in wants.items():      # the value the interpreter tracked step by step is the closed-form statement
        assert float(np.abs(m.cts[n].value - w).max()) < 2.0 ** -18, n


@pytest.mark.parametrize("chain", CHAINS)
def test_levels_and_scales_of_the_polynomial(chain):
    """the bookkeeping the program relies on, said once in plain numbers: every power meets its partners at one level and one scale"""
    m, _ = run("P", chain)
    q, c = m.o.moduli, m.cts
    D = Fraction(P.CHAINS[chain]["ct_scale"])
    D1 = D * D / q[6]
    D2 = D1 * D1 / q[5]
    assert [(c[n].level, c[n].scale) for n in ("z", "z2", "z1")] == [(7, D), (6, D1), (6, D1)]
    assert all((c[n].level, c[n].scale) == (5, D2) for n in ("z3", "z4", "y1", "y2"))
    assert all((c[n].level, c[n].scale) == (5, D2 * P.CHAINS[chain]["S"]) for n in ("q_lo", "q_hi"))
    assert (c["out"].level, c["out"].scale) == (4, D2 * P.CHAINS[chain]["S"] * D2 / q[4])
    assert [r.op for r in m.recs] == ["hsquare", "hlincomb", "hmult", "hsquare", "hmlincomb", "hmlincomb", "hdotadd"]
    assert m.recs[1].consts["scale1"] == [int(D) % q[j] for j in range(7)]      # T = 1, the scalar is the integer scale itself


@pytest.mark.parametrize("chain", CHAINS)
def test_both_routes_of_the_matrix_give_the_same_slots(chain):
    m, wants = run("M", chain)
    a, b = (m.env.slots_of(m.cts[n].limbs, m.cts[n].level, m.cts[n].scale) for n in ("yA_r", "yB_r"))
    diff = float(np.abs(a - b).max())
    print(f"M {chain}: max |route 1 - route 2| = {diff:.4g}")
    assert diff <= 2 * 2 * P.REF_ERR[("M", chain)]      # each within twice the recorded error of the one statement
    assert float(np.abs(wants["yA_r"]).max()) > 1       # a signal
    assert [r.op for r in m.recs] == ["hbsgs", "hrescale", "hrotate", "hlintrans", "hlintrans", "hrotsum", "hrescale", "hlincomb", "hplincomb"]


@pytest.mark.parametrize("chain", CHAINS)
def test_the_weights_one_and_i_return_the_input(chain):
    m, wants = run("C_identity", chain)
    z = P.uniform_disc(P.Z_SEED["C_identity"])
    assert np.array_equal(wants["out"], np.conj(z).astype(P.CLD))
    assert np.array_equal(m.cts["lin"].value, m.cts["z"].value)      # S / 2 is an integer: the weights are exactly 1/2 and i/2


NEGATIVE = [("M", "unrotated"), ("C_generic", "swap_ab"), ("C_identity", "swap_ab"), ("P", "post_rescale_const")]


@pytest.mark.parametrize("chain", CHAINS)
@pytest.mark.parametrize("name,broken", NEGATIVE)
def test_a_broken_convention_fails_the_statement_by_orders_of_magnitude(name, broken, chain):
    """diagonals not pre-rotated; b_t and a_t swapped; a constant scaled by the scale after the rescale instead of the scale before it"""
    err = P.program_error(name, chain, broken)
    rec = P.REF_ERR[(name, chain)]
    print(f"{name} {chain} {broken}: max |slots - statement| = {err:.4g}, {err / rec:.3g} x the recorded {rec:.4g}")
    assert err >= 1e3 * rec


def test_the_interpreter_refuses_an_addition_across_levels_and_a_value_without_headroom():
    m = P.Machine("generic")
    z = P.uniform_disc(1)
    m.put("z", z, 1)
    m.finish(m.prepare(dict(op="hsquare", ins=["z"], outs="z2")))
    with pytest.raises(AssertionError, match="levels differ"):
        m.prepare(dict(op="hlincomb", ins=["z", "z2"], outs="s", rows=[[1, 1]]))
    m.put("zz", z, 2, scale=1 << 30)
    with pytest.raises(AssertionError, match="scales differ"):
        m.prepare(dict(op="hrotsum", ins=["z", "zz"], outs="s", giant=1))
    with pytest.raises(AssertionError, match="headroom"):
        m.finish(m.prepare(dict(op="hlincomb", ins=["z"], outs="big", rows=[[1]], S=1 << 220)))

