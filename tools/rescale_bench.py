"""The rescale against what it replaces on the same build, interleaved on one device (default config_4 45/35/15), every op at
the largest batch that fits the 16-bit limb index (searched downwards from --batch-max):
    (a) pmult rescale = 1 with pass (4p) on      against   the same with fuse_pmul_rescale = 0 (three launches of kernels the parent has)
    (b) hrescale, and pmult + hrescale as two ops   against   (a)
    (c) hlintrans / hbsgs with rescale = 1        against   the same op with rescale = 0 followed by hrescale
plus the per-launch stage times of pmult rescale = 1, pass on and off.  --only-base: hmult, pmult and hlintrans / hbsgs with rescale = 0 only (a build
without the rescale runs this too: parent / head / parent).  Appends what it prints to --out.
    python3 tools/rescale_bench.py [--rounds 5] [--iters 10] [--warmup-rounds 0] [--batch-max 24] [--only-base] [--only-pmult] [--chain-bits 60] [--label head] [--out profiles/rescale.txt]"""
import argparse
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from homulator_amd import host  # noqa: E402


def largest_batch(cfg, name, L, ell, alpha, bmax, ov):
    """limb-polys are addressed by 16-bit indices over the whole batch: the largest batch <= bmax that builds (bmax is printed when it is reached)"""
    b = bmax
    while True:
        op = host.Op(cfg, name, L, ell, alpha, overrides=dict(ov, batch=b))
        try:
            op.execute(3)   # first-use tables
            return op, b
        except host.HostError as e:
            op.close()
            if "exceeds 65535" not in str(e) or b == 1:
                raise
            b -= 1


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cfg", default="config_4.cfg")
    ap.add_argument("--levels", default="45,35,15")
    ap.add_argument("--batch-max", type=int, default=24)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--warmup-rounds", type=int, default=0, help="untimed interleaved rounds in front of the timed ones")
    ap.add_argument("--only-base", action="store_true")
    ap.add_argument("--only-pmult", action="store_true", help="(a) alone: one form of the transforms at a time (HOMULATOR_NTT_FUSED_SMALL / _SMALL_LIMBS pick it)")
    ap.add_argument("--chain-bits", type=int, default=0, help="60: the generic arithmetic back-end on the 60-bit chain (default: mont32)")
    ap.add_argument("--label", default="")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    L, ell, alpha = (int(x) for x in a.levels.split(","))
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)
    fmt = lambda v: ", ".join(f"{x:.1f}" for x in v)
    med, spread = statistics.median, lambda v: max(v) - min(v)
    warm = f", after {a.warmup_rounds} untimed round(s)" if a.warmup_rounds else ""
    say(f"# {a.label + ': ' if a.label else ''}{a.cfg} {L} {ell} {alpha}, every op at its largest batch <= {a.batch_max} (us per op of the batch, "
        f"median of {a.rounds} interleaved rounds x {a.iters} iterations{warm}; spread = max - min over the rounds)")
    chain = {"chain_bits": a.chain_bits} if a.chain_bits else {}
    make = lambda name, ov, lvl=ell: largest_batch(a.cfg, name, L, lvl, alpha, a.batch_max, dict(ov, **chain))

    def timed(ops):
        """ops: {name: (op, batch)}; one list of per-op times per name, the ops interleaved round by round"""
        t = {k: [] for k in ops}
        for r in range(a.warmup_rounds + a.rounds):
            for k, (op, b) in ops.items():
                v = op.execute(a.iters) / b / 1e3
                if r >= a.warmup_rounds:
                    t[k].append(v)
        return t

    def report(name, b, v, n):
        say(f"{name:40s} batch {b:2d} {med(v):9.1f} us/op   launches {n}   spread {spread(v):.1f}   (rounds: {fmt(v)})")

    def composed(name, parts, t, ops):
        v = [sum(x) for x in zip(*(t[k] for k in parts))]
        say(f"{name:40s}          {med(v):9.1f} us/op   launches {sum(ops[k][0].launch_count() for k in parts)}   spread {spread(v):.1f}   (rounds: {fmt(v)})")
        return v

    if a.only_base:
        ops = {"hmult": make("hmult", {}), "pmult": make("pmult", {}), "hlintrans R=4": make("hlintrans", {"rotations": 4}),
               "hbsgs 4x4": make("hbsgs", {"rotations": 4, "giants": 4})}
        for k, v in timed(ops).items():
            report(k, ops[k][1], v, ops[k][0].launch_count())
    elif a.only_pmult:
        ops = {"on": make("pmult", {"rescale": 1, "fuse_pmul_rescale": 1}), "off": make("pmult", {"rescale": 1, "fuse_pmul_rescale": 0})}
        t = timed(ops)
        report("pmult rescale=1 fuse_pmul_rescale=1", ops["on"][1], t["on"], ops["on"][0].launch_count())
        report("pmult rescale=1 fuse_pmul_rescale=0", ops["off"][1], t["off"], ops["off"][0].launch_count())
        say(f"  on / off = {med(t['on']) / med(t['off']):5.3f}   difference {med(t['off']) - med(t['on']):.1f} us, spreads {spread(t['on']):.1f} / {spread(t['off']):.1f}")
        for k in ("on", "off"):
            for kind, stage, ns in ops[k][0].stage_times(5):
                say(f"  {k:3s} {kind:14s} {ns / ops[k][1] / 1e3:8.1f}   {stage[:60]}")
    else:
        ops = {"on": make("pmult", {"rescale": 1, "fuse_pmul_rescale": 1}), "off": make("pmult", {"rescale": 1, "fuse_pmul_rescale": 0}), "pmult": make("pmult", {}),
               "hrescale": make("hrescale", {}),
               "lin1": make("hlintrans", {"rotations": 4, "rescale": 1}), "lin0": make("hlintrans", {"rotations": 4}),
               "bsgs1": make("hbsgs", {"rotations": 4, "giants": 4, "rescale": 1}), "bsgs0": make("hbsgs", {"rotations": 4, "giants": 4})}
        t = timed(ops)
        say("# (a) pmult rescale = 1: pass (4p) on against off")
        report("pmult rescale=1 fuse_pmul_rescale=1", ops["on"][1], t["on"], ops["on"][0].launch_count())
        report("pmult rescale=1 fuse_pmul_rescale=0", ops["off"][1], t["off"], ops["off"][0].launch_count())
        say(f"  on / off = {med(t['on']) / med(t['off']):5.3f}   difference {med(t['off']) - med(t['on']):.1f} us, spreads {spread(t['on']):.1f} / {spread(t['off']):.1f}")
        say("# (b) the rescale as an op of its own")
        report("hrescale", ops["hrescale"][1], t["hrescale"], ops["hrescale"][0].launch_count())
        report("pmult", ops["pmult"][1], t["pmult"], ops["pmult"][0].launch_count())
        two = composed("pmult + hrescale (two ops)", ("pmult", "hrescale"), t, ops)
        say(f"  pmult rescale=1 / (pmult + hrescale) = {med(t['on']) / med(two):5.3f}")
        say("# (c) the summing ops: rescale = 1 against rescale = 0 followed by hrescale")
        for one, zero, name in (("lin1", "lin0", "hlintrans R=4"), ("bsgs1", "bsgs0", "hbsgs 4x4")):
            report(name + " rescale=0", ops[zero][1], t[zero], ops[zero][0].launch_count())
            comp = composed(name + " rescale=0 + hrescale", (zero, "hrescale"), t, ops)
            report(name + " rescale=1", ops[one][1], t[one], ops[one][0].launch_count())
            say(f"  rescale=1 / composed = {med(t[one]) / med(comp):5.3f}   rescale=1 / rescale=0 = {med(t[one]) / med(t[zero]):5.3f}")
        say("# stage times, pmult rescale = 1 (each launch alone, us per op of the batch): pass on, then pass off")
        for k in ("on", "off"):
            for kind, stage, ns in ops[k][0].stage_times(5):
                say(f"  {k:3s} {kind:14s} {ns / ops[k][1] / 1e3:8.1f}   {stage[:60]}")
    for op, _ in ops.values():
        op.close()
    if a.out:
        with open(a.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
