"""hbsgs and hlintrans with identity = 1 against the compositions that yield the same diagonals from unchanged ops on the same build, interleaved on
one device (default config_4 45/35/15), every op at the largest batch that fits the 16-bit limb index (searched downwards from --batch-max):
    hbsgs R x G, identity = 1      against   hbsgs R x G + hlintrans R (galois g) + hlintrans G (galois h) + pmult + 3 hadd
    hlintrans R, identity = 1      against   hlintrans R + pmult + hadd
plus the per-launch stage times of the launches the identity steps change.  --only-base: hbsgs 4 x 4 and hlintrans R = 4 with identity = 0 only
(a build without the identity steps runs this too: parent / head / parent).  Appends what it prints to --out.
    python3 tools/bsgs_id_bench.py [--shapes 4x4,3x3] [--rounds 5] [--iters 10] [--batch-max 24] [--only-base] [--label head] [--out profiles/bsgs_identity.txt]"""
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
    ap.add_argument("--shapes", default="4x4,3x3", help="RxG: baby rotations x giant steps")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--only-base", action="store_true")
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
    say(f"# {a.label + ': ' if a.label else ''}{a.cfg} {L} {ell} {alpha}, every op at its largest batch <= {a.batch_max} (us per op of the batch, "
        f"median of {a.rounds} interleaved rounds x {a.iters} iterations; spread = max - min over the rounds)")

    def timed(ops):
        """ops: {name: (op, batch)}; one list of per-op times per name, the ops interleaved round by round"""
        t = {k: [] for k in ops}
        for _ in range(a.rounds):
            for k, (op, b) in ops.items():
                t[k].append(op.execute(a.iters) / b / 1e3)
        return t

    def report(name, b, v, n):
        say(f"{name:34s} batch {b:2d} {med(v):9.1f} us/op   launches {n}   spread {spread(v):.1f}   (rounds: {fmt(v)})")

    if a.only_base:
        ops = {"hbsgs 4x4 identity=0": largest_batch(a.cfg, "hbsgs", L, ell, alpha, a.batch_max, {"rotations": 4, "giants": 4}),
               "hlintrans R=4 identity=0": largest_batch(a.cfg, "hlintrans", L, ell, alpha, a.batch_max, {"rotations": 4})}
        for k, v in timed(ops).items():
            report(k, ops[k][1], v, ops[k][0].launch_count())
        for op, _ in ops.values():
            op.close()
    else:
        N2 = 2 << 16   # 2N of config_4 (the giant element h = g^(R+1) mod 2N is also given to the composition's ops)
        for R, G in (tuple(int(v) for v in s.split("x")) for s in a.shapes.split(",")):
            h = pow(5, R + 1, N2)
            ops = {"id": largest_batch(a.cfg, "hbsgs", L, ell, alpha, a.batch_max, {"rotations": R, "giants": G, "identity": 1}),
                   "bsgs": largest_batch(a.cfg, "hbsgs", L, ell, alpha, a.batch_max, {"rotations": R, "giants": G, "galois_giant": h}),
                   "linR": largest_batch(a.cfg, "hlintrans", L, ell, alpha, a.batch_max, {"rotations": R}),
                   "linG": largest_batch(a.cfg, "hlintrans", L, ell, alpha, a.batch_max, {"rotations": G, "galois": h}),
                   "pmult": largest_batch(a.cfg, "pmult", L, ell, alpha, a.batch_max, {}),
                   "hadd": largest_batch(a.cfg, "hadd", L, ell, alpha, a.batch_max, {})}
            t = timed(ops)
            comp = [w + x + y + z + 3 * u for w, x, y, z, u in zip(t["bsgs"], t["linR"], t["linG"], t["pmult"], t["hadd"])]
            nl = sum(ops[k][0].launch_count() for k in ("bsgs", "linR", "linG", "pmult")) + 3 * ops["hadd"][0].launch_count()
            for k, nm in (("bsgs", f"hbsgs {R}x{G} identity=0"), ("linR", f"hlintrans R={R} (g)"), ("linG", f"hlintrans R={G} (h)"), ("pmult", "pmult"), ("hadd", "hadd")):
                report(nm, ops[k][1], t[k], ops[k][0].launch_count())
            say(f"{'composed ' + str(R) + 'x' + str(G):34s}          {med(comp):9.1f} us/op   launches {nl}   spread {spread(comp):.1f}   (rounds: {fmt(comp)})")
            report(f"hbsgs {R}x{G} identity=1", ops["id"][1], t["id"], ops["id"][0].launch_count())
            say(f"  identity=1 / composed = {med(t['id']) / med(comp):5.3f}   identity=1 / identity=0 = {med(t['id']) / med(t['bsgs']):5.3f}")
            say(f"# stage times, hbsgs {R}x{G} (each launch alone, us per op of the batch): identity = 1 | identity = 0")
            for (kind, stage, ns), (_, _, ns0) in zip(ops["id"][0].stage_times(5), ops["bsgs"][0].stage_times(5)):
                mark = "  <- changed" if kind in ("IP_LINTRANS_MULTI", "IP_ROTSUM") or stage.startswith("ModDownNTTOut_Key") else ""
                say(f"  {kind:17s} {ns / ops['id'][1] / 1e3:8.1f} | {ns0 / ops['bsgs'][1] / 1e3:8.1f}   {stage[:50]}{mark}")
            for op, _ in ops.values():
                op.close()
        R = 4
        ops = {"id": largest_batch(a.cfg, "hlintrans", L, ell, alpha, a.batch_max, {"rotations": R, "identity": 1}),
               "lin": largest_batch(a.cfg, "hlintrans", L, ell, alpha, a.batch_max, {"rotations": R}),
               "pmult": largest_batch(a.cfg, "pmult", L, ell, alpha, a.batch_max, {}),
               "hadd": largest_batch(a.cfg, "hadd", L, ell, alpha, a.batch_max, {})}
        t = timed(ops)
        comp = [x + y + z for x, y, z in zip(t["lin"], t["pmult"], t["hadd"])]
        report(f"hlintrans R={R} identity=0", ops["lin"][1], t["lin"], ops["lin"][0].launch_count())
        say(f"{'composed R=' + str(R) + ' (+ pmult + hadd)':34s}          {med(comp):9.1f} us/op   launches {sum(o.launch_count() for o, _ in (ops['lin'], ops['pmult'], ops['hadd']))}   spread {spread(comp):.1f}   (rounds: {fmt(comp)})")
        report(f"hlintrans R={R} identity=1", ops["id"][1], t["id"], ops["id"][0].launch_count())
        say(f"  identity=1 / composed = {med(t['id']) / med(comp):5.3f}   identity=1 / identity=0 = {med(t['id']) / med(t['lin']):5.3f}")
        say(f"# stage times, hlintrans R = {R} (each launch alone, us per op of the batch): identity = 1 | identity = 0")
        for (kind, stage, ns), (_, _, ns0) in zip(ops["id"][0].stage_times(5), ops["lin"][0].stage_times(5)):
            mark = "  <- changed" if kind in ("IP_LINTRANS", "NTT_SUBSCALE") else ""
            say(f"  {kind:17s} {ns / ops['id'][1] / 1e3:8.1f} | {ns0 / ops['lin'][1] / 1e3:8.1f}   {stage[:50]}{mark}")
        for op, _ in ops.values():
            op.close()
    if a.out:
        with open(a.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
