"""hdot against the composition it replaces, T x hmult + (T - 1) x hadd, interleaved on one device (default config_4 45/35/15, batch 10), plus
the per-launch stage times of hdot and, at T = 1, hdot against hmult itself (the two plans differ in their first launch only).
    python3 tools/dot_bench.py [--batch 10] [--terms 1,2,4,8] [--rounds 5] [--iters 10] [--graph 0] [--no-stages]"""
import argparse
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from homulator_amd import host  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cfg", default="config_4.cfg")
    ap.add_argument("--levels", default="45,35,15")
    ap.add_argument("--batch", type=int, default=10)
    ap.add_argument("--terms", default="1,2,4,8")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--graph", type=int, default=0)
    ap.add_argument("--no-stages", action="store_true")
    a = ap.parse_args()
    L, ell, alpha = (int(x) for x in a.levels.split(","))
    terms = [int(x) for x in a.terms.split(",")]
    B = a.batch
    print(f"# {a.cfg} {L} {ell} {alpha} batch {B} graph {a.graph}: hdot T against T hmult + (T - 1) hadd "
          f"(us per op of the batch, median of {a.rounds} interleaved rounds x {a.iters} iterations)")
    base = {"batch": B, "graph": a.graph}
    # the composition adds the products: hadd runs a level down, on what hmult's rescale leaves
    parts = {"hmult": host.Op(a.cfg, "hmult", L, ell, alpha, overrides=base), "hadd": host.Op(a.cfg, "hadd", L, ell - 1, alpha, overrides=base)}
    dots = {T: host.Op(a.cfg, "hdot", L, ell, alpha, overrides=dict(base, terms=T)) for T in terms}
    for op in list(parts.values()) + list(dots.values()):
        op.execute(3)   # first-use tables, graph capture
    t_part = {n: [] for n in parts}
    t_dot = {T: [] for T in terms}
    for _ in range(a.rounds):
        for n, op in parts.items():
            t_part[n].append(op.execute(a.iters) / B / 1e3)
        for T in terms:
            t_dot[T].append(dots[T].execute(a.iters) / B / 1e3)
    fmt = lambda v: ", ".join(f"{x:.1f}" for x in v)
    for n in parts:
        print(f"{n:10s} {statistics.median(t_part[n]):9.1f} us/op   launches {parts[n].launch_count()}   (rounds: {fmt(t_part[n])})")
    for T in terms:
        comp = [T * m + (T - 1) * d for m, d in zip(t_part["hmult"], t_part["hadd"])]   # round by round: its spread is the spread of the sum
        m, c = statistics.median(t_dot[T]), statistics.median(comp)
        print(f"composed T={T:<2d} {c:9.1f} us/op   launches {T * parts['hmult'].launch_count() + (T - 1) * parts['hadd'].launch_count()}   (rounds: {fmt(comp)})")
        print(f"hdot     T={T:<2d} {m:9.1f} us/op   launches {dots[T].launch_count()}   {m / c:5.3f} x composed   "
              f"spread {max(t_dot[T]) - min(t_dot[T]):.1f} / {max(comp) - min(comp):.1f}   (rounds: {fmt(t_dot[T])})")
    if 1 in terms:
        hm, d1 = statistics.median(t_part["hmult"]), statistics.median(t_dot[1])
        print(f"hdot T=1 against hmult: {d1:.1f} / {hm:.1f} us/op = {d1 / hm:5.3f}")
    if not a.no_stages:
        for name, op in [("hmult", parts["hmult"])] + [(f"hdot T={T}", dots[T]) for T in terms]:
            print(f"# stage times, {name} batch {B} (each launch alone, us per op of the batch)")
            for kind, stage, ns in op.stage_times(5):
                print(f"  {kind:13s} {ns / B / 1e3:8.1f}   {stage[:90]}")
    for op in list(parts.values()) + list(dots.values()):
        op.close()


if __name__ == "__main__":
    main()
