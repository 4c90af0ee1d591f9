"""hrotsum against the composition it replaces, G x hrotate + (G - 1) x hadd, interleaved on one device (default config_4 45/35/15, batch 10),
plus the per-launch stage times of hrotsum and, at G = 1, hrotsum against hrotate_hoisted with rotations = 1 (the same plan).
    python3 tools/rotsum_bench.py [--batch 10] [--cts 1,2,4,8,16] [--rounds 5] [--iters 10] [--graph 0] [--no-stages]"""
import argparse
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from homulator_amd import host  # noqa: E402


def largest_batch(cfg, name, L, ell, alpha, B, ov):
    """limb-polys are addressed by 16-bit indices over the whole batch: an op with many ciphertexts runs at the largest batch that fits"""
    b = B
    while True:
        op = host.Op(cfg, name, L, ell, alpha, overrides=dict(ov, batch=b))
        try:
            op.execute(3)   # first-use tables, graph capture
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
    ap.add_argument("--batch", type=int, default=10)
    ap.add_argument("--cts", default="1,2,4,8,16")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--graph", type=int, default=0)
    ap.add_argument("--no-stages", action="store_true")
    a = ap.parse_args()
    L, ell, alpha = (int(x) for x in a.levels.split(","))
    cts = [int(x) for x in a.cts.split(",")]
    print(f"# {a.cfg} {L} {ell} {alpha} batch {a.batch} graph {a.graph}: hrotsum G against G hrotate + (G - 1) hadd "
          f"(us per op of the batch, median of {a.rounds} interleaved rounds x {a.iters} iterations)")
    base = {"graph": a.graph}
    rot, bat = {}, {}
    for G in cts:
        rot[G], bat[G] = largest_batch(a.cfg, "hrotsum", L, ell, alpha, a.batch, dict(base, rotations=G))
    parts = {}   # the composition's ops, at every batch a comparison runs at
    for b in sorted(set(bat.values())):
        parts[b] = {n: host.Op(a.cfg, n, L, ell, alpha, overrides=dict(base, batch=b)) for n in ("hrotate", "hadd")}
        if 1 in cts and bat[1] == b:
            parts[b]["hrotate_hoisted"] = host.Op(a.cfg, "hrotate_hoisted", L, ell, alpha, overrides=dict(base, batch=b, rotations=1))
        for op in parts[b].values():
            op.execute(3)
    t_rot = {G: [] for G in cts}
    t_part = {b: {n: [] for n in parts[b]} for b in parts}
    for _ in range(a.rounds):
        for b in parts:
            for n, op in parts[b].items():
                t_part[b][n].append(op.execute(a.iters) / b / 1e3)
        for G in cts:
            t_rot[G].append(rot[G].execute(a.iters) / bat[G] / 1e3)
    fmt = lambda v: ", ".join(f"{x:.1f}" for x in v)
    for b in parts:
        for n in parts[b]:
            print(f"{n:16s} batch {b:2d} {statistics.median(t_part[b][n]):9.1f} us/op   launches {parts[b][n].launch_count()}   (rounds: {fmt(t_part[b][n])})")
    for G in cts:
        b = bat[G]
        comp = [G * r + (G - 1) * d for r, d in zip(t_part[b]["hrotate"], t_part[b]["hadd"])]   # round by round: its spread is the spread of the sum
        m, c = statistics.median(t_rot[G]), statistics.median(comp)
        print(f"composed G={G:<2d} batch {b:2d} {c:9.1f} us/op   launches {G * parts[b]['hrotate'].launch_count() + (G - 1) * parts[b]['hadd'].launch_count()}"
              f"   (rounds: {fmt(comp)})")
        print(f"hrotsum  G={G:<2d} batch {b:2d} {m:9.1f} us/op   launches {rot[G].launch_count()}   {m / c:5.3f} x composed   "
              f"spread {max(t_rot[G]) - min(t_rot[G]):.1f} / {max(comp) - min(comp):.1f}   (rounds: {fmt(t_rot[G])})")
    if 1 in cts:
        h, r1 = statistics.median(t_part[bat[1]]["hrotate_hoisted"]), statistics.median(t_rot[1])
        print(f"hrotsum G=1 against hrotate_hoisted rotations=1: {r1:.1f} / {h:.1f} us/op = {r1 / h:5.3f}")
    if not a.no_stages:
        for G in cts:
            print(f"# stage times, hrotsum G={G} batch {bat[G]} (each launch alone, us per op of the batch)")
            for kind, stage, ns in rot[G].stage_times(5):
                print(f"  {kind:13s} {ns / bat[G] / 1e3:8.1f}   {stage[:90]}")
    for op in list(rot.values()) + [op for b in parts for op in parts[b].values()]:
        op.close()


if __name__ == "__main__":
    main()
