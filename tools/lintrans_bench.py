"""hlintrans against the composition it replaces, hrotate_hoisted R + R x pmult + (R - 1) x hadd, interleaved on one device (default config_4
45/35/15, batch 10), plus the per-launch stage times of hlintrans.
    python3 tools/lintrans_bench.py [--batch 10] [--rots 1,2,4,8] [--rounds 5] [--iters 10] [--no-stages]"""
import argparse
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from homulator_amd import host  # noqa: E402


def largest_batch(cfg, name, L, ell, alpha, B, R):
    """limb-polys are addressed by 16-bit indices over the whole batch: an op with many rotations runs at the largest batch that fits"""
    b = B
    while True:
        op = host.Op(cfg, name, L, ell, alpha, overrides={"batch": b, "rotations": R})
        try:
            op.execute(2)
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
    ap.add_argument("--rots", default="1,2,4,8")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--no-stages", action="store_true")
    a = ap.parse_args()
    L, ell, alpha = (int(x) for x in a.levels.split(","))
    rots = [int(x) for x in a.rots.split(",")]
    print(f"# {a.cfg} {L} {ell} {alpha} batch {a.batch}: hlintrans R against hrotate_hoisted R + R pmult + (R - 1) hadd "
          f"(us per op of the batch, median of {a.rounds} interleaved rounds x {a.iters} iterations)")
    lin, hoi, bat = {}, {}, {}
    for R in rots:   # both sides of a comparison at the same batch: the smaller of the two that fit
        lin[R], b1 = largest_batch(a.cfg, "hlintrans", L, ell, alpha, a.batch, R)
        hoi[R], b2 = largest_batch(a.cfg, "hrotate_hoisted", L, ell, alpha, b1, R)
        if b2 != b1:
            lin[R].close()
            lin[R], b1 = largest_batch(a.cfg, "hlintrans", L, ell, alpha, b2, R)
        bat[R] = b2
    ewe = {}
    for b in sorted(set(bat.values())):
        ewe[b] = {n: host.Op(a.cfg, n, L, ell, alpha, overrides={"batch": b}) for n in ("pmult", "hadd")}
        for op in ewe[b].values():
            op.execute(2)
    t_lin, t_hoi = {R: [] for R in rots}, {R: [] for R in rots}
    t_ewe = {b: {"pmult": [], "hadd": []} for b in ewe}
    for _ in range(a.rounds):
        for b in ewe:
            for n, op in ewe[b].items():
                t_ewe[b][n].append(op.execute(a.iters) / b / 1e3)
        for R in rots:
            t_hoi[R].append(hoi[R].execute(a.iters) / bat[R] / 1e3)
            t_lin[R].append(lin[R].execute(a.iters) / bat[R] / 1e3)
    fmt = lambda v: ", ".join(f"{x:.1f}" for x in v)
    for b in ewe:
        for n in ("pmult", "hadd"):
            print(f"{n:15s} batch {b:2d} {statistics.median(t_ewe[b][n]):9.1f} us/op   (rounds: {fmt(t_ewe[b][n])})")
    for R in rots:
        b = bat[R]
        # the composition round by round, so that its spread is the spread of the sum
        comp = [h + R * p + (R - 1) * d for h, p, d in zip(t_hoi[R], t_ewe[b]["pmult"], t_ewe[b]["hadd"])]
        m, c = statistics.median(t_lin[R]), statistics.median(comp)
        print(f"hoisted   R={R:<2d} batch {b:2d} {statistics.median(t_hoi[R]):9.1f} us/op   launches {hoi[R].launch_count()}   (rounds: {fmt(t_hoi[R])})")
        print(f"composed  R={R:<2d} batch {b:2d} {c:9.1f} us/op   launches {hoi[R].launch_count() + 2 * R - 1}   (rounds: {fmt(comp)})")
        print(f"hlintrans R={R:<2d} batch {b:2d} {m:9.1f} us/op   launches {lin[R].launch_count()}   {m / c:5.3f} x composed   "
              f"spread {max(t_lin[R]) - min(t_lin[R]):.1f} / {max(comp) - min(comp):.1f}   (rounds: {fmt(t_lin[R])})")
    if not a.no_stages:
        for R in rots:
            print(f"# stage times, hlintrans R={R} batch {bat[R]} (each launch alone, us per op of the batch)")
            for kind, name, ns in lin[R].stage_times(5):
                print(f"  {kind:13s} {ns / bat[R] / 1e3:8.1f}   {name[:90]}")
    for d in (lin, hoi):
        for op in d.values():
            op.close()
    for b in ewe:
        for op in ewe[b].values():
            op.close()


if __name__ == "__main__":
    main()
