"""hsquare on one device, interleaved (default config_4 45/35/15), at batch 1 and --batch (default 10), on both arithmetic
back-ends:
    (a) hsquare with both keys 1 against hmult in the same run;
    (b) hsquare with both keys 1 against the same op with fuse_square = 0 (TENSOR + element-wise launches);
    (c) its launch alone, hm_tensor_square with scalars and constants, against hm_tensor with aliased operands (a, a, c, c) on the same entry count
        (level x batch): 5 limb-polys per entry against 7 by the byte model.
Median of --rounds interleaved rounds x --iters iterations behind --warmup-rounds untimed rounds, with the spread (max - min over the rounds).  The
kernel stays if in (a) and (c) it is not slower than its comparison by more than both spreads.  Appends what it prints to --out.
    python3 tools/square_bench.py [--rounds 5] [--iters 20] [--warmup-rounds 1] [--batch 10] [--label head] [--out profiles/square.txt]"""
import argparse
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from homulator_amd import hip, host  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cfg", default="config_4.cfg")
    ap.add_argument("--logN", type=int, default=16, help="ring of --cfg (the launch-alone part makes its own contexts)")
    ap.add_argument("--levels", default="45,35,15")
    ap.add_argument("--batch", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup-rounds", type=int, default=1, help="untimed interleaved rounds in front of the timed ones")
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

    def verdict(new, old):
        d = med(new) - med(old)
        return f"{d:+7.1f} us (spreads {spread(new):.1f} / {spread(old):.1f}): " + ("SLOWER by more than both spreads" if d > max(spread(new), spread(old)) else "stays")

    say(f"# {a.label + ': ' if a.label else ''}{a.cfg} {L} {ell} {alpha} (us, median of {a.rounds} interleaved rounds x {a.iters} iterations; "
        f"spread = max - min over the rounds, after {a.warmup_rounds} untimed round(s))")

    # ---- (a), (b) the ops
    say("# (a) hsquare (sq_scale = sq_const = 1) against hmult, (b) against itself with fuse_square = 0; us per op of the batch")
    for chain_bits in (0, 60):
        base = {"chain_bits": chain_bits} if chain_bits else {}
        for batch in (1, a.batch):
            ov = dict(base, batch=batch)
            sq = dict(ov, sq_scale=1, sq_const=1)
            ops = {"hmult": host.Op(a.cfg, "hmult", L, ell, alpha, overrides=ov),
                   "hsquare": host.Op(a.cfg, "hsquare", L, ell, alpha, overrides=sq),
                   "hsquare fuse_square=0": host.Op(a.cfg, "hsquare", L, ell, alpha, overrides=dict(sq, fuse_square=0))}
            for op in ops.values():
                op.execute(3)   # first-use tables
            t = {k: [] for k in ops}
            for r in range(a.warmup_rounds + a.rounds):
                for k, op in ops.items():
                    v = op.execute(a.iters) / batch / 1e3
                    if r >= a.warmup_rounds:
                        t[k].append(v)
            name = "generic" if chain_bits else "mont32 "
            for k, op in ops.items():
                say(f"{name} batch {batch:2d} {k:22s} {med(t[k]):9.1f} us/op   launches {op.launch_count()}   spread {spread(t[k]):.1f}   (rounds: {fmt(t[k])})")
            say(f"{name} batch {batch:2d} (a) hsquare - hmult              {verdict(t['hsquare'], t['hmult'])}")
            say(f"{name} batch {batch:2d} (b) hsquare - hsquare unfused    {verdict(t['hsquare'], t['hsquare fuse_square=0'])}")
            if batch == 1:
                for k in ("hmult", "hsquare"):
                    kind, stage, ns = ops[k].stage_times(5)[0]
                    say(f"    first launch of {k:8s} {kind:14s} {ns / 1e3:8.1f}   {stage[:60]}")
            for op in ops.values():
                op.close()

    # ---- (c) the launch alone against hm_tensor with aliased operands
    for batch in (1, a.batch):
        n = ell * batch
        say(f"# (c) one launch of {n} entries, N = 2^{a.logN}: hm_tensor_square (scalars and constants) against hm_tensor(a, a, c, c), us per launch")
        mods = [i % ell for i in range(n)]
        for backend in ("mont32", "generic"):
            if backend == "mont32":
                ctx = hip.Context(a.logN, L, alpha)
            else:
                from oracle.homoracle import chain_below
                m = chain_below(a.logN, 60, L + alpha)
                ctx = hip.Context(a.logN, L, alpha, q=m[:L], p=m[L:])
            ca, cc = ctx.alloc(n), ctx.alloc(n)
            outs = [ctx.alloc(n) for _ in range(3)]
            ctx.fill_uniform(ca, mods, 1)
            ctx.fill_uniform(cc, mods, 2)
            s = [2 + i for i in range(n)]
            k = [ctx.moduli[m] - 1 - i for i, m in enumerate(mods)]
            calls = {"square": lambda: ctx.tensor_square(ca, cc, *outs, mods, scale=s, addend=k),
                     "tensor": lambda: ctx.tensor(ca, ca, cc, cc, *outs, mods)}
            for f in calls.values():
                f()   # first-use tables
            ctx.sync()
            t = {key: [] for key in calls}
            for r in range(a.warmup_rounds + a.rounds):
                for key, f in calls.items():
                    ctx.timer_start()
                    for _ in range(a.iters):
                        f()
                    v = ctx.timer_stop() / a.iters / 1e3
                    if r >= a.warmup_rounds:
                        t[key].append(v)
            sq, te = t["square"], t["tensor"]
            gb = lambda lp, us: lp * n * 8 * (1 << a.logN) / us / 1e3
            say(f"{backend:8s} square {med(sq):7.1f} (spread {spread(sq):.1f}, {gb(5, med(sq)):5.0f} GB/s of 5 limb-polys)   tensor {med(te):7.1f} "
                f"(spread {spread(te):.1f}, {gb(7, med(te)):5.0f} GB/s of 7)   (rounds: {fmt(sq)} | {fmt(te)})")
            say(f"{backend:8s} (c) square - tensor {verdict(sq, te)}")
            ctx.close()
    if a.out:
        with open(a.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
