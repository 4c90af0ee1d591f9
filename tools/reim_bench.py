"""hreim on one device, interleaved (default config_4 45/35/15), on both arithmetic back-ends:
    (a) hreim against the same op with fuse_reim = 0 (hrotate's launches plus element-wise launches) in the same run, at batch 1 and --batch
        (default 10);
    (b) hreim against TWO hrotate ops with galois = 2N - 1 run back to back in the same run (the cost floor of any two-op way to both parts), and
        against one hrotate plus the launch alone;
    (c) its launch alone, hm_reim_split, against hm_lincomb with T = 2 at 2 l and 2 l --batch records (70 and 700): us per launch and achieved
        bytes per second by the 4 (3) limb-poly model.
Median of --rounds interleaved rounds x --iters iterations behind --warmup-rounds untimed rounds, with the spread (max - min over the rounds).
Appends what it prints to --out.
    python3 tools/reim_bench.py [--rounds 5] [--iters 20] [--warmup-rounds 1] [--batch 10] [--label head] [--out profiles/reim.txt]"""
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
    ap.add_argument("--parts", default="abc")
    ap.add_argument("--label", default="")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    L, ell, alpha = (int(x) for x in a.levels.split(","))
    conj = 2 * (1 << a.logN) - 1
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)
    fmt = lambda v: ", ".join(f"{x:.1f}" for x in v)
    med, spread = statistics.median, lambda v: max(v) - min(v)

    def race(ops, batch):
        """us per op of the batch of every op in `ops`, interleaved"""
        for op in ops.values():
            op.execute(3)   # first-use tables
        t = {k: [] for k in ops}
        for r in range(a.warmup_rounds + a.rounds):
            for k, op in ops.items():
                v = op.execute(a.iters) / batch / 1e3
                if r >= a.warmup_rounds:
                    t[k].append(v)
        return t

    say(f"# {a.label + ': ' if a.label else ''}{a.cfg} {L} {ell} {alpha} (us, median of {a.rounds} interleaved rounds x {a.iters} iterations; "
        f"spread = max - min over the rounds, after {a.warmup_rounds} untimed round(s))")

    for chain_bits in ((0, 60) if ("a" in a.parts or "b" in a.parts) else ()):
        base = {"chain_bits": chain_bits} if chain_bits else {}
        name = "generic" if chain_bits else "mont32 "
        for batch in (1, a.batch):
            ov = dict(base, batch=batch)
            ops = {"hreim": host.Op(a.cfg, "hreim", L, ell, alpha, overrides=ov),
                   "fuse_reim=0": host.Op(a.cfg, "hreim", L, ell, alpha, overrides=dict(ov, fuse_reim=0)),
                   "hrotate 1": host.Op(a.cfg, "hrotate", L, ell, alpha, overrides=dict(ov, galois=conj)),
                   "hrotate 2": host.Op(a.cfg, "hrotate", L, ell, alpha, overrides=dict(ov, galois=conj, seed=host.SEED + 31))}
            t = race(ops, batch)
            for k, op in ops.items():
                say(f"{name} batch {batch:2d} {k:12s} {med(t[k]):9.1f} us/op   launches {op.launch_count()}   spread {spread(t[k]):.1f}   (rounds: {fmt(t[k])})")
            f, u = t["hreim"], t["fuse_reim=0"]
            d = med(f) - med(u)
            say(f"{name} batch {batch:2d} (a) fused - fuse_reim=0 {d:+9.1f} us (spreads {spread(f):.1f} / {spread(u):.1f}): "
                + ("faster by more than both spreads" if -d > max(spread(f), spread(u)) else "NOT faster by more than both spreads"))
            two = [x + y for x, y in zip(t["hrotate 1"], t["hrotate 2"])]     # back to back: the two ops of every round
            say(f"{name} batch {batch:2d} (b) two hrotate {med(two):9.1f} us (spread {spread(two):.1f}); hreim / two hrotate = {med(f) / med(two):.3f}; "
                f"hreim - one hrotate = {med(f) - med(t['hrotate 1']):+.1f} us")
            for op in ops.values():
                op.close()

    # ---- (c) the launch alone against hm_lincomb with two terms
    for batch in ((1, a.batch) if "c" in a.parts else ()):
        n = 2 * ell * batch
        say(f"# (c) one launch of {n} records, N = 2^{a.logN}: hm_reim_split against hm_lincomb with T = 2, us per launch and GB/s by the byte model")
        mods = [i % ell for i in range(n)]
        for backend in ("mont32", "generic"):
            if backend == "mont32":
                ctx = hip.Context(a.logN, L, alpha)
            else:
                from oracle.homoracle import chain_below
                m = chain_below(a.logN, 60, L + alpha)
                ctx = hip.Context(a.logN, L, alpha, q=m[:L], p=m[L:])
            src = ctx.alloc(2 * n)
            small = min(range(ell), key=lambda m: ctx.moduli[m])   # residues of the smallest modulus are reduced under every record's
            ctx.fill_uniform(src, [small] * (2 * n), 1)
            out = ctx.alloc(2 * n)
            lx, ly = list(range(n)), list(range(n, 2 * n))
            li = [v for i in range(n) for v in (lx[i], ly[i])]
            s = [2 + i for i in range(2 * n)]
            calls = {"reim_split": lambda: ctx.reim_split(src, src, out, out, mods, limbs=[lx, ly, lx, ly]),
                     "lincomb T=2": lambda: ctx.lincomb(src, li, out, lx, mods, 2, s)}
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
            gb = lambda lp, us: lp * n * 8 * (1 << a.logN) / us / 1e3
            v, h = t["reim_split"], t["lincomb T=2"]
            say(f"{backend:8s} lincomb T=2  {med(h):8.1f} (spread {spread(h):.1f}, {gb(3, med(h)):5.0f} GB/s of 3 limb-polys)   (rounds: {fmt(h)})")
            say(f"{backend:8s} reim_split   {med(v):8.1f} (spread {spread(v):.1f}, {gb(4, med(v)):5.0f} GB/s of 4 limb-polys)   reim - lincomb {med(v) - med(h):+.1f} us"
                f"   (rounds: {fmt(v)})")
            src.free(); out.free()
            ctx.close()
    if a.out:
        with open(a.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
