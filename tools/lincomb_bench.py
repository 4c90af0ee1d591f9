"""hlincomb on one device, interleaved (default config_4 45/35/15), on both arithmetic back-ends:
    (a) hlincomb (lc_const = 1) against the same op with fuse_lincomb = 0 (element-wise launches) in the same run, T in --terms (default 2, 4, 16),
        at batch 1 and --batch (default 10);
    (b) its launch alone, hm_lincomb with scalars and constants, at 2 l and 2 l --batch records (70 and 700), T in --terms: achieved bytes per second
        by its (T + 1) limb-poly model, against hadd's element-wise launch (hm_ewe ADD, 3 limb-polys per record) on the same record counts in the
        same rounds, and the ratio of the two.
Median of --rounds interleaved rounds x --iters iterations behind --warmup-rounds untimed rounds, with the spread (max - min over the rounds).
Appends what it prints to --out.
    python3 tools/lincomb_bench.py [--rounds 5] [--iters 20] [--warmup-rounds 1] [--batch 10] [--label head] [--out profiles/lincomb.txt]"""
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
    ap.add_argument("--terms", default="2,4,16")
    ap.add_argument("--batch", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup-rounds", type=int, default=1, help="untimed interleaved rounds in front of the timed ones")
    ap.add_argument("--label", default="")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    L, ell, alpha = (int(x) for x in a.levels.split(","))
    terms = [int(x) for x in a.terms.split(",")]
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)
    fmt = lambda v: ", ".join(f"{x:.1f}" for x in v)
    med, spread = statistics.median, lambda v: max(v) - min(v)

    say(f"# {a.label + ': ' if a.label else ''}{a.cfg} {L} {ell} {alpha} (us, median of {a.rounds} interleaved rounds x {a.iters} iterations; "
        f"spread = max - min over the rounds, after {a.warmup_rounds} untimed round(s))")

    # ---- (a) the op, fused against fuse_lincomb = 0
    say("# (a) hlincomb (lc_const = 1) against itself with fuse_lincomb = 0; us per op of the batch")
    for chain_bits in (0, 60):
        base = {"chain_bits": chain_bits} if chain_bits else {}
        name = "generic" if chain_bits else "mont32 "
        for batch in (1, a.batch):
            for T in terms:
                ov = dict(base, batch=batch, terms=T, lc_const=1)
                ops = {"fused": host.Op(a.cfg, "hlincomb", L, ell, alpha, overrides=ov),
                       "fuse_lincomb=0": host.Op(a.cfg, "hlincomb", L, ell, alpha, overrides=dict(ov, fuse_lincomb=0))}
                for op in ops.values():
                    op.execute(3)   # first-use tables
                t = {k: [] for k in ops}
                for r in range(a.warmup_rounds + a.rounds):
                    for k, op in ops.items():
                        v = op.execute(a.iters) / batch / 1e3
                        if r >= a.warmup_rounds:
                            t[k].append(v)
                for k, op in ops.items():
                    say(f"{name} batch {batch:2d} T {T:2d} {k:15s} {med(t[k]):9.1f} us/op   launches {op.launch_count()}   spread {spread(t[k]):.1f}   (rounds: {fmt(t[k])})")
                f, u = t["fused"], t["fuse_lincomb=0"]
                d = med(f) - med(u)
                say(f"{name} batch {batch:2d} T {T:2d} (a) fused - unfused {d:+9.1f} us (spreads {spread(f):.1f} / {spread(u):.1f}): "
                    + ("faster by more than both spreads" if -d > max(spread(f), spread(u)) else "NOT faster by more than both spreads"))
                for op in ops.values():
                    op.close()

    # ---- (b) the launch alone against hadd's element-wise launch
    for batch in (1, a.batch):
        n = 2 * ell * batch
        say(f"# (b) one launch of {n} records, N = 2^{a.logN}: hm_lincomb against hm_ewe ADD (hadd's launch), us per launch and GB/s by the byte model")
        mods = [i % ell for i in range(n)]
        for backend in ("mont32", "generic"):
            if backend == "mont32":
                ctx = hip.Context(a.logN, L, alpha)
            else:
                from oracle.homoracle import chain_below
                m = chain_below(a.logN, 60, L + alpha)
                ctx = hip.Context(a.logN, L, alpha, q=m[:L], p=m[L:])
            Tmax = max(terms)
            src = ctx.alloc(n * Tmax)
            small = min(range(ell), key=lambda m: ctx.moduli[m])   # residues of the smallest modulus are reduced under every record's
            ctx.fill_uniform(src, [small] * (n * Tmax), 1)
            out = ctx.alloc(n)
            k = [ctx.moduli[m] - 1 - i for i, m in enumerate(mods)]

            def lincomb_call(T):
                li = list(range(n * T))
                s = [2 + i for i in range(n * T)]
                return lambda: ctx.lincomb(src, li, out, None, mods, T, s, k)
            second = list(range(n, 2 * n))
            calls = {f"lincomb T={T}": lincomb_call(T) for T in terms}
            calls["hadd"] = lambda: ctx.ewe(hip.OP_ADD, out, mods, a=src, c=src, lc=second)
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
            h = t["hadd"]
            hadd_gb = gb(3, med(h))
            say(f"{backend:8s} hadd          {med(h):8.1f} (spread {spread(h):.1f}, {hadd_gb:5.0f} GB/s of 3 limb-polys)   (rounds: {fmt(h)})")
            for T in terms:
                v = t[f"lincomb T={T}"]
                g = gb(T + 1, med(v))
                lo, hi = gb(T + 1, max(v)) / gb(3, min(h)), gb(T + 1, min(v)) / gb(3, max(h))
                say(f"{backend:8s} lincomb T={T:2d}  {med(v):8.1f} (spread {spread(v):.1f}, {g:5.0f} GB/s of {T + 1} limb-polys)   ratio to hadd {g / hadd_gb:.2f} "
                    f"(over the rounds' extremes {lo:.2f} .. {hi:.2f})   (rounds: {fmt(v)})")
            src.free(); out.free()
            ctx.close()
    if a.out:
        with open(a.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
