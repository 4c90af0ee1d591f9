"""hmuladd on one device, interleaved (default config_4 45/35/15), on both arithmetic back-ends:
    (a) hmuladd (ma_scale = ma_const = 1) against the same op with fuse_muladd = 0 (TENSOR plus element-wise launches) in the same run, A in --addends
        (default 0, 1, 4, 8), at batch 1 and --batch (default 10);
    (b) hmuladd with A = 0 and both keys 0 against hmult in the same run, at batch 1 and --batch;
    (c) its launch alone, hm_tensor_muladd with A = 0 and no constants, against hm_tensor at l and l --batch records (35 and 350), and with A in
        --addends, scalars and constants: us per launch and achieved bytes per second by the (7 + 2A) limb-poly model.
Median of --rounds interleaved rounds x --iters iterations behind --warmup-rounds untimed rounds, with the spread (max - min over the rounds).
Appends what it prints to --out.
    python3 tools/muladd_bench.py [--rounds 5] [--iters 20] [--warmup-rounds 1] [--batch 10] [--label head] [--out profiles/muladd.txt]"""
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
    ap.add_argument("--addends", default="0,1,4,8")
    ap.add_argument("--batch", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup-rounds", type=int, default=1, help="untimed interleaved rounds in front of the timed ones")
    ap.add_argument("--parts", default="abc")
    ap.add_argument("--label", default="")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    L, ell, alpha = (int(x) for x in a.levels.split(","))
    addends = [int(x) for x in a.addends.split(",")]
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

    for chain_bits in (0, 60):
        base = {"chain_bits": chain_bits} if chain_bits else {}
        name = "generic" if chain_bits else "mont32 "
        for batch in (1, a.batch):
            if "a" in a.parts:   # ---- (a) the op, fused against fuse_muladd = 0
                for A in addends:
                    ov = dict(base, batch=batch, addends=A, ma_scale=1, ma_const=1)
                    ops = {"fused": host.Op(a.cfg, "hmuladd", L, ell, alpha, overrides=ov),
                           "fuse_muladd=0": host.Op(a.cfg, "hmuladd", L, ell, alpha, overrides=dict(ov, fuse_muladd=0))}
                    t = race(ops, batch)
                    for k, op in ops.items():
                        say(f"{name} batch {batch:2d} A {A} {k:14s} {med(t[k]):9.1f} us/op   launches {op.launch_count()}   spread {spread(t[k]):.1f}   (rounds: {fmt(t[k])})")
                    f, u = t["fused"], t["fuse_muladd=0"]
                    d = med(f) - med(u)
                    say(f"{name} batch {batch:2d} A {A} (a) fused - unfused {d:+9.1f} us (spreads {spread(f):.1f} / {spread(u):.1f}): "
                        + ("faster by more than both spreads" if -d > max(spread(f), spread(u)) else "NOT faster by more than both spreads"))
                    for op in ops.values():
                        op.close()
            if "b" in a.parts:   # ---- (b) A = 0 without constants against hmult
                ops = {"hmuladd A=0": host.Op(a.cfg, "hmuladd", L, ell, alpha, overrides=dict(base, batch=batch, addends=0)),
                       "hmult": host.Op(a.cfg, "hmult", L, ell, alpha, overrides=dict(base, batch=batch))}
                t = race(ops, batch)
                for k in ops:
                    say(f"{name} batch {batch:2d} {k:12s} {med(t[k]):9.1f} us/op   spread {spread(t[k]):.1f}   (rounds: {fmt(t[k])})")
                m, h = t["hmuladd A=0"], t["hmult"]
                d = med(m) - med(h)
                say(f"{name} batch {batch:2d} (b) hmuladd - hmult {d:+9.1f} us (spreads {spread(m):.1f} / {spread(h):.1f}): "
                    + ("level within the spreads" if abs(d) <= max(spread(m), spread(h)) else "NOT level within the spreads"))
                for op in ops.values():
                    op.close()

    # ---- (c) the launch alone against hm_tensor
    for batch in ((1, a.batch) if "c" in a.parts else ()):
        n = ell * batch
        say(f"# (c) one launch of {n} records, N = 2^{a.logN}: hm_tensor_muladd against hm_tensor, us per launch and GB/s by the byte model")
        mods = [i % ell for i in range(n)]
        for backend in ("mont32", "generic"):
            if backend == "mont32":
                ctx = hip.Context(a.logN, L, alpha)
            else:
                from oracle.homoracle import chain_below
                m = chain_below(a.logN, 60, L + alpha)
                ctx = hip.Context(a.logN, L, alpha, q=m[:L], p=m[L:])
            Amax = max(addends)
            src = ctx.alloc(n * (4 + 2 * Amax))
            small = min(range(ell), key=lambda m: ctx.moduli[m])   # residues of the smallest modulus are reduced under every record's
            ctx.fill_uniform(src, [small] * (n * (4 + 2 * Amax)), 1)
            out = ctx.alloc(3 * n)
            ops = [list(range(r * n, (r + 1) * n)) for r in range(4)]
            lo = [list(range(r * n, (r + 1) * n)) for r in range(3)]
            s = [2 + i for i in range(n)]
            k = [ctx.moduli[m] - 1 - i for i, m in enumerate(mods)]

            def muladd_call(A, plain):
                lx0 = [4 * n + (2 * t) * n + i for i in range(n) for t in range(A)]
                lx1 = [4 * n + (2 * t + 1) * n + i for i in range(n) for t in range(A)]
                u = [3 + i for i in range(n * A)]
                if plain:
                    return lambda: ctx.tensor_muladd(src, src, src, src, None, out, out, out, mods, 0, limbs=ops + lo)
                return lambda: ctx.tensor_muladd(src, src, src, src, src if A else None, out, out, out, mods, A, lx0 if A else None, lx1 if A else None, s,
                                                 u if A else None, k, limbs=ops + lo)
            calls = {"tensor": lambda: ctx.tensor(src, src, src, src, out, out, out, mods, limbs=ops + lo), "muladd plain": muladd_call(0, True)}
            for A in addends:
                calls[f"muladd A={A}"] = muladd_call(A, False)
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
            h = t["tensor"]
            say(f"{backend:8s} tensor        {med(h):8.1f} (spread {spread(h):.1f}, {gb(7, med(h)):5.0f} GB/s of 7 limb-polys)   (rounds: {fmt(h)})")
            v = t["muladd plain"]
            say(f"{backend:8s} muladd plain  {med(v):8.1f} (spread {spread(v):.1f}, {gb(7, med(v)):5.0f} GB/s of 7 limb-polys)   muladd - tensor {med(v) - med(h):+.1f} us"
                f"   (rounds: {fmt(v)})")
            for A in addends:
                v = t[f"muladd A={A}"]
                say(f"{backend:8s} muladd A={A}    {med(v):8.1f} (spread {spread(v):.1f}, {gb(7 + 2 * A, med(v)):5.0f} GB/s of {7 + 2 * A} limb-polys)   (rounds: {fmt(v)})")
            src.free(); out.free()
            ctx.close()
    if a.out:
        with open(a.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
