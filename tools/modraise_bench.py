"""ModRaise on one device, interleaved (default config_4 45/1/15):
    (a) the op hmodraise at batch 1 and at the largest batch that fits the 16-bit limb index (searched downwards from --batch-max);
    (b) its lifted launch alone (hm_ntt_lift, entries that read 2 sources) against a plain forward hm_ntt launch of the same entry count on stored
        inputs (form 0), in every geometry of the table: the one-launch form (default options), the 8-coefficient two-kernel form
        (ntt_fused_small = 0) and the 16-coefficient one (ntt_small_limbs = 0 as well), on both arithmetic back-ends, at two entry counts: 2 T (the
        op's own launch at batch 1: above the 8-coefficient form's limit of 64 limb-polys of N = 2^16, so that option runs 16-coefficient kernels
        there) and --small-entries (default 64: the largest launch the 8-coefficient form takes).  The plain sibling in the same run is the
        yardstick of the prologue's price; the 16-coefficient form of the same call is the fallback a geometry has to beat.
One untimed interleaved round runs in front of the timed ones (--warmup-rounds).  Appends what it prints to --out.
    python3 tools/modraise_bench.py [--rounds 5] [--iters 20] [--warmup-rounds 1] [--batch-max 24] [--small-entries 64] [--label head] [--out profiles/modraise.txt]"""
import argparse
import os
import statistics
import sys


sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from homulator_amd import hip, host  # noqa: E402

FORMS = [("one-launch", {}), ("two-kernel-8", {"ntt_fused_small": 0}), ("two-kernel-16", {"ntt_fused_small": 0, "ntt_small_limbs": 0})]


def largest_batch(cfg, L, ell, alpha, bmax, ov):
    """limb-polys are addressed by 16-bit indices over the whole batch: the largest batch <= bmax that builds"""
    b = bmax
    while True:
        op = host.Op(cfg, "hmodraise", L, ell, alpha, overrides=dict(ov, batch=b))
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
    ap.add_argument("--logN", type=int, default=16, help="ring of --cfg (the launch-alone part makes its own contexts)")
    ap.add_argument("--levels", default="45,1,15")
    ap.add_argument("--batch-max", type=int, default=24)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup-rounds", type=int, default=1, help="untimed interleaved rounds in front of the timed ones")
    ap.add_argument("--small-entries", type=int, default=64, help="second entry count of part (b), even")
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
    say(f"# {a.label + ': ' if a.label else ''}{a.cfg} {L} {ell} {alpha} (us, median of {a.rounds} interleaved rounds x {a.iters} iterations; "
        f"spread = max - min over the rounds, after {a.warmup_rounds} untimed round(s))")

    # ---- (a) the op
    say("# (a) hmodraise, us per op of the batch")
    for chain_bits in (0, 60):
        ov = {"chain_bits": chain_bits} if chain_bits else {}
        ops = {"batch 1": (host.Op(a.cfg, "hmodraise", L, ell, alpha, overrides=ov or None), 1)}
        ops["batch 1"][0].execute(3)
        ops["largest batch"] = largest_batch(a.cfg, L, ell, alpha, a.batch_max, ov)
        t = {k: [] for k in ops}
        for r in range(a.warmup_rounds + a.rounds):
            for k, (op, b) in ops.items():
                v = op.execute(a.iters) / b / 1e3
                if r >= a.warmup_rounds:
                    t[k].append(v)
        for k, (op, b) in ops.items():
            say(f"{'generic' if chain_bits else 'mont32 '} {k:14s} batch {b:2d} {med(t[k]):9.1f} us/op   launches {op.launch_count()}   spread {spread(t[k]):.1f}   "
                f"(rounds: {fmt(t[k])})")
            if b == 1:
                for kind, stage, ns in op.stage_times(5):
                    say(f"    {kind:6s} {ns / 1e3:8.1f}   {stage[:60]}")
            op.close()

    # ---- (b) the lifted launch alone against its plain sibling, per entry count, geometry and back-end
    for n in (2 * L, a.small_entries):
        say(f"# (b) one launch of {n} limb-polys, N = 2^{a.logN}: lifted (2 sources, hm_ntt_lift) against plain (stored inputs, hm_ntt), us per launch")
        mods = [i % L for i in range(n // 2)] * 2
        for backend in ("mont32", "generic"):
            ctxs = {}
            for form, opts in FORMS:
                if backend == "mont32":
                    ctx = hip.Context(a.logN, L, alpha)
                else:
                    from oracle.homoracle import chain_below
                    m = chain_below(a.logN, 60, L + alpha)
                    ctx = hip.Context(a.logN, L, alpha, q=m[:L], p=m[L:])
                for k, v in opts.items():
                    ctx.set_option(k, v)
                src, stored, out = ctx.alloc(2), ctx.alloc(n), ctx.alloc(n)
                ctx.fill_uniform(src, [0, 0], 1)
                ctx.fill_uniform(stored, mods, 2)
                lifted = lambda ctx=ctx, src=src, out=out: ctx.ntt_lift(src, out, mods, [0] * n, in_limbs=[0] * (n // 2) + [1] * (n // 2))
                plain = lambda ctx=ctx, stored=stored, out=out: ctx.ntt(stored, out, mods)
                for f in (lifted, plain):
                    f()   # first-use tables
                ctx.sync()
                ctxs[form] = (ctx, {"lifted": lifted, "plain": plain})
            t = {(form, k): [] for form in ctxs for k in ("lifted", "plain")}
            for r in range(a.warmup_rounds + a.rounds):
                for form, (ctx, calls) in ctxs.items():
                    for k, f in calls.items():
                        ctx.timer_start()
                        for _ in range(a.iters):
                            f()
                        v = ctx.timer_stop() / a.iters / 1e3
                        if r >= a.warmup_rounds:
                            t[(form, k)].append(v)
            for form in ctxs:
                lf, pl = t[(form, "lifted")], t[(form, "plain")]
                say(f"{backend:8s} {form:14s} lifted {med(lf):7.1f} (spread {spread(lf):.1f})   plain {med(pl):7.1f} (spread {spread(pl):.1f})   "
                    f"lifted - plain {med(lf) - med(pl):+6.1f}   (rounds: {fmt(lf)} | {fmt(pl)})")
            base = t[("two-kernel-16", "lifted")]
            for form in ("one-launch", "two-kernel-8"):
                lf = t[(form, "lifted")]
                d = med(lf) - med(base)
                verdict = "slower than its fallback by more than both spreads" if d > max(spread(lf), spread(base)) else "stays"
                say(f"{backend:8s} {form:14s} lifted - 16-coefficient lifted {d:+6.1f} us (spreads {spread(lf):.1f} / {spread(base):.1f}): {verdict}")
            for ctx, _ in ctxs.values():
                ctx.close()
    if a.out:
        with open(a.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
