"""hclincomb on one device, interleaved (default config_4 45/35/15), on both arithmetic back-ends:
    (a) hclincomb against the same op with fuse_clincomb = 0 (element-wise launches) in the same run, for --terms (default 2,4,16) at batch 1 and
        --batch (default 10; cut to what the pool of 65 535 limb-polys holds), with the byte model 2 (13 T - 3) + 2 against 2 (T + 1) limb-polys per limb beside the measured ratio;
    (b) its launch alone, hm_clincomb, against hm_lincomb at the same T and record counts (2 l and 2 l --batch records: 70 and 700) in the same
        rounds: both move T + 1 limb-polys per record; us per launch, achieved bytes per second and the ratio of the rates.
Median of --rounds interleaved rounds x --iters iterations behind --warmup-rounds untimed rounds, with the spread (max - min over the rounds).
Appends what it prints to --out.
    python3 tools/clincomb_bench.py [--rounds 5] [--iters 20] [--warmup-rounds 1] [--batch 10] [--label head] [--out profiles/clincomb.txt]"""
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
    ap.add_argument("--parts", default="ab")
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

    # ---- (a) the op, fused against fuse_clincomb = 0
    for chain_bits in ((0, 60) if "a" in a.parts else ()):
        base = {"chain_bits": chain_bits} if chain_bits else {}
        name = "generic" if chain_bits else "mont32 "
        for want in (1, a.batch):
            for T in terms:
                # the op's buffers, used or not, share one pool of at most 65 535 limb-polys: per copy 2 T l inputs, the stored monomial and the
                # (5 T - 1) 2 l outputs of the element-wise stages; a batch that does not fit is cut to the largest that does, and the row says so
                per = ell * (2 * T + 1 + 2 * (5 * T - 1))
                batch = min(want, 65535 // per)
                if batch != want:
                    say(f"{name} batch {want:2d} T={T:2d}: {want} x {per} limb-polys exceed the pool's 65535; run at batch {batch}")
                ov = dict(base, batch=batch, terms=T)
                ops = {"hclincomb": host.Op(a.cfg, "hclincomb", L, ell, alpha, overrides=ov),
                       "fuse_clincomb=0": host.Op(a.cfg, "hclincomb", L, ell, alpha, overrides=dict(ov, fuse_clincomb=0))}
                for op in ops.values():
                    op.execute(3)   # first-use tables
                t = {k: [] for k in ops}
                for r in range(a.warmup_rounds + a.rounds):
                    for k, op in ops.items():
                        v = op.execute(a.iters) / batch / 1e3
                        if r >= a.warmup_rounds:
                            t[k].append(v)
                for k, op in ops.items():
                    say(f"{name} batch {batch:2d} T={T:2d} {k:16s} {med(t[k]):9.1f} us/op   launches {op.launch_count()}   spread {spread(t[k]):.1f}   (rounds: {fmt(t[k])})")
                f, u = t["hclincomb"], t["fuse_clincomb=0"]
                d = med(f) - med(u)
                model = (2 * (13 * T - 3) + 2) / (2 * (T + 1))
                say(f"{name} batch {batch:2d} T={T:2d} (a) fused - fuse_clincomb=0 {d:+9.1f} us (spreads {spread(f):.1f} / {spread(u):.1f}): "
                    + ("faster by more than both spreads" if -d > max(spread(f), spread(u)) else "NOT faster by more than both spreads")
                    + f"; measured ratio {med(u) / med(f):.2f}, byte model {model:.2f}")
                for op in ops.values():
                    op.close()

    # ---- (b) the launch alone against hm_lincomb at the same T and record count
    for backend in (("mont32", "generic") if "b" in a.parts else ()):
        if backend == "mont32":
            ctx = hip.Context(a.logN, L, alpha)
        else:
            from oracle.homoracle import chain_below
            m = chain_below(a.logN, 60, L + alpha)
            ctx = hip.Context(a.logN, L, alpha, q=m[:L], p=m[L:])
        small = min(range(ell), key=lambda m: ctx.moduli[m])   # residues of the smallest modulus are reduced under every record's
        for batch in (1, a.batch):
            n = 2 * ell * batch
            mods = [i % ell for i in range(n)]
            for T in terms:
                src, out = ctx.alloc(T * n), ctx.alloc(n)
                ctx.fill_uniform(src, [small] * (T * n), 1)
                li = list(range(T * n))      # every term its own limb-poly: T + 1 limb-polys of traffic per record
                re = [2 + i for i in range(T * n)]
                im = [3 + 2 * i for i in range(T * n)]
                k = [5 + i for i in range(n)]
                # the lists are marshalled once, outside the timed region: a call costs what the entry point costs, not what Python's lists do
                keep = [hip._u32(li), hip._u32(mods), hip._u64(re), hip._u64(im), hip._u64(k)]
                pli, pm, pre, pim, pk = (x[1] for x in keep)
                calls = {"lincomb": lambda: ctx._ck(ctx.L.hm_lincomb(ctx.h, src.ptr, pli, out.ptr, None, pm, n, T, pre, pk)),
                         "clincomb": lambda: ctx._ck(ctx.L.hm_clincomb(ctx.h, src.ptr, pli, out.ptr, None, pm, n, T, pre, pim, pk, None))}
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
                gb = lambda us: (T + 1) * n * 8 * (1 << a.logN) / us / 1e3
                c, h = t["clincomb"], t["lincomb"]
                ratio = med(h) / med(c)      # the ratio of the rates: the same bytes, so the inverse ratio of the times
                below = med(c) - med(h) > max(spread(c), spread(h))
                say(f"{backend:8s} (b) n={n:3d} T={T:2d} lincomb {med(h):8.1f} us (spread {spread(h):.1f}, {gb(med(h)):5.0f} GB/s)   clincomb {med(c):8.1f} us "
                    f"(spread {spread(c):.1f}, {gb(med(c)):5.0f} GB/s)   rate clincomb / lincomb = {ratio:.3f}"
                    + ("  BELOW 1 by more than the spreads" if below else "") + f"   (rounds: {fmt(h)} | {fmt(c)})")
                src.free(); out.free()
        ctx.close()
    if a.out:
        with open(a.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
