"""hplincomb on one device, interleaved (default config_4 45/35/15), on both arithmetic back-ends:
    (a) hplincomb against the same op with fuse_plincomb = 0 (element-wise launches) in the same run, for --terms (default 2,4,16) at batch 1 and
        --batch (default 10), with the byte model 8 T - 2 against 3 T + 2 limb-polys per limb beside the measured ratio;
    (b) its launch alone, hm_plincomb at l and l --batch records (35 and 350), against hm_lincomb at a matching number of limb-polys moved in the
        same rounds: hm_plincomb moves 3 T + 2 per record, hm_lincomb T' + 1, so hm_lincomb runs T' = min(16, 3 T / 2) terms on
        round((3 T + 2) n / (T' + 1)) records (T = 2: 3 terms on 2 n records, T = 4: 6 on 2 n, T = 16: 16 on 50 n / 17); us per launch, achieved
        bytes per second by each one's own byte count, and the ratio of the rates.  The lists are marshalled once, outside the timed region.
Median of --rounds interleaved rounds x --iters iterations behind --warmup-rounds untimed rounds, with the spread (max - min over the rounds).
Appends what it prints to --out.
    python3 tools/plincomb_bench.py [--rounds 5] [--iters 20] [--warmup-rounds 1] [--batch 10] [--label head] [--out profiles/plincomb.txt]"""
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

    # ---- (a) the op, fused against fuse_plincomb = 0
    for chain_bits in ((0, 60) if "a" in a.parts else ()):
        base = {"chain_bits": chain_bits} if chain_bits else {}
        name = "generic" if chain_bits else "mont32 "
        for want in (1, a.batch):
            for T in terms:
                # the op's buffers, used or not, share one pool of at most 65 535 limb-polys: per copy 2 T l ciphertext limbs, T l plaintext limbs and
                # the 2 T l outputs of the element-wise stages; a batch that does not fit is cut to the largest that does, and the row says so
                per = ell * 5 * T
                batch = min(want, 65535 // per)
                if batch != want:
                    say(f"{name} batch {want:2d} T={T:2d}: {want} x {per} limb-polys exceed the pool's 65535; run at batch {batch}")
                ov = dict(base, batch=batch, terms=T)
                ops = {"hplincomb": host.Op(a.cfg, "hplincomb", L, ell, alpha, overrides=ov),
                       "fuse_plincomb=0": host.Op(a.cfg, "hplincomb", L, ell, alpha, overrides=dict(ov, fuse_plincomb=0))}
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
                f, u = t["hplincomb"], t["fuse_plincomb=0"]
                d = med(f) - med(u)
                model = (8 * T - 2) / (3 * T + 2)
                say(f"{name} batch {batch:2d} T={T:2d} (a) fused - fuse_plincomb=0 {d:+9.1f} us (spreads {spread(f):.1f} / {spread(u):.1f}): "
                    + ("faster by more than both spreads" if -d > max(spread(f), spread(u)) else "NOT faster by more than both spreads")
                    + f"; measured ratio {med(u) / med(f):.2f}, byte model {model:.2f}")
                for op in ops.values():
                    op.close()

    # ---- (b) the launch alone against hm_lincomb at a matching number of limb-polys moved
    for backend in (("mont32", "generic") if "b" in a.parts else ()):
        if backend == "mont32":
            ctx = hip.Context(a.logN, L, alpha)
        else:
            from oracle.homoracle import chain_below
            m = chain_below(a.logN, 60, L + alpha)
            ctx = hip.Context(a.logN, L, alpha, q=m[:L], p=m[L:])
        small = min(range(ell), key=lambda m: ctx.moduli[m])   # residues of the smallest modulus are reduced under every record's
        for batch in (1, a.batch):
            n = ell * batch
            for T in terms:
                Tl = min(16, 3 * T // 2)
                nl = round((3 * T + 2) * n / (Tl + 1))
                mods, lmods = [i % ell for i in range(n)], [i % ell for i in range(nl)]
                # every term its own limb-polys: 3 T + 2 (T' + 1) limb-polys of traffic per record
                x, p, out = ctx.alloc(2 * T * n), ctx.alloc(T * n), ctx.alloc(2 * n)
                lsrc, lout = ctx.alloc(Tl * nl), ctx.alloc(nl)
                ctx.fill_uniform(x, [small] * (2 * T * n), 1)
                ctx.fill_uniform(p, [small] * (T * n), 2)
                ctx.fill_uniform(lsrc, [small] * (Tl * nl), 3)
                # the lists are marshalled once, outside the timed region: a call costs what the entry point costs, not what Python's lists do
                keep = [hip._u32(list(range(T * n))), hip._u32(list(range(T * n))), hip._u32(list(range(T * n, 2 * T * n))), hip._u32(list(range(n))),
                        hip._u32(list(range(n, 2 * n))), hip._u32(mods), hip._u32(list(range(Tl * nl))), hip._u32(lmods),
                        hip._u64([2 + i for i in range(Tl * nl)])]
                plp, plx0, plx1, pl0, pl1, pm, pli, plm, pls = (v[1] for v in keep)
                calls = {"lincomb": lambda: ctx._ck(ctx.L.hm_lincomb(ctx.h, lsrc.ptr, pli, lout.ptr, None, plm, nl, Tl, pls, None)),
                         "plincomb": lambda: ctx._ck(ctx.L.hm_plincomb(ctx.h, p.ptr, plp, x.ptr, plx0, plx1, None, None, out.ptr, pl0, pl1, pm, n, T))}
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
                lp = {"plincomb": (3 * T + 2) * n, "lincomb": (Tl + 1) * nl}      # limb-polys moved per launch
                gb = lambda key: lp[key] * 8 * (1 << a.logN) / med(t[key]) / 1e3
                c, h = t["plincomb"], t["lincomb"]
                say(f"{backend:8s} (b) T={T:2d} plincomb n={n:3d} ({lp['plincomb']:5d} limb-polys) {med(c):8.1f} us (spread {spread(c):.1f}, {gb('plincomb'):5.0f} GB/s)   "
                    f"lincomb T'={Tl:2d} n={nl:4d} ({lp['lincomb']:5d} limb-polys) {med(h):8.1f} us (spread {spread(h):.1f}, {gb('lincomb'):5.0f} GB/s)   "
                    f"rate plincomb / lincomb = {gb('plincomb') / gb('lincomb'):.3f}   (rounds: {fmt(c)} | {fmt(h)})")
                for buf in (x, p, out, lsrc, lout):
                    buf.free()
        ctx.close()
    if a.out:
        with open(a.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
