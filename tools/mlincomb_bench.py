"""hmlincomb on one device, interleaved (default config_4 45/35/15), on both arithmetic back-ends:
    (a) hmlincomb (ml_const = 1) in three forms in the same rounds, at (T, M) in --shapes (default 4x4, 8x8, 16x16, 8x2), at batch 1 and the largest
        batch the pool of 65 535 limb-polys holds up to --batch (default 10), us per op of the batch: fused (one LINCOMB_MULTI launch), the same op
        with fuse_mlincomb = 0 (one LINCOMB launch of M times the records), and M hlincomb ops (lc_const = 1) run one after the other; each ratio
        beside the byte model's M (T + 1) / (ceil(M / TILE) T + M);
    (b) the launch alone, hm_lincomb_multi with scalars and constants, at 2 l and 2 l --batch entries (70 and 700), the same shapes, with both built
        tiles (hm_set_option "lincomb_multi_tile") in the same rounds: us per launch and achieved bytes per second by each tile's own byte model.
Median of --rounds interleaved rounds x --iters iterations behind --warmup-rounds untimed rounds, with the spread (max - min over the rounds).
Appends what it prints to --out.  --part and --backend select a piece, so that a caller can give every piece a time limit of its own.
    python3 tools/mlincomb_bench.py [--part a|b|ab] [--backend mont32|generic|both] [--rounds 5] [--iters 20] [--label head] [--out profiles/mlincomb.txt]"""
import argparse
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from homulator_amd import hip, host  # noqa: E402

POOL = 65535


def limb_polys(T, M, ell):
    """a copy of hmlincomb with ml_const = 1 (Pool)"""
    return 2 * T * ell + M * (2 * (2 * T - 1) + 1) * ell


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cfg", default="config_4.cfg")
    ap.add_argument("--logN", type=int, default=16, help="ring of --cfg (the launch-alone part makes its own contexts)")
    ap.add_argument("--levels", default="45,35,15")
    ap.add_argument("--shapes", default="4x4,8x8,16x16,8x2", help="TxM, comma-separated")
    ap.add_argument("--batch", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup-rounds", type=int, default=1, help="untimed interleaved rounds in front of the timed ones")
    ap.add_argument("--part", default="ab")
    ap.add_argument("--backend", default="both", choices=["mont32", "generic", "both"])
    ap.add_argument("--label", default="")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    L, ell, alpha = (int(x) for x in a.levels.split(","))
    shapes = [tuple(int(v) for v in s.split("x")) for s in a.shapes.split(",")]
    backends = ["mont32", "generic"] if a.backend == "both" else [a.backend]
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)
    fmt = lambda v: ", ".join(f"{x:.1f}" for x in v)
    med, spread = statistics.median, lambda v: max(v) - min(v)
    tiles_of = lambda M, tile: -(-M // tile)

    say(f"# {a.label + ': ' if a.label else ''}{a.cfg} {L} {ell} {alpha} (us, median of {a.rounds} interleaved rounds x {a.iters} iterations; "
        f"spread = max - min over the rounds, after {a.warmup_rounds} untimed round(s)); default tile {hip.LINCOMB_MULTI_TILE}")

    # ---- (a) the op: fused, fuse_mlincomb = 0, M hlincomb ops
    if "a" in a.part:
        say("# (a) hmlincomb (ml_const = 1): fused, fuse_mlincomb = 0, and M hlincomb ops one after the other; us per op of the batch")
        for backend in backends:
            base = {"chain_bits": 60} if backend == "generic" else {}
            for T, M in shapes:
                for batch in sorted({1, min(a.batch, POOL // limb_polys(T, M, ell))}):
                    ov = dict(base, batch=batch, terms=T, outputs=M, ml_const=1)
                    fused = host.Op(a.cfg, "hmlincomb", L, ell, alpha, overrides=ov)
                    off = host.Op(a.cfg, "hmlincomb", L, ell, alpha, overrides=dict(ov, fuse_mlincomb=0))
                    singles = [host.Op(a.cfg, "hlincomb", L, ell, alpha, overrides=dict(base, batch=batch, terms=T, lc_const=1, seed=host.SEED + 31 * m))
                               for m in range(M)]
                    runs = {"fused": lambda it: fused.execute(it), "fuse_mlincomb=0": lambda it: off.execute(it),
                            "M hlincomb": lambda it: sum(op.execute(it) for op in singles)}
                    launches = {"fused": fused.launch_count(), "fuse_mlincomb=0": off.launch_count(), "M hlincomb": sum(op.launch_count() for op in singles)}
                    for f in runs.values():
                        f(3)   # first-use tables
                    t = {k: [] for k in runs}
                    for r in range(a.warmup_rounds + a.rounds):
                        for k, f in runs.items():
                            v = f(a.iters) / batch / 1e3
                            if r >= a.warmup_rounds:
                                t[k].append(v)
                    tag = f"{backend:8s} batch {batch:2d} T {T:2d} M {M:2d}"
                    for k in runs:
                        say(f"{tag} {k:16s} {med(t[k]):9.1f} us/op   launches {launches[k]}   spread {spread(t[k]):.1f}   (rounds: {fmt(t[k])})")
                    f, u, s = t["fused"], t["fuse_mlincomb=0"], t["M hlincomb"]
                    model = M * (T + 1) / (tiles_of(M, hip.LINCOMB_MULTI_TILE) * T + M)
                    say(f"{tag} (a) M hlincomb / fused {med(s) / med(f):.2f}, fuse_mlincomb=0 / fused {med(u) / med(f):.2f}, byte model {model:.2f}")
                    d = med(f) - med(s)
                    say(f"{tag} (a) fused - M hlincomb {d:+9.1f} us (spreads {spread(f):.1f} / {spread(s):.1f}): "
                        + ("faster by more than both spreads" if -d > max(spread(f), spread(s)) else "NOT faster by more than both spreads"))
                    d = med(u) - med(f)
                    say(f"{tag} (a) fuse_mlincomb=0 - fused {d:+9.1f} us (spreads {spread(u):.1f} / {spread(f):.1f}): "
                        + ("fuse_mlincomb=0 is faster by more than both spreads" if -d > max(spread(f), spread(u)) else "fuse_mlincomb=0 is not faster beyond the spreads"))
                    for op in [fused, off] + singles:
                        op.close()

    # ---- (b) the launch alone, both tiles
    if "b" in a.part:
        for batch in (1, a.batch):
            n = 2 * ell * batch
            say(f"# (b) one launch of {n} entries, N = 2^{a.logN}: hm_lincomb_multi with tile 4 and tile 8, us per launch and GB/s by each tile's byte model")
            mods = [i % ell for i in range(n)]
            for backend in backends:
                if backend == "mont32":
                    ctx = hip.Context(a.logN, L, alpha)
                else:
                    from oracle.homoracle import chain_below
                    m = chain_below(a.logN, 60, L + alpha)
                    ctx = hip.Context(a.logN, L, alpha, q=m[:L], p=m[L:])
                Tmax, Mmax = max(T for T, _ in shapes), max(M for _, M in shapes)
                src = ctx.alloc(n * Tmax)
                small = min(range(ell), key=lambda m: ctx.moduli[m])   # residues of the smallest modulus are reduced under every entry's
                ctx.fill_uniform(src, [small] * (n * Tmax), 1)
                out = ctx.alloc(n * Mmax)

                def call(T, M, tile):
                    # the lists as C arrays, made once: a launch of 700 entries of 16 x 16 scalars must not wait for Python to convert them
                    keep = [hip._u32(list(range(n * T))), hip._u32(mods), hip._u64([2 + i for i in range(n * M * T)]),
                            hip._u64([ctx.moduli[mods[i]] - 1 - i for i in range(n) for _ in range(M)])]

                    def f():
                        ctx.set_option("lincomb_multi_tile", tile)
                        ctx._ck(ctx.L.hm_lincomb_multi(ctx.h, src.ptr, keep[0][1], out.ptr, None, keep[1][1], n, T, M, keep[2][1], keep[3][1]))
                    return f
                calls = {(T, M, tile): call(T, M, tile) for T, M in shapes for tile in (4, 8)}
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
                for T, M in shapes:
                    for tile in (4, 8):
                        v = t[(T, M, tile)]
                        lp = tiles_of(M, tile) * T + M
                        say(f"{backend:8s} n {n:4d} T {T:2d} M {M:2d} tile {tile}  {med(v):8.1f} (spread {spread(v):.1f}, {lp * n * 8 * (1 << a.logN) / med(v) / 1e3:5.0f} GB/s of "
                            f"{lp} limb-polys per entry)   (rounds: {fmt(v)})")
                    v4, v8 = t[(T, M, 4)], t[(T, M, 8)]
                    d = med(v8) - med(v4)
                    say(f"{backend:8s} n {n:4d} T {T:2d} M {M:2d} (b) tile 8 - tile 4 {d:+8.1f} us (spreads {spread(v8):.1f} / {spread(v4):.1f}): "
                        + ("tile 8 faster" if -d > max(spread(v4), spread(v8)) else "tile 4 faster" if d > max(spread(v4), spread(v8)) else "level within the spreads"))
                ctx.set_option("lincomb_multi_tile", 0)
                src.free(); out.free()
                ctx.close()
    if a.out:
        with open(a.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
