"""hbsgs against the composition it replaces, G x hlintrans (R rotations each) + one hrotsum of G, interleaved on one device (default config_4
45/35/15, both sides at the largest batch that fits the 16-bit limb index), plus the per-launch stage times of hbsgs and, with --tiles, the
merged baby-step launch with each of the two built tile sizes (hm_inner_product_lintrans_multi, option ip_multi_tile).
    python3 tools/bsgs_bench.py [--batch 10] [--shapes 1x1,2x2,4x4,8x2,4x8] [--rounds 5] [--iters 10] [--graph 0] [--no-stages] [--tiles]"""
import argparse
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from homulator_amd import host  # noqa: E402


def largest_batch(cfg, name, L, ell, alpha, B, ov):
    """limb-polys are addressed by 16-bit indices over the whole batch: an op with many buffers runs at the largest batch that fits"""
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


def tile_ab(a, L, ell, alpha):
    """the merged launch alone, on the kernel's own entry point, at the op's shape (n = batch x (l + alpha) entries, beta digits, R rotations, G
    outputs, the Q entries with an addend), once per built tile size, interleaved"""
    from homulator_amd import hip
    R, G, B = 4, 4, a.batch
    beta, n, nQ = -(-ell // alpha), B * (ell + alpha), B * ell
    ctx = hip.Context(16, L, alpha)
    mods = [(i // B) if i // B < ell else L + (i // B - ell) for i in range(n)]
    nx, ny, npt = n * beta, R * (ell + alpha) * 2 * beta, G * R * n
    xb, yb, pb, cb, ob, ab = (ctx.alloc(k) for k in (nx, ny, npt, nQ, G * 2 * n, G * nQ))
    for buf, k in ((xb, nx), (yb, ny), (pb, npt), (cb, nQ)):
        ctx.fill_uniform(buf, [L + alpha - 1] * k, 7 + k)   # timing only: residues below the smallest modulus are reduced for every entry
    xl = list(range(nx))
    yl = [(((r * (ell + alpha) + i // B) * 2 + k) * beta + j) for r in range(R) for i in range(n) for k in range(2) for j in range(beta)]   # a batch shares its keys
    pl, ol = list(range(npt)), list(range(G * 2 * n))
    cl = [i if i < nQ else hip.NO_LIMB for i in range(n)]
    al = [m * nQ + i if i < nQ else hip.NO_LIMB for m in range(G) for i in range(n)]
    gs = [pow(5, r, 1 << 17) for r in range(1, R + 1)]
    call = lambda: ctx.inner_product_lintrans_multi(xb, xl, yb, yl, pb, pl, ob, ol, mods, beta, gs, G, addend=cb, addend_limbs=cl, addend_out=ab,
                                                    addend_out_limbs=al)
    times = {2: [], 4: []}
    for t in times:
        ctx.set_option("ip_multi_tile", t)
        call()
    ctx.sync()
    for _ in range(a.rounds):
        for t in times:
            ctx.set_option("ip_multi_tile", t)
            ctx.timer_start()
            for _ in range(a.iters):
                call()
            times[t].append(ctx.timer_stop() / a.iters / B / 1e3)
    print(f"# hm_inner_product_lintrans_multi alone, n = {n} entries of {beta} digits, R = {R}, G = {G} (device events around the calls; "
          f"us per op of the batch, median of {a.rounds} interleaved rounds x {a.iters} calls)")
    for t in times:
        print(f"tile {t}: {statistics.median(times[t]):8.1f} us/op   (rounds: {', '.join(f'{x:.1f}' for x in times[t])})")
    ctx.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cfg", default="config_4.cfg")
    ap.add_argument("--levels", default="45,35,15")
    ap.add_argument("--batch", type=int, default=10)
    ap.add_argument("--shapes", default="1x1,2x2,4x4,8x2,4x8", help="RxG: baby rotations x giant steps")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--graph", type=int, default=0)
    ap.add_argument("--no-stages", action="store_true")
    ap.add_argument("--tiles", action="store_true", help="only the A/B of the merged launch between the two built tile sizes")
    a = ap.parse_args()
    L, ell, alpha = (int(x) for x in a.levels.split(","))
    if a.tiles:
        return tile_ab(a, L, ell, alpha)
    shapes = [tuple(int(v) for v in s.split("x")) for s in a.shapes.split(",")]
    print(f"# {a.cfg} {L} {ell} {alpha} batch <= {a.batch} graph {a.graph}: hbsgs RxG against G hlintrans(R) + hrotsum(G) "
          f"(us per op of the batch, median of {a.rounds} interleaved rounds x {a.iters} iterations)")
    base = {"graph": a.graph}
    for R, G in shapes:   # one shape at a time: the buffers of all of them together do not fit the device
        op, b = largest_batch(a.cfg, "hbsgs", L, ell, alpha, a.batch, dict(base, rotations=R, giants=G))
        lin = host.Op(a.cfg, "hlintrans", L, ell, alpha, overrides=dict(base, batch=b, rotations=R))
        rs = host.Op(a.cfg, "hrotsum", L, ell, alpha, overrides=dict(base, batch=b, rotations=G))
        lin.execute(3)
        rs.execute(3)
        t_op, t_lin, t_rs = [], [], []
        for _ in range(a.rounds):
            t_lin.append(lin.execute(a.iters) / b / 1e3)
            t_rs.append(rs.execute(a.iters) / b / 1e3)
            t_op.append(op.execute(a.iters) / b / 1e3)
        fmt = lambda v: ", ".join(f"{x:.1f}" for x in v)
        comp = [G * x + y for x, y in zip(t_lin, t_rs)]   # round by round: its spread is the spread of the sum
        m, c = statistics.median(t_op), statistics.median(comp)
        print(f"hlintrans R={R:<2d}      batch {b:2d} {statistics.median(t_lin):9.1f} us/op   launches {lin.launch_count()}   (rounds: {fmt(t_lin)})")
        print(f"hrotsum   G={G:<2d}      batch {b:2d} {statistics.median(t_rs):9.1f} us/op   launches {rs.launch_count()}   (rounds: {fmt(t_rs)})")
        print(f"composed  {R}x{G:<2d}      batch {b:2d} {c:9.1f} us/op   launches {G * lin.launch_count() + rs.launch_count()}   (rounds: {fmt(comp)})")
        print(f"hbsgs     {R}x{G:<2d}      batch {b:2d} {m:9.1f} us/op   launches {op.launch_count()}   {m / c:5.3f} x composed   "
              f"spread {max(t_op) - min(t_op):.1f} / {max(comp) - min(comp):.1f}   (rounds: {fmt(t_op)})")
        if not a.no_stages:
            print(f"# stage times, hbsgs {R}x{G} batch {b} (each launch alone, us per op of the batch)")
            for kind, stage, ns in op.stage_times(5):
                print(f"  {kind:17s} {ns / b / 1e3:8.1f}   {stage[:80]}")
        for o in (op, lin, rs):
            o.close()


if __name__ == "__main__":
    main()
