"""hrotate_hoisted against R x hrotate, interleaved on one device (default config_4 45/35/15, batch 10), plus per-launch stage times and the
hoisted key-product kernel against R gathered inner products (hm_inner_product_ex, x_galois) at the op's launch size.
    python3 tools/hoist_bench.py [--batch 10] [--rots 1,2,4,8] [--rounds 5] [--iters 10] [--no-stages] [--no-kernel]"""
import argparse
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from homulator_amd import host  # noqa: E402


def kernel_ab(logN, L, K, n, terms, R, iters):
    """device us of one hm_inner_product_hoisted call against R hm_inner_product_ex calls on the same limb-polys"""
    from homulator_amd import hip
    ctx = hip.Context(logN, L, K)
    mods = [i % (L + K) for i in range(n)]
    galois = [pow(5, r + 1, 2 << logN) for r in range(R)]
    xb, yb, ob = ctx.alloc(n * terms), ctx.alloc(R * n * 2 * terms), ctx.alloc(R * n * 2)
    ctx.fill_uniform(xb, [mods[i // terms] for i in range(n * terms)], 1)
    ctx.fill_uniform(yb, [mods[(i // (2 * terms)) % n] for i in range(R * n * 2 * terms)], 2)
    xl, yl, ol = list(range(n * terms)), list(range(R * n * 2 * terms)), list(range(R * n * 2))

    def hoisted():
        ctx.inner_product_hoisted(xb, xl, yb, yl, ob, ol, mods, terms, galois)

    def gathered():
        for r, g in enumerate(galois):
            ctx.inner_product(xb, xl, yb, yl[r * n * 2 * terms:(r + 1) * n * 2 * terms], ob, ol[r * n * 2:(r + 1) * n * 2], mods, terms, 2, x_galois=g)

    out = {}
    for name, f in (("hoisted", hoisted), ("gathered", gathered)):
        f()
        ctx.sync()
        ctx.timer_start()
        for _ in range(iters):
            f()
        out[name] = ctx.timer_stop() / iters / 1e3
    for b in (xb, yb, ob):
        b.free()
    ctx.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cfg", default="config_4.cfg")
    ap.add_argument("--levels", default="45,35,15")
    ap.add_argument("--batch", type=int, default=10)
    ap.add_argument("--rots", default="1,2,4,8")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--no-stages", action="store_true")
    ap.add_argument("--no-kernel", action="store_true")
    a = ap.parse_args()
    L, ell, alpha = (int(x) for x in a.levels.split(","))
    rots = [int(x) for x in a.rots.split(",")]
    B = a.batch
    print(f"# {a.cfg} {L} {ell} {alpha} batch {B}: hrotate_hoisted R against R x hrotate (us per op of the batch, median of {a.rounds} interleaved rounds x {a.iters} iterations)")
    # limb-polys are addressed by 16-bit indices over the whole batch: an op with many rotations runs at the largest batch that fits
    ops, bat = {}, {}
    for R in rots:
        b = B
        while True:
            op = host.Op(a.cfg, "hrotate_hoisted", L, ell, alpha, overrides={"batch": b, "rotations": R})
            try:
                op.execute(2)
                break
            except host.HostError as e:
                op.close()
                if "exceeds 65535" not in str(e) or b == 1:
                    raise
                b -= 1
        ops[R], bat[R] = op, b
    hrs = {b: host.Op(a.cfg, "hrotate", L, ell, alpha, overrides={"batch": b}) for b in sorted(set(bat.values()))}
    for h in hrs.values():
        h.execute(2)
    t_hr, t = {b: [] for b in hrs}, {R: [] for R in rots}
    for _ in range(a.rounds):
        for b, h in hrs.items():
            t_hr[b].append(h.execute(a.iters) / b / 1e3)
        for R in rots:
            t[R].append(ops[R].execute(a.iters) / bat[R] / 1e3)
    for b in hrs:
        print(f"hrotate       batch {b:2d} {statistics.median(t_hr[b]):9.1f} us/op   launches {hrs[b].launch_count()}   (rounds: {', '.join(f'{x:.1f}' for x in t_hr[b])})")
    for R in rots:
        m, one = statistics.median(t[R]), statistics.median(t_hr[bat[R]])
        print(f"hoisted R={R:<2d} batch {bat[R]:2d} {m:9.1f} us/op   launches {ops[R].launch_count()}   {m / R:7.1f} us per rotation   "
              f"{m / (R * one):5.3f} x R hrotates   (rounds: {', '.join(f'{x:.1f}' for x in t[R])})")
    hr = hrs[B] if B in hrs else hrs[max(hrs)]
    if not a.no_stages:
        for R in rots:
            print(f"# stage times, hrotate_hoisted R={R} batch {bat[R]} (each launch alone, us per op of the batch)")
            for kind, name, ns in ops[R].stage_times(5):
                print(f"  {kind:13s} {ns / bat[R] / 1e3:8.1f}   {name[:90]}")
        print("# stage times, hrotate")
        for kind, name, ns in hr.stage_times(5):
            print(f"  {kind:13s} {ns / hr.batch / 1e3:8.1f}   {name[:90]}")
    for h in hrs.values():
        h.close()
    for op in ops.values():
        op.close()
    if not a.no_kernel:
        beta = (ell + alpha - 1) // alpha
        logN = 16 if a.cfg == "config_4.cfg" else 15
        n = (ell + alpha) * B
        print(f"# key-product kernel alone: n = {n} entries (batch {B} x {ell + alpha} extended limbs), n_terms = {beta}; device us per call")
        for R in rots:
            k = kernel_ab(logN, L, alpha, n, beta, R, a.iters)
            print(f"  R={R:<2d} hoisted {k['hoisted']:8.1f}   {R} x gathered {k['gathered']:8.1f}   ratio {k['hoisted'] / k['gathered']:.3f}")


if __name__ == "__main__":
    main()
