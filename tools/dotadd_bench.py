"""hdotadd on one device, interleaved (default config_4 45/35/15), on both arithmetic back-ends:
    (a) hdotadd (da_scale = da_const = 1) against the same op with fuse_dotadd = 0 (TENSOR plus element-wise launches) in the same run, (T, A) in
        --shapes (default 2:1, 4:2, 8:4), at batch 1 and --batch (default 10; the largest batch that fits the pool of 65 535 limb-polys if smaller);
    (b) hdotadd with da_scale = 0 and da_const = 1 against the composition from existing ops in the same run: hdot(T), hlincomb(A, lc_const = 1,
        rescale = 1) and hadd a level down, the sum of the three ops' times, with the launch counts;
    (c) hdotadd with A = 0 and both keys 0 against hdot at the same T in the same run;
    (d) its launch alone at l and l --batch records (35 and 350), the lists marshalled outside the timed region: hm_tensor_dotadd with A = 0 and
        scale = NULL against hm_tensor_dot at the same T, and with everything on: us per launch and achieved bytes per second by the
        (4T + 2A + 3) limb-poly model.
Median of --rounds interleaved rounds x --iters iterations behind --warmup-rounds untimed rounds, with the spread (max - min over the rounds).
Appends what it prints to --out.
    python3 tools/dotadd_bench.py [--rounds 5] [--iters 20] [--warmup-rounds 1] [--batch 10] [--label head] [--out profiles/dotadd.txt]"""
import argparse
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from homulator_amd import hip, host  # noqa: E402

POOL = 65535


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cfg", default="config_4.cfg")
    ap.add_argument("--logN", type=int, default=16, help="ring of --cfg (the launch-alone part makes its own contexts)")
    ap.add_argument("--levels", default="45,35,15")
    ap.add_argument("--shapes", default="2:1,4:2,8:4")
    ap.add_argument("--batch", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup-rounds", type=int, default=1, help="untimed interleaved rounds in front of the timed ones")
    ap.add_argument("--parts", default="abcd")
    ap.add_argument("--label", default="")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    L, ell, alpha = (int(x) for x in a.levels.split(","))
    shapes = [tuple(int(v) for v in x.split(":")) for x in a.shapes.split(",")]
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)
    fmt = lambda v: ", ".join(f"{x:.1f}" for x in v)
    med, spread = statistics.median, lambda v: max(v) - min(v)

    def race(ops, batch):
        """us per op of the batch of every entry of `ops` (an op, or a list of ops run one after the other: the sum), interleaved"""
        run = lambda op, iters: sum(o.execute(iters) for o in op) if isinstance(op, list) else op.execute(iters)
        for op in ops.values():
            run(op, 3)   # first-use tables
        t = {k: [] for k in ops}
        for r in range(a.warmup_rounds + a.rounds):
            for k, op in ops.items():
                v = run(op, a.iters) / batch / 1e3
                if r >= a.warmup_rounds:
                    t[k].append(v)
        return t

    def close(ops):
        for op in ops.values():
            for o in (op if isinstance(op, list) else [op]):
                o.close()
    launches = lambda op: sum(o.launch_count() for o in op) if isinstance(op, list) else op.launch_count()

    def fits(T, A, s, k, batch):
        """the largest batch up to `batch` whose limb-polys fit the pool: a copy takes hmult's plus (10 T + 3 T s + 6 A + k - 10) l"""
        probe = host.Op(a.cfg, "hmult", L, ell, alpha, backend=host.BACKEND_COUNT)
        import re
        top = max(int(x) for ln in probe.plan(full=True) for f in re.findall(r"[ {](?:a|b|c|d|out|out1|out2|in)=([\d,]+)", ln) for x in f.split(",") if int(x) != hip.NO_LIMB)
        probe.close()
        per = top + 1 + (10 * T + 3 * T * s + 6 * A + k - 10) * ell
        return min(batch, POOL // per)

    say(f"# {a.label + ': ' if a.label else ''}{a.cfg} {L} {ell} {alpha} (us, median of {a.rounds} interleaved rounds x {a.iters} iterations; "
        f"spread = max - min over the rounds, after {a.warmup_rounds} untimed round(s))")

    for chain_bits in (0, 60):
        base = {"chain_bits": chain_bits} if chain_bits else {}
        name = "generic" if chain_bits else "mont32 "
        for want in (1, a.batch):
            for T, A in shapes:
                tag = f"{name} batch {{b:2d}} T {T} A {A}"
                if "a" in a.parts:   # ---- (a) the op, fused against fuse_dotadd = 0, all keys on
                    batch = fits(T, A, 1, 1, want)
                    ov = dict(base, batch=batch, terms=T, addends=A, da_scale=1, da_const=1)
                    ops = {"fused": host.Op(a.cfg, "hdotadd", L, ell, alpha, overrides=ov),
                           "fuse_dotadd=0": host.Op(a.cfg, "hdotadd", L, ell, alpha, overrides=dict(ov, fuse_dotadd=0))}
                    t = race(ops, batch)
                    for k, op in ops.items():
                        say(f"{tag.format(b=batch)} {k:14s} {med(t[k]):9.1f} us/op   launches {launches(op)}   spread {spread(t[k]):.1f}   (rounds: {fmt(t[k])})")
                    f, u = t["fused"], t["fuse_dotadd=0"]
                    d = med(f) - med(u)
                    say(f"{tag.format(b=batch)} (a) fused - fuse_dotadd=0 {d:+9.1f} us, {med(u) / med(f):.2f} x (spreads {spread(f):.1f} / {spread(u):.1f}): "
                        + ("faster by more than both spreads" if -d > max(spread(f), spread(u)) else "NOT faster by more than both spreads")
                        + (f"   [batch {batch}: the largest that fits the pool]" if batch != want else ""))
                    close(ops)
                if "b" in a.parts:   # ---- (b) without pair scalars, against hdot + hlincomb(rescale) + hadd
                    batch = fits(T, A, 0, 1, want)
                    ops = {"hdotadd": host.Op(a.cfg, "hdotadd", L, ell, alpha, overrides=dict(base, batch=batch, terms=T, addends=A, da_const=1)),
                           "composition": [host.Op(a.cfg, "hdot", L, ell, alpha, overrides=dict(base, batch=batch, terms=T)),
                                           host.Op(a.cfg, "hlincomb", L, ell, alpha, overrides=dict(base, batch=batch, terms=A, lc_const=1, rescale=1)),
                                           host.Op(a.cfg, "hadd", L, ell - 1, alpha, overrides=dict(base, batch=batch))]}
                    t = race(ops, batch)
                    for k, op in ops.items():
                        say(f"{tag.format(b=batch)} {k:14s} {med(t[k]):9.1f} us/op   launches {launches(op)}   spread {spread(t[k]):.1f}   (rounds: {fmt(t[k])})")
                    f, u = t["hdotadd"], t["composition"]
                    say(f"{tag.format(b=batch)} (b) hdotadd - composition {med(f) - med(u):+9.1f} us, {med(u) / med(f):.2f} x (spreads {spread(f):.1f} / {spread(u):.1f})")
                    close(ops)
                if "c" in a.parts:   # ---- (c) A = 0 without keys against hdot
                    batch = fits(T, 0, 0, 0, want)
                    ops = {"hdotadd A=0": host.Op(a.cfg, "hdotadd", L, ell, alpha, overrides=dict(base, batch=batch, terms=T, addends=0)),
                           "hdot": host.Op(a.cfg, "hdot", L, ell, alpha, overrides=dict(base, batch=batch, terms=T))}
                    t = race(ops, batch)
                    for k, op in ops.items():
                        say(f"{tag.format(b=batch)} {k:14s} {med(t[k]):9.1f} us/op   launches {launches(op)}   bytes {op.stage_bytes()}   spread {spread(t[k]):.1f}   (rounds: {fmt(t[k])})")
                    m, h = t["hdotadd A=0"], t["hdot"]
                    d = med(m) - med(h)
                    say(f"{tag.format(b=batch)} (c) hdotadd - hdot {d:+9.1f} us (spreads {spread(m):.1f} / {spread(h):.1f}): "
                        + ("level within the spreads" if abs(d) <= max(spread(m), spread(h)) else "NOT level within the spreads"))
                    close(ops)

    # ---- (d) the launch alone against hm_tensor_dot, the lists marshalled once
    for batch in ((1, a.batch) if "d" in a.parts else ()):
        n = ell * batch
        say(f"# (d) one launch of {n} records, N = 2^{a.logN}: hm_tensor_dotadd against hm_tensor_dot, us per launch and GB/s by the byte model")
        mods = [i % ell for i in range(n)]
        for backend in ("mont32", "generic"):
            if backend == "mont32":
                ctx = hip.Context(a.logN, L, alpha)
            else:
                from oracle.homoracle import chain_below
                m = chain_below(a.logN, 60, L + alpha)
                ctx = hip.Context(a.logN, L, alpha, q=m[:L], p=m[L:])
            Tmax, Amax = max(T for T, _ in shapes), max(A for _, A in shapes)
            W = 4 * Tmax + 2 * Amax
            src = ctx.alloc(n * W)
            small = min(range(ell), key=lambda m: ctx.moduli[m])   # residues of the smallest modulus are reduced under every record's
            ctx.fill_uniform(src, [small] * (n * W), 1)
            out = ctx.alloc(3 * n)
            lo = [hip._u32(list(range(r * n, (r + 1) * n))) for r in range(3)]
            km = hip._u32(mods)
            calls, model = {}, {}
            keep = []
            for T, A in shapes:
                ops = [hip._u32([(4 * t + r) * n + i for i in range(n) for t in range(T)]) for r in range(4)]
                lx0 = hip._u32([(4 * Tmax + 2 * r) * n + i for i in range(n) for r in range(A)])
                lx1 = hip._u32([(4 * Tmax + 2 * r + 1) * n + i for i in range(n) for r in range(A)])
                s = hip._u64([2 + i for i in range(n * T)])
                u = hip._u64([3 + i for i in range(n * A)])
                k = hip._u64([ctx.moduli[m] - 1 - i for i, m in enumerate(mods)])
                keep += [ops, lx0, lx1, s, u, k]
                P, O = src.ptr, out.ptr
                head = lambda ops=ops: (ctx.h, P, ops[0][1], P, ops[1][1], P, ops[2][1], P, ops[3][1])
                tail = (O, lo[0][1], O, lo[1][1], O, lo[2][1], km[1], n)
                calls[f"dot T={T}"] = lambda T=T, head=head: ctx._ck(ctx.L.hm_tensor_dot(*head(), *tail, T))
                calls[f"dotadd T={T} plain"] = lambda T=T, head=head: ctx._ck(ctx.L.hm_tensor_dotadd(*head(), None, None, None, *tail, T, 0, None, None, None))
                calls[f"dotadd T={T} A={A} all"] = lambda T=T, A=A, head=head, lx0=lx0, lx1=lx1, s=s, u=u, k=k: ctx._ck(
                    ctx.L.hm_tensor_dotadd(*head(), P, lx0[1], lx1[1], *tail, T, A, s[1], u[1], k[1]))
                model[f"dot T={T}"] = model[f"dotadd T={T} plain"] = 4 * T + 3
                model[f"dotadd T={T} A={A} all"] = 4 * T + 2 * A + 3
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
            for T, A in shapes:
                h = t[f"dot T={T}"]
                for key in (f"dot T={T}", f"dotadd T={T} plain", f"dotadd T={T} A={A} all"):
                    v = t[key]
                    say(f"{backend:8s} {key:22s} {med(v):8.1f} (spread {spread(v):.1f}, {gb(model[key], med(v)):5.0f} GB/s of {model[key]} limb-polys)"
                        + (f"   - dot {med(v) - med(h):+.1f} us" if key.endswith("plain") else "") + f"   (rounds: {fmt(v)})")
            src.free(); out.free()
            ctx.close()
    if a.out:
        with open(a.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
