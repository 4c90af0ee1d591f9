"""hm_encode on one device: encodes per second at N = 2^16 onto n_mod = 50 moduli (config_4 45/35/15's extended basis,
l + alpha = 35 + 15), n_vec = 1 and 16, on device-resident slots; beside it the slot transform's share of the call (the same call with n_mod = 0:
the two k_slot_fft launches alone) and the same encode on the host through tests/slots_ref.py's transform path (longdouble) and through the same
radix-2 network in numpy complex128 (what a caller without the library would run), each followed by the oracle's 50 forward transforms.
One untimed interleaved round runs in front of the timed ones.  No threshold is set.  Appends what it prints to --out.
    python3 tools/encode_bench.py [--rounds 5] [--iters 20] [--host-iters 1] [--out profiles/encode.txt]"""
import argparse
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from homulator_amd import hip  # noqa: E402


def host_encode_double(z, logN, scale):
    """slots_ref.fft_coeffs's network in complex128: coefficients as int64"""
    import slots_ref as R
    N, n = 1 << logN, 1 << (logN - 1)
    e = R.rot_group(logN)
    v = np.array(z, dtype=np.complex128)
    ln = n
    while ln >= 2:
        h = ln // 2
        w = np.exp(-1j * np.pi * ((e[:h] % (4 * ln)) * (n // ln)) / N)
        v2 = v.reshape(-1, ln)
        a, b = v2[:, :h].copy(), v2[:, h:].copy()
        v2[:, :h], v2[:, h:] = a + b, (a - b) * w
        ln //= 2
    u = np.empty(n, dtype=np.complex128)
    u[R._bitrev(n)] = v
    return np.rint(np.concatenate([u.real, u.imag]) * (scale / n)).astype(np.int64)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--logN", type=int, default=16)
    ap.add_argument("--levels", default="45,15", help="L, K of the context")
    ap.add_argument("--n-mod", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--host-iters", type=int, default=1)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    L, K = (int(x) for x in a.levels.split(","))
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)
    med, spread = statistics.median, lambda v: max(v) - min(v)
    N, n, scale = 1 << a.logN, 1 << (a.logN - 1), 2.0 ** 40
    mods = list(range(a.n_mod - K)) + [L + i for i in range(K)]
    say(f"# hm_encode, N = 2^{a.logN}, n_mod = {a.n_mod}, Delta = 2^40 (us per call, median of {a.rounds} interleaved rounds x {a.iters} iterations behind one "
        f"untimed round; spread = max - min)")
    for backend in ("mont32", "generic"):
        if backend == "mont32":
            ctx = hip.Context(a.logN, L, K)
        else:
            from oracle.homoracle import chain_below
            m = chain_below(a.logN, 60, L + K)
            ctx = hip.Context(a.logN, L, K, q=m[:L], p=m[L:])
        calls = {}
        rng = np.random.default_rng(1)
        for n_vec in (1, 16):
            z = np.sqrt(rng.uniform(0, 1, (n_vec, n))) * np.exp(2j * np.pi * rng.uniform(0, 1, (n_vec, n)))
            zb = ctx.from_host(z.view(np.uint64).reshape(n_vec, N))
            work, out = ctx.alloc(n_vec), ctx.alloc(n_vec * a.n_mod)
            calls[(n_vec, "encode")] = lambda zb=zb, work=work, out=out, n_vec=n_vec: ctx.encode(zb, scale, mods, n_vec=n_vec, work=work, out=out)
            calls[(n_vec, "transform")] = lambda zb=zb, work=work, n_vec=n_vec: ctx.encode(zb, scale, [], n_vec=n_vec, work=work)
        for f in calls.values():
            f()   # first-use tables
        ctx.sync()
        assert ctx.counter("encode_overflow") == 0
        t = {k: [] for k in calls}
        for r in range(1 + a.rounds):
            for k, f in calls.items():
                ctx.timer_start()
                for _ in range(a.iters):
                    f()
                v = ctx.timer_stop() / a.iters / 1e3
                if r:
                    t[k].append(v)
        for n_vec in (1, 16):
            e, tr = t[(n_vec, "encode")], t[(n_vec, "transform")]
            say(f"{backend:8s} n_vec {n_vec:2d}: encode {med(e):8.1f} us (spread {spread(e):.1f}) = {n_vec * 1e6 / med(e):9.0f} encodes/s   slot transform alone "
                f"{med(tr):7.1f} us (spread {spread(tr):.1f}) = {100 * med(tr) / med(e):4.1f} % of the call")
        ctx.close()
    # the host paths, one vector
    import slots_ref as R
    from oracle.homoracle import Oracle
    o = Oracle(a.logN, L, K)
    o.set_threads(16)
    z = np.sqrt(rng.uniform(0, 1, n)) * np.exp(2j * np.pi * rng.uniform(0, 1, n))
    for name, coeffs in (("longdouble (tests/slots_ref.py)", lambda: R.encode_int(z, a.logN, scale, R.fft_coeffs)),
                         ("complex128 (numpy)", lambda: host_encode_double(z, a.logN, scale))):
        ts, tn = [], []
        for _ in range(a.host_iters):
            t0 = time.perf_counter()
            c = coeffs()
            t1 = time.perf_counter()
            res = np.stack([np.array([int(x) % o.moduli[m] for x in c], dtype=np.uint64) for m in mods])
            o.ntt(mods, res)
            t2 = time.perf_counter()
            ts.append(t1 - t0)
            tn.append(t2 - t1)
        say(f"host     n_vec  1: {name}: transform and rounding {med(ts) * 1e3:8.1f} ms, residues and {a.n_mod} oracle transforms (16 threads) {med(tn) * 1e3:8.1f} ms "
            f"= {1 / (med(ts) + med(tn)):6.2f} encodes/s")
    if a.out:
        with open(a.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
