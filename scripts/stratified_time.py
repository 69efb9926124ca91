"""Stratified resampler against the Metropolis chain (B = 10) on the same weights, in one process.

Per (N, weight family): both device entry points on the torch stream, alternating A, B, A, B ... after a warm-up,
each call between two device events; the median of the per-call times is reported with the bytes model of the
stratified passes (8 N per pass over w -- two --, 8 N written and read for the tile-local prefix sums, 4 N for a)
as a fraction of 8 TB/s.  Then run() at N = 1e6, T = 100, d = 2 under each resampler (wall time, host loop
included).  Kernel times proper come from a separate `rocprofv3 --kernel-trace --stats` run of
`python scripts/stratified_time.py --trace` (the same calls, fewer repetitions, no run() leg).

    python scripts/stratified_time.py [--reps 50] [--json out.json] [--trace]
"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402
import torch  # noqa: E402

import cusmc_amd  # noqa: E402

HBM = 8e12


def families(N, g):
    x = torch.randn(N, 2, dtype=torch.float64, device="cuda", generator=g)
    dens = torch.exp(-0.5 * (x ** 2).sum(1) / 0.05) / (2 * np.pi * 0.05)  # d = 2 filter-like densities
    heavy = torch.full((N,), 1e-300, dtype=torch.float64, device="cuda")
    heavy[N // 3] = 1.0  # collapsed: one particle carries the mass
    return {"density_d2": dens, "uniform": torch.ones(N, dtype=torch.float64, device="cuda"), "collapsed": heavy}


def time_pair(fa, fb, reps, warm):
    for _ in range(warm):
        fa()
        fb()
    torch.cuda.synchronize()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(2 * reps)]
    for r in range(reps):
        for k, f in enumerate((fa, fb)):
            s, e = ev[2 * r + k]
            s.record()
            f()
            e.record()
    torch.cuda.synchronize()
    ta = [ev[2 * r][0].elapsed_time(ev[2 * r][1]) * 1e3 for r in range(reps)]
    tb = [ev[2 * r + 1][0].elapsed_time(ev[2 * r + 1][1]) * 1e3 for r in range(reps)]
    return float(np.median(ta)), float(np.median(tb))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--json", default=None)
    ap.add_argument("--trace", action="store_true", help="resampler calls only, 10 repetitions (for rocprofv3)")
    args = ap.parse_args()
    reps = 10 if args.trace else args.reps
    torch.cuda.set_device(0)
    ctx = cusmc_amd.api.default_context()
    ctx.use_torch_stream()
    g = torch.Generator(device="cuda").manual_seed(7)
    rows = []
    for N in (100_000, 1_000_000, 10_000_000):
        a = torch.empty(N, dtype=torch.int32, device="cuda")
        for fam, w in families(N, g).items():
            st = [0]

            def strat():
                st[0] += 1
                cusmc_amd.Sampler.stratified_dev(w, a, t=st[0], seed=3, ctx=ctx)

            def mh():
                st[0] += 1
                cusmc_amd.Sampler.metropolis_hastings_dev(w, a, B=10, t=st[0], seed=3, ctx=ctx)

            ts, tm = time_pair(strat, mh, reps, 3)
            model = 8 * N * 2 + 8 * N * 2 + 4 * N
            row = dict(N=N, weights=fam, stratified_us=round(ts, 2), metropolis_B10_us=round(tm, 2),
                       speedup=round(tm / ts, 2), model_bytes=model, hbm_fraction=round(model / (ts * 1e-6) / HBM, 3))
            rows.append(row)
            print(json.dumps(row), flush=True)
        del a
    out = {"resampler": rows}
    if not args.trace:
        # run() at N = 1e6, T = 100, d = 2 under each resampler (one warm-up call each, then alternating)
        rng = np.random.default_rng(1)
        d, T, N = 2, 100, 1_000_000
        I = np.eye(d)
        Y = np.cumsum(rng.standard_normal((T, d)) * 0.03, axis=0)
        runs = {"metropolis": [], "stratified": []}
        for it in range(4):
            for res in runs:
                t0 = time.perf_counter()
                cusmc_amd.run(N, d, T, Y.T, np.zeros(d), I, I, I, 1e-3 * I, 1e-3 * I, 0.0, res, "mvn", seed=11 + it)
                if it:
                    runs[res].append(time.perf_counter() - t0)
        out["run_N1e6_T100_d2_s"] = {k: round(float(np.median(v)), 4) for k, v in runs.items()}
        print(json.dumps(out["run_N1e6_T100_d2_s"]), flush=True)
    if args.json:
        with open(args.json, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
