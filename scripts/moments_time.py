"""Times of the weighted-moments kernels and of run() with and without history (profiles/moments_time.md).

    python scripts/moments_time.py             device-event times per call at N = 1e6, then run() at T = 100
    python scripts/moments_time.py --kernels   only the moments calls (for rocprofv3 --kernel-trace --stats)
    python scripts/moments_time.py --split DB  median kernel time per d from that run's rocprofv3 database (the
                                               torch kernels that make each d's inputs separate the d values)

Floors: two reads of X at 8 TB/s and N d (d + 1) flops at the 78.6 TF f64 matrix peak."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


DIMS = (2, 8, 16, 64, 128, 200, 256)


def split(db):
    import re
    import sqlite3
    rows = sqlite3.connect(db).execute("select name, duration from kernels order by start").fetchall()
    seg, prev, out = -1, True, {}
    for name, dur in rows:
        if "moments" not in name:
            seg += prev  # the first non-moments kernel after a run of moments kernels starts the next d
            prev = False
            continue
        prev = True
        short = re.sub(r"\(.*", "", re.sub(r"^(void )?(cusmc::)?", "", name))
        out.setdefault((DIMS[seg], short), []).append(dur / 1e3)
    for (d, k), v in out.items():
        v.sort()
        print(json.dumps({"d": d, "kernel": k, "calls": len(v), "median_us": round(v[len(v) // 2], 1)}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--kernels", action="store_true")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--split", metavar="DB")
    args = ap.parse_args()
    if args.split:
        return split(args.split)
    import torch
    import cusmc_amd
    from cusmc_amd import api
    N = 1000000
    ctx = api.default_context()
    ctx.use_torch_stream()
    rows = []
    for d in DIMS:
        X = torch.randn(N, d, dtype=torch.float64, device="cuda")
        w = torch.rand(N, dtype=torch.float64, device="cuda")
        m = torch.empty(d, dtype=torch.float64, device="cuda")
        P = torch.empty(d * d, dtype=torch.float64, device="cuda")
        st = torch.empty(2, dtype=torch.float64, device="cuda")
        for cov in (False, True):
            for _ in range(3):
                api.weighted_moments_dev(X, w, m, P if cov else None, st, ctx=ctx)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(args.reps):
                api.weighted_moments_dev(X, w, m, P if cov else None, st, ctx=ctx)
            e1.record()
            torch.cuda.synchronize()
            us = e0.elapsed_time(e1) * 1e3 / args.reps
            floor = max((2 if cov else 1) * 8.0 * N * d / 8e12, (N * d * (d + 1) / 78.6e12) if cov else 0.0) * 1e6
            rows.append({"d": d, "cov": cov, "us": round(us, 1), "floor_us": round(floor, 1),
                         "of_floor": round(floor / us, 3)})
            print(json.dumps(rows[-1]), flush=True)
        del X, w
    if args.kernels:
        return
    T = 100
    for d in (2, 64):
        I = np.eye(d)
        Y = np.zeros((d, T))
        for mode, kw in (("history", {}), ("summaries", {"summaries": True, "history": False}),
                         ("both", {"summaries": True})):
            kw = dict(kw)
            cusmc_amd.run(N, d, T, Y, np.zeros(d), I, I, 0.9 * I, I, 0.5 * I, 0.0, "stratified", "mvn", seed=1, **kw)
            best = 1e9
            for _ in range(3):
                t0 = time.perf_counter()
                cusmc_amd.run(N, d, T, Y, np.zeros(d), I, I, 0.9 * I, I, 0.5 * I, 0.0, "stratified", "mvn", seed=1,
                              **kw)
                best = min(best, time.perf_counter() - t0)
            print(json.dumps({"run": mode, "d": d, "N": N, "T": T, "ms": round(best * 1e3, 1)}), flush=True)


if __name__ == "__main__":
    main()
