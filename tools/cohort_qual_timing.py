#!/usr/bin/env python3
"""svjg_cohort_qual on one GPU: every row has a slot, counts 0..60, e = 5e-5, theta = 1e-3.

  (a) 100 000 rows x 64 samples, every item diploid (ploidy NULL)
  (b) the same matrix with ploidies 1..8 mixed within rows at max_ploidy 8
  (c) 2 000 rows x 1 024 samples, diploid: a row's y takes 32 trips of the wave over k at the end

Median of 30 calls behind 5, genotype_ms of svjg_last_kernel_ms (the event pair around the call's one launch), the legs run twice in one process.
Beside it the wall time of a call from Python and the mean of chroms.  One JSON line per reading.  A first reading: nothing is compared against it.

    python tools/cohort_qual_timing.py [--rows N] [--big-rows N] [--calls K] [--warmup W]
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "svjedi-graph_amd"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=100_000)
    ap.add_argument("--big-rows", type=int, default=2_000)
    ap.add_argument("--calls", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    args = ap.parse_args()
    from svjg import capi
    e, theta = 5e-5, 1e-3
    ctx = capi.Context(0)
    ctx.logfact_reserve(1 << 16)

    def leg(fn):
        k, w, last = [], [], None
        for _ in range(args.warmup + args.calls):
            t0 = time.perf_counter()
            last = fn()
            w.append((time.perf_counter() - t0) * 1e3)
            k.append(ctx.kernel_ms()[2])
        return statistics.median(k[args.warmup:]), statistics.median(w[args.warmup:]), last

    for S, R in ((64, args.rows), (1024, args.big_rows)):
        rng = np.random.default_rng(100 + S)
        t = rng.integers(0, 4, size=R).astype(np.uint8)
        slot = np.arange(R, dtype=np.uint32)
        ok1 = np.full(R, 1, np.uint8)
        counts = rng.integers(0, 61, size=(R, S, 2)).astype(np.uint32)
        mixed = rng.integers(1, 9, size=(R, S)).astype(np.uint8)
        ctx.cohort_alloc(S, R)
        for s in range(S):
            ctx.cohort_set_counts(s, slot, counts[:, s])
        legs = [("cohort_qual", lambda: ctx.cohort_qual(t, slot, ok1, None, 2, e, theta))]
        if S == 64:
            legs.append(("cohort_qual_1to8", lambda: ctx.cohort_qual(t, slot, ok1, mixed, 8, e, theta)))
        for turn in (1, 2):
            for name, fn in legs:
                k, w, last = leg(fn)
                print(json.dumps({"samples": S, "leg": name, "turn": turn, "rows": R, "kernel_ms": round(k, 4), "wall_ms": round(w, 3),
                                  "chroms_mean": round(float(last[2].mean()), 2), "qual_nan": int(np.isnan(last[0]).sum())}), flush=True)
    ctx.close()


if __name__ == "__main__":
    main()
