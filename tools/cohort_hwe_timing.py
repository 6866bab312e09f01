#!/usr/bin/env python3
"""svjg_cohort_hwe on one GPU: 100 000 rows x 64 samples and 10 000 rows x 2 048 samples, genotypes drawn in Hardy-Weinberg proportions at an
allele frequency per row between 0.01 and 0.5, every item diploid (ploidy NULL).

Median of `--calls` calls behind `--warmup`, genotype_ms of svjg_last_kernel_ms (the event pair around the kernel), every shape run twice in one
process; beside it the wall time of a call from Python and, once per shape, the single-thread wall time of the host harness (tests/geno_sim, topic hwe: the
kernel's own routines and loops compiled with g++ -O2) for the same call, with which the call's counts are compared bit for bit and its p-values
to 1e-9 relative.  One JSON line per reading.  A first reading: nothing is compared against the times.

    python tools/cohort_hwe_timing.py [--shapes ROWSxSAMPLES ...] [--calls K] [--warmup W]
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
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", nargs="+", default=["100000x64", "10000x2048"])
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    args = ap.parse_args()
    from svjg import capi
    from tests.geno_sim import hwe as hwe_sim
    ctx = capi.Context(0)
    hwe_sim.constants()                                          # (the harness library is built here, not inside a timed call)
    for shape in args.shapes:
        rows, S = (int(x) for x in shape.split("x"))
        rng = np.random.default_rng(500 + S)
        f = rng.uniform(0.01, 0.5, (rows, 1))
        gt = ((rng.random((rows, S)) < f).astype(np.uint8) + (rng.random((rows, S)) < f).astype(np.uint8)).astype(np.uint8)
        t0 = time.perf_counter()
        want = hwe_sim.run(gt)
        harness_s = time.perf_counter() - t0
        for turn in (1, 2):
            k, w, last = [], [], None
            for _ in range(args.warmup + args.calls):
                t0 = time.perf_counter()
                last = ctx.cohort_hwe(gt)
                w.append((time.perf_counter() - t0) * 1e3)
                k.append(ctx.kernel_ms()[2])
            rel = float(np.max(np.abs(last[1] - want[1]) / want[1]))
            agrees = bool(np.array_equal(last[0], want[0]) and rel <= 1e-9)
            print(json.dumps({"rows": rows, "samples": S, "turn": turn, "kernel_ms": round(statistics.median(k[args.warmup:]), 4),
                              "wall_ms": round(statistics.median(w[args.warmup:]), 3), "harness_wall_s": round(harness_s, 3),
                              "largest_relative_difference": rel, "agrees_with_harness": agrees}), flush=True)
            if not agrees:
                sys.exit(1)
    ctx.close()


if __name__ == "__main__":
    main()
