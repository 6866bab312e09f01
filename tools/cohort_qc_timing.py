#!/usr/bin/env python3
"""svjg_cohort_qc on one GPU: 10 000 rows x 64, 256 and 2 048 samples, calls 0 / 1 / 2 / no call at 0.45 / 0.3 / 0.15 / 0.1, every item diploid
(ploidy NULL).

Median of `--calls` calls behind `--warmup`, genotype_ms of svjg_last_kernel_ms (the event pair around the memset and both kernels), every shape
run twice in one process; beside it the wall time of a call from Python and, once per shape, the wall time of the numpy model
(tests/cohort_qc_model.py) on the same machine, with which the call's outputs are compared.  One JSON line per reading.  A first reading: nothing
is compared against the times.

    python tools/cohort_qc_timing.py [--rows N] [--samples S ...] [--calls K] [--warmup W]
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
    ap.add_argument("--rows", type=int, default=10_000)
    ap.add_argument("--samples", type=int, nargs="+", default=[64, 256, 2048])
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    args = ap.parse_args()
    from svjg import capi
    from tests import cohort_qc_model
    ctx = capi.Context(0)
    for S in args.samples:
        rng = np.random.default_rng(300 + S)
        gt = rng.choice(np.array([0, 1, 2, 3], np.uint8), size=(args.rows, S), p=[0.45, 0.3, 0.15, 0.1])
        t0 = time.perf_counter()
        want = cohort_qc_model.qc(gt)
        model_s = time.perf_counter() - t0
        for turn in (1, 2):
            k, w, last = [], [], None
            for _ in range(args.warmup + args.calls):
                t0 = time.perf_counter()
                last = ctx.cohort_qc(gt)
                w.append((time.perf_counter() - t0) * 1e3)
                k.append(ctx.kernel_ms()[2])
            equal = bool(np.array_equal(last[0], want[0]) and np.array_equal(last[1], want[1]))
            print(json.dumps({"samples": S, "rows": args.rows, "pairs": int(len(last[1])), "turn": turn, "kernel_ms": round(statistics.median(k[args.warmup:]), 4),
                              "wall_ms": round(statistics.median(w[args.warmup:]), 3), "model_wall_s": round(model_s, 3), "equals_model": equal}), flush=True)
            if not equal:
                sys.exit(1)
    ctx.close()


if __name__ == "__main__":
    main()
