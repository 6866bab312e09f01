#!/usr/bin/env python3
"""svjg_genotype_cohort_ploidy against what it replaces, on one GPU: 100 000 rows with a slot each, 64 samples, counts 0..60, e = 5e-5.

  (a) the new call, "sex" pattern (ploidy 0 / 1 / 2 by row class and sample), max_ploidy 2
  (b) the new call, ploidies 1..8 mixed within rows, max_ploidy 8
  (c) svjg_genotype_cohort on the same matrix: the diploid kernel, the cost of generality
  (d) the loop 64 x (svjg_set_counts + svjg_genotype_ploidy) with the columns of (a) and of (b): kernels summed, and wall time

Median of 30 calls behind 5, genotype_ms of svjg_last_kernel_ms (the event pair around the launch), the legs alternated twice in one process;
beside it the wall time of one Python call and the bytes it moves.  One JSON line per reading.

    python tools/cohort_ploidy_timing.py [--rows N] [--samples S] [--calls K] [--warmup W]
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
    ap.add_argument("--samples", type=int, default=64)
    ap.add_argument("--calls", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    args = ap.parse_args()
    from svjg import capi
    R, S, ms, e = args.rows, args.samples, 3, 5e-5
    rng = np.random.default_rng(1)
    counts = rng.integers(0, 61, size=(R, S, 2)).astype(np.uint32)
    t = rng.integers(0, 4, size=R).astype(np.uint8)
    slot = np.arange(R, dtype=np.uint32)
    ok1, ok3 = np.full(R, 1, np.uint8), np.full(R, 3, np.uint8)
    male = rng.random(S) < 0.5
    sex = np.array([[2, 2], [2, 1], [0, 1]], np.uint8)[rng.integers(0, 3, R)][:, male.astype(np.int64)]
    mixed = rng.integers(1, 9, size=(R, S)).astype(np.uint8)

    ctx = capi.Context(0)
    ctx.cohort_alloc(S, R)
    for s in range(S):
        ctx.cohort_set_counts(s, slot, counts[:, s])
    ctx.alloc_counts(R)
    ctx.logfact_reserve(1 << 16)

    def one_call(fn):
        def leg():
            k, w = [], []
            for i in range(args.warmup + args.calls):
                t0 = time.perf_counter()
                fn()
                w.append((time.perf_counter() - t0) * 1e3)
                k.append(ctx.kernel_ms()[2])
            return statistics.median(k[args.warmup:]), statistics.median(w[args.warmup:])
        return leg

    def loop(ploidy):
        def leg():
            k, w = [], []
            for i in range(args.warmup + args.calls):
                t0 = time.perf_counter()
                ksum = 0.0
                for s in range(S):
                    ctx.set_counts(counts[:, s])
                    ctx.genotype_ploidy(t, slot, ok3, ploidy[:, s], ms, e)
                    ksum += ctx.kernel_ms()[2]
                w.append((time.perf_counter() - t0) * 1e3)
                k.append(ksum)
            return statistics.median(k[args.warmup:]), statistics.median(w[args.warmup:])
        return leg

    def moved(mp):
        n = R * S
        return {"to_host": n * (8 * (mp + 1) + 11) + 16 * R + 8, "to_device": 720 + 6 * R + n}

    legs = [("a_cohort_ploidy_sex_max2", one_call(lambda: ctx.genotype_cohort_ploidy(t, slot, ok1, sex, 2, ms, e)), moved(2)),
            ("b_cohort_ploidy_1to8_max8", one_call(lambda: ctx.genotype_cohort_ploidy(t, slot, ok1, mixed, 8, ms, e)), moved(8)),
            ("c_cohort_diploid", one_call(lambda: ctx.genotype_cohort(t, slot, ok1, ms, e)), {"to_host": R * S * 35 + 8 * R + 8, "to_device": 6 * R}),
            ("d_loop_ploidy_sex", loop(sex), None),
            ("d_loop_ploidy_1to8", loop(mixed), None)]
    out = {}
    for turn in (1, 2):
        for name, leg, b in legs:
            k, w = leg()
            out[(name, turn)] = k
            line = {"leg": name, "turn": turn, "rows": R, "samples": S, "kernel_ms": round(k, 4), "wall_ms": round(w, 3)}
            if b:
                line["bytes"] = b
            print(json.dumps(line), flush=True)
    ctx.close()
    for turn in (1, 2):
        for new, old in (("a_cohort_ploidy_sex_max2", "d_loop_ploidy_sex"), ("b_cohort_ploidy_1to8_max8", "d_loop_ploidy_1to8")):
            a, d = out[(new, turn)], out[(old, turn)]
            print(json.dumps({"turn": turn, "claim": "%s below %s (kernels summed)" % (new, old), "holds": bool(a < d), "ratio": round(d / a, 2) if a else None}), flush=True)


if __name__ == "__main__":
    main()
