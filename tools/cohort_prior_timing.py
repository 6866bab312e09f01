#!/usr/bin/env python3
"""svjg_genotype_cohort_prior against the cohort call without the prior, on one GPU: 100 000 rows with a slot each, counts 0..60, e = 5e-5.

  (a) svjg_genotype_cohort alone against svjg_genotype_cohort_prior (ploidy NULL), 64 samples
  (b) svjg_genotype_cohort_ploidy against svjg_genotype_cohort_prior, ploidies 1..8 mixed within rows at max_ploidy 8, 64 samples
  (c) the pair of (a) at 4 samples (16 rows a wave) and at 256 samples (a lane strides over four items)
  (d) at 256 samples: the further items of a lane recomputed at every EM step against staged in LDS (SVJG_PRIOR_STAGE)

Median of 30 calls behind 5, genotype_ms of svjg_last_kernel_ms (the event pair around the call's launches: both kernels of the prior call), the
legs alternated twice in one process; the added milliseconds are prior - alone.  Beside it the mean and the maximum of the EM steps.  One JSON
line per reading.

    python tools/cohort_prior_timing.py [--rows N] [--calls K] [--warmup W]
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
FLAG = 1 << 31


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=100_000)
    ap.add_argument("--calls", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    args = ap.parse_args()
    from svjg import capi
    R, ms, e = args.rows, 3, 5e-5
    t = np.random.default_rng(1).integers(0, 4, size=R).astype(np.uint8)
    slot = np.arange(R, dtype=np.uint32)
    ok1 = np.full(R, 1, np.uint8)
    ctx = capi.Context(0)
    ctx.logfact_reserve(1 << 16)
    out = {}

    def leg(fn, stage=None):
        if stage is None:
            os.environ.pop("SVJG_PRIOR_STAGE", None)
        else:
            os.environ["SVJG_PRIOR_STAGE"] = stage
        k, w, last = [], [], None
        for i in range(args.warmup + args.calls):
            t0 = time.perf_counter()
            last = fn()
            w.append((time.perf_counter() - t0) * 1e3)
            k.append(ctx.kernel_ms()[2])
        os.environ.pop("SVJG_PRIOR_STAGE", None)
        return statistics.median(k[args.warmup:]), statistics.median(w[args.warmup:]), last

    for S in (64, 4, 256):
        rng = np.random.default_rng(100 + S)
        counts = rng.integers(0, 61, size=(R, S, 2)).astype(np.uint32)
        mixed = rng.integers(1, 9, size=(R, S)).astype(np.uint8)
        ctx.cohort_alloc(S, R)
        for s in range(S):
            ctx.cohort_set_counts(s, slot, counts[:, s])
        legs = [("cohort", lambda: ctx.genotype_cohort(t, slot, ok1, ms, e), None),
                ("cohort_prior", lambda: ctx.genotype_cohort_prior(t, slot, ok1, None, 2, ms, e), None)]
        if S == 64:
            legs += [("cohort_ploidy_1to8", lambda: ctx.genotype_cohort_ploidy(t, slot, ok1, mixed, 8, ms, e), None),
                     ("cohort_prior_1to8", lambda: ctx.genotype_cohort_prior(t, slot, ok1, mixed, 8, ms, e), None)]
        if S == 256:
            legs = [legs[0], ("cohort_prior_recompute", legs[1][1], "recompute"), ("cohort_prior_lds", legs[1][1], "lds")]
        for turn in (1, 2):
            for name, fn, stage in legs:
                k, w, last = leg(fn, stage)
                out[(S, name, turn)] = k
                line = {"samples": S, "leg": name, "turn": turn, "rows": R, "kernel_ms": round(k, 4), "wall_ms": round(w, 3)}
                if len(last) == 9:
                    steps = last[8] & ~np.uint32(FLAG)
                    line.update(em_steps_mean=round(float(steps.mean()), 3), em_steps_max=int(steps.max()), not_converged=int(((last[8] & FLAG) != 0).sum()))
                print(json.dumps(line), flush=True)
    ctx.close()
    for (S, name, turn), k in sorted(out.items()):
        if name.startswith("cohort_prior"):
            base = out[(S, "cohort_ploidy_1to8" if name.endswith("1to8") else "cohort", turn)]
            print(json.dumps({"samples": S, "leg": name, "turn": turn, "added_ms": round(k - base, 4)}), flush=True)


if __name__ == "__main__":
    main()
