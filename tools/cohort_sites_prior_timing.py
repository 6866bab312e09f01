#!/usr/bin/env python3
"""svjg_genotype_cohort_sites_prior against svjg_genotype_cohort_sites alone on the same matrix, on one GPU: 10 000 candidate sites, 64 and 256
samples, K mixed 2..6, every candidate present for a sample with probability 0.9, counts 0..60, e = 5e-5.  The parent has no such kernel: the only
comparison is the first kernel alone, and what the second one adds.

  (a) svjg_genotype_cohort_sites: k_genotype_cohort_sites
  (b) svjg_genotype_cohort_sites_prior: the same kernel and k_cohort_sites_prior behind it (both in genotype_ms)

Median of 30 calls behind 5, genotype_ms of svjg_last_kernel_ms (the event pair around the launches), the legs alternated twice in one process;
beside it the mean and the maximum of the EM's steps over the sites with an estimate.  One JSON line per reading; nothing is asserted.

Measured once, with the change that added it (one MI355X, 2026-10-21, ROCm 7.2.0, the defaults): see DESIGN.md 4.3.

    python tools/cohort_sites_prior_timing.py [--sites N] [--samples S [S ...]] [--calls K] [--warmup W]
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "svjedi-graph_amd"))
NONE = 0xFFFFFFFF


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sites", type=int, default=10_000)
    ap.add_argument("--samples", type=int, nargs="+", default=[64, 256])
    ap.add_argument("--calls", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    args = ap.parse_args()
    from svjg import capi
    N, ms, e = args.sites, 3, 5e-5
    for S in args.samples:
        rng = np.random.default_rng(1)
        K = rng.integers(2, 7, N)
        slots = np.full((N, 6), NONE, np.uint32)
        ok = np.arange(6)[None, :] < K[:, None]
        n_slots = int(K.sum())
        slots[ok] = np.arange(n_slots, dtype=np.uint32)
        counts = rng.integers(0, 61, size=(S, n_slots, 2)).astype(np.uint32)
        present = rng.random((S, n_slots)) < 0.9
        ctx = capi.Context(0)
        ctx.cohort_alloc(S, n_slots)
        for s in range(S):
            sl = np.flatnonzero(present[s]).astype(np.uint32)
            ctx.cohort_set_counts(s, sl, counts[s, sl])
        ctx.logfact_reserve(1 << 16)
        steps = {}

        def leg(call):
            k = []
            for i in range(args.warmup + args.calls):
                out = call(slots, ms, e)
                k.append(ctx.kernel_ms()[2])
            if len(out) == 11:
                st = out[9][~np.isnan(out[8][:, 0])] & 0x7FFFFFFF
                steps.update(mean=round(float(st.mean()), 2), max=int(st.max()), not_converged=int((out[9] >> 31).sum()))
            return statistics.median(k[args.warmup:])

        for turn in (1, 2):
            a = leg(ctx.genotype_cohort_sites)
            b = leg(ctx.genotype_cohort_sites_prior)
            print(json.dumps({"turn": turn, "sites": N, "samples": S, "a_cohort_sites_ms": round(a, 4), "b_cohort_sites_prior_ms": round(b, 4),
                              "second_kernel_ms": round(b - a, 4), "em_steps": steps}), flush=True)
        ctx.close()


if __name__ == "__main__":
    main()
