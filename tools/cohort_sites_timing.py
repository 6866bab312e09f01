#!/usr/bin/env python3
"""svjg_genotype_cohort_sites against what it replaces, on one GPU: 10 000 candidate sites, 64 samples, K mixed 2..6, every candidate present for a
sample with probability 0.9, counts 0..60, e = 5e-5.

  (a) the new call: one launch over all (site, sample) items
  (b) the loop 64 x (svjg_set_counts + svjg_genotype_sites) on the same columns, each sample's sites compacted to its present members ahead of
      the timing: kernels summed, and wall time

Median of 30 calls behind 5, genotype_ms of svjg_last_kernel_ms (the event pair around the launch), the legs alternated twice in one process;
beside it the wall time of one Python call and the bytes it moves.  One JSON line per reading.

    python tools/cohort_sites_timing.py [--sites N] [--samples S] [--calls K] [--warmup W]
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
NONE = 0xFFFFFFFF


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sites", type=int, default=10_000)
    ap.add_argument("--samples", type=int, default=64)
    ap.add_argument("--calls", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    args = ap.parse_args()
    from svjg import capi
    N, S, ms, e = args.sites, args.samples, 3, 5e-5
    rng = np.random.default_rng(1)
    K = rng.integers(2, 7, N)
    slots = np.full((N, 6), NONE, np.uint32)
    ok = np.arange(6)[None, :] < K[:, None]
    n_slots = int(K.sum())
    slots[ok] = np.arange(n_slots, dtype=np.uint32)
    counts = rng.integers(0, 61, size=(S, n_slots, 2)).astype(np.uint32)
    present = rng.random((S, n_slots)) < 0.9
    own = []                                                     # per sample: its sites of two present members or more, compacted
    for s in range(S):
        bits = present[s][np.where(ok, slots, 0)] & ok
        has = np.flatnonzero(bits.sum(axis=1) >= 2)
        o = np.full((len(has), 6), NONE, np.uint32)
        for n, k in enumerate(has.tolist()):
            m = slots[k, bits[k]]
            o[n, :len(m)] = m
        own.append(o)

    ctx = capi.Context(0)
    ctx.cohort_alloc(S, n_slots)
    for s in range(S):
        sl = np.flatnonzero(present[s]).astype(np.uint32)
        ctx.cohort_set_counts(s, sl, counts[s, sl])
    ctx.alloc_counts(n_slots)
    ctx.logfact_reserve(1 << 16)

    def one_call():
        k, w = [], []
        for i in range(args.warmup + args.calls):
            t0 = time.perf_counter()
            ctx.genotype_cohort_sites(slots, ms, e)
            w.append((time.perf_counter() - t0) * 1e3)
            k.append(ctx.kernel_ms()[2])
        return statistics.median(k[args.warmup:]), statistics.median(w[args.warmup:])

    def loop():
        k, w = [], []
        for i in range(args.warmup + args.calls):
            t0 = time.perf_counter()
            ksum = 0.0
            for s in range(S):
                ctx.set_counts(counts[s])
                ctx.genotype_sites(own[s], ms, e)
                ksum += ctx.kernel_ms()[2]
            w.append((time.perf_counter() - t0) * 1e3)
            k.append(ksum)
        return statistics.median(k[args.warmup:]), statistics.median(w[args.warmup:])

    items = sum(len(o) for o in own)
    legs = [("a_cohort_sites", one_call, {"to_host": N * S * 256 + 48 * N + 8, "to_device": 128 + 24 * N}),
            ("b_loop_sites", loop, {"to_host": items * 255 + 8 * S, "to_device": S * (8 * n_slots + 128) + 24 * items})]
    out = {}
    for turn in (1, 2):
        for name, leg, b in legs:
            k, w = leg()
            out[(name, turn)] = k
            print(json.dumps({"leg": name, "turn": turn, "sites": N, "samples": S, "items_with_a_site": items, "kernel_ms": round(k, 4), "wall_ms": round(w, 3),
                              "bytes": b}), flush=True)
    ctx.close()
    for turn in (1, 2):
        a, b = out[("a_cohort_sites", turn)], out[("b_loop_sites", turn)]
        print(json.dumps({"turn": turn, "claim": "a_cohort_sites below b_loop_sites (kernels summed)", "holds": bool(a < b), "ratio": round(b / a, 2) if a else None}), flush=True)


if __name__ == "__main__":
    main()
