#!/usr/bin/env python3
"""Writes tests/golden/cohort_prior/<case>.npz: the answers of the 60-digit model (tests/cohort_prior_model.py) for the cases of
tests/cohort_prior_cases.py, at min_support 0 (the support gate is a comparison of counts: the tests apply it).  Per case: f as two doubles
(f = f_hi + f_lo), steps, flag, the rows and items that the comparisons leave out (the deciding step within 1e-6 of EM_TOL; -10 log10(rest) within
1e-6 of an integer; the two largest posteriors within 1e-9 of each other), the calls, a digest of the inputs, and how many items the prior
calls differently from the likelihood alone.  Refuses a case whose left-out share exceeds the cap (pick another seed).  Minutes on a few cores.

    python tests/golden/make_cohort_prior.py [case ...]
"""
import multiprocessing
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [ROOT, os.path.join(ROOT, "svjedi-graph_amd")]
from tests import cohort_prior_cases as CC      # noqa: E402
from tests import cohort_prior_model as M       # noqa: E402


def independent_gt(c, done, raw):
    """the call of the likelihood alone at min_support 0: the g with the largest l_g, no call for a tie or an item without reads"""
    from decimal import localcontext
    R, S = done.shape
    gt = np.full((R, S), M.NO_CALL, np.uint8)
    with localcontext() as ctx:
        ctx.prec = M.PREC
        for r in range(R):
            for s in np.flatnonzero(done[r]):
                P = 2 if c["ploidy"] is None else int(c["ploidy"][r, s])
                c1, c2 = M.norm_counts(int(c["t"][r]), int(raw[r, s, 0]), int(raw[r, s, 1]))
                w, gmax = M.weights(c1, c2, P, CC.ERR)
                if c1 + c2 > 0 and sum(1 for v in w if v == 1) == 1:
                    gt[r, s] = gmax
    return gt


def make(name):
    c = CC.inputs(name)
    done, raw = CC.gate(c)
    m = M.run(c["t"], raw, done, c["ploidy"], CC.ERR, 0)
    has = ~np.isnan(m["f_hi"])
    row_out = has & (np.abs(m["ratio"] - 1) <= CC.RATIO_BAND)
    part = ~np.isnan(m["gap"])
    item_out = part & ((m["gq_margin"] < CC.GQ_MARGIN) | (m["gap"] < CC.TOP_GAP))
    differs = int(((independent_gt(c, done, raw) != m["gt"]) & part & ~item_out & ~row_out[:, None]).sum())
    shares = (float(row_out.mean()), float((item_out | row_out[:, None]).mean()))
    if max(shares) > CC.CAP:
        raise ValueError("%s: %.4f of the rows and %.4f of the items would be left out: another seed" % ((name,) + shares))   # (an exception a pool hands on)
    os.makedirs(CC.GOLDEN, exist_ok=True)
    np.savez_compressed(CC.golden_path(name), digest=CC.digest(c), f_hi=m["f_hi"], f_lo=m["f_lo"].astype(np.float32), steps=m["steps"].astype(np.uint8),
                        flag=m["flag"], row_out=row_out, gt=m["gt"], gq=m["gq"], item_out=np.packbits(item_out), prior_differs=differs)
    return name, shares, differs, int(m["steps"].max()), float(m["steps"][has].mean()) if has.any() else 0.0, int(m["flag"].sum())


if __name__ == "__main__":
    names = sys.argv[1:] or [c[0] for c in CC.CASES]
    with multiprocessing.Pool(min(len(names), os.cpu_count() or 1)) as pool:
        for got in pool.imap_unordered(make, names):
            print("%s: left out %.4f of the rows, %.4f of the items; the prior changes %d calls; steps max %d mean %.1f, %d rows not converged" % (
                got[0], got[1][0], got[1][1], got[2], got[3], got[4], got[5]), flush=True)
