#!/usr/bin/env python3
"""Writes tests/golden/cohort_qual/<case>.npz: the answers of the 60-digit model (tests/cohort_qual_model.py) for the cases of
tests/cohort_qual_cases.py.  Per case: chroms, mlac, qual as two doubles (qual = qual + qual_lo; NaN where no item takes part), the rows that a
comparison leaves out — mlac where the two largest phi_k y_k lie within a relative 1e-9 of each other, the script's text where 100 SVQ lies within
1e-6 of a half-integer — and a digest of the inputs.  Refuses a case whose left-out share exceeds the cap (pick another seed).  No device takes
part: this runs on the CPU, minutes on a few cores (het_2048: two rows of 2 048 steps over up to 4 097 entries each; the 18 cases of
cohort_qual_cases.SHAPE_CASES together: 15 s on eight cores, shallow_poly_512's two rows of 512 steps at ploidy 8 being the longest).

    python tests/golden/make_cohort_qual.py [case ...]
"""
import multiprocessing
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [ROOT, os.path.join(ROOT, "svjedi-graph_amd")]
from tests import cohort_qual_cases as QC       # noqa: E402
from tests import cohort_qual_model as M        # noqa: E402


def _rows(job):
    name, rows = job
    c = QC.inputs(name)
    done, raw = QC.gate(c)
    return name, rows, M.run(c["t"], raw, done, c["ploidy"], QC.ERR, QC.THETA, rows=rows)


def make(name, parts):
    c = QC.inputs(name)
    R = len(c["t"])
    m = None
    for _, rows, got in parts:
        if m is None:
            m = got
        else:
            for k in m:
                m[k][rows] = got[k][rows]
    has = ~np.isnan(m["qual"])
    mlac_out = has & (m["gap"] < QC.TOP_GAP)
    text_out = has & (m["half"] < QC.HALF_BAND)
    shares = (float(mlac_out.mean()), float(text_out.mean()))
    if max(shares) > QC.CAP:
        raise ValueError("%s: mlac of %.4f of the rows and the text of %.4f would be left out: another seed" % ((name,) + shares))
    os.makedirs(QC.GOLDEN, exist_ok=True)
    np.savez_compressed(QC.golden_path(name), digest=QC.digest(c), chroms=m["chroms"], mlac=m["mlac"], qual=m["qual"], qual_lo=m["qual_lo"].astype(np.float32),
                        mlac_out=mlac_out, text_out=text_out)
    return "%s: %d rows, %d with a quality (min %.3g, max %.6g), left out: mlac %d, text %d" % (
        name, R, int(has.sum()), float(np.nanmin(m["qual"])) if has.any() else 0.0, float(np.nanmax(m["qual"])) if has.any() else 0.0,
        int(mlac_out.sum()), int(text_out.sum()))


if __name__ == "__main__":
    names = sys.argv[1:] or [c[0] for c in QC.CASES + QC.EXTRA]
    jobs = []
    for name in names:
        _, S, R, _, _ = next(c for c in QC.CASES + QC.EXTRA if c[0] == name)
        step = 1 if S > 500 else 5 if S > 100 else 25               # the large rows one by one: the pool stays busy
        jobs += [(name, list(range(lo, min(R, lo + step)))) for lo in range(0, R, step)]
    jobs.sort(key=lambda j: -next(c[1] for c in QC.CASES + QC.EXTRA if c[0] == j[0]))
    parts = {name: [] for name in names}
    with multiprocessing.Pool(min(len(jobs), os.cpu_count() or 1)) as pool:
        for got in pool.imap_unordered(_rows, jobs):
            parts[got[0]].append(got)
    for name in names:
        print(make(name, parts[name]), flush=True)
