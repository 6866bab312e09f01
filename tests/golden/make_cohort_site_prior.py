"""Writes tests/golden/cohort_site_prior/<case>.npz: the 60-digit model's answers (tests/site_prior_model.py) for the cases of
tests/cohort_site_prior_cases.py at min_support 0.  Run from the repository root: python tests/golden/make_cohort_site_prior.py [case ...]
(minutes over all cases; several processes).  A case's seed must keep the undecided items within the model's cap of 1 % and leave no site inside
the stopping rule's band (the steps are compared on EVERY site): with --search the first seed of seed + 1000 k that does is printed, to be entered
in tests/cohort_site_prior_cases.py: _SEED_OVERRIDE; without it a case outside fails."""
import multiprocessing
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", ".."))

from tests import cohort_site_prior_cases as CS  # noqa: E402
from tests import site_prior_model as M  # noqa: E402


def answer(name, seed=None):
    c = CS.inputs(name, seed)
    members, raw = CS.first_kernel(c)
    res = M.run(raw, members, c["C"], CS.ERR, 0)
    site_out, item_out = M.outside(res)
    return c, res, site_out, item_out


def make(arg):
    name, search = arg
    seed = CS.case_of(name)[4]
    while True:
        c, res, site_out, item_out = answer(name, seed)
        share = item_out.mean()
        if share <= M.CAP and not site_out.any():
            break
        if not search:
            raise SystemExit("%s: %.2f %% of the items undecided, %d sites in the band: run with --search" % (name, 100 * share, site_out.sum()))
        seed += 1000
    if seed != CS.case_of(name)[4]:
        return "%s: enter seed %d in _SEED_OVERRIDE and run again" % (name, seed)
    os.makedirs(CS.GOLDEN, exist_ok=True)
    np.savez_compressed(CS.golden_path(name), digest=CS.digest(c), p_hi=res["p_hi"], p_lo=res["p_lo"].astype(np.float32), steps=res["steps"], flag=res["flag"],
                        site_out=site_out, sgt=res["sgt"], sgq=res["sgq"], item_out=np.packbits(item_out.reshape(-1)))
    est = ~np.isnan(res["p_hi"][:, 0])
    return "%s: %d sites with an estimate, steps mean %.1f max %d, %d not converged, %.3f %% of the items undecided" % (
        name, est.sum(), res["steps"][est].mean() if est.any() else 0, res["steps"].max(), res["flag"].sum(), 100 * item_out.mean())


if __name__ == "__main__":
    args = [a for a in sys.argv[1:] if a != "--search"]
    names = args or [c[0] for c in CS.CASES]
    with multiprocessing.Pool(min(16, os.cpu_count() or 1)) as pool:
        for line in pool.imap_unordered(make, [(n, "--search" in sys.argv) for n in names]):
            print(line, flush=True)
