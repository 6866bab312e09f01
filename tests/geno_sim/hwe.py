"""The cohort site test for Hardy-Weinberg equilibrium (svjg_geno.h's HWE routines inside a restatement of the loops of k_cohort_hwe) through the
host harness (tests only)."""
import numpy as np

from tests.geno_sim import HWE, PTR, U32, U64, INT, calls, call, layout as _layout
from tests.geno_sim import build_main                                                  # noqa: F401
from tests.geno_sim.prior import width as segment_width                                # noqa: F401  (prior_segment_width: the lanes a row takes)

RUN_CODES = {1: "a store outside its field", 2: "an output word written twice or never", 3: "a table entry beyond the reserved ones",
             4: "the lanes of a segment disagree"}


def constants():
    """-> dict: max_samples, tpb (lanes a block), blocks_per_cu (the cap of the launch's grid)"""
    out = np.zeros(3, np.uint32)
    call("genosim_hwe_constants", None, [PTR], out)
    return dict(zip(("max_samples", "tpb", "blocks_per_cu"), (int(x) for x in out)))


def layout(n_rows, S, per_item):
    """svjg_geno.h: hwe_layout -> dict of byte offsets (and in_bytes, total)"""
    return _layout(HWE, n_rows, S, 0, int(bool(per_item)))


def row(n_ref, n_het, n_alt):
    """-> dict of hwe_row: n, m, par, het, h0 (the h the terms are relative to), terms"""
    out = np.zeros(6, np.uint32)
    call("genosim_hwe_row", None, [U32, U32, U32, PTR], int(n_ref), int(n_het), int(n_alt), out)
    return dict(zip(("n", "m", "par", "het", "h0", "terms"), (int(x) for x in out)))


def run(gt, ploidy=None, grid=0, n_cu=256):
    """the kernel's loops over a call (a grid of that many blocks; 0: the launch's own on n_cu units) -> (counts[n, 3] uint32, p[n, 2] float64)"""
    gt, ploidy, n, S = calls(gt, ploidy)
    counts, p = np.zeros((n, 3), np.uint32), np.zeros((n, 2), np.float64)
    rc = call("genosim_hwe_run", INT, [PTR, PTR, U64, U32, U32, U32, PTR, PTR], gt, ploidy, n, S, int(grid), int(n_cu), counts, p)
    assert rc == 0, RUN_CODES.get(rc, rc)
    return counts, p


class SimHwe:
    """cohort_hwe as capi.Context has it, answered by the harness"""

    def cohort_hwe(self, gt, ploidy=None):
        return run(gt, ploidy)
