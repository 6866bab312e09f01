"""The any-ploidy genotype row arithmetic through the host harness (tests only)."""
import numpy as np

from tests.geno_sim import PLOIDY, PTR, U32, U64, F64, u8, u32, f64, call, layout as _layout
from tests.geno_sim import build_main, logfact_table, ploidy_log_table as log_table    # noqa: F401
from tests.hostsim.sim import genotype_rows as genotype_rows_diploid                   # noqa: F401  (geno_row has ONE exported driver)

NPL = 9                                  # svjg_geno.h: MAX_PLOIDY + 1


def genotype_rows(sv_type, counts, ploidy, min_support, err, tab):
    """geno_row_ploidy -> (gt: alt copies or 0xFF, pl[n, 9], near, status: 0 ok, 1 table too short, 2 beyond the cap)"""
    sv_type, counts, ploidy, tab = u8(sv_type), u32(counts), u8(ploidy), f64(tab)
    assert ploidy.min() >= 1 and ploidy.max() <= 8
    n = len(sv_type)
    gt, pl, near, st = np.zeros(n, np.uint8), np.zeros((n, NPL), np.int64), np.zeros(n, np.uint8), np.zeros(n, np.uint8)
    call("genosim_ploidy_rows", None, [PTR] * 3 + [U64, U32, F64, PTR, U32] + [PTR] * 4,
         sv_type, counts, ploidy, n, int(min_support), float(err), tab, len(tab), gt, pl, near, st)
    return gt, pl, near, st


def layout(n):
    """svjg_geno.h: ploidy_layout -> dict of byte offsets (and in_bytes, total)"""
    return _layout(PLOIDY, n)
