"""The cohort genotype leg's integer pieces through the host harness (tests only)."""
import numpy as np

from tests.geno_sim import COHORT, PTR, U64, u8, call, layout as _layout
from tests.geno_sim import build_main                                                  # noqa: F401


def wave(w0, S, n_items):
    """svjg_geno.h: cohort_segment for the 64 lanes of the wave whose first item is w0 -> (mask uint64[64], leader uint8[64])"""
    mask, leader = np.zeros(64, np.uint64), np.zeros(64, np.uint8)
    call("genosim_cohort_wave", None, [U64] * 3 + [PTR] * 2, int(w0), int(S), int(n_items), mask, leader)
    return mask, leader


def sums(w0, S, n_items, gt, ploidy=None):
    """the wave whose first item is w0: the kernel's nine ballots from gt / ploidy (uint8 per item; gt 0xFF: no call), or with ploidy None the
    diploid kernel's three from gt (3: no call); svjg_geno.h: cohort_segment and cohort_ploidy_sums / cohort_diploid_sums -> (leader uint8[64], ns, an, ac uint32[64], word uint64[64]); the sums are 0 on a lane that is no leader"""
    gt = u8(gt)
    if ploidy is not None:
        ploidy = u8(ploidy)
    assert len(gt) == n_items and (ploidy is None or len(ploidy) == n_items)
    leader = np.zeros(64, np.uint8)
    ns, an, ac = (np.zeros(64, np.uint32) for _ in range(3))
    word = np.zeros(64, np.uint64)
    call("genosim_cohort_sums", None, [U64] * 3 + [PTR] * 7, int(w0), int(S), int(n_items), gt, ploidy, leader, ns, an, ac, word)
    return leader, ns, an, ac, word


def layout(n_rows, S, max_ploidy=2, per_item=False, prior=False):
    """svjg_geno.h: cohort_layout -> dict of byte offsets (and in_bytes, total); a field the call does not have is 0"""
    return _layout(COHORT, n_rows, S, max_ploidy, int(bool(per_item)) | int(bool(prior)) << 1)
