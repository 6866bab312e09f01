"""The cohort call with an allele-frequency prior through the host harness (tests only)."""
import numpy as np

from tests.geno_sim import PTR, U32, U64, F64, u8, u32, call
from tests.geno_sim import build_main                                                  # noqa: F401
from tests.geno_sim import cohort


def rows(sv_type, raw, done, ploidy, err, min_support, wave=False):
    """every row through genosim_prior_row, or with wave through genosim_prior_row_wave (every step's sum in the kernel's order)
    -> (f[R], steps[R] (bit 31: not converged), gt[R, S], gq[R, S], site[R, 3])"""
    raw, done = u32(raw), u8(done)
    R, S = done.shape
    if ploidy is not None:
        ploidy = u8(ploidy)
    f, steps = np.zeros(R), np.zeros(R, np.uint32)
    gt, gq, site = np.zeros((R, S), np.uint8), np.zeros((R, S), np.uint8), np.zeros((R, 3), np.uint32)
    for r in range(R):
        call("genosim_prior_row_wave" if wave else "genosim_prior_row", None, [U32, PTR, PTR, PTR, U64, F64, U32] + [PTR] * 5,
             int(sv_type[r]), raw[r], done[r], None if ploidy is None else ploidy[r], S, float(err), int(min_support), f[r:], steps[r:], gt[r], gq[r], site[r])
    return f, steps, gt, gq, site


def item(sv_type, ref, alt, P, err):
    """-> (the ploidy the EM sees, w[9], gmax)"""
    w, gmax = np.zeros(9), np.zeros(1, np.uint32)
    p = call("genosim_prior_item", U32, [U32] * 4 + [F64, PTR, PTR], int(sv_type), int(ref), int(alt), int(P), float(err), w, gmax)
    return p, w, int(gmax[0])


def width(S):
    return call("genosim_prior_width", U32, [U64], int(S))


def segment_grid(n_rows, S, tpb, n_cu, blocks_per_cu):
    """the blocks of a launch that gives every row a segment of width(S) lanes (k_cohort_prior, k_cohort_sites_prior, k_cohort_hwe)"""
    return call("genosim_segment_grid", U32, [U64, U64, U32, U32, U32], int(n_rows), int(S), int(tpb), int(n_cu), int(blocks_per_cu))


def constants(site=False):
    """-> (EM_TOL, EM_MAX_IT, EM_NOT_CONVERGED, EM_F_BOUND, or with site SITE_EM_P_BOUND)"""
    tol, f_bound, p_bound = np.zeros(1), np.zeros(1), np.zeros(1)
    it, bit = np.zeros(1, np.uint32), np.zeros(1, np.uint32)
    call("genosim_prior_constants", None, [PTR] * 5, tol, it, bit, f_bound, p_bound)
    return float(tol[0]), int(it[0]), int(bit[0]), float((p_bound if site else f_bound)[0])


def layout(n_rows, S, max_ploidy, per_item):
    """svjg_geno.h: cohort_layout with the prior -> dict of byte offsets (and in_bytes, total)"""
    return cohort.layout(n_rows, S, max_ploidy, per_item, prior=True)
