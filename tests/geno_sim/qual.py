"""The cohort site quality through the host harness (tests only)."""
import numpy as np

from tests.geno_sim import QUAL, PTR, U32, U64, INT, F64, u8, u32, call, layout as _layout
from tests.geno_sim import build_main                                                  # noqa: F401


def rows(sv_type, raw, done, ploidy, max_ploidy, err, theta, wave=False, every=0, only=None):
    """every row (or the rows `only`) through genosim_qual_row; wave: the sums over k in the kernel's order; every: steps between two rescalings (0: the
    call's own) -> (qual[R], mlac[R], chroms[R]); rows not asked for: NaN, 0, 0"""
    raw, done = u32(raw), u8(done)
    R, S = done.shape
    if ploidy is not None:
        ploidy = u8(ploidy)
    qual, mlac, chroms = np.full(R, np.nan), np.zeros(R, np.uint32), np.zeros(R, np.uint32)
    for r in (range(R) if only is None else only):
        call("genosim_qual_row", None, [INT, U32, PTR, PTR, PTR, U64, U32, F64, F64, U32] + [PTR] * 3,
             int(bool(wave)), int(sv_type[r]), raw[r], done[r], None if ploidy is None else ploidy[r], S, int(max_ploidy), float(err), float(theta), int(every),
             qual[r:], mlac[r:], chroms[r:])
    return qual, mlac, chroms


def item(sv_type, ref, alt, P, err):
    """-> (the ploidy the recurrence sees, w[9], (d0 hi, d0 lo))"""
    w, d0 = np.zeros(9), np.zeros(2)
    p = call("genosim_qual_item", U32, [U32] * 4 + [F64, PTR, PTR], int(sv_type), int(ref), int(alt), int(P), float(err), w, d0)
    return p, w, (float(d0[0]), float(d0[1]))


def every(m_max, max_ploidy):
    return call("genosim_qual_every", U32, [U32, U32], int(m_max), int(max_ploidy))


def constants():
    """-> dict: QUAL_ABS, QUAL_REL, the two measured values, QUAL_MAX_CHROMS, QUAL_THETA_MAX"""
    out = np.zeros(6)
    call("genosim_qual_constants", None, [PTR], out)
    return {"abs": float(out[0]), "rel": float(out[1]), "abs_measured": float(out[2]), "rel_measured": float(out[3]), "max_chroms": int(out[4]),
            "theta_max": float(out[5])}


def layout(n_rows, S, m_max, per_item):
    """svjg_geno.h: qual_layout -> dict of byte offsets (and total)"""
    return _layout(QUAL, n_rows, S, m_max, int(bool(per_item)))
