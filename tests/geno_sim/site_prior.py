"""The cohort site prior (svjg_geno.h's site_prior_* routines behind k_cohort_sites_prior) through the host harness (tests only)."""
import ctypes

import numpy as np

from tests.geno_sim import SITES, PTR, U32, U64, INT, F64, u8, u32, call, layout as _layout
from tests.geno_sim import build_main                                                  # noqa: F401
from tests.geno_sim import prior
from tests.geno_sim.prior import width                                                 # noqa: F401  (prior_segment_width: the lanes a site takes)
from tests.geno_sim.site import MAX_ALTS, NPL

ALLELES = 7                              # svjg_geno.h: SITE_ALLELES


def sites(raw, members, slots, err, min_support, wave):
    """raw[n, S, 7], members[n, S], slots[n, 6] -> dict p[n, 7], steps[n] (the kernel's word), sgt[n, S, 2], sgq[n, S], psite[n, 6, 2]"""
    raw, members, slots = u32(raw), u8(members), u32(slots)
    n, S = members.shape
    assert raw.shape == (n, S, ALLELES) and slots.shape == (n, MAX_ALTS)
    out = {"p": np.full((n, ALLELES), -1.0), "steps": np.zeros(n, np.uint32), "sgt": np.full((n, S, 2), 0xEE, np.uint8),
           "sgq": np.full((n, S), 0xEE, np.uint8), "psite": np.full((n, MAX_ALTS, 2), 0xEEEEEEEE, np.uint32)}
    call("genosim_site_prior_sites", None, [INT] + [PTR] * 3 + [U64, U64, F64, U32] + [PTR] * 5, int(bool(wave)), raw, members, slots, n, S, float(err),
         int(min_support), out["p"], out["steps"], out["sgt"], out["sgq"], out["psite"])
    return out


def item(raw, members, err, stride=1):
    """-> (w[28] in candidate order, top slot, N, takes part); stride: the weights are written that many doubles apart (the rest must stay untouched)"""
    raw = u32(raw)
    assert raw.shape == (ALLELES,)
    buf = np.full(NPL * stride, -7.0)
    top, N = ctypes.c_uint32(0), ctypes.c_double(0)
    part = call("genosim_site_prior_item", U32, [PTR, U32, F64, PTR, U32, PTR, PTR], raw, int(members), float(err), buf, int(stride), ctypes.addressof(top), ctypes.addressof(N))
    if stride > 1:
        assert (buf.reshape(NPL, stride)[:, 1:] == -7.0).all()
    return buf[::stride].copy(), top.value, N.value, bool(part)


def lik(K, ref, alt, err):
    """site_lik in member numbering -> (hi[28], lo[28])"""
    a = np.zeros(MAX_ALTS, np.uint32)
    a[:len(alt)] = alt
    hi, lo = np.zeros(NPL), np.zeros(NPL)
    call("genosim_site_prior_lik", None, [U32, U32, PTR, F64, PTR, PTR], int(K), int(ref), a, float(err), hi, lo)
    return hi, lo


def layout(n, S, cohort, prior):
    """svjg_geno.h: sites_layout(n, S, cohort, prior) -> dict of byte offsets (and in_bytes, total); a field the call does not have is 0"""
    return _layout(SITES, n, S, 0, int(bool(cohort)) | (4 if prior else 8))


def constants():
    """-> (EM_TOL, EM_MAX_IT, EM_NOT_CONVERGED, SITE_EM_P_BOUND)"""
    return prior.constants(site=True)
