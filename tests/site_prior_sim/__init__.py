"""The host harness of the cohort site prior (tests only): svjg_geno.h's site_prior_* routines compiled with g++ by tests/sim_build.py, a
translation unit of its own, and the stand-alone sanitizer program."""
import ctypes
import os

import numpy as np

from tests import sim_build

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "site_prior_sim.cpp")
CSRC = os.path.join(HERE, "..", "..", "svjedi-graph_amd", "csrc")
DEPS = [os.path.join(CSRC, "svjg_geno.h"), os.path.join(CSRC, "svjg_pass.h")]
PTR, U32, U64, INT, F64 = ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint64, ctypes.c_int, ctypes.c_double
MAX_ALTS, ALLELES, NPL, NO_CALL = 6, 7, 28, 0xFF
LAYOUT_FIELDS = ("pl", "raw", "gt", "members", "boundary", "sgt", "sgq", "af", "psite", "steps", "site", "maxn", "in_at", "logs", "slots", "in_bytes", "total")


def call(name, restype, argtypes, *args):
    return sim_build.call(sim_build.shared(os.path.join(HERE, "_site_prior_sim.so"), SRC, DEPS), name, restype, argtypes, *args)


def build_main():
    """the stand-alone program under AddressSanitizer and UBSan"""
    return sim_build.program(os.path.join(HERE, "_site_prior_sim_main"), SRC, DEPS, ["SITE_PRIOR_SIM_MAIN"])


def sites(raw, members, slots, err, min_support, wave):
    """raw[n, S, 7], members[n, S], slots[n, 6] -> dict p[n, 7], steps[n] (the kernel's word), sgt[n, S, 2], sgq[n, S], psite[n, 6, 2]"""
    raw, members, slots = np.ascontiguousarray(raw, np.uint32), np.ascontiguousarray(members, np.uint8), np.ascontiguousarray(slots, np.uint32)
    n, S = members.shape
    assert raw.shape == (n, S, ALLELES) and slots.shape == (n, MAX_ALTS)
    out = {"p": np.full((n, ALLELES), -1.0), "steps": np.zeros(n, np.uint32), "sgt": np.full((n, S, 2), 0xEE, np.uint8),
           "sgq": np.full((n, S), 0xEE, np.uint8), "psite": np.full((n, MAX_ALTS, 2), 0xEEEEEEEE, np.uint32)}
    call("sitepriorsim_sites", None, [INT] + [PTR] * 3 + [U64, U64, F64, U32] + [PTR] * 5, int(bool(wave)), raw, members, slots, n, S, float(err),
         int(min_support), out["p"], out["steps"], out["sgt"], out["sgq"], out["psite"])
    return out


def item(raw, members, err, stride=1):
    """-> (w[28] in candidate order, top slot, N, takes part); stride: the weights are written that many doubles apart (the rest must stay untouched)"""
    raw = np.ascontiguousarray(raw, np.uint32)
    assert raw.shape == (ALLELES,)
    buf = np.full(NPL * stride, -7.0)
    top, N = ctypes.c_uint32(0), ctypes.c_double(0)
    part = call("sitepriorsim_item", U32, [PTR, U32, F64, PTR, U32, PTR, PTR], raw, int(members), float(err), buf, int(stride), ctypes.addressof(top), ctypes.addressof(N))
    if stride > 1:
        assert (buf.reshape(NPL, stride)[:, 1:] == -7.0).all()
    return buf[::stride].copy(), top.value, N.value, bool(part)


def lik(K, ref, alt, err):
    """site_lik in member numbering -> (hi[28], lo[28])"""
    a = np.zeros(MAX_ALTS, np.uint32)
    a[:len(alt)] = alt
    hi, lo = np.zeros(NPL), np.zeros(NPL)
    call("sitepriorsim_lik", None, [U32, U32, PTR, F64, PTR, PTR], int(K), int(ref), a, float(err), hi, lo)
    return hi, lo


def layout(n, S, cohort, prior):
    at = np.zeros(len(LAYOUT_FIELDS), np.uint64)
    call("sitepriorsim_layout", None, [U64, U64, INT, INT, PTR], int(n), int(S), int(bool(cohort)), int(bool(prior)), at)
    return dict(zip(LAYOUT_FIELDS, (int(v) for v in at)))


def width(S):
    """svjg_geno.h: prior_segment_width, the lanes a site takes"""
    return call("sitepriorsim_width", U32, [U64], int(S))


def constants():
    tol, bound, it, bit = ctypes.c_double(0), ctypes.c_double(0), ctypes.c_uint32(0), ctypes.c_uint32(0)
    call("sitepriorsim_constants", None, [PTR] * 4, ctypes.addressof(tol), ctypes.addressof(it), ctypes.addressof(bit), ctypes.addressof(bound))
    return tol.value, it.value, bit.value, bound.value
