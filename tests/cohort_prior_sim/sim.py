"""Build + call the host harness of the cohort call with an allele-frequency prior (tests only)."""
import ctypes
import os
import subprocess

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
SO = os.path.join(HERE, "_cohort_prior_sim.so")
MAIN = os.path.join(HERE, "_cohort_prior_sim_main")
CSRC = os.path.join(HERE, "..", "..", "svjedi-graph_amd", "csrc")
SRC = [os.path.join(HERE, "cohort_prior_sim.cpp"), os.path.join(CSRC, "svjg_geno.h"), os.path.join(CSRC, "svjg_pass.h")]
LAYOUT_FIELDS = ("pl", "raw", "gt", "flags", "boundary", "gq", "af", "psite", "steps", "site", "maxn", "in_at", "logtab", "slot", "type", "ok",
                 "ploidy", "total", "in_bytes")


def _stale(target):
    return not os.path.exists(target) or os.path.getmtime(target) < max(os.path.getmtime(s) for s in SRC)


def build():
    if _stale(SO):
        subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-ffp-contract=off", "-shared", "-fPIC", "-o", SO, SRC[0]], check=True)
    return SO


def build_main():
    """the stand-alone program under AddressSanitizer and UBSan (its own main: nothing is preloaded into anything)"""
    if _stale(MAIN):
        subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-ffp-contract=off", "-DCOHORT_PRIOR_SIM_MAIN", "-fsanitize=address,undefined",
                        "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", "-o", MAIN, SRC[0]], check=True)
    return MAIN


def _lib():
    lib = ctypes.CDLL(build())
    for fn in (lib.cprsim_row, lib.cprsim_row_wave):
        fn.restype = None
        fn.argtypes = [ctypes.c_uint32, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_double, ctypes.c_uint32] + [ctypes.c_void_p] * 5
    lib.cprsim_item.restype = ctypes.c_uint32
    lib.cprsim_item.argtypes = [ctypes.c_uint32] * 4 + [ctypes.c_double, ctypes.c_void_p, ctypes.c_void_p]
    lib.cprsim_width.restype = ctypes.c_uint32
    lib.cprsim_width.argtypes = [ctypes.c_uint64]
    lib.cprsim_layout.restype = None
    lib.cprsim_layout.argtypes = [ctypes.c_uint64, ctypes.c_uint64, ctypes.c_uint32, ctypes.c_int, ctypes.c_void_p]
    lib.cprsim_constants.restype = None
    lib.cprsim_constants.argtypes = [ctypes.c_void_p] * 4
    return lib


def rows(sv_type, raw, done, ploidy, err, min_support, wave=False):
    """every row through cprsim_row, or with wave through cprsim_row_wave (every step's sum in the kernel's order)
    -> (f[R], steps[R] (bit 31: not converged), gt[R, S], gq[R, S], site[R, 3])"""
    lib = _lib()
    row = lib.cprsim_row_wave if wave else lib.cprsim_row
    raw, done = np.ascontiguousarray(raw, np.uint32), np.ascontiguousarray(done, np.uint8)
    R, S = done.shape
    if ploidy is not None:
        ploidy = np.ascontiguousarray(ploidy, np.uint8)
    f, steps = np.zeros(R), np.zeros(R, np.uint32)
    gt, gq, site = np.zeros((R, S), np.uint8), np.zeros((R, S), np.uint8), np.zeros((R, 3), np.uint32)
    for r in range(R):
        row(int(sv_type[r]), raw[r].ctypes.data, done[r].ctypes.data, None if ploidy is None else ploidy[r].ctypes.data, S, float(err),
            int(min_support), f[r:].ctypes.data, steps[r:].ctypes.data, gt[r].ctypes.data, gq[r].ctypes.data, site[r].ctypes.data)
    return f, steps, gt, gq, site


def item(sv_type, ref, alt, P, err):
    """-> (the ploidy the EM sees, w[9], gmax)"""
    w, gmax = np.zeros(9), np.zeros(1, np.uint32)
    p = _lib().cprsim_item(int(sv_type), int(ref), int(alt), int(P), float(err), w.ctypes.data, gmax.ctypes.data)
    return p, w, int(gmax[0])


def width(S):
    return _lib().cprsim_width(int(S))


def constants():
    """-> (EM_TOL, EM_MAX_IT, EM_NOT_CONVERGED, EM_F_BOUND)"""
    tol, bound = np.zeros(1), np.zeros(1)
    it, bit = np.zeros(1, np.uint32), np.zeros(1, np.uint32)
    _lib().cprsim_constants(tol.ctypes.data, it.ctypes.data, bit.ctypes.data, bound.ctypes.data)
    return float(tol[0]), int(it[0]), int(bit[0]), float(bound[0])


def layout(n_rows, S, max_ploidy, per_item):
    """svjg_geno.h: cohort_layout with the prior -> dict of byte offsets (and in_bytes, total)"""
    out = np.zeros(19, np.uint64)
    _lib().cprsim_layout(int(n_rows), int(S), int(max_ploidy), int(bool(per_item)), out.ctypes.data)
    return dict(zip(LAYOUT_FIELDS, (int(x) for x in out)))
