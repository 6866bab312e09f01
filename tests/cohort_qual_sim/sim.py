"""Build + call the host harness of the cohort site quality (tests only)."""
import ctypes
import os
import subprocess

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
SO = os.path.join(HERE, "_cohort_qual_sim.so")
MAIN = os.path.join(HERE, "_cohort_qual_sim_main")
CSRC = os.path.join(HERE, "..", "..", "svjedi-graph_amd", "csrc")
SRC = [os.path.join(HERE, "cohort_qual_sim.cpp"), os.path.join(CSRC, "svjg_geno.h"), os.path.join(CSRC, "svjg_pass.h")]
LAYOUT_FIELDS = ("qual", "mlac", "chroms", "maxn", "in_at", "logtab", "harm", "slot", "type", "ok", "ploidy", "total")


def _stale(target):
    return not os.path.exists(target) or os.path.getmtime(target) < max(os.path.getmtime(s) for s in SRC)


def build():
    if _stale(SO):
        subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-ffp-contract=off", "-shared", "-fPIC", "-o", SO, SRC[0]], check=True)
    return SO


def build_main():
    """the stand-alone program under AddressSanitizer and UBSan (its own main: nothing is preloaded into anything)"""
    if _stale(MAIN):
        subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-ffp-contract=off", "-DCOHORT_QUAL_SIM_MAIN", "-fsanitize=address,undefined",
                        "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", "-o", MAIN, SRC[0]], check=True)
    return MAIN


_LIB = None


def _lib():
    global _LIB
    if _LIB is None:
        lib = ctypes.CDLL(build())
        lib.cqsim_row.restype = None
        lib.cqsim_row.argtypes = [ctypes.c_int, ctypes.c_uint32, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_uint32,
                                  ctypes.c_double, ctypes.c_double, ctypes.c_uint32] + [ctypes.c_void_p] * 3
        lib.cqsim_item.restype = ctypes.c_uint32
        lib.cqsim_item.argtypes = [ctypes.c_uint32] * 4 + [ctypes.c_double, ctypes.c_void_p, ctypes.c_void_p]
        lib.cqsim_every.restype = ctypes.c_uint32
        lib.cqsim_every.argtypes = [ctypes.c_uint32, ctypes.c_uint32]
        lib.cqsim_constants.restype = None
        lib.cqsim_constants.argtypes = [ctypes.c_void_p]
        lib.cqsim_layout.restype = None
        lib.cqsim_layout.argtypes = [ctypes.c_uint64, ctypes.c_uint64, ctypes.c_uint32, ctypes.c_int, ctypes.c_void_p]
        _LIB = lib
    return _LIB


def rows(sv_type, raw, done, ploidy, max_ploidy, err, theta, wave=False, every=0, only=None):
    """every row (or the rows `only`) through cqsim_row; wave: the sums over k in the kernel's order; every: steps between two rescalings (0: the
    call's own) -> (qual[R], mlac[R], chroms[R]); rows not asked for: NaN, 0, 0"""
    lib = _lib()
    raw, done = np.ascontiguousarray(raw, np.uint32), np.ascontiguousarray(done, np.uint8)
    R, S = done.shape
    if ploidy is not None:
        ploidy = np.ascontiguousarray(ploidy, np.uint8)
    qual, mlac, chroms = np.full(R, np.nan), np.zeros(R, np.uint32), np.zeros(R, np.uint32)
    for r in (range(R) if only is None else only):
        lib.cqsim_row(int(bool(wave)), int(sv_type[r]), raw[r].ctypes.data, done[r].ctypes.data, None if ploidy is None else ploidy[r].ctypes.data, S,
                      int(max_ploidy), float(err), float(theta), int(every), qual[r:].ctypes.data, mlac[r:].ctypes.data, chroms[r:].ctypes.data)
    return qual, mlac, chroms


def item(sv_type, ref, alt, P, err):
    """-> (the ploidy the recurrence sees, w[9], (d0 hi, d0 lo))"""
    w, d0 = np.zeros(9), np.zeros(2)
    p = _lib().cqsim_item(int(sv_type), int(ref), int(alt), int(P), float(err), w.ctypes.data, d0.ctypes.data)
    return p, w, (float(d0[0]), float(d0[1]))


def every(m_max, max_ploidy):
    return _lib().cqsim_every(int(m_max), int(max_ploidy))


def constants():
    """-> dict: QUAL_ABS, QUAL_REL, the two measured values, QUAL_MAX_CHROMS, QUAL_THETA_MAX"""
    out = np.zeros(6)
    _lib().cqsim_constants(out.ctypes.data)
    return {"abs": float(out[0]), "rel": float(out[1]), "abs_measured": float(out[2]), "rel_measured": float(out[3]), "max_chroms": int(out[4]),
            "theta_max": float(out[5])}


def layout(n_rows, S, m_max, per_item):
    """svjg_geno.h: qual_layout -> dict of byte offsets (and total)"""
    out = np.zeros(12, np.uint64)
    _lib().cqsim_layout(int(n_rows), int(S), int(m_max), int(bool(per_item)), out.ctypes.data)
    return dict(zip(LAYOUT_FIELDS, (int(x) for x in out)))
