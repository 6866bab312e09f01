"""Build + call the host harness of the cohort genotype leg's integer pieces (tests only)."""
import ctypes
import os
import subprocess

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
SO = os.path.join(HERE, "_cohort_sim.so")
MAIN = os.path.join(HERE, "_cohort_sim_main")
CSRC = os.path.join(HERE, "..", "..", "svjedi-graph_amd", "csrc")
SRC = [os.path.join(HERE, "cohort_sim.cpp"), os.path.join(CSRC, "svjg_geno.h"), os.path.join(CSRC, "svjg_pass.h")]
LAYOUT_FIELDS = ("pl", "raw", "gt", "flags", "boundary", "gq", "af", "psite", "steps", "site", "maxn", "in_at", "logtab", "slot", "type", "ok",
                 "ploidy", "total", "in_bytes")


def _stale(target):
    return not os.path.exists(target) or os.path.getmtime(target) < max(os.path.getmtime(s) for s in SRC)


def build():
    if _stale(SO):
        subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-shared", "-fPIC", "-o", SO, SRC[0]], check=True)
    return SO


def build_main():
    """the stand-alone program under AddressSanitizer and UBSan (its own main: nothing is preloaded into anything)"""
    if _stale(MAIN):
        subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-DCOHORT_SIM_MAIN", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                        "-fno-omit-frame-pointer", "-o", MAIN, SRC[0]], check=True)
    return MAIN


def wave(w0, S, n_items):
    """svjg_geno.h: cohort_segment for the 64 lanes of the wave whose first item is w0 -> (mask uint64[64], leader uint8[64])"""
    lib = ctypes.CDLL(build())
    mask, leader = np.zeros(64, np.uint64), np.zeros(64, np.uint8)
    lib.cohortsim_wave.restype = None
    lib.cohortsim_wave.argtypes = [ctypes.c_uint64] * 3 + [ctypes.c_void_p] * 2
    lib.cohortsim_wave(int(w0), int(S), int(n_items), mask.ctypes.data, leader.ctypes.data)
    return mask, leader


def sums(w0, S, n_items, gt, ploidy=None):
    """the wave whose first item is w0: the kernel's nine ballots from gt / ploidy (uint8 per item; gt 0xFF: no call), or with ploidy None the
    diploid kernel's three from gt (3: no call); svjg_geno.h: cohort_segment and cohort_ploidy_sums / cohort_diploid_sums -> (leader uint8[64], ns, an, ac uint32[64], word uint64[64]); the sums are 0 on a lane that is no leader"""
    lib = ctypes.CDLL(build())
    gt = np.ascontiguousarray(gt, np.uint8)
    if ploidy is not None:
        ploidy = np.ascontiguousarray(ploidy, np.uint8)
    assert len(gt) == n_items and (ploidy is None or len(ploidy) == n_items)
    leader = np.zeros(64, np.uint8)
    ns, an, ac = (np.zeros(64, np.uint32) for _ in range(3))
    word = np.zeros(64, np.uint64)
    lib.cohortsim_sums.restype = None
    lib.cohortsim_sums.argtypes = [ctypes.c_uint64] * 3 + [ctypes.c_void_p] * 7
    lib.cohortsim_sums(int(w0), int(S), int(n_items), gt.ctypes.data, None if ploidy is None else ploidy.ctypes.data, leader.ctypes.data, ns.ctypes.data, an.ctypes.data,
                       ac.ctypes.data, word.ctypes.data)
    return leader, ns, an, ac, word


def layout(n_rows, S, max_ploidy=2, per_item=False, prior=False):
    """svjg_geno.h: cohort_layout -> dict of byte offsets (and in_bytes, total); a field the call does not have is 0"""
    lib = ctypes.CDLL(build())
    out = np.zeros(19, np.uint64)
    lib.cohortsim_layout.restype = None
    lib.cohortsim_layout.argtypes = [ctypes.c_uint64, ctypes.c_uint64, ctypes.c_uint32, ctypes.c_int, ctypes.c_int, ctypes.c_void_p]
    lib.cohortsim_layout(int(n_rows), int(S), int(max_ploidy), int(bool(per_item)), int(bool(prior)), out.ctypes.data)
    return dict(zip(LAYOUT_FIELDS, (int(x) for x in out)))
