"""Build + call the host harness of the cohort-at-per-sample-ploidy leg's integer pieces (tests only)."""
import ctypes
import os
import subprocess

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
SO = os.path.join(HERE, "_cohort_ploidy_sim.so")
MAIN = os.path.join(HERE, "_cohort_ploidy_sim_main")
CSRC = os.path.join(HERE, "..", "..", "svjedi-graph_amd", "csrc")
SRC = [os.path.join(HERE, "cohort_ploidy_sim.cpp"), os.path.join(CSRC, "svjg_geno.h"), os.path.join(CSRC, "svjg_pass.h")]
LAYOUT_FIELDS = ("pl", "raw", "gt", "flags", "boundary", "site", "maxn", "in_at", "logtab", "slot", "type", "ok", "ploidy", "total", "in_bytes")


def _stale(target):
    return not os.path.exists(target) or os.path.getmtime(target) < max(os.path.getmtime(s) for s in SRC)


def build():
    if _stale(SO):
        subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-shared", "-fPIC", "-o", SO, SRC[0]], check=True)
    return SO


def build_main():
    """the stand-alone program under AddressSanitizer and UBSan (its own main: nothing is preloaded into anything)"""
    if _stale(MAIN):
        subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-DCOHORT_PLOIDY_SIM_MAIN", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                        "-fno-omit-frame-pointer", "-o", MAIN, SRC[0]], check=True)
    return MAIN


def wave(w0, S, n_items, gt, ploidy):
    """the wave whose first item is w0: the kernel's nine ballots from gt / ploidy (uint8 per item), svjg_geno.h: cohort_segment and
    cohort_ploidy_sums -> (leader uint8[64], ns, an, ac uint32[64], word uint64[64]); the sums are 0 on a lane that is no leader"""
    lib = ctypes.CDLL(build())
    gt, ploidy = np.ascontiguousarray(gt, np.uint8), np.ascontiguousarray(ploidy, np.uint8)
    assert len(gt) == len(ploidy) == n_items
    leader = np.zeros(64, np.uint8)
    ns, an, ac = (np.zeros(64, np.uint32) for _ in range(3))
    word = np.zeros(64, np.uint64)
    lib.cpsim_wave.restype = None
    lib.cpsim_wave.argtypes = [ctypes.c_uint64] * 3 + [ctypes.c_void_p] * 7
    lib.cpsim_wave(int(w0), int(S), int(n_items), gt.ctypes.data, ploidy.ctypes.data, leader.ctypes.data, ns.ctypes.data, an.ctypes.data,
                   ac.ctypes.data, word.ctypes.data)
    return leader, ns, an, ac, word


def layout(n_rows, S, max_ploidy):
    """svjg_geno.h: cohort_ploidy_layout -> dict of byte offsets (and in_bytes, total)"""
    lib = ctypes.CDLL(build())
    out = np.zeros(15, np.uint64)
    lib.cpsim_layout.restype = None
    lib.cpsim_layout.argtypes = [ctypes.c_uint64, ctypes.c_uint64, ctypes.c_uint32, ctypes.c_void_p]
    lib.cpsim_layout(int(n_rows), int(S), int(max_ploidy), out.ctypes.data)
    return dict(zip(LAYOUT_FIELDS, (int(x) for x in out)))
