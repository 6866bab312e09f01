"""Build + call the host harness of the cohort genotype leg's integer pieces (tests only)."""
import ctypes
import os
import subprocess

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
SO = os.path.join(HERE, "_cohort_sim.so")
CSRC = os.path.join(HERE, "..", "..", "svjedi-graph_amd", "csrc")
LAYOUT_FIELDS = ("pl", "raw", "gt", "flags", "boundary", "site", "maxn", "slot", "type", "ok", "in_bytes", "total")


def build():
    src = [os.path.join(HERE, "cohort_sim.cpp"), os.path.join(CSRC, "svjg_geno.h"), os.path.join(CSRC, "svjg_pass.h")]
    if not os.path.exists(SO) or os.path.getmtime(SO) < max(os.path.getmtime(s) for s in src):
        subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-shared", "-fPIC", "-o", SO, src[0]], check=True)
    return SO


def wave(w0, S, n_items):
    """svjg_geno.h: cohort_segment for the 64 lanes of the wave whose first item is w0 -> (mask uint64[64], leader uint8[64])"""
    lib = ctypes.CDLL(build())
    mask, leader = np.zeros(64, np.uint64), np.zeros(64, np.uint8)
    lib.cohortsim_wave.restype = None
    lib.cohortsim_wave.argtypes = [ctypes.c_uint64] * 3 + [ctypes.c_void_p] * 2
    lib.cohortsim_wave(int(w0), int(S), int(n_items), mask.ctypes.data, leader.ctypes.data)
    return mask, leader


def layout(n_rows, S):
    """svjg_geno.h: cohort_layout -> dict of byte offsets"""
    lib = ctypes.CDLL(build())
    out = np.zeros(12, np.uint64)
    lib.cohortsim_layout.restype = None
    lib.cohortsim_layout.argtypes = [ctypes.c_uint64, ctypes.c_uint64, ctypes.c_void_p]
    lib.cohortsim_layout(int(n_rows), int(S), out.ctypes.data)
    return dict(zip(LAYOUT_FIELDS, (int(x) for x in out)))
