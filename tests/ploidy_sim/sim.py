"""Build + call the host harness of the any-ploidy genotype row arithmetic (tests only)."""
import ctypes
import os
import subprocess

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
SO = os.path.join(HERE, "_ploidy_sim.so")
CSRC = os.path.join(HERE, "..", "..", "svjedi-graph_amd", "csrc")
NPL = 9                                  # svjg_geno.h: MAX_PLOIDY + 1


def build():
    src = [os.path.join(HERE, "ploidy_sim.cpp"), os.path.join(CSRC, "svjg_geno.h"), os.path.join(CSRC, "svjg_pass.h")]
    if not os.path.exists(SO) or os.path.getmtime(SO) < max(os.path.getmtime(s) for s in src):
        subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-shared", "-fPIC", "-o", SO, src[0]], check=True)
    return SO


def logfact_table(n):
    """log10(i!) for i < n in double-double (float64[n, 2]), with the host libm's log10"""
    lib = ctypes.CDLL(build())
    tab = np.zeros((n, 2), np.float64)
    lib.ploidysim_logfact.restype = None
    lib.ploidysim_logfact.argtypes = [ctypes.c_void_p, ctypes.c_uint32]
    lib.ploidysim_logfact(tab.ctypes.data, n)
    return tab


def log_table(err):
    """(Lr[45], La[45]) of svjg_geno.h: ploidy_log_table; entry P (P + 1) / 2 + g"""
    lib = ctypes.CDLL(build())
    tab = np.zeros(90, np.float64)
    lib.ploidysim_log_table.restype = None
    lib.ploidysim_log_table.argtypes = [ctypes.c_double, ctypes.c_void_p]
    lib.ploidysim_log_table(float(err), tab.ctypes.data)
    return tab[:45], tab[45:]


def genotype_rows(sv_type, counts, ploidy, min_support, err, tab):
    """geno_row_ploidy -> (gt: alt copies or 0xFF, pl[n, 9], near, status: 0 ok, 1 table too short, 2 beyond the cap)"""
    lib = ctypes.CDLL(build())
    sv_type = np.ascontiguousarray(sv_type, np.uint8)
    counts = np.ascontiguousarray(counts, np.uint32)
    ploidy = np.ascontiguousarray(ploidy, np.uint8)
    assert ploidy.min() >= 1 and ploidy.max() <= 8
    tab = np.ascontiguousarray(tab, np.float64)
    n = len(sv_type)
    gt, pl, near, st = np.zeros(n, np.uint8), np.zeros((n, NPL), np.int64), np.zeros(n, np.uint8), np.zeros(n, np.uint8)
    lib.ploidysim_genotype.restype = None
    lib.ploidysim_genotype.argtypes = [ctypes.c_void_p] * 3 + [ctypes.c_uint64, ctypes.c_uint32, ctypes.c_double, ctypes.c_void_p, ctypes.c_uint32] + [ctypes.c_void_p] * 4
    lib.ploidysim_genotype(sv_type.ctypes.data, counts.ctypes.data, ploidy.ctypes.data, n, int(min_support), float(err), tab.ctypes.data, len(tab),
                           gt.ctypes.data, pl.ctypes.data, near.ctypes.data, st.ctypes.data)
    return gt, pl, near, st


def genotype_rows_diploid(sv_type, counts, min_support, err, tab):
    """geno_row -> (gt: 0..2 or 3, pl[n, 3], near, status)"""
    lib = ctypes.CDLL(build())
    sv_type = np.ascontiguousarray(sv_type, np.uint8)
    counts = np.ascontiguousarray(counts, np.uint32)
    tab = np.ascontiguousarray(tab, np.float64)
    n = len(sv_type)
    gt, pl, near, st = np.zeros(n, np.uint8), np.zeros((n, 3), np.int64), np.zeros(n, np.uint8), np.zeros(n, np.uint8)
    lib.ploidysim_genotype_diploid.restype = None
    lib.ploidysim_genotype_diploid.argtypes = [ctypes.c_void_p] * 2 + [ctypes.c_uint64, ctypes.c_uint32, ctypes.c_double, ctypes.c_void_p, ctypes.c_uint32] + [ctypes.c_void_p] * 4
    lib.ploidysim_genotype_diploid(sv_type.ctypes.data, counts.ctypes.data, n, int(min_support), float(err), tab.ctypes.data, len(tab),
                                   gt.ctypes.data, pl.ctypes.data, near.ctypes.data, st.ctypes.data)
    return gt, pl, near, st
