"""The host harness of the cohort site test for Hardy-Weinberg equilibrium (tests only): svjg_geno.h's HWE routines and a plain C++ restatement of the
loops of k_cohort_hwe (hwe_sim.cpp), as a library driven from numpy and as a stand-alone sanitizer program, both built by tests/sim_build.py."""
import ctypes
import os

import numpy as np

from tests import sim_build

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "hwe_sim.cpp")
CSRC = os.path.join(HERE, "..", "..", "svjedi-graph_amd", "csrc")
DEPS = [os.path.join(HERE, "..", "host_logfact.h"), os.path.join(CSRC, "svjg_geno.h"), os.path.join(CSRC, "svjg_pass.h")]
PTR, U32, U64, INT = ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint64, ctypes.c_int
RUN_CODES = {1: "a store outside its field", 2: "an output word written twice or never", 3: "a table entry beyond the reserved ones",
             4: "the lanes of a segment disagree"}


def call(name, restype, argtypes, *args):
    return sim_build.call(sim_build.shared(os.path.join(HERE, "_hwe_sim.so"), SRC, DEPS), name, restype, argtypes, *args)


def build_main():
    """the stand-alone program under AddressSanitizer and UBSan: it runs its seeded random calls against a brute-force count and a recurrence in
    long double"""
    return sim_build.program(os.path.join(HERE, "_hwe_sim_main"), SRC, DEPS, ["HWE_SIM_MAIN"])


def constants():
    """-> dict: max_samples, tpb (lanes a block), blocks_per_cu (the cap of the launch's grid)"""
    out = np.zeros(3, np.uint32)
    call("hwesim_constants", None, [PTR], out)
    return dict(zip(("max_samples", "tpb", "blocks_per_cu"), (int(x) for x in out)))


def segment_width(S):
    return call("hwesim_segment_width", U32, [U64], int(S))


def layout(n_rows, S, per_item):
    out = np.zeros(8, np.uint64)
    call("hwesim_layout", None, [U64, U64, INT, PTR], int(n_rows), int(S), int(bool(per_item)), out)
    return dict(zip(("p", "counts", "maxn", "in_at", "in_bytes", "gt", "ploidy", "total"), (int(x) for x in out)))


def row(n_ref, n_het, n_alt):
    """-> dict of hwe_row: n, m, par, het, h0 (the h the terms are relative to), terms"""
    out = np.zeros(6, np.uint32)
    call("hwesim_row", None, [U32, U32, U32, PTR], int(n_ref), int(n_het), int(n_alt), out)
    return dict(zip(("n", "m", "par", "het", "h0", "terms"), (int(x) for x in out)))


def run(gt, ploidy=None, grid=0, n_cu=256):
    """the kernel's loops over a call (a grid of that many blocks; 0: the launch's own on n_cu units) -> (counts[n, 3] uint32, p[n, 2] float64)"""
    gt = np.ascontiguousarray(gt, np.uint8)
    n, S = gt.shape
    if ploidy is not None:
        ploidy = np.ascontiguousarray(ploidy, np.uint8)
        assert ploidy.shape == gt.shape
    counts, p = np.zeros((n, 3), np.uint32), np.zeros((n, 2), np.float64)
    rc = call("hwesim_run", INT, [PTR, PTR, U64, U32, U32, U32, PTR, PTR], gt, ploidy, n, S, int(grid), int(n_cu), counts, p)
    assert rc == 0, RUN_CODES.get(rc, rc)
    return counts, p


class SimHwe:
    """cohort_hwe as capi.Context has it, answered by the harness"""

    def cohort_hwe(self, gt, ploidy=None):
        return run(gt, ploidy)
