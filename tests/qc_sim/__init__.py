"""The host harness of the cohort sample QC (tests only): svjg_geno.h's QC routines and a plain C++ restatement of the loops of k_qc_planes and
k_qc_pairs (qc_sim.cpp), as a library driven from numpy and as a stand-alone sanitizer program, both built by tests/sim_build.py."""
import ctypes
import os

import numpy as np

from tests import sim_build

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "qc_sim.cpp")
CSRC = os.path.join(HERE, "..", "..", "svjedi-graph_amd", "csrc")
DEPS = [os.path.join(CSRC, "svjg_geno.h"), os.path.join(CSRC, "svjg_pass.h")]
PTR, U32, U64, INT = ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint64, ctypes.c_int
RUN_CODES = {1: "a store outside its field", 2: "a pair written twice or never", 3: "a plane word never written", 4: "a bit set behind the last row"}


def call(name, restype, argtypes, *args):
    return sim_build.call(sim_build.shared(os.path.join(HERE, "_qc_sim.so"), SRC, DEPS), name, restype, argtypes, *args)


def build_main():
    """the stand-alone program under AddressSanitizer and UBSan: it runs its seeded random calls against a brute-force count"""
    return sim_build.program(os.path.join(HERE, "_qc_sim_main"), SRC, DEPS, ["QC_SIM_MAIN"])


def constants():
    """-> dict: TI, TJ (the pair kernel's tile), stage (64-row words a stage), max_samples, RI (pairs a lane), plane_words (words a lane of the
    plane kernel takes), waves, lds_slots"""
    out = np.zeros(8, np.uint32)
    call("qcsim_constants", None, [PTR], out)
    return dict(zip(("TI", "TJ", "stage", "max_samples", "RI", "plane_words", "waves", "lds_slots"), (int(x) for x in out)))


def qc_class(g, P):
    """-> the six predicate bits of an item (bit q: field q of sample[s][6])"""
    return call("qcsim_class", U32, [U32, U32], int(g), int(P))


def tiles(S):
    return call("qcsim_tiles", U32, [U32], int(S))


def tile_at(t, S):
    ij = np.zeros(2, np.uint32)
    call("qcsim_tile_at", None, [U32, U32, PTR], int(t), int(S), ij)
    return int(ij[0]), int(ij[1])


def layout(n_rows, S, per_item):
    out = np.zeros(9, np.uint64)
    call("qcsim_layout", None, [U64, U64, INT, PTR], int(n_rows), int(S), int(bool(per_item)), out)
    return dict(zip(("pair", "sample", "maxn", "in_at", "in_bytes", "gt", "ploidy", "planes", "total"), (int(x) for x in out)))


def pair_word(i3, j3):
    """(dip, het, homalt) words of i and of j -> the five counts of the word"""
    c = np.zeros(5, np.uint32)
    call("qcsim_pair_word", None, [PTR, PTR, PTR], np.ascontiguousarray(i3, np.uint64), np.ascontiguousarray(j3, np.uint64), c)
    return c


def run(gt, ploidy=None, grid_planes=0, grid_pairs=0):
    """both kernels' loops over a call (grids of that many blocks, 0: a block per unit of work) -> (sample[S, 6], pair[S (S - 1) / 2, 5]) uint32"""
    gt = np.ascontiguousarray(gt, np.uint8)
    n, S = gt.shape
    if ploidy is not None:
        ploidy = np.ascontiguousarray(ploidy, np.uint8)
        assert ploidy.shape == gt.shape
    sample, pair = np.zeros((S, 6), np.uint32), np.zeros((S * (S - 1) // 2 + 1, 5), np.uint32)
    rc = call("qcsim_run", INT, [PTR, PTR, U64, U32, U32, U32, PTR, PTR], gt, ploidy, n, S, int(grid_planes), int(grid_pairs), sample, pair)
    assert rc == 0, RUN_CODES.get(rc, rc)
    return sample, pair[:-1]


class SimQc:
    """cohort_qc as capi.Context has it, answered by the harness"""

    def cohort_qc(self, gt, ploidy=None):
        return run(gt, ploidy)
