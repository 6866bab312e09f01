"""The host harness of svjg_geno.h (tests only): ONE library (geno_sim.cpp and the topic files it includes) and ONE stand-alone sanitizer program,
built by tests/sim_build.py.  ploidy.py, site.py, cohort.py, prior.py, qual.py, site_prior.py, qc.py and hwe.py hold the numpy-facing functions of a topic
each; what they share is here."""
import ctypes
import os

import numpy as np

from tests import sim_build

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "geno_sim.cpp")
CSRC = os.path.join(HERE, "..", "..", "svjedi-graph_amd", "csrc")
# exactly the files geno_sim.cpp includes; svjg_pass.h through svjg_geno.h (run_layout's DevStatus and GUARD_WORDS)
DEPS = [os.path.join(HERE, t + ".inc") for t in ("ploidy", "site", "cohort", "prior", "qual", "site_prior", "qc", "hwe")] + [
    os.path.join(HERE, "..", "host_logfact.h"), os.path.join(CSRC, "svjg_geno.h"), os.path.join(CSRC, "svjg_pass.h")]
PTR, U32, U64, INT, F64 = ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint64, ctypes.c_int, ctypes.c_double
ROWS, PLOIDY, SITES, COHORT, QUAL, QC, HWE = range(7)           # geno_sim.cpp: LAYOUT_*


def call(name, restype, argtypes, *args):
    return sim_build.call(sim_build.shared(os.path.join(HERE, "_geno_sim.so"), SRC, DEPS), name, restype, argtypes, *args)


def build_main():
    """the stand-alone program under AddressSanitizer and UBSan; it takes the topic as its argument"""
    return sim_build.program(os.path.join(HERE, "_geno_sim_main"), SRC, DEPS, ["GENO_SIM_MAIN"])


def u8(x):
    return np.ascontiguousarray(x, np.uint8)


def u32(x):
    return np.ascontiguousarray(x, np.uint32)


def f64(x):
    return np.ascontiguousarray(x, np.float64)


def calls(gt, ploidy):
    """a run's calls as the harness takes them -> (gt[n, S] uint8, ploidy the same or None, n, S)"""
    gt = u8(gt)
    if ploidy is not None:
        ploidy = u8(ploidy)
        assert ploidy.shape == gt.shape
    return (gt, ploidy) + gt.shape


def logfact_table(n):
    """log10(i!) for i < n in double-double (float64[n, 2]), with the host libm's log10"""
    tab = np.zeros((n, 2), np.float64)
    call("genosim_logfact", None, [PTR, U32], tab, n)
    return tab


def ploidy_log_table(err):
    """(Lr[45], La[45]) of svjg_geno.h: ploidy_log_table; entry P (P + 1) / 2 + g"""
    tab = np.zeros(90, np.float64)
    call("genosim_ploidy_log_table", None, [F64, PTR], float(err), tab)
    return tab[:45], tab[45:]


def layout(kind, n, S=1, p=0, flags=0):
    """a layout of svjg_geno.h -> dict of byte offsets (and sizes) by field name, names and values as geno_sim.cpp: genosim_layout lists them"""
    names, at = (ctypes.c_char_p * 32)(), np.zeros(32, np.uint64)
    count = call("genosim_layout", INT, [INT, U64, U64, U32, INT, PTR, PTR], kind, int(n), int(S), int(p), int(flags), ctypes.addressof(names), at)
    return {names[i].decode(): int(at[i]) for i in range(count)}
