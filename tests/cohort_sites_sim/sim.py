"""Build + call the host harness of the cohort call for insertions that share a position (tests only)."""
import ctypes
import os
import subprocess

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
SO = os.path.join(HERE, "_cohort_sites_sim.so")
MAIN = os.path.join(HERE, "_cohort_sites_sim_main")
CSRC = os.path.join(HERE, "..", "..", "svjedi-graph_amd", "csrc")
SRC = [os.path.join(HERE, "cohort_sites_sim.cpp"), os.path.join(CSRC, "svjg_geno.h"), os.path.join(CSRC, "svjg_pass.h")]
MAX_ALTS = 6                             # svjg_geno.h: MAX_SITE_ALTS
NPL = 28                                 # svjg_geno.h: SITE_GENOTYPES
LAYOUT_FIELDS = ("pl", "raw", "gt", "members", "boundary", "site", "maxn", "in_at", "logs", "slots", "in_bytes", "total")


def _stale(target):
    return not os.path.exists(target) or os.path.getmtime(target) < max(os.path.getmtime(s) for s in SRC)


def build():
    if _stale(SO):
        subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-shared", "-fPIC", "-o", SO, SRC[0]], check=True)
    return SO


def build_main():
    """the stand-alone program under AddressSanitizer and UBSan (its own main: nothing is preloaded into anything)"""
    if _stale(MAIN):
        subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-DCOHORT_SITES_SIM_MAIN", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                        "-fno-omit-frame-pointer", "-o", MAIN, SRC[0]], check=True)
    return MAIN


def compact(bits, cref, calt):
    """svjg_geno.h: site_compact -> (K, ref, alt[6])"""
    lib = ctypes.CDLL(build())
    cref, calt = np.ascontiguousarray(cref, np.uint32), np.ascontiguousarray(calt, np.uint32)
    assert len(cref) == len(calt) == MAX_ALTS
    out = np.zeros(8, np.uint32)
    lib.csitesim_compact.restype = None
    lib.csitesim_compact.argtypes = [ctypes.c_uint32] + [ctypes.c_void_p] * 3
    lib.csitesim_compact(int(bits), cref.ctypes.data, calt.ctypes.data, out.ctypes.data)
    return int(out[0]), int(out[1]), out[2:].tolist()


def sums(w0, S, n_items, members, gt):
    """the wave whose first item is w0: the kernel's 18 ballots from members[n_items] / gt[n_items, 2] under cohort_segment's masks
    -> (leader uint8[64], ns uint32[64, 6], ac uint32[64, 6], word uint64[64, 6]); the sums are 0 on a lane that is no leader"""
    lib = ctypes.CDLL(build())
    members, gt = np.ascontiguousarray(members, np.uint8), np.ascontiguousarray(gt, np.uint8)
    assert members.shape == (n_items,) and gt.shape == (n_items, 2)
    leader = np.zeros(64, np.uint8)
    ns, ac, word = np.zeros((64, MAX_ALTS), np.uint32), np.zeros((64, MAX_ALTS), np.uint32), np.zeros((64, MAX_ALTS), np.uint64)
    lib.csitesim_sums.restype = None
    lib.csitesim_sums.argtypes = [ctypes.c_uint64] * 3 + [ctypes.c_void_p] * 6
    lib.csitesim_sums(int(w0), int(S), int(n_items), members.ctypes.data, gt.ctypes.data, leader.ctypes.data, ns.ctypes.data, ac.ctypes.data, word.ctypes.data)
    return leader, ns, ac, word


def items(bits, cref, calt, min_support, err, tab):
    """items as a lane of k_genotype_cohort_sites runs them: bits[n], cref[n, 6], calt[n, 6] -> (gt[n, 2], pl[n, 28], raw[n, 7], near, status, n = s_K)"""
    lib = ctypes.CDLL(build())
    bits = np.ascontiguousarray(bits, np.uint8)
    n = len(bits)
    cref, calt = np.ascontiguousarray(cref, np.uint32), np.ascontiguousarray(calt, np.uint32)
    assert cref.shape == calt.shape == (n, MAX_ALTS)
    tab = np.ascontiguousarray(tab, np.float64)
    gt, pl, raw = np.zeros((n, 2), np.uint8), np.full((n, NPL), -1, np.int64), np.full((n, MAX_ALTS + 1), 0xFFFFFFFF, np.uint32)
    near, st, n_out = np.zeros(n, np.uint8), np.zeros(n, np.uint8), np.zeros(n, np.uint64)
    lib.csitesim_items.restype = None
    lib.csitesim_items.argtypes = [ctypes.c_uint64] + [ctypes.c_void_p] * 3 + [ctypes.c_uint32, ctypes.c_double, ctypes.c_void_p, ctypes.c_uint32] + [ctypes.c_void_p] * 6
    lib.csitesim_items(n, bits.ctypes.data, cref.ctypes.data, calt.ctypes.data, int(min_support), float(err), tab.ctypes.data, len(tab),
                       gt.ctypes.data, pl.ctypes.data, raw.ctypes.data, near.ctypes.data, st.ctypes.data, n_out.ctypes.data)
    return gt, pl, raw, near, st, n_out


def layout(n_sites, S):
    """svjg_geno.h: cohort_sites_layout -> dict of byte offsets (and in_bytes, total)"""
    lib = ctypes.CDLL(build())
    out = np.zeros(12, np.uint64)
    lib.csitesim_layout.restype = None
    lib.csitesim_layout.argtypes = [ctypes.c_uint64, ctypes.c_uint64, ctypes.c_void_p]
    lib.csitesim_layout(int(n_sites), int(S), out.ctypes.data)
    return dict(zip(LAYOUT_FIELDS, (int(v) for v in out)))
