"""Build + call the host harness of the site calls for insertions that share a position, single-sample and cohort (tests only)."""
import ctypes
import os
import subprocess

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
SO = os.path.join(HERE, "_site_sim.so")
MAIN = os.path.join(HERE, "_site_sim_main")
CSRC = os.path.join(HERE, "..", "..", "svjedi-graph_amd", "csrc")
SRC = [os.path.join(HERE, "site_sim.cpp"), os.path.join(CSRC, "svjg_geno.h"), os.path.join(CSRC, "svjg_pass.h")]
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
        subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-DSITE_SIM_MAIN", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                        "-fno-omit-frame-pointer", "-o", MAIN, SRC[0]], check=True)
    return MAIN


def _call(name, argtypes, *args):
    fn = getattr(ctypes.CDLL(build()), name)
    fn.restype, fn.argtypes = None, argtypes
    fn(*args)


def logfact_table(n):
    """log10(i!) for i < n in double-double (float64[n, 2]), with the host libm's log10"""
    tab = np.zeros((n, 2), np.float64)
    _call("sitesim_logfact", [ctypes.c_void_p, ctypes.c_uint32], tab.ctypes.data, n)
    return tab


def log_table(err):
    """svjg_geno.h: site_log_table -> float64[16]: [0] = L_ok, [K] = L_x[K], [8 + K] = L_he[K]"""
    tab = np.zeros(16, np.float64)
    _call("sitesim_log_table", [ctypes.c_double, ctypes.c_void_p], float(err), tab.ctypes.data)
    return tab


def genotype_sites(sites, min_support, err, tab):
    """geno_site over [(ref, [alt_1 .. alt_K])] -> (gt[n, 2]: the pair or 0xFF, 0xFF; pl[n, 28]; near; status: 0 ok, 1 table too short, 2 beyond
    the cap; n = s_K)"""
    n = len(sites)
    K = np.array([len(a) for _, a in sites], np.uint8)
    assert n == 0 or (K.min() >= 2 and K.max() <= MAX_ALTS)
    ref = np.array([r for r, _ in sites], np.uint32)
    alt = np.zeros((n, MAX_ALTS), np.uint32)
    for s, (_, a) in enumerate(sites):
        alt[s, :len(a)] = a
    tab = np.ascontiguousarray(tab, np.float64)
    gt, pl, near, st = np.zeros((n, 2), np.uint8), np.full((n, NPL), -1, np.int64), np.zeros(n, np.uint8), np.zeros(n, np.uint8)
    n_out = np.zeros(n, np.uint64)
    _call("sitesim_genotype", [ctypes.c_void_p] * 3 + [ctypes.c_uint64, ctypes.c_uint32, ctypes.c_double, ctypes.c_void_p, ctypes.c_uint32] + [ctypes.c_void_p] * 5,
          K.ctypes.data, ref.ctypes.data, alt.ctypes.data, n, int(min_support), float(err), tab.ctypes.data, len(tab),
          gt.ctypes.data, pl.ctypes.data, near.ctypes.data, st.ctypes.data, n_out.ctypes.data)
    return gt, pl, near, st, n_out


def _matrix(counts, present):
    """counts[n_slots, S, 2] (ref, alt) -> the slot-major packed matrix uint64[n_slots * S], its presence bytes (None stays None), S, n_slots"""
    counts = np.asarray(counts, np.uint64)
    n_slots, S = counts.shape[:2]
    packed = np.ascontiguousarray((counts[..., 0] | (counts[..., 1] << np.uint64(32))).reshape(-1))
    if present is not None:
        present = np.ascontiguousarray(present, np.uint8).reshape(-1)
        assert len(present) == n_slots * S
    return packed, present, S, n_slots


def gather(counts, present, s, slots):
    """svjg_geno.h: site_gather as the lane of sample s does it.  counts[n_slots, S, 2], present[n_slots, S] or None (the single-sample call: every
    named slot is a member), slots[6] -> (members, bad, cref[6], calt[6])"""
    packed, present, S, n_slots = _matrix(counts, present)
    slots = np.ascontiguousarray(slots, np.uint32)
    assert slots.shape == (MAX_ALTS,)
    out = np.zeros(14, np.uint32)
    _call("sitesim_gather", [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_uint64, ctypes.c_uint32, ctypes.c_void_p, ctypes.c_void_p],
          packed.ctypes.data, None if present is None else present.ctypes.data, S, int(s), n_slots, slots.ctypes.data, out.ctypes.data)
    return int(out[0]), bool(out[1]), out[2:8].tolist(), out[8:14].tolist()


def site_items(counts, present, slots, min_support, err, tab):
    """svjg_geno.h: site_item over every (site, sample) item as the lanes run it.  counts[n_slots, S, 2], present[n_slots, S] or None, slots[n, 6] ->
    (gt[n, S, 2], pl[n, S, 28], raw[n, S, 7], boundary[n, S], members[n, S], status[n, S], n = s_K [n, S], bad[n, S])"""
    packed, present, S, n_slots = _matrix(counts, present)
    slots = np.ascontiguousarray(slots, np.uint32)
    n = len(slots)
    assert slots.shape == (n, MAX_ALTS)
    tab = np.ascontiguousarray(tab, np.float64)
    gt, pl, raw = np.zeros((n, S, 2), np.uint8), np.full((n, S, NPL), -1, np.int64), np.full((n, S, MAX_ALTS + 1), 0xFFFFFFFF, np.uint32)
    boundary, members, st, bad = (np.full((n, S), 0xEE, np.uint8) for _ in range(4))
    n_out = np.zeros((n, S), np.uint64)
    _call("sitesim_site_items", [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_uint32, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_uint32, ctypes.c_double,
                                 ctypes.c_void_p, ctypes.c_uint32] + [ctypes.c_void_p] * 8,
          packed.ctypes.data, None if present is None else present.ctypes.data, S, n_slots, slots.ctypes.data, n, int(min_support), float(err), tab.ctypes.data, len(tab),
          gt.ctypes.data, pl.ctypes.data, raw.ctypes.data, boundary.ctypes.data, members.ctypes.data, st.ctypes.data, n_out.ctypes.data, bad.ctypes.data)
    return gt, pl, raw, boundary, members, st, n_out, bad


def compact(bits, cref, calt):
    """svjg_geno.h: site_compact -> (K, ref, alt[6])"""
    cref, calt = np.ascontiguousarray(cref, np.uint32), np.ascontiguousarray(calt, np.uint32)
    assert len(cref) == len(calt) == MAX_ALTS
    out = np.zeros(8, np.uint32)
    _call("sitesim_compact", [ctypes.c_uint32] + [ctypes.c_void_p] * 3, int(bits), cref.ctypes.data, calt.ctypes.data, out.ctypes.data)
    return int(out[0]), int(out[1]), out[2:].tolist()


def sums(w0, S, n_items, members, gt):
    """the wave whose first item is w0: the kernel's 18 ballots from members[n_items] / gt[n_items, 2] under cohort_segment's masks
    -> (leader uint8[64], ns uint32[64, 6], ac uint32[64, 6], word uint64[64, 6]); the sums are 0 on a lane that is no leader"""
    members, gt = np.ascontiguousarray(members, np.uint8), np.ascontiguousarray(gt, np.uint8)
    assert members.shape == (n_items,) and gt.shape == (n_items, 2)
    leader = np.zeros(64, np.uint8)
    ns, ac, word = np.zeros((64, MAX_ALTS), np.uint32), np.zeros((64, MAX_ALTS), np.uint32), np.zeros((64, MAX_ALTS), np.uint64)
    _call("sitesim_sums", [ctypes.c_uint64] * 3 + [ctypes.c_void_p] * 6,
          int(w0), int(S), int(n_items), members.ctypes.data, gt.ctypes.data, leader.ctypes.data, ns.ctypes.data, ac.ctypes.data, word.ctypes.data)
    return leader, ns, ac, word


def items(bits, cref, calt, min_support, err, tab):
    """items from the gathered counts, the compaction and geno_site step by step: bits[n], cref[n, 6], calt[n, 6] -> (gt[n, 2], pl[n, 28], raw[n, 7],
    near, status, n = s_K)"""
    bits = np.ascontiguousarray(bits, np.uint8)
    n = len(bits)
    cref, calt = np.ascontiguousarray(cref, np.uint32), np.ascontiguousarray(calt, np.uint32)
    assert cref.shape == calt.shape == (n, MAX_ALTS)
    tab = np.ascontiguousarray(tab, np.float64)
    gt, pl, raw = np.zeros((n, 2), np.uint8), np.full((n, NPL), -1, np.int64), np.full((n, MAX_ALTS + 1), 0xFFFFFFFF, np.uint32)
    near, st, n_out = np.zeros(n, np.uint8), np.zeros(n, np.uint8), np.zeros(n, np.uint64)
    _call("sitesim_items", [ctypes.c_uint64] + [ctypes.c_void_p] * 3 + [ctypes.c_uint32, ctypes.c_double, ctypes.c_void_p, ctypes.c_uint32] + [ctypes.c_void_p] * 6,
          n, bits.ctypes.data, cref.ctypes.data, calt.ctypes.data, int(min_support), float(err), tab.ctypes.data, len(tab),
          gt.ctypes.data, pl.ctypes.data, raw.ctypes.data, near.ctypes.data, st.ctypes.data, n_out.ctypes.data)
    return gt, pl, raw, near, st, n_out


def layout(n_sites, S=1, cohort=True):
    """svjg_geno.h: sites_layout(n_sites, S, cohort) -> dict of byte offsets (and in_bytes, total); a field the call does not have is 0"""
    out = np.zeros(12, np.uint64)
    _call("sitesim_layout", [ctypes.c_uint64, ctypes.c_uint64, ctypes.c_int, ctypes.c_void_p], int(n_sites), int(S), int(bool(cohort)), out.ctypes.data)
    return dict(zip(LAYOUT_FIELDS, (int(v) for v in out)))
