"""The site calls for insertions that share a position, single-sample and cohort, through the host harness (tests only)."""
import numpy as np

from tests.geno_sim import SITES, PTR, U32, U64, F64, u8, u32, f64, call, layout as _layout
from tests.geno_sim import build_main, logfact_table                                   # noqa: F401

MAX_ALTS = 6                             # svjg_geno.h: MAX_SITE_ALTS
NPL = 28                                 # svjg_geno.h: SITE_GENOTYPES


def log_table(err):
    """svjg_geno.h: site_log_table -> float64[16]: [0] = L_ok, [K] = L_x[K], [8 + K] = L_he[K]"""
    tab = np.zeros(16, np.float64)
    call("genosim_site_log_table", None, [F64, PTR], float(err), tab)
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
    tab = f64(tab)
    gt, pl, near, st = np.zeros((n, 2), np.uint8), np.full((n, NPL), -1, np.int64), np.zeros(n, np.uint8), np.zeros(n, np.uint8)
    n_out = np.zeros(n, np.uint64)
    call("genosim_site_genotype", None, [PTR] * 3 + [U64, U32, F64, PTR, U32] + [PTR] * 5,
         K, ref, alt, n, int(min_support), float(err), tab, len(tab), gt, pl, near, st, n_out)
    return gt, pl, near, st, n_out


def _matrix(counts, present):
    """counts[n_slots, S, 2] (ref, alt) -> the slot-major packed matrix uint64[n_slots * S], its presence bytes (None stays None), S, n_slots"""
    counts = np.asarray(counts, np.uint64)
    n_slots, S = counts.shape[:2]
    packed = np.ascontiguousarray((counts[..., 0] | (counts[..., 1] << np.uint64(32))).reshape(-1))
    if present is not None:
        present = u8(present).reshape(-1)
        assert len(present) == n_slots * S
    return packed, present, S, n_slots


def gather(counts, present, s, slots):
    """svjg_geno.h: site_gather as the lane of sample s does it.  counts[n_slots, S, 2], present[n_slots, S] or None (the single-sample call: every
    named slot is a member), slots[6] -> (members, bad, cref[6], calt[6])"""
    packed, present, S, n_slots = _matrix(counts, present)
    slots = u32(slots)
    assert slots.shape == (MAX_ALTS,)
    out = np.zeros(14, np.uint32)
    call("genosim_site_gather", None, [PTR, PTR, U64, U64, U32, PTR, PTR], packed, present, S, int(s), n_slots, slots, out)
    return int(out[0]), bool(out[1]), out[2:8].tolist(), out[8:14].tolist()


def site_items(counts, present, slots, min_support, err, tab):
    """svjg_geno.h: site_item over every (site, sample) item as the lanes run it.  counts[n_slots, S, 2], present[n_slots, S] or None, slots[n, 6] ->
    (gt[n, S, 2], pl[n, S, 28], raw[n, S, 7], boundary[n, S], members[n, S], status[n, S], n = s_K [n, S], bad[n, S])"""
    packed, present, S, n_slots = _matrix(counts, present)
    slots = u32(slots)
    n = len(slots)
    assert slots.shape == (n, MAX_ALTS)
    tab = f64(tab)
    gt, pl, raw = np.zeros((n, S, 2), np.uint8), np.full((n, S, NPL), -1, np.int64), np.full((n, S, MAX_ALTS + 1), 0xFFFFFFFF, np.uint32)
    boundary, members, st, bad = (np.full((n, S), 0xEE, np.uint8) for _ in range(4))
    n_out = np.zeros((n, S), np.uint64)
    call("genosim_site_items", None, [PTR, PTR, U64, U32, PTR, U64, U32, F64, PTR, U32] + [PTR] * 8,
         packed, present, S, n_slots, slots, n, int(min_support), float(err), tab, len(tab), gt, pl, raw, boundary, members, st, n_out, bad)
    return gt, pl, raw, boundary, members, st, n_out, bad


def compact(bits, cref, calt):
    """svjg_geno.h: site_compact -> (K, ref, alt[6])"""
    cref, calt = u32(cref), u32(calt)
    assert len(cref) == len(calt) == MAX_ALTS
    out = np.zeros(8, np.uint32)
    call("genosim_site_compact", None, [U32] + [PTR] * 3, int(bits), cref, calt, out)
    return int(out[0]), int(out[1]), out[2:].tolist()


def sums(w0, S, n_items, members, gt):
    """the wave whose first item is w0: the kernel's 18 ballots from members[n_items] / gt[n_items, 2] under cohort_segment's masks
    -> (leader uint8[64], ns uint32[64, 6], ac uint32[64, 6], word uint64[64, 6]); the sums are 0 on a lane that is no leader"""
    members, gt = u8(members), u8(gt)
    assert members.shape == (n_items,) and gt.shape == (n_items, 2)
    leader = np.zeros(64, np.uint8)
    ns, ac, word = np.zeros((64, MAX_ALTS), np.uint32), np.zeros((64, MAX_ALTS), np.uint32), np.zeros((64, MAX_ALTS), np.uint64)
    call("genosim_site_sums", None, [U64] * 3 + [PTR] * 6, int(w0), int(S), int(n_items), members, gt, leader, ns, ac, word)
    return leader, ns, ac, word


def items(bits, cref, calt, min_support, err, tab):
    """items from the gathered counts, the compaction and geno_site step by step: bits[n], cref[n, 6], calt[n, 6] -> (gt[n, 2], pl[n, 28], raw[n, 7],
    near, status, n = s_K)"""
    bits = u8(bits)
    n = len(bits)
    cref, calt = u32(cref), u32(calt)
    assert cref.shape == calt.shape == (n, MAX_ALTS)
    tab = f64(tab)
    gt, pl, raw = np.zeros((n, 2), np.uint8), np.full((n, NPL), -1, np.int64), np.full((n, MAX_ALTS + 1), 0xFFFFFFFF, np.uint32)
    near, st, n_out = np.zeros(n, np.uint8), np.zeros(n, np.uint8), np.zeros(n, np.uint64)
    call("genosim_site_items_by_steps", None, [U64] + [PTR] * 3 + [U32, F64, PTR, U32] + [PTR] * 6,
         n, bits, cref, calt, int(min_support), float(err), tab, len(tab), gt, pl, raw, near, st, n_out)
    return gt, pl, raw, near, st, n_out


def layout(n_sites, S=1, cohort=True, own_fields=False):
    """svjg_geno.h: sites_layout(n_sites, S, cohort) -> dict of byte offsets (and in_bytes, total); a field the call does not have is 0, or with
    own_fields (the single-sample call) is left out"""
    return _layout(SITES, n_sites, S, 0, int(bool(cohort)) | int(bool(own_fields)) << 1)
