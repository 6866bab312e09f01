"""What both site kernels do per item, on the CPU (svjg_geno.h: site_gather, site_item, sites_layout, compiled with g++ by tests/geno_sim): the slot
gather against picking the candidates out one by one, bad slots, the item of the single-sample call against geno_site on the same (K, ref, alt),
the item of the cohort call against the compaction and geno_site step by step, and the one layout in both of its cases."""
import numpy as np
import pytest

from tests import site_model as SM
from tests.geno_sim import site as sim

NONE = 0xFFFFFFFF
NO_CALL = 0xFF
E, MS = 5e-5, 3


@pytest.fixture(scope="module")
def tab():
    return sim.logfact_table(1 << 17)


# ---- the gather ----

@pytest.mark.parametrize("K", [2, 3, 4, 5, 6])
def test_gather_of_every_presence_pattern(K):
    """one site of K candidates in a matrix of three samples, sample 1's column set to each of the 64 presence patterns: members, cref and calt are
    the candidates picked out one by one; present = None (the count vector) is the all-present pattern"""
    rng = np.random.default_rng(40 + K)
    n_slots, S, s = 11, 3, 1
    counts = rng.integers(1, 1000, (n_slots, S, 2))
    slots = np.full(6, NONE, np.uint32)
    slots[:K] = rng.choice(n_slots, K, replace=False)
    for bits in range(64):
        present = rng.random((n_slots, S)) < 0.5
        present[slots[:K], s] = [(bits >> j) & 1 for j in range(K)]
        at = [j for j in range(K) if (bits >> j) & 1]
        members, bad, cref, calt = sim.gather(counts, present, s, slots)
        assert not bad and members == sum(1 << j for j in at), (K, bits)
        assert cref == [int(counts[slots[j], s, 0]) if j in at else 0 for j in range(6)], (K, bits)
        assert calt == [int(counts[slots[j], s, 1]) if j in at else 0 for j in range(6)], (K, bits)
    vec = counts[:, s:s + 1]
    want = sim.gather(vec, np.ones((n_slots, 1), bool), 0, slots)
    assert sim.gather(vec, None, 0, slots) == want and want[0] == (1 << K) - 1 and not want[1]


@pytest.mark.parametrize("S", [1, 3])
def test_bad_slots(S):
    """a hole in front of a slot, and a slot equal to n_slots, give `bad`; the slots in front of the bad one are still gathered, nothing is read
    through it (the arrays are exactly n_slots x S: the sanitizer program holds that, test_cohort_joint_ins.py runs it)"""
    rng = np.random.default_rng(7)
    n_slots = 9
    counts = rng.integers(1, 50, (n_slots, S, 2))
    present = None if S == 1 else np.ones((n_slots, S), bool)
    s = S - 1
    good = [4, 2, 7, NONE, NONE, NONE]
    assert sim.gather(counts, present, s, good)[:2] == (0b111, False)
    for slots in ([NONE, 2, 7, NONE, NONE, NONE], [4, NONE, 7, NONE, NONE, NONE], [4, 2, NONE, NONE, NONE, 0], [NONE, 0x7FFFFFFF, NONE, NONE, NONE, NONE]):
        members, bad, cref, calt = sim.gather(counts, present, s, slots)
        first = slots.index(NONE)
        assert bad and members == (1 << first) - 1 and not any(cref[first:]) and not any(calt[first:]), slots
    for slots in ([4, n_slots, 7, NONE, NONE, NONE], [n_slots, 2, NONE, NONE, NONE, NONE], [4, 2, 7, 1, 3, n_slots], [4, 0xFFFFFFFE, NONE, NONE, NONE, NONE]):
        members, bad, cref, calt = sim.gather(counts, present, s, slots)
        out = next(j for j, v in enumerate(slots) if v != NONE and v >= n_slots)
        assert bad and not (members >> out) & 1 and cref[out] == 0 and calt[out] == 0, slots
    # the item behind a bad gather: no members, no call, zeros, and `bad` for the kernel's flag
    gt, pl, raw, boundary, members, st, _, bad = sim.site_items(counts, present, [good, [4, NONE, 7, NONE, NONE, NONE], [4, n_slots, 7, NONE, NONE, NONE]], MS, E,
                                                                sim.logfact_table(4096))
    assert bad[:, s].tolist() == [0, 1, 1] and members[:, s].tolist() == [0b111, 0, 0] and not st.any()
    assert (gt[1:] == NO_CALL).all() and not pl[1:].any() and not raw[1:].any() and not boundary[1:].any()
    assert raw[0, s, 0] == counts[[4, 2, 7], s, 0].max() and raw[0, s, 1:4].tolist() == counts[[4, 2, 7], s, 1].tolist()


# ---- the item ----

def test_single_sample_item_is_geno_site_on_the_same_counts(tab):
    """site_item on a count vector with present = None gives the bytes of sitesim_genotype (geno_site) on the same (K, ref, alt): the random set of
    tests/site_model.py, each site's members at slots of their own, the ref maximum at a random member"""
    rng = np.random.default_rng(21)
    sites = SM.random_sites(400, seed=5)
    n_slots = sum(len(a) for _, a in sites)
    counts, slots, at = np.zeros((n_slots, 1, 2), np.uint32), np.full((len(sites), 6), NONE, np.uint32), 0
    order = rng.permutation(n_slots)
    for k, (ref, alts) in enumerate(sites):
        m = order[at:at + len(alts)]
        at += len(alts)
        slots[k, :len(alts)] = m
        counts[m, 0, 1] = alts
        counts[m, 0, 0] = rng.integers(0, ref + 1, len(alts))
        counts[m[rng.integers(len(m))], 0, 0] = ref
    for ms, e in ((MS, E), (0, 0.3)):
        w_gt, w_pl, w_near, w_st, w_n = sim.genotype_sites(sites, ms, e, tab)
        gt, pl, raw, boundary, members, st, n, bad = sim.site_items(counts, None, slots, ms, e, tab)
        assert not bad.any() and members[:, 0].tolist() == [(1 << len(a)) - 1 for _, a in sites]
        assert gt[:, 0].tobytes() == w_gt.tobytes() and pl[:, 0].tobytes() == w_pl.tobytes() and boundary[:, 0].tobytes() == w_near.tobytes()
        assert st[:, 0].tobytes() == w_st.tobytes() and n[:, 0].tobytes() == w_n.tobytes()
        assert raw[:, 0].tolist() == [[ref] + alts + [0] * (6 - len(alts)) for ref, alts in sites]
    # a site of one member: the host refuses it; the kernel's item counts it as bad and leaves no call
    gt, pl, raw, boundary, members, st, n, bad = sim.site_items(counts, None, [[int(slots[0, 0])] + [NONE] * 5], MS, E, tab)
    assert bad[0, 0] == 1 and (gt == NO_CALL).all() and not pl.any() and not raw.any() and not boundary.any() and not st.any()


def test_cohort_item_is_the_compaction_and_geno_site_on_the_gathered_counts(tab):
    """site_item at S = 3 gives the bytes of the harness's items() entry (site_compact and geno_site step by step) on the gathered (bits, cref,
    calt): K' = 0..6, items with K' < 2 are zeros and 0xFF, 0xFF, and an item whose s_K lies beyond the table handed in answers status 1 and touches
    no entry"""
    rng = np.random.default_rng(33)
    n_sites, S = 300, 3
    K = 2 + np.arange(n_sites) % 5
    n_slots = int(K.sum())                                                    # every candidate a slot of its own, in no order
    counts = rng.integers(0, 61, (n_slots, S, 2)).astype(np.uint32)
    present = rng.random((n_slots, S)) < 0.6
    slots = np.full((n_sites, 6), NONE, np.uint32)
    slots[np.arange(6)[None, :] < K[:, None]] = rng.permutation(n_slots)
    deep = slots[7, :2]                                                       # s_K = 2 500 beyond a table of 2 048 entries, for sample 2 only
    counts[deep, 2], present[deep, 2] = (1500, 2000), True
    short = tab[:2048]
    gt, pl, raw, boundary, members, st, n, bad = sim.site_items(counts, present, slots, MS, E, short)
    bits, cref, calt = np.zeros((n_sites, S), np.uint8), np.zeros((n_sites, S, 6), np.uint32), np.zeros((n_sites, S, 6), np.uint32)
    for k, s in np.ndindex(n_sites, S):
        bits[k, s], b, cref[k, s], calt[k, s] = sim.gather(counts, present, s, slots[k])
        assert not b
    w_gt, w_pl, w_raw, w_near, w_st, w_n = sim.items(bits.reshape(-1), cref.reshape(-1, 6), calt.reshape(-1, 6), MS, E, short)
    assert not bad.any() and members.tobytes() == bits.tobytes()
    assert gt.tobytes() == w_gt.tobytes() and pl.tobytes() == w_pl.tobytes() and raw.tobytes() == w_raw.tobytes() and boundary.tobytes() == w_near.tobytes()
    assert st.tobytes() == w_st.tobytes() and n.tobytes() == w_n.tobytes()
    k_of = np.array([bin(int(b)).count("1") for b in bits.reshape(-1)]).reshape(n_sites, S)
    assert set(k_of.reshape(-1).tolist()) == set(range(7))
    few = k_of < 2
    assert few.sum() > 100 and (gt[few] == NO_CALL).all() and not pl[few].any() and not raw[few].any() and not boundary[few].any() and not st[few].any()
    assert st[7, 2] == 1 and n[7, 2] >= 2048 and st.sum() == 1               # (status 1 = GENO_ROW_GROW; the run under the sanitizers reads no entry beyond)


# ---- the one layout ----

@pytest.mark.parametrize("S", [1, 3, 64, 65])
@pytest.mark.parametrize("n", [1, 7, 1000])
def test_one_sites_layout_in_both_cases(n, S):
    """sites_layout(n, S, true) gives the offsets tests/test_cohort_joint_ins.py pins for the cohort call, sites_layout(n, 1, false) those
    tests/test_rows_layout.py pins for the single-sample call; a field the call does not have is 0"""
    L, items = sim.layout(n, S, True), n * S
    site = (256 * items + 7) & ~7
    assert L == {"pl": 0, "raw": 224 * items, "gt": 252 * items, "members": 254 * items, "boundary": 255 * items, "site": site, "maxn": site + 48 * n,
                 "in_at": site + 48 * n + 8, "logs": site + 48 * n + 8, "slots": site + 48 * n + 8 + 128, "in_bytes": 128 + 24 * n,
                 "total": site + 48 * n + 8 + 128 + 24 * n + 64}
    L = sim.layout(n, 1, False)
    maxn = (255 * n + 7) & ~7
    assert L == {"pl": 0, "raw": 224 * n, "gt": 252 * n, "members": 0, "boundary": 254 * n, "site": 0, "maxn": maxn, "in_at": maxn + 8, "logs": maxn + 8,
                 "slots": maxn + 8 + 128, "in_bytes": 128 + 24 * n, "total": maxn + 8 + 128 + 24 * n + 64}
