"""The cases of the cohort-site-prior tests: inputs from seeds, and where the model's answers for them are stored (tests/golden/cohort_site_prior/,
written by tests/golden/make_cohort_site_prior.py with tests/site_prior_model.py: the model at 60 digits takes minutes over all cases, so the suite
loads its answers and tests/test_cohort_site_prior.py recomputes a sample of sites of every case on every run).  Shared by the CPU tests, the GPU
tests and the generator."""
import hashlib
import os

import numpy as np

NONE = 0xFFFFFFFF
ERR = 5e-5
SITES = 200
MAX_ALTS = 6
# segment widths 1, 2, 4, 8, 16 and 64; one item a lane up to 64 samples, two at 65, three at 130
SIZES = (1, 2, 3, 8, 9, 63, 64, 65, 130)
# mixed: C mixed 2..6, presence 0.9, counts 0..60; null: no alt reads; rare: one carrier of one candidate, every other sample ref; deep: counts up
# to 6e4 (weights underflow to 0 in doubles); absent: no sample has two members (no estimate, 0 steps)
KINDS = ("mixed", "null", "rare", "deep", "absent")
_KIND_SEED = {"mixed": 9100, "null": 9300, "rare": 9500, "deep": 9700, "absent": 9900}
# (name, S, sites, kind, seed).  The seed of a case is the first of base + S + 1000 k whose draw keeps the model's undecided items within the 1 % cap
# (tests/golden/make_cohort_site_prior.py searches and prints it; at 1..3 samples exact ties between two candidates with equal counts are common).
_SEED_OVERRIDE = {"mixed_1": 26101, "mixed_2": 10102}
CASES = tuple([("%s_%d" % (kind, S), S, SITES, kind, _SEED_OVERRIDE.get("%s_%d" % (kind, S), _KIND_SEED[kind] + S)) for kind in KINDS for S in SIZES]
              # a site count that is no multiple of 64 / W (W = 4: 16 sites a wave; 77 = 4 x 16 + 13)
              + [("mixed_3_odd", 3, 77, "mixed", _SEED_OVERRIDE.get("mixed_3_odd", 9163))])
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "cohort_site_prior")


def case_of(name):
    return next(c for c in CASES if c[0] == name)


def inputs(name, seed=None):
    """-> dict: S, n_slots, counts[n_slots, S, 2] (ref, alt), present[n_slots, S], slots[n, 6] (the candidates' slots, NONE behind them), C[n]"""
    _, S, n, kind, case_seed = case_of(name)
    rng = np.random.default_rng(case_seed if seed is None else seed)
    C = rng.integers(2, MAX_ALTS + 1, size=n)
    C[:5] = (2, 3, 4, 5, 6)
    n_slots = int(C.sum())
    order = rng.permutation(n_slots).astype(np.uint32)                # the candidates' slots lie anywhere in the matrix
    slots = np.full((n, MAX_ALTS), NONE, np.uint32)
    at = 0
    for k in range(n):
        slots[k, :C[k]] = order[at:at + C[k]]
        at += C[k]
    counts = rng.integers(0, 61, size=(n_slots, S, 2)).astype(np.uint64)
    present = (rng.random((n_slots, S)) < 0.9).astype(np.uint8)
    if kind == "mixed":
        low = rng.random((n_slots, S)) < 0.3                          # a few informative reads: where the prior decides
        counts[low] = rng.integers(0, 5, size=(int(low.sum()), 2))
    elif kind == "null":
        counts[:, :, 1] = 0
    elif kind == "rare":
        counts[:, :, 1] = 0
        counts[:, :, 0] = rng.integers(12, 40, size=(n_slots, S))
        present[:] = 1
        for k in range(n):
            j, s = int(rng.integers(0, C[k])), int(rng.integers(0, S))
            counts[slots[k, j], s, 1] = counts[slots[k, j], s, 0]
    elif kind == "deep":
        deep = rng.random((n_slots, S)) < 0.5
        counts[deep] = rng.integers(0, 60001, size=(int(deep.sum()), 2))
    elif kind == "absent":
        present[:] = 0
        for k in range(n):
            one = rng.integers(-1, C[k], size=S)                      # at most one member a sample
            for s in np.flatnonzero(one >= 0):
                present[slots[k, one[s]], s] = 1
    return {"name": name, "S": S, "n_slots": n_slots, "counts": counts, "present": present, "slots": slots, "C": C.astype(np.uint32)}


def first_kernel(c):
    """what svjg_genotype_cohort_sites leaves per item: members[n, S] (bit j = candidate j present) and raw[n, S, 7] (the ref maximum over the
    members and the members' alt counts compacted; zeros without a site, K' < 2)"""
    slots, S = c["slots"], c["S"]
    n = len(slots)
    members, raw = np.zeros((n, S), np.uint8), np.zeros((n, S, MAX_ALTS + 1), np.uint32)
    for k in range(n):
        for s in range(S):
            here = [j for j in range(MAX_ALTS) if slots[k, j] != NONE and c["present"][slots[k, j], s]]
            members[k, s] = sum(1 << j for j in here)
            if len(here) >= 2:
                raw[k, s, 0] = max(int(c["counts"][slots[k, j], s, 0]) for j in here)
                raw[k, s, 1:1 + len(here)] = [int(c["counts"][slots[k, j], s, 1]) for j in here]
    return members, raw


def digest(c):
    """of everything the model's answer depends on: a stored answer is only ever held against the inputs it was computed from"""
    h = hashlib.sha256()
    members, raw = first_kernel(c)
    for a in (members, raw, c["C"]):
        h.update(np.ascontiguousarray(a).tobytes())
    return h.hexdigest()


def golden_path(name):
    return os.path.join(GOLDEN, name + ".npz")


def load_golden(name, c):
    """the model's stored answer for case c at min_support 0 -> dict (p_hi, p_lo, steps, flag, site_out, sgt, sgq, item_out); the support gate is
    applied by with_support"""
    z = np.load(golden_path(name))
    assert str(z["digest"]) == digest(c), "tests/golden/cohort_site_prior/%s.npz was made from other inputs: run tests/golden/make_cohort_site_prior.py" % name
    n, S = len(c["slots"]), c["S"]
    out = {k: z[k] for k in ("p_hi", "p_lo", "steps", "flag", "site_out", "sgt", "sgq")}
    out["p_lo"] = out["p_lo"].astype(np.float64)
    out["item_out"] = np.unpackbits(z["item_out"])[:n * S].reshape(n, S).astype(bool)
    return out


def with_support(sgt, sgq, raw, min_support):
    """the model's calls at min_support 0 -> at min_support: N = ref + sum alt / 2 < min_support is a no-call"""
    N = raw[:, :, 0] + raw[:, :, 1:].sum(axis=2) / 2
    off = N < min_support
    return np.where(off[:, :, None], 0xFF, sgt).astype(np.uint8), np.where(off, 0xFF, sgq).astype(np.uint8)
