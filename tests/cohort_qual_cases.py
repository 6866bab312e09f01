"""The cases of the cohort site-quality tests: inputs from seeds, and where the model's answers for them are stored (tests/golden/cohort_qual/,
written by tests/golden/make_cohort_qual.py with tests/cohort_qual_model.py — the model at 60 digits takes minutes over all cases, so the suite
loads its answers, and tests/test_cohort_qual.py recomputes a sample of rows of every case on every run).  Shared by the CPU tests, the GPU tests
and the generator.  Counts are drawn as tests/cohort_prior_cases.py draws them, with its planted rows and three more."""
import os

import numpy as np

from tests import cohort_prior_cases as PC
from tests.test_cohort_gpu import _random_case

NONE = 0xFFFFFFFF
ERR = 5e-5
THETA = 1e-3
ROWS = 300
# every item diploid: M + 1 on both sides of 64 and 128 (one, two and three trips of a lane over k)
NULL_SIZES = (1, 2, 31, 32, 33, 63, 64, 65)
# ploidies 0..8 mixed within rows, max_ploidy 8
MIXED_SIZES = (1, 3, 8, 9, 17)
# (name, S, rows, pattern, seed).  deep: up to 5 000 reads on one allele, weights underflow to 0.  shallow: 600 diploid samples at one read each, the
# regime that forces the normalised recurrence.  het: 2 048 diploid samples, every one confidently het: the row's maximum shrinks by 2^-2048
# without rescaling and M is exactly QUAL_MAX_CHROMS (2 rows: the golden takes minutes, not hours)
CASES = tuple([("null_%d" % S, S, ROWS, None, 9000 + S) for S in NULL_SIZES] + [("mixed_%d" % S, S, ROWS, "mixed", 9200 + S) for S in MIXED_SIZES]
              + [("deep_33", 33, 100, "deep", 9533), ("shallow_600", 600, 20, "shallow", 9600), ("het_2048", 2048, 2, "het", 9648)])
# for the CPU tests only: twice the shallow case's samples in one row, where a plain convolution in doubles breaks down
EXTRA = (("shallow_1200", 1200, 1, "shallow", 9700),)
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "cohort_qual")
# the planted rows of cohort_prior_cases and three rows where every sample has one or two reads, most of them alt: no sample reaches min_support 3,
# together they leave no doubt ("the cohort decides")
WHISPER = ("whisper_0", "whisper_1", "whisper_2")
PLANTED = PC.PLANTED + WHISPER
# what may be left out of a comparison (the issue's margins), and the cap on it per case
TOP_GAP, HALF_BAND, CAP = 1e-9, 1e-6, 0.01


def _drawn(name, S, R, pattern, seed):
    n_slots, counts, present, t, slot, ok = _random_case(S, R, seed)
    rng = np.random.default_rng(seed + 1)
    low = rng.random((n_slots, S)) < 0.35
    counts[low] = rng.integers(0, 5, size=(int(low.sum()), 2))
    if pattern == "deep":
        deep = rng.random((n_slots, S)) < 0.5
        side = rng.integers(0, 2, size=int(deep.sum()))
        v = np.stack([rng.integers(0, 5001, size=len(side)), rng.integers(0, 61, size=len(side))], axis=1)
        counts[deep] = np.where(side[:, None] == 0, v, v[:, ::-1])
    t[:4] = (0, 1, 2, 3)
    live = np.flatnonzero((slot != NONE) & ((ok & 1) != 0))
    at = live[rng.permutation(len(live))[:len(PLANTED)]]
    planted = dict(zip(PLANTED, (int(r) for r in at)))
    depth = rng.integers(12, 40, size=(len(PLANTED), S))
    for r in at:
        present[slot[r]] = 1
        counts[slot[r]] = 0
    counts[slot[planted["hom_ref"]], :, 0] = depth[0]
    counts[slot[planted["hom_alt"]], :, 1] = depth[1]
    counts[slot[planted["one_carrier"]], :, 0] = depth[2]
    counts[slot[planted["one_carrier"]], S // 2] = (depth[2, 0], depth[2, 0])
    present[slot[planted["absent"]]] = 0
    for k, w in enumerate(WHISPER):                                  # (0, 1), (0, 2) or (1, 1): c1 + c2 <= 2 whatever the row's type
        pick = rng.integers(0, 3 + k, size=S)
        counts[slot[planted[w]]] = np.array([(0, 1), (0, 2), (1, 1), (0, 1), (0, 2)], np.uint32)[pick]
    ploidy = PC._mixed_ploidy(R, S, seed + 2) if pattern == "mixed" else None
    return n_slots, counts, present, t, slot, ok, planted, ploidy


def _shallow(S, R, seed):
    """every sample present with ONE ref read; from row 10 on, row r has r - 9 samples whose one read is alt instead"""
    rng = np.random.default_rng(seed)
    n_slots = R + 2
    counts = np.zeros((n_slots, S, 2), np.uint32)
    counts[:, :, 0] = 1
    slot = np.arange(R, dtype=np.uint32)
    for r in range(10, R):
        s = rng.permutation(S)[:r - 9]
        counts[r, s] = (0, 1)
    t = (np.arange(R) % 4).astype(np.uint8)
    return n_slots, counts, np.ones((n_slots, S), np.uint8), t, slot, np.ones(R, np.uint8)


def _het(S, R, seed):
    """every sample present, 15..40 reads on EACH allele (types 2 and 3: no count is halved)"""
    rng = np.random.default_rng(seed)
    n_slots = R + 2
    d = rng.integers(15, 41, size=(n_slots, S)).astype(np.uint32)
    counts = np.stack([d, d], axis=2)
    return n_slots, counts, np.ones((n_slots, S), np.uint8), np.array([2, 3] * R, np.uint8)[:R], np.arange(R, dtype=np.uint32), np.ones(R, np.uint8)


def inputs(name):
    """-> dict as tests/cohort_prior_cases.inputs: S, n_slots, counts[n_slots, S, 2], present[n_slots, S], t, slot, ok, planted (name -> row; empty
    for the two large cases), ploidy[R, S] or None, max_ploidy"""
    _, S, R, pattern, seed = next(c for c in CASES + EXTRA if c[0] == name)
    planted, ploidy = {}, None
    if pattern == "shallow":
        n_slots, counts, present, t, slot, ok = _shallow(S, R, seed)
    elif pattern == "het":
        n_slots, counts, present, t, slot, ok = _het(S, R, seed)
    else:
        n_slots, counts, present, t, slot, ok, planted, ploidy = _drawn(name, S, R, pattern, seed)
    return {"name": name, "S": S, "n_slots": n_slots, "counts": counts, "present": present, "t": t, "slot": slot, "ok": ok, "planted": planted,
            "ploidy": ploidy, "max_ploidy": 2 if ploidy is None else 8}


gate, digest = PC.gate, PC.digest


def golden_path(name):
    return os.path.join(GOLDEN, name + ".npz")


def load_golden(name, c):
    """the model's stored answer for case c -> dict: chroms, mlac, qual, qual_lo (float64), mlac_out, text_out (bool[R])"""
    z = np.load(golden_path(name))
    assert str(z["digest"]) == digest(c), "tests/golden/cohort_qual/%s.npz was made from other inputs: run tests/golden/make_cohort_qual.py" % name
    out = {k: z[k] for k in ("chroms", "mlac", "qual", "mlac_out", "text_out")}
    out["qual_lo"] = z["qual_lo"].astype(np.float64)
    return out


def check_planted(c, done, raw, qual, mlac, chroms):
    """what the planted rows say whatever the arithmetic: all hom-ref: mlac 0 and a small quality; all hom-alt: every chromosome alt; absent and
    zero reads: no quality; one carrier among diploid samples: mlac 1; the whisper rows: no sample has three reads, and the quality is beyond doubt"""
    p = c["planted"]
    if not p:
        return
    part = (done != 0) & (raw.sum(axis=2) > 0)
    if part[p["hom_ref"]].any():
        assert mlac[p["hom_ref"]] == 0 and qual[p["hom_ref"]] < 1
    if part[p["hom_alt"]].any():
        assert mlac[p["hom_alt"]] == chroms[p["hom_alt"]] > 0 and qual[p["hom_alt"]] > 100
    for r in (p["absent"], p["zero_reads"]):
        assert np.isnan(qual[r]) and mlac[r] == 0 and chroms[r] == 0
    if c["ploidy"] is None and c["S"] > 1:
        assert mlac[p["one_carrier"]] == 1 and qual[p["one_carrier"]] > 100
    for w in WHISPER:
        assert (raw[p[w]].sum(axis=1) <= 2).all()
        if part[p[w]].sum() >= 2:
            assert qual[p[w]] > 30 and mlac[p[w]] > 0
