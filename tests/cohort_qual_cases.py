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
# The shapes that max_ploidy and the ploidy array decide.  sex: cohort_prior_cases._sex_ploidy (rows in three classes, samples in two sexes: 2 / 2,
# 2 / 1, 0 / 1), max_ploidy 2, the chrX / chrY shape of --cohort-ploidy.  hap: ploidy 1 with about one item in ten at 0, max_ploidy 1, M + 1 on both
# sides of 64 and 128; on the first 50 rows every sample is present at ploidy 1 with a read, so M = S there.  mixed_mP_20: ploidies 0..P, every
# value present, max_ploidy P.  mixed_128: 0..8 with every sample present: M around 500, cadence 5, lanes on their eighth trip over k at P up to 8
SEX_SIZES, HAP_SIZES, MIXED_UPTO = (33, 65, 129), (63, 64, 65, 129), (3, 4, 5, 6, 7)
# the shallow regime (one read a sample, qualities from about 0.01 to tens: where QUAL_ABS is what is tested) at mixed ploidy, on the chrX shape
# (every row of class X: 2 / 1 by sex), haploid, and at the call's limit at max_ploidy 8 (512 samples of ploidy 8: M = 4 096, more than 64 KiB of
# LDS, cadence 4, about 128 rescalings).  steep: 64 samples of ploidy 8, half of them 40 reads ref only and half 40 reads alt only, the second
# row the first in reverse sample order: the largest shrink per step and the largest E the suite sees
SHAPE_CASES = tuple([("sex_%d" % S, S, ROWS, "sex", 9300 + S) for S in SEX_SIZES] + [("hap_%d" % S, S, ROWS, "hap", 9400 + S) for S in HAP_SIZES]
                    + [("mixed_m%d_20" % P, 20, 100, "mixed%d" % P, 9800 + P) for P in MIXED_UPTO]
                    + [("mixed_128", 128, 60, "mixed_full", 9328), ("shallow_mixed_128", 128, 40, "shallow_mixed", 9828),
                       ("shallow_sex_300", 300, 20, "shallow_sex", 9830), ("shallow_hap_600", 600, 10, "shallow_hap", 9860),
                       ("shallow_poly_512", 512, 2, "shallow_poly", 9851), ("steep_64", 64, 2, "steep", 9864)])
CASES += SHAPE_CASES
NEW = tuple(c[0] for c in SHAPE_CASES)
# the call's max_ploidy by pattern (production passes max(1, ploidy.max()); the model does not depend on it, and neither does a stored answer)
MAX_PLOIDY = dict([(None, 2), ("deep", 2), ("shallow", 2), ("het", 2), ("mixed", 8), ("sex", 2), ("hap", 1), ("mixed_full", 8), ("shallow_mixed", 8),
                   ("shallow_sex", 2), ("shallow_hap", 1), ("shallow_poly", 8), ("steep", 8)] + [("mixed%d" % P, P) for P in MIXED_UPTO])
# for the CPU tests only: twice the shallow case's samples in one row, where a plain convolution in doubles breaks down
EXTRA = (("shallow_1200", 1200, 1, "shallow", 9700),)
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "cohort_qual")
# the planted rows of cohort_prior_cases and three rows where every sample has one or two reads, most of them alt: no sample reaches min_support 3,
# together they leave no doubt ("the cohort decides")
WHISPER = ("whisper_0", "whisper_1", "whisper_2")
PLANTED = PC.PLANTED + WHISPER
# what may be left out of a comparison (the issue's margins), and the cap on it per case
TOP_GAP, HALF_BAND, CAP = 1e-9, 1e-6, 0.01


def _ploidy_upto(R, S, P, seed):
    """0..P, every value present, mixed within rows (cohort_prior_cases._mixed_ploidy with another top)"""
    rng = np.random.default_rng(seed)
    p = rng.integers(0, P + 1, size=(R, S)).astype(np.uint8)
    p.reshape(-1)[rng.permutation(R * S)[:P + 1]] = np.arange(P + 1)
    return p


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
    ploidy = None
    if pattern in ("mixed", "mixed_full"):
        ploidy = PC._mixed_ploidy(R, S, seed + 2)
    elif pattern == "sex":
        ploidy = PC._sex_ploidy(R, S, seed + 2)
    elif pattern == "hap":
        ploidy = (np.random.default_rng(seed + 2).random((R, S)) >= 0.1).astype(np.uint8)
        ploidy[:50] = 1
        for r in np.flatnonzero(slot[:50] != NONE):                  # M = S on these rows (but for the planted ones among them)
            present[slot[r]] = 1
            counts[slot[r], counts[slot[r]].sum(axis=1) == 0, 0] = 1
    elif pattern is not None and pattern.startswith("mixed"):
        ploidy = _ploidy_upto(R, S, int(pattern[5:]), seed + 2)
    if pattern == "mixed_full":
        present[:] = 1
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
    return n_slots, counts, present, t, slot, ok, planted, ploidy


def _shallow(S, R, seed, quiet=10):
    """every sample present with ONE ref read; from row `quiet` on, row r has r - quiet + 1 samples whose one read is alt instead"""
    rng = np.random.default_rng(seed)
    n_slots = R + 2
    counts = np.zeros((n_slots, S, 2), np.uint32)
    counts[:, :, 0] = 1
    slot = np.arange(R, dtype=np.uint32)
    for r in range(quiet, R):
        s = rng.permutation(S)[:r - quiet + 1]
        counts[r, s] = (0, 1)
    t = (np.arange(R) % 4).astype(np.uint8)
    return n_slots, counts, np.ones((n_slots, S), np.uint8), t, slot, np.ones(R, np.uint8)


def _shallow_ploidy(S, R, pattern, seed):
    """the ploidy array of a shallow case: 0..8 mixed within rows; 2 / 1 by sex on every row; 1; 8"""
    if pattern == "shallow_mixed":
        return PC._mixed_ploidy(R, S, seed + 2)
    if pattern == "shallow_sex":
        male = np.random.default_rng(seed + 2).random(S) < 0.5
        male[0], male[-1] = False, True
        return np.tile(np.where(male, 1, 2).astype(np.uint8), (R, 1))
    return np.full((R, S), 1 if pattern == "shallow_hap" else 8, np.uint8)


def _steep(S, R):
    """the first half of the samples 40 reads ref only, the second half 40 reads alt only, at types 2 and 3 (no count is halved); row 1 is row 0 in
    reverse sample order; ploidy 8 everywhere"""
    n_slots = R + 2
    counts = np.zeros((n_slots, S, 2), np.uint32)
    counts[:, :S // 2, 0] = 40
    counts[:, S // 2:, 1] = 40
    counts[1] = counts[0, ::-1]
    return n_slots, counts, np.ones((n_slots, S), np.uint8), np.array([2, 3] * R, np.uint8)[:R], np.arange(R, dtype=np.uint32), np.ones(R, np.uint8)


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
    elif pattern is not None and pattern.startswith("shallow_"):
        n_slots, counts, present, t, slot, ok = _shallow(S, R, seed, quiet=max(1, R // 3))     # a third of the rows and more stay below a quality of 100
        ploidy = _shallow_ploidy(S, R, pattern, seed)
    elif pattern == "steep":
        n_slots, counts, present, t, slot, ok = _steep(S, R)
        ploidy = np.full((R, S), 8, np.uint8)
    elif pattern == "het":
        n_slots, counts, present, t, slot, ok = _het(S, R, seed)
    else:
        n_slots, counts, present, t, slot, ok, planted, ploidy = _drawn(name, S, R, pattern, seed)
    return {"name": name, "S": S, "n_slots": n_slots, "counts": counts, "present": present, "t": t, "slot": slot, "ok": ok, "planted": planted,
            "ploidy": ploidy, "max_ploidy": MAX_PLOIDY[pattern]}


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
