"""The cases of the cohort-prior tests: inputs from seeds, and where the model's answers for them are stored (tests/golden/cohort_prior/, written
by tests/golden/make_cohort_prior.py with tests/cohort_prior_model.py — the model at 60 digits takes minutes over all cases, so the suite loads
its answers, and tests/test_cohort_prior.py recomputes a sample of rows of every case on every run).  Shared by the CPU tests, the GPU tests and
the generator."""
import hashlib
import os

import numpy as np

from tests.test_cohort_gpu import _random_case

NONE = 0xFFFFFFFF
ERR = 5e-5
ROWS = 1500
SIZES = (1, 3, 4, 5, 31, 32, 33, 63, 64, 65, 130)
# the shapes that only the kernel's body knows (300 rows each): segment width 2, width 8 full and plus one, width 16 full and plus one; two
# further items on every lane (192), the third from its first sample to full (193, 256), one and then 64 items behind the three staged ones,
# which are recomputed at every step (257, 320)
SHAPE_SIZES, SHAPE_ROWS = (2, 8, 9, 16, 17, 192, 193, 256, 257, 320), 300
# (At S = 1 an item of odd ploidy with c1 = c2 keeps f = 1/2 and ties g with P - g exactly: such items are undecidable and left out, and with the
# low counts they are about 1.5 % of a draw; the seed of mixed_1 is the first of 7201 + 1000 k whose draw stays inside the 1 % cap.)
# (name, S, rows, ploidy pattern, seed): every S once with every item diploid (ploidy NULL) and once with 0..8 mixed within rows; the sex pattern
# (0 / 1 / 2 by row class and sample) on both sides of a wave; one case of deep counts (up to 5 000 reads on one allele: w_g underflows to 0)
CASES = tuple([("null_%d" % S, S, ROWS, None, 7000 + S) for S in SIZES] + [("mixed_%d" % S, S, ROWS, "mixed", 7200 + S if S > 1 else 33201) for S in SIZES]
              + [("sex_4", 4, ROWS, "sex", 7404), ("sex_65", 65, ROWS, "sex", 7465), ("deep_33", 33, 400, "deep", 7533)]
              + [("null_%d" % S, S, SHAPE_ROWS, None, 7000 + S) for S in SHAPE_SIZES] + [("mixed_%d" % S, S, SHAPE_ROWS, "mixed", 7200 + S) for S in SHAPE_SIZES]
              # staged slots that hold items of ploidy 0 (sex); weights that underflow to 0 in the staged and the recomputed arm (deep)
              + [("sex_193", 193, SHAPE_ROWS, "sex", 7593), ("deep_257", 257, 200, "deep", 7757)])
SHAPE_CASES = tuple(c[0] for c in CASES[-2 * len(SHAPE_SIZES) - 2:])
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "cohort_prior")
PLANTED = ("hom_ref", "hom_alt", "one_carrier", "absent", "zero_reads")
# what may be left out of the comparisons (the issue's margins), and the cap on it per case
RATIO_BAND, GQ_MARGIN, TOP_GAP, CAP = 1e-6, 1e-6, 1e-9, 0.01


def _mixed_ploidy(R, S, seed):
    """0..8, every value present (where there are nine items), mixed within rows"""
    rng = np.random.default_rng(seed)
    p = rng.integers(0, 9, size=(R, S)).astype(np.uint8)
    p.reshape(-1)[rng.permutation(R * S)[:9]] = np.arange(9)
    return p


def _sex_ploidy(R, S, seed):
    """rows in three classes (autosome, X, Y), samples in two sexes: 2 / 2, 2 / 1, 0 / 1"""
    rng = np.random.default_rng(seed)
    cls = rng.integers(0, 3, R)
    cls[:3] = (0, 1, 2)
    male = rng.random(S) < 0.5
    male[0], male[-1] = False, True
    table = np.array([[2, 2], [2, 1], [0, 1]], np.uint8)            # [class][male]
    return table[cls][:, male.astype(np.int64)]


def inputs(name):
    """-> dict: S, n_slots, counts[n_slots, S, 2], present[n_slots, S], t, slot, ok (as _random_case of tests/test_cohort_gpu.py makes them: counts 0..60,
    some deep, absent entries, rows without a slot or with the gate off), a share of low counts 0..4, the planted rows (`planted`: name -> row),
    ploidy[R, S] or None, max_ploidy"""
    _, S, R, pattern, seed = next(c for c in CASES if c[0] == name)
    n_slots, counts, present, t, slot, ok = _random_case(S, R, seed)
    rng = np.random.default_rng(seed + 1)
    low = rng.random((n_slots, S)) < 0.35                          # three or four informative reads: where the prior decides
    counts[low] = rng.integers(0, 5, size=(int(low.sum()), 2))
    if pattern == "deep":
        deep = rng.random((n_slots, S)) < 0.5
        side = rng.integers(0, 2, size=int(deep.sum()))
        v = np.stack([rng.integers(0, 5001, size=len(side)), rng.integers(0, 61, size=len(side))], axis=1)
        counts[deep] = np.where(side[:, None] == 0, v, v[:, ::-1])
    t[:4] = (0, 1, 2, 3)                                            # all four SV types, whatever the draw gave
    live = np.flatnonzero((slot != NONE) & ((ok & 1) != 0))
    at = live[rng.permutation(len(live))[:len(PLANTED)]]
    planted = dict(zip(PLANTED, (int(r) for r in at)))
    depth = rng.integers(12, 40, size=(len(PLANTED), S))
    for k, r in enumerate(at):
        present[slot[r]] = 1
        counts[slot[r]] = 0
    counts[slot[planted["hom_ref"]], :, 0] = depth[0]
    counts[slot[planted["hom_alt"]], :, 1] = depth[1]
    counts[slot[planted["one_carrier"]], :, 0] = depth[2]
    counts[slot[planted["one_carrier"]], S // 2] = (depth[2, 0], depth[2, 0])
    present[slot[planted["absent"]]] = 0
    if pattern == "mixed":
        ploidy = _mixed_ploidy(R, S, seed + 2)
    elif pattern == "sex":
        ploidy = _sex_ploidy(R, S, seed + 2)
    else:
        ploidy = None
    max_ploidy = 2 if ploidy is None else max(1, int(ploidy.max()))
    return {"name": name, "S": S, "n_slots": n_slots, "counts": counts, "present": present, "t": t, "slot": slot, "ok": ok, "planted": planted,
            "ploidy": ploidy, "max_ploidy": max_ploidy}


def gate(c):
    """what the cohort call leaves per item: done[R, S] (ok bit 0, a slot, the presence byte, a ploidy of 1 or more) and raw[R, S, 2] (0, 0 unless done)"""
    slot, ok = c["slot"], c["ok"]
    at = np.where(slot != NONE, slot, 0)
    done = ((slot != NONE) & ((ok & 1) != 0))[:, None] & (c["present"][at] != 0)
    if c["ploidy"] is not None:
        done &= c["ploidy"] != 0
    raw = np.where(done[:, :, None], c["counts"][at], 0).astype(np.uint32)
    return done.astype(np.uint8), raw


def digest(c):
    """of everything the model's answer depends on: a stored answer is only ever held against the inputs it was computed from"""
    h = hashlib.sha256()
    done, raw = gate(c)
    for a in (c["t"], done, raw, c["ploidy"] if c["ploidy"] is not None else np.zeros(0, np.uint8)):
        h.update(np.ascontiguousarray(a).tobytes())
    return h.hexdigest()


def golden_path(name):
    return os.path.join(GOLDEN, name + ".npz")


def load_golden(name, c):
    """the model's stored answer for case c at min_support 0 -> dict (f_hi, f_lo, steps, flag, row_out, gt, gq, item_out); the support gate is
    applied by with_support"""
    z = np.load(golden_path(name))
    assert str(z["digest"]) == digest(c), "tests/golden/cohort_prior/%s.npz was made from other inputs: run tests/golden/make_cohort_prior.py" % name
    R, S = len(c["t"]), c["S"]
    out = {k: z[k] for k in ("f_hi", "f_lo", "steps", "flag", "row_out", "gt", "gq")}
    out["f_lo"] = out["f_lo"].astype(np.float64)
    out["item_out"] = np.unpackbits(z["item_out"])[:R * S].reshape(R, S).astype(bool)
    return out


def with_support(model_gt, model_gq, sv_type, raw, min_support):
    """the model's calls at min_support 0 -> at min_support: c1 + c2 < min_support is a no-call"""
    c1 = np.where((sv_type[:, None] == 0) & (raw[:, :, 0] > 0), raw[:, :, 0] / 2, raw[:, :, 0])
    c2 = np.where((sv_type[:, None] == 1) & (raw[:, :, 1] > 0), raw[:, :, 1] / 2, raw[:, :, 1])
    off = c1 + c2 < min_support
    return np.where(off, 0xFF, model_gt).astype(np.uint8), np.where(off, 0xFF, model_gq).astype(np.uint8)
