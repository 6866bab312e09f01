"""The model of svjg_cohort_hwe (svjg.h) in Python integers, straight from the definitions: the counts of a row's called diploid items, the exact
weights w(h) = 2^h n! / (a! h! b!) of Wigginton et al. 2005 by their integer recurrence, the two-sided test with the tie rule of R's fisher.test
and the one-sided test for excess heterozygotes.  No float before the last division (Python's int / int is correctly rounded, subnormals and 0
included), so it is exact: a fixture stores what it gives, and the tolerances of the tests are the device's own error, not the model's."""
import functools
import math

import numpy as np

TIE = 10 ** 7                            # w(h) TIE <= w(n_het) (TIE + 1): the 1e-7 slack
NEAR = 10 ** 8                           # a row is `near` when some w(h) / w(n_het) lies within 1 / NEAR of 1 + 1 / TIE


def row_counts(gt, ploidy=None):
    """-> counts[n, 3] int64 = n_ref, n_het, n_alt of the called diploid items (P = 2 and g <= 2) of every row"""
    g = np.asarray(gt).astype(np.int64)
    P = np.full(g.shape, 2, np.int64) if ploidy is None else np.asarray(ploidy).astype(np.int64)
    dip = (P == 2) & (g <= 2)
    return np.stack([(dip & (g == k)).sum(axis=1, dtype=np.int64) for k in range(3)], axis=1).reshape(len(g), 3)


def weights(n_ref, n_het, n_alt):
    """-> (m, {h: w(h)}) for every h of m's parity in 0..m, by w(h + 2) = w(h) 4 a b / ((h + 2) (h + 1)) from the exact w(m mod 2)"""
    n = n_ref + n_het + n_alt
    nA, nB = 2 * n_alt + n_het, 2 * n_ref + n_het
    m = min(nA, nB)
    h = m % 2
    a, b = (m - h) // 2, (2 * n - m - h) // 2
    w = 2 ** h * math.factorial(n) // (math.factorial(a) * math.factorial(h) * math.factorial(b))
    out = {h: w}
    while h + 2 <= m:
        num = w * 4 * a * b
        assert num % ((h + 2) * (h + 1)) == 0
        w = num // ((h + 2) * (h + 1))
        h, a, b = h + 2, a - 1, b - 1
        out[h] = w
    assert sum(out.values()) == math.comb(2 * n, m)                       # the self-test: every way to place m minor alleles on 2 n chromosomes
    return m, out


@functools.lru_cache(maxsize=None)
def row(n_ref, n_het, n_alt):
    """-> (HWE, EXCHET, near): floats (1.0, 1.0 where m = 0; NaN, NaN where n = 0) and whether a weight lies so close to the tie rule's edge
    that a float could decide it the other way (within 1e-8 of 1 + 1e-7: such a row is never stored in a fixture)"""
    n_ref, n_het, n_alt = int(n_ref), int(n_het), int(n_alt)
    if n_ref + n_het + n_alt == 0:
        return math.nan, math.nan, False
    m, w = weights(n_ref, n_het, n_alt)
    if m == 0:
        return 1.0, 1.0, False
    total, w0 = sum(w.values()), w[n_het]
    sel = sum(x for x in w.values() if x * TIE <= w0 * (TIE + 1))
    exc = sum(x for h, x in w.items() if h >= n_het)
    near = any(abs(x * NEAR - w0 * (NEAR + NEAR // TIE)) <= w0 for x in w.values())
    return sel / total, exc / total, near


def hwe(gt, ploidy=None):
    """-> (counts[n, 3] int64, p[n, 2] float64, near[n] bool) of a call"""
    counts = row_counts(gt, ploidy)
    rows = [row(*c) for c in counts.tolist()]
    p = np.array([r[:2] for r in rows], np.float64).reshape(len(counts), 2)
    return counts, p, np.array([r[2] for r in rows], bool)


def fis(n_ref, n_het, n_alt):
    """the inbreeding coefficient from the integers, one true division: 1 - n_het 2 n / (nA nB); None where m = 0"""
    n = n_ref + n_het + n_alt
    nA, nB = 2 * n_alt + n_het, 2 * n_ref + n_het
    return None if min(nA, nB) == 0 else 1 - n_het * 2 * n / (nA * nB)


def exact_ties(n_max):
    """every (n, m, h, h2), h < h2, n <= n_max, with w(h) == w(h2) exactly"""
    out = []
    for n in range(1, n_max + 1):
        for m in range(2, n + 1):
            _, w = weights(0, m, n - m)                                   # (any counts with this n and m: all het, m of them)
            seen = {}
            for h, x in w.items():
                if x in seen:
                    out.append((n, m, seen[x], h))
                seen[x] = h
    return out


def counts_row(n_ref, n_het, n_alt, S, rng):
    """a row of S calls with these diploid counts in a random order, 3 (no call) behind them"""
    g = np.array([0] * n_ref + [1] * n_het + [2] * n_alt + [3] * (S - n_ref - n_het - n_alt), np.uint8)
    return rng.permutation(g)


def fixture_families(seed):
    """-> {name: (gt, ploidy or None, done or None)}: the seven families of tests/golden/cohort_hwe"""
    rng = np.random.default_rng(seed)
    out = {}
    S, n = 100, 120
    f = rng.uniform(0.01, 0.5, (n, 1))
    out["hwe"] = ((rng.random((n, S)) < f).astype(np.uint8) + (rng.random((n, S)) < f).astype(np.uint8), None, None)
    S = 50
    out["excess"] = (np.stack([counts_row(0, k, 0, S, rng) for k in range(1, S + 1)]), None, None)
    S = 60
    out["deficit"] = (np.stack([counts_row(a, 0, b, S, rng) for a in range(0, S, 7) for b in range(1, S - a, 5)]), None, None)
    S = 40
    out["mono"] = (np.stack([counts_row(k, 0, 0, S, rng) for k in (0, 1, 17, S)] + [counts_row(0, 0, k, S, rng) for k in (1, 23, S)]), None, None)
    S, ties = 48, exact_ties(48)
    rows = [(n_ - h - (m - h) // 2, h, (m - h) // 2) for n_, m, h1, h2 in ties for h in (h1, h2)]
    out["ties"] = (np.stack([counts_row(*r, S, rng) for r in rows]), None, None)
    S, n = 70, 90
    gt = rng.choice(np.array([0, 0, 0, 1, 1, 2, 2, 3, 4, 8, 0xFF], np.uint8), size=(n, S))
    out["mixed"] = (gt, rng.choice(np.array([2, 2, 2, 2, 0, 1, 3, 4, 5, 6, 7, 8], np.uint8), size=(n, S)), (rng.random((n, S)) < 0.85).astype(np.uint8))
    S = 2048
    deep = [counts_row(1024, 0, 1024, S, rng), counts_row(1000, 48, 1000, S, rng), counts_row(2038, 0, 10, S, rng), counts_row(2040, 1, 7, S, rng),
            counts_row(0, 2048, 0, S, rng), counts_row(24, 2000, 24, S, rng), counts_row(700, 600, 700, S, rng)]
    f = rng.uniform(0.01, 0.5, (5, 1))
    deep += list((rng.random((5, S)) < f).astype(np.uint8) + (rng.random((5, S)) < f).astype(np.uint8))
    out["deep"] = (np.stack(deep), None, None)
    return out


def masked(gt, done):
    """the calls as cohort_hwe_rows hands them on: an item with done == 0 is 0xFF"""
    return gt if done is None else np.where(done != 0, gt, 0xFF).astype(np.uint8)


def write_fixtures(directory, seed=2300):
    """the families as directory/NAME.npz (gt, ploidy and done where the family has them, counts and p of the model).  No stored row may have a
    weight within 1e-8 of the tie rule's edge (`near`): a family that has one is drawn again with the next seed"""
    import os
    while True:
        fam = fixture_families(seed)
        res = {k: hwe(masked(gt, done), ploidy) for k, (gt, ploidy, done) in fam.items()}
        if not any(near.any() for _, _, near in res.values()):
            break
        seed += 1
    assert (res["deep"][1][:, 0] < 1e-300).any() and len(fam["ties"][0]) >= 2
    for k, (gt, ploidy, done) in fam.items():
        arrays = {"gt": gt, "counts": res[k][0].astype(np.uint32), "p": res[k][1]}
        if ploidy is not None:
            arrays["ploidy"] = ploidy
        if done is not None:
            arrays["done"] = done
        np.savez_compressed(os.path.join(directory, k + ".npz"), **arrays)
    return seed


class ModelHwe:
    """cohort_hwe as capi.Context has it, answered by the model"""

    def cohort_hwe(self, gt, ploidy=None):
        counts, p, _ = hwe(gt, ploidy)
        return counts.astype(np.uint32), p
