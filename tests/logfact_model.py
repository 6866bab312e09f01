"""The log10(i!) table of the genotype kernels (k_logfact_*; svjg_geno.h: geno_row) against 60-digit values of the same quantity.

Helpers and checks only, no product code.  A table is a float64[n, 2] array of (hi, lo) pairs: the device's (capi.Context.logfact_table) or
a CPU stand-in's (tests/hostsim and its two siblings, built with the host libm).  The check_* functions hold the assertions that
tests/test_logfact.py applies to the stand-in and tests/test_logfact_gpu.py to the device, so both are held to the same bounds; each prints
the figure it measured before it asserts and returns it.

The bounds are the terms of the guard's budget in svjg_geno.h (the comment above PL_GUARD), not anything a table was seen to reach:
  ABS_BOUND   2^24 * 2^-50 = 1.49e-8   an entry: at most 2^24 terms log10(i) < 8, each within one ulp of that range (2^-50)
  INC_BOUND   2^-50 + 2^-59            table[i] - table[i-1] against log10(i): the one ulp, plus what the 80-bit log10 it is compared with
                                       may itself be off (measured against mpmath by check_longdouble_log10: 0.57 * 2^-60, asserted < 2^-59)
  COMB_BOUND  3.6e-7                   10 * |log10 comb from the table - the reference's double|: the budget's total, which PL_GUARD (1e-6)
                                       and a sixth of SITE_PL_GUARD (2.5e-6) must exceed
"""
import math
import random

import mpmath
import numpy as np

from tests import lik_model

DPS = 60
LOGFACT_CAP = 1 << 24                          # svjg_geno.h
BLOCK = 1024                                   # svjg_geno.h: LOGFACT_BLOCK
ULP = 2.0 ** -50                               # of a double in [4, 8): log10(i) for 10^4 <= i < 10^8
ABS_BOUND = LOGFACT_CAP * ULP
INC_BOUND = np.longdouble(2.0) ** -50 + np.longdouble(2.0) ** -59
COMB_BOUND = 3.6e-7
SLICE = 1 << 20
HAVE_80_BITS = np.finfo(np.longdouble).nmant >= 63
FALLBACK_SAMPLE = 200_000

# the pairs (n, k) that are checked whatever the fixtures hold: the cap's last entry against the middle, both ends and an odd place, and
# both sides of the first table's end and of the first block boundaries
EXTRA_PAIRS = [(2**24 - 1, 2**23), (2**24 - 1, 1), (2**24 - 1, 65), (2**24 - 1, 2**24 - 2), (2**24 - 1, 1000003),
               (65535, 32767), (65536, 32768), (1024, 512), (1025, 1), (2048, 1024)]


def log10_factorial(i):
    """log10(i!) as an mpf of 60 digits"""
    with mpmath.workdps(DPS):
        return mpmath.loggamma(int(i) + 1) / mpmath.log(10)


# ---- svjg_geno.h's double-double, operation for operation, on numpy float64 arrays (a dd is a pair (hi, lo)) ----

def two_sum(a, b):
    s = a + b
    bb = s - a
    return s, (a - (s - bb)) + (b - bb)


def dd_add(a, b):
    s_hi, s_lo = two_sum(a[0], b[0])
    t_hi, t_lo = two_sum(a[1], b[1])
    s_lo = s_lo + t_hi
    s_hi, s_lo = two_sum(s_hi, s_lo)
    s_lo = s_lo + t_lo
    return two_sum(s_hi, s_lo)


def comb_hi(table, n, k):
    """the double geno_row adds to the likelihoods: dd_add(dd_add(t[n], -t[n - k]), -t[k]).hi (svjg_geno.h: geno_row's
    table line and the rounding to a double behind it)"""
    n, k = np.asarray(n, np.int64), np.asarray(k, np.int64)
    t = np.asarray(table, np.float64)

    def at(i, sign):
        return sign * t[i, 0], sign * t[i, 1]
    return dd_add(dd_add(at(n, 1.0), at(n - k, -1.0)), at(k, -1.0))[0]


def increments(table, first, last):
    """table[i] - table[i - 1] for first <= i < last (first >= 1) as np.longdouble: (hi_i - hi_(i-1)) + (lo_i - lo_(i-1)) in 80-bit arithmetic.
    The difference of the high parts is exact there: both are multiples of the smaller one's ulp and less than 8 apart."""
    t = np.asarray(table[first - 1:last], np.float64).astype(np.longdouble)
    return (t[1:, 0] - t[:-1, 0]) + (t[1:, 1] - t[:-1, 1])


# ---- what is checked ----

def index_sample(n, seed=11):
    """the entries whose absolute value is checked in a table of n: every i < 2050, both sides of 2^16, the cap's last entry, both sides of
    200 seeded block boundaries, 3 000 seeded random indices (all cut to the table)"""
    rng = random.Random(seed)
    idx = set(range(min(n, 2050))) | {65535, 65536, 65537, LOGFACT_CAP - 1}
    for _ in range(200):
        b = rng.randrange(1, max(2, n // BLOCK)) * BLOCK
        idx |= {b - 1, b}
    idx |= {rng.randrange(n) for _ in range(3000)}
    return np.array(sorted(i for i in idx if i < n), dtype=np.int64)


def check_shape(table):
    """entries 0 and 1 are (0, 0); |lo| <= ulp(hi) / 2 everywhere; hi strictly increasing from i = 2"""
    t = np.asarray(table)
    assert t.dtype == np.float64 and t.ndim == 2 and t.shape[1] == 2 and len(t) >= 3
    assert not t[:2].any(), t[:2]
    hi, lo = t[:, 0], t[:, 1]
    assert np.isfinite(t).all()
    bad = np.flatnonzero(np.abs(lo) > np.spacing(hi) / 2)
    assert len(bad) == 0, (bad[:5], t[bad[:5]])
    bad = np.flatnonzero(np.diff(hi[1:]) <= 0) + 2
    assert len(bad) == 0, (bad[:5], t[bad[:5]])


def check_absolute(table, name="table"):
    """|hi + lo - log10(i!)| <= ABS_BOUND on index_sample -> (worst error, its index)"""
    idx = index_sample(len(table))
    worst, at = mpmath.mpf(0), -1
    with mpmath.workdps(DPS):
        ln10 = mpmath.log(10)
        for i in idx.tolist():
            e = abs(mpmath.mpf(float(table[i, 0])) + mpmath.mpf(float(table[i, 1])) - mpmath.loggamma(i + 1) / ln10)
            if e > worst:
                worst, at = e, i
    worst = float(worst)
    print(f"[logfact] {name}: worst |entry - log10(i!)| over {len(idx)} entries = {worst:.3e} at i = {at} (bound {ABS_BOUND:.3e})")
    assert worst <= ABS_BOUND, (worst, at)
    return worst, at


def check_longdouble_log10(n, seed=12, count=2000):
    """the reference of check_increments against mpmath: 80-bit log10(i) on `count` seeded indices below n -> worst error.  INC_BOUND's second
    term rests on it.  (Without an 80-bit longdouble check_increments compares with mpmath itself and there is nothing to measure.)"""
    if not HAVE_80_BITS:
        print("[logfact] NO 80-bit longdouble here: check_increments compares with mpmath on a sample")
        return None
    rng = random.Random(seed)
    idx = sorted({rng.randrange(2, n) for _ in range(count)} | {2, 3, 10, 9999, 10000, n - 1})
    got = np.log10(np.array(idx, dtype=np.longdouble))
    worst = mpmath.mpf(0)
    with mpmath.workdps(DPS):
        for i, g in zip(idx, got):
            hi = float(g)                                            # the 64-bit significand as two doubles: exact
            worst = max(worst, abs(mpmath.mpf(hi) + mpmath.mpf(float(g - np.longdouble(hi))) - mpmath.log10(i)))
    worst = float(worst)
    print(f"[logfact] 80-bit log10 against mpmath on {len(idx)} indices: within {worst / 2.0 ** -60:.3f} * 2^-60")
    assert worst < 2.0 ** -59, worst
    return worst


def check_increments(table, name="table"):
    """every table[i] - table[i - 1], 2 <= i < n, against log10(i): <= INC_BOUND -> (worst error in units of 2^-50, its index).  In 80-bit
    arithmetic over slices of 2^20; where numpy's longdouble is narrower, against mpmath on FALLBACK_SAMPLE seeded indices (and says so)."""
    n = len(table)
    worst, at = 0.0, -1
    if HAVE_80_BITS:
        for lo in range(2, n, SLICE):
            hi = min(n, lo + SLICE)
            err = np.abs(increments(table, lo, hi) - np.log10(np.arange(lo, hi, dtype=np.longdouble)))
            j = int(np.argmax(err))
            if float(err[j]) > worst:
                worst, at = float(err[j]), lo + j
        how = f"all {n - 2} increments, 80-bit log10"
    else:
        rng = random.Random(13)
        idx = sorted({rng.randrange(2, n) for _ in range(min(FALLBACK_SAMPLE, n))} | set(range(2, min(n, 2050))))
        with mpmath.workdps(DPS):
            for i in idx:
                d = (mpmath.mpf(float(table[i, 0])) - mpmath.mpf(float(table[i - 1, 0]))) + (mpmath.mpf(float(table[i, 1])) - mpmath.mpf(float(table[i - 1, 1])))
                e = float(abs(d - mpmath.log10(i)))
                if e > worst:
                    worst, at = e, i
        how = f"NO 80-bit longdouble here: mpmath on a seeded sample of {len(idx)} of the {n - 2} increments"
    print(f"[logfact] {name}: worst |increment - log10(i)| = {worst / ULP:.4f} * 2^-50 at i = {at} ({how}; bound 1 + 2^-9)")
    assert worst <= float(INC_BOUND), (name, at, worst / ULP)
    return worst / ULP, at


def _norm(t, ref, alt):
    """the reference's allele normalisation and rounding, as tests/test_lik_deep.py has it"""
    c1 = round(ref / 2, 1) if t == 0 and ref > 0 else ref
    c2 = round(alt / 2, 1) if t == 1 and alt > 0 else alt
    return int(round(c1, 0)), int(round(c2, 0))


def fixture_pairs(golden):
    """the unique (n, k) = (r1 + r2, r1) of all rows of the four golden/lik files with r1, r2 > 0 and n < LOGFACT_CAP, sorted"""
    pairs = set()
    for name in ("lik_kat.npz", "lik_boundary.npz", "lik_deep.npz", "lik_deep_hp.npz"):
        cases = np.load(f"{golden}/lik/{name}")["cases"]
        for t, ref, alt in {tuple(r) for r in cases[:, 0:3].tolist()}:
            r1, r2 = _norm(int(t), int(ref), int(alt))
            if r1 > 0 and r2 > 0 and r1 + r2 < LOGFACT_CAP:
                pairs.add((r1 + r2, r1))
    return sorted(pairs)


def all_pairs(golden):
    """fixture_pairs and EXTRA_PAIRS, each pair once"""
    return sorted(set(fixture_pairs(golden)) | set(EXTRA_PAIRS))


_want = {}


def reference_comb(pairs):
    """lik_model.log10_comb of every pair (the double the reference adds), computed once and shared; lik_model.Undecided is not caught: no
    pair may be left out"""
    for p in pairs:
        if p not in _want:
            _want[p] = lik_model.log10_comb(*p)
    return np.array([_want[p] for p in pairs], np.float64)


def check_pairs(table, pairs, name="table"):
    """10 * |comb_hi - the reference's log10 comb| < COMB_BOUND on every pair that fits the table -> (worst, its pair)"""
    pairs = [p for p in pairs if p[0] < len(table)]
    want = reference_comb(pairs)
    p = np.array(pairs, np.int64)
    d = 10.0 * np.abs(comb_hi(table, p[:, 0], p[:, 1]) - want)
    j = int(np.argmax(d))
    print(f"[logfact] {name}: worst 10 * |comb_hi - log10 comb| over {len(pairs)} pairs = {d[j]:.3e} at (n, k) = {pairs[j]} "
          f"(log10 comb = {want[j]:.6g}, one ulp of it times ten = {10 * math.ulp(want[j]):.2e}; bound {COMB_BOUND:.1e})")
    assert (d < COMB_BOUND).all(), (pairs[j], float(d[j]))
    return float(d[j]), pairs[j]


def compare_tables(a, b, name="a against b"):
    """-> (entries that differ in a bit, max |a - b| over all entries and its index), by slices"""
    assert a.shape == b.shape
    differ, worst, at = 0, 0.0, -1
    for lo in range(0, len(a), SLICE):
        x, y = a[lo:lo + SLICE], b[lo:lo + SLICE]
        differ += int(((x[:, 0] != y[:, 0]) | (x[:, 1] != y[:, 1])).sum())
        d = np.abs((x[:, 0] - y[:, 0]) + (x[:, 1] - y[:, 1]))              # (the high parts lie within a few ulps of each other: their difference is exact)
        j = int(np.argmax(d))
        if d[j] > worst:
            worst, at = float(d[j]), lo + j
    print(f"[logfact] {name}: {differ} of {len(a)} entries differ, max |difference| = {worst:.3e} at i = {at}")
    return differ, worst, at
