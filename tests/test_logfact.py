"""The log10(i!) table on the CPU: the helpers and bounds of tests/logfact_model.py on the host-libm table of tests/hostsim at LOGFACT_CAP
entries.  What the reference arithmetic alone meets here is what tests/test_logfact_gpu.py asks of the device's table (k_logfact_*), entry
by entry.  Measured on the host table (glibc's log10, x86-64): worst absolute error 2.8e-11 (bound 1.49e-8), worst increment
0.58 * 2^-50 (bound 2^-50 + 2^-59), 80-bit log10 within 0.57 * 2^-60 of mpmath, worst 10 * |comb_hi - log10 comb| 2.3e-9 (bound 3.6e-7)."""
import random

import mpmath
import numpy as np
import pytest

from tests import lik_model
from tests import logfact_model as LM

CAP = LM.LOGFACT_CAP


@pytest.fixture(scope="module")
def host_table():
    from tests.hostsim import sim
    assert sim.geno_constants()[2] == CAP
    return sim.logfact_table(CAP)


def test_log10_factorial_against_exact_integers():
    """the 60-digit value against the factorial itself where that is cheap, and against the recurrence log10(i!) = log10((i-1)!) + log10(i)"""
    import math
    with mpmath.workdps(LM.DPS):
        for i in (0, 1, 2, 3, 20, 170, 171, 1000, 5000):
            assert abs(LM.log10_factorial(i) - mpmath.log10(math.factorial(i))) < mpmath.mpf("1e-50"), i
        for i in (65536, 1 << 20, CAP - 1):
            assert abs(LM.log10_factorial(i) - LM.log10_factorial(i - 1) - mpmath.log10(i)) < mpmath.mpf("1e-48"), i


def test_dd_helpers_mirror_the_header():
    """two_sum is error-free and dd_add's error is far below a double's ulp (against exact rationals); comb_hi on a table equals geno_row's
    own binomial term: a row's PLs from tests/hostsim change exactly as the model says when the term changes"""
    from fractions import Fraction
    rng = random.Random(5)
    a = np.array([rng.uniform(-1e8, 1e8) for _ in range(2000)])
    b = np.array([rng.uniform(-1, 1) * 10.0 ** rng.randint(-12, 8) for _ in range(2000)])
    s, e = LM.two_sum(a, b)
    for x, y, p, q in zip(a.tolist(), b.tolist(), s.tolist(), e.tolist()):
        assert Fraction(x) + Fraction(y) == Fraction(p) + Fraction(q)
    lo_a, lo_b = a * 2.0 ** -54 * 0.9, b * 2.0 ** -55
    h, l = LM.dd_add((a, lo_a), (b, lo_b))
    for i in range(0, 2000, 7):
        exact = Fraction(float(a[i])) + Fraction(float(lo_a[i])) + Fraction(float(b[i])) + Fraction(float(lo_b[i]))
        got = Fraction(float(h[i])) + Fraction(float(l[i]))
        assert abs(got - exact) <= abs(exact) * Fraction(1, 2 ** 100), i
        assert abs(l[i]) <= np.spacing(abs(h[i])) / 2


def test_comb_hi_is_the_row_arithmetic(host_table):
    """comb_hi against svjg_geno.h itself (tests/hostsim: geno_row) on rows of type BND with counts (r1, r2): PL_i = trunc(-10 (lik_i + comb_hi))
    computed here in exact rationals equals the harness's integer on every row it does not flag"""
    import math
    from fractions import Fraction
    from tests.hostsim import sim
    rng = random.Random(6)
    rows = [(3, rng.randint(1, 4000), rng.randint(1, 4000)) for _ in range(300)] + [(3, 70_000, 70_000), (3, CAP - 2, 1), (3, 1 << 23, (1 << 23) - 1)]
    c = np.array(rows, np.int64)
    e = 5e-5
    gt, pl, near, st = sim.genotype_rows(c[:, 0], c[:, 1:3], 3, e, host_table)
    assert not st.any()
    ch = LM.comb_hi(host_table, c[:, 1] + c[:, 2], c[:, 1])
    l_ok, l_err, l_half = math.log10(1 - e), math.log10(e), math.log10(1 / 2)
    seen = 0
    for (t, r1, r2), comb, got, flagged in zip(rows, ch.tolist(), pl.tolist(), near.tolist()):
        if flagged:
            continue
        liks = (Fraction(r1 * l_ok) + Fraction(r2 * l_err), Fraction((r1 + r2) * l_half), Fraction(r2 * l_ok) + Fraction(r1 * l_err))
        want = [int(-10 * (x + Fraction(comb))) for x in liks]
        assert want == got, (r1, r2)
        seen += 1
    assert seen >= 290


def test_table_sizes():
    """svjg_geno.h: logfact_built (what a build makes of a request) and logfact_reserve_to (what svjg_logfact_reserve builds)"""
    from tests.hostsim import sim
    built, reserve_to = sim.logfact_sizes()
    _, first, cap, grow_to = sim.geno_constants()
    assert [built(x) for x in (0, 1, 1024, 1025, first, first + 1, cap - 1, cap, cap + 1, 2**32 - 1)] == \
        [0, 1024, 1024, 2048, first, first + 1024, cap, cap, cap, cap]
    assert built(grow_to(140_000)) == 141_312 and built(grow_to(cap - 1)) == cap
    assert reserve_to(0, 0) == 0 and reserve_to(0, 1) == 1024 and reserve_to(first, 1) == 0 and reserve_to(first, first) == 0
    assert reserve_to(first, first + 1) == first + 1024 and reserve_to(141_312, 141_000) == 0
    assert reserve_to(first, 2**32 - 1) == cap and reserve_to(cap, 2**32 - 1) == 0 and reserve_to(cap, cap) == 0


def test_shape(host_table):
    LM.check_shape(host_table)


def test_absolute_value(host_table):
    idx = LM.index_sample(CAP)
    assert len(idx) > 5000 and {0, 2049, 65535, 65536, 65537, CAP - 1} <= set(idx.tolist())
    assert sum(1 for i in idx.tolist() if i % LM.BLOCK == 0 and i > 2050) >= 150
    worst, _ = LM.check_absolute(host_table, "host table")
    assert worst > 0.0                                       # (a sum of 2^24 rounded logarithms is not exact: the check measures something)


def test_every_increment(host_table):
    LM.check_longdouble_log10(CAP)
    # increments() itself: entry i of a table made of exact small integers
    t = np.zeros((6, 2))
    t[:, 0] = [0, 0, 3, 7, 12, 12]
    t[:, 1] = [0, 0, 0.25, -0.25, 0.5, 0.5]
    assert LM.increments(t, 2, 6).tolist() == [3.25, 3.5, 5.75, 0.0]
    worst, _ = LM.check_increments(host_table, "host table")
    assert 0.25 < worst                                      # (a double's log10 is at least a quarter ulp off somewhere in 2^24 values)


def test_a_wrong_entry_is_seen(host_table):
    """the checks see the two faults they are there for: one entry 1e-7 off (absolute value, increments), a block's offset dropped"""
    t = host_table[:70_000].copy()
    t[65536, 0] += 1e-7
    with pytest.raises(AssertionError):
        LM.check_absolute(t)
    with pytest.raises(AssertionError):
        LM.check_increments(t)
    t = host_table[:70_000].copy()
    t[3072:4096] = t[3072:4096] - t[3071]                    # the block's local scan without its offset
    with pytest.raises(AssertionError):
        LM.check_shape(t)
    with pytest.raises(AssertionError):
        LM.check_increments(t)
    with pytest.raises(AssertionError):
        LM.check_pairs(t, [(4000, 2000)])


def test_binomial_term(golden, host_table):
    """every (n, k) of the four golden/lik files and the ten of LM.EXTRA_PAIRS: 8 839 + 10, three of them in both"""
    pairs = LM.all_pairs(golden)
    assert len(LM.fixture_pairs(golden)) == 8839 and len(pairs) == 8846 and set(LM.EXTRA_PAIRS) <= set(pairs)
    try:
        LM.check_pairs(host_table, pairs, "host table")
    except lik_model.Undecided as e:                         # no pair may be left out
        pytest.fail(f"the model cannot decide a pair: {e}")


def test_the_two_harness_libraries_build_one_table(host_table):
    """tests/hostsim and tests/geno_sim build the table with one loop (tests/host_logfact.h) in two libraries: byte-equal on the first table's
    size, which they stay only while both are built to round alike"""
    import tests.geno_sim as geno_sim
    assert geno_sim.logfact_table(65536).tobytes() == host_table[:65536].tobytes()
