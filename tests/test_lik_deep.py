"""The likelihood at deep counts, on the CPU: the high-precision model of the reference's likelihood() (tests/lik_model.py) against
CPython's own math.log10 and against every known answer of the reference; the host recomputation svjg.genotype.exact_pl against the
model where the reference cannot finish; and k_genotype's per-row arithmetic (svjg_geno.h, compiled for the host by tests/hostsim)
against the fixtures."""
import math
import random
import time

import mpmath
import numpy as np
import pytest

from tests import lik_model as M

TYPES = ("DEL", "INS", "INV", "BND")
GT = {"0/0": 0, "0/1": 1, "1/1": 2, "./.": 3}
LOGFACT_CAP = 1 << 24                          # svjg_geno.h


def _load(golden, name):
    z = np.load(f"{golden}/lik/{name}")
    return z["cases"], z["err"]


def test_model_log10_of_big_integers():
    """the loghelper emulation against math.log10 on 10 000 random integers of 900 .. 1150 bits (across the 2^1024 switch between
    PyLong_AsDouble and _PyLong_Frexp), with the integer known exactly and with only its 80-digit logarithm known; and on integers
    whose top 53 bits are a tie or carry when rounded"""
    rng = random.Random(7)
    for i in range(10_000):
        b = rng.randint(900, 1150)
        c = rng.getrandbits(b) | (1 << (b - 1))
        want = math.log10(c)
        assert M.log10_int(c) == want, c
        if i % 4 == 0:
            with mpmath.workdps(M.DPS):
                assert M.log10_of_ln(mpmath.log(c)) == want, c
    for b in (1023, 1024, 1025, 1100):
        for top in ((1 << 53) - 1, (1 << 52) + 1, (1 << 52) + 2):
            for tail in (0, 1, 1 << (b - 55), (1 << (b - 54)) - 1):
                c = (top << (b - 53)) | (tail & ((1 << (b - 53)) - 1))
                assert M.log10_int(c) == math.log10(c), (b, top, tail)
                c = (top << (b - 53)) + (1 << (b - 54))                          # exactly half way: ties to even
                assert M.log10_int(c) == math.log10(c), (b, top, "tie")


def test_model_comb_against_math_comb():
    """log10 comb(n, k) of the model (80-digit log-gamma) equals math.log10(math.comb(n, k)) on 3 000 random (n, k), n <= 12 000"""
    rng = random.Random(8)
    for _ in range(3000):
        n = rng.randint(65, 12_000)
        k = rng.randint(65, n - 65) if n > 130 else rng.randint(0, n)
        assert M.log10_comb(n, k) == math.log10(math.comb(n, k)), (n, k)


@pytest.mark.parametrize("name", ["lik_kat.npz", "lik_boundary.npz", "lik_deep.npz", "lik_products.npz"])
def test_model_reproduces_the_reference(golden, name):
    """the model against every known answer of the reference: GT and the three PLs, no difference"""
    cases, errs = _load(golden, name)
    bad = []
    for c, e in zip(cases.tolist(), errs.tolist()):
        gt, pl = M.likelihood([c[1], c[2]], TYPES[c[0]], c[3], e)
        if GT[gt] != c[4] or [int(x) for x in pl] != c[5:8]:
            bad.append((c, gt, pl))
    assert not bad, bad[:5]


def test_exact_pl_on_rows_the_reference_cannot_finish(golden):
    """svjg.genotype.exact_pl (the host recomputation of flagged rows) against the model on lik_deep_hp.npz: both counts between
    10^6 and 2^32 - 1, the wrapping pairs, PLs next to an integer; each row within a second (math.comb would take minutes)"""
    from svjg import genotype
    cases, errs = _load(golden, "lik_deep_hp.npz")
    worst = 0.0
    for c, e in zip(cases.tolist(), errs.tolist()):
        t0 = time.perf_counter()
        got = genotype.exact_pl(c[0], c[1], c[2], e)
        worst = max(worst, time.perf_counter() - t0)
        assert got == c[5:8], c
    assert worst < 1.0, worst


def test_exact_pl_on_the_reference_answers(golden):
    """exact_pl against the reference itself where it is cheap: every deep row of lik_deep.npz"""
    from svjg import genotype
    cases, errs = _load(golden, "lik_deep.npz")
    for c, e in zip(cases.tolist(), errs.tolist()):
        assert genotype.exact_pl(c[0], c[1], c[2], e) == c[5:8], c


@pytest.fixture(scope="module")
def host_table():
    from tests.hostsim import sim
    return sim.logfact_table(LOGFACT_CAP)


@pytest.mark.parametrize("name", ["lik_kat.npz", "lik_boundary.npz", "lik_deep.npz", "lik_deep_hp.npz", "lik_products.npz"])
def test_kernel_row_arithmetic_on_the_host(golden, host_table, name):
    """k_genotype's per-row arithmetic (svjg_geno.h: geno_row, compiled with g++) with a log10(i!) table of LOGFACT_CAP entries built
    with the HOST libm's log10 — not the device's (the -m gpu tests check that one).  Every row: GT equals the fixture; a row the
    routine does not flag has the fixture's PLs; a flagged row gets them from exact_pl; a row with n >= LOGFACT_CAP (both counts > 0)
    is flagged for the host and never asks for a larger table; a row whose PL lies within 1e-7 of an integer is flagged; a one-sided
    row (lik_products.npz: fused, onesided — its binomial term is log10(1)) is never flagged, so its PLs are the routine's own."""
    from svjg import genotype
    from tests.hostsim import sim
    cases, errs = _load(golden, name)
    z = np.load(f"{golden}/lik/{name}")
    one_sided = np.isin(z["src"], ("fused", "onesided")) if "src" in z.files else np.zeros(len(cases), bool)
    for e in np.unique(errs):
        for ms in np.unique(cases[:, 3]):
            sel = np.flatnonzero((errs == e) & (cases[:, 3] == ms))
            if not len(sel):
                continue
            c = cases[sel]
            gt, pl, near, st = sim.genotype_rows(c[:, 0], c[:, 1:3], int(ms), float(e), host_table)
            assert np.array_equal(gt, c[:, 4]), c[gt != c[:, 4]][:5]
            assert not (st == 1).any()
            r = np.array([sum(x) for x in (_norm(int(t), int(a), int(b)) for t, a, b in c[:, 0:3])], dtype=np.int64)
            k = np.array([min(_norm(int(t), int(a), int(b))) for t, a, b in c[:, 0:3]], dtype=np.int64)
            beyond = (r >= LOGFACT_CAP) & (k > 0)
            assert np.array_equal(st == 2, beyond)
            assert near[beyond].all()
            assert not near[one_sided[sel]].any(), c[one_sided[sel] & (near != 0)][:5]
            ok = near == 0
            bad = np.flatnonzero(ok & (pl != c[:, 5:8]).any(axis=1))
            assert len(bad) == 0, (c[bad[:5]], pl[bad[:5]])
            for i in np.flatnonzero(near):
                assert genotype.exact_pl(int(c[i, 0]), int(c[i, 1]), int(c[i, 2]), float(e)) == c[i, 5:8].tolist(), c[i]
    if "src" in np.load(f"{golden}/lik/{name}").files:
        src = np.load(f"{golden}/lik/{name}")["src"]
        tight = np.flatnonzero(src == "near")
        if len(tight):
            c = cases[tight]
            _, _, near, _ = sim.genotype_rows(c[:, 0], c[:, 1:3], 3, float(errs[0]), host_table)
            assert near.all(), c[near == 0][:5]


def _norm(t, ref, alt):
    c1 = round(ref / 2, 1) if t == 0 and ref > 0 else ref
    c2 = round(alt / 2, 1) if t == 1 and alt > 0 else alt
    return int(round(c1, 0)), int(round(c2, 0))


def test_kernel_row_never_indexes_with_a_wrapped_sum(host_table):
    """the pairs whose 32-bit sum r1 + r2 wraps (ref = alt = 2^31, ref = 2^32 - 1 with alt = 1, ...): n is computed in 64 bits, the
    rows beyond the table are flagged for the host, and the ones with k = 0 need no table at all (comb(n, 0) = 1)"""
    from tests.hostsim import sim
    rows = [(3, 2**31, 2**31), (3, 2**32 - 1, 1), (2, 1, 2**32 - 1), (3, 2**32 - 1, 2**32 - 1), (0, 2**32 - 1, 2**31),
            (3, 4 * 10**9, 0), (1, 0, 2**32 - 1), (3, 1000, 69_000)]
    c = np.array(rows, dtype=np.int64)
    gt, pl, near, st = sim.genotype_rows(c[:, 0], c[:, 1:3], 3, 5e-5, host_table[:65536])
    assert st.tolist() == [2, 2, 2, 2, 2, 0, 0, 1]              # 2: beyond the cap (the host), 1: the table must grow (n = 70 000)
    assert near.tolist()[:5] == [1] * 5
    for i in (5, 6):
        t, a, b = rows[i]
        assert near[i] == 0 and pl[i].tolist() == [int(x) for x in M.likelihood([a, b], TYPES[t], 3, 5e-5)[1]]
