"""The genotype model at any ploidy P in 1..8, as the issue defines it: independent of the product (svjg.genotype.exact_pl_ploidy) and
of the kernel.  Decimal at precision 28, Python floats for the products and logarithms, the binomial term from tests/lik_model.

A row of SV type t with raw counts (ref, alt): normalised counts c1, c2 and their rounded images rc1, rc2 as the reference computes
them; for g = 0..P alt copies

    g == 0      lik = Decimal(c1 * log10(1 - e)) + Decimal(c2 * log10(e))
    g == P      lik = Decimal(c2 * log10(1 - e)) + Decimal(c1 * log10(e))
    2 g == P    lik = Decimal((c1 + c2) * log10(1 / 2))
    otherwise   lik = Decimal(c1 * Lr) + Decimal(c2 * La),  Lr = log10(((P - g) (1 - e) + g e) / P),  La = log10((g (1 - e) + (P - g) e) / P)

GT = the g that alone attains the maximum (None: a tie, or c1 + c2 below min_support); PL_g = int(-10 * (lik_g + Decimal(log10 comb(rc1 + rc2, rc1)))).
"""
import functools
import math
from decimal import Decimal, localcontext

import mpmath

from tests import lik_model

TYPES = ("DEL", "INS", "INV", "BND")
_log10_comb = functools.lru_cache(maxsize=None)(lik_model.log10_comb)      # (the model, the fractions and both test files ask for the same terms)


def normalised(svtype_code, ref, alt):
    c = [ref, alt]
    if TYPES[svtype_code] in ("DEL", "INS"):
        i = 0 if TYPES[svtype_code] == "DEL" else 1
        if c[i] > 0:
            c[i] = round(c[i] / 2, 1)
    return c[0], c[1], int(round(c[0], 0)), int(round(c[1], 0))


def log_pair(P, g, e):
    """(Lr, La, single): single = the likelihood is ONE product (c1 + c2) * Lr"""
    if g == 0:
        return math.log10(1 - e), math.log10(e), False
    if g == P:
        return math.log10(e), math.log10(1 - e), False
    if 2 * g == P:
        return math.log10(1 / 2), math.log10(1 / 2), True
    return math.log10(((P - g) * (1 - e) + g * e) / P), math.log10((g * (1 - e) + (P - g) * e) / P), False


def products(svtype_code, ref, alt, P, e):
    """per g: the tuple of double products whose exact sum is lik_g"""
    c1, c2, _, _ = normalised(svtype_code, ref, alt)
    out = []
    for g in range(P + 1):
        lr, la, single = log_pair(P, g, e)
        out.append(((c1 + c2) * lr,) if single else (c1 * lr, c2 * la))
    return out


def genotype(svtype_code, ref, alt, P, min_support, e):
    """-> (gt: alt copies or None, [PL_0 .. PL_P])"""
    assert 1 <= P <= 8
    c1, c2, rc1, rc2 = normalised(svtype_code, ref, alt)
    with localcontext() as ctx:
        ctx.prec = 28
        lik = [Decimal(t[0]) if len(t) == 1 else Decimal(t[0]) + Decimal(t[1]) for t in products(svtype_code, ref, alt, P, e)]      # (ONE rounded sum)
        top = max(lik)
        best = [g for g, x in enumerate(lik) if x == top]
        gt = best[0] if len(best) == 1 else None
        if not (c1 + c2 >= min_support):
            gt = None
        comb = Decimal(_log10_comb(rc1 + rc2, rc1))
        return gt, [int(-10 * (x + comb)) for x in lik]


def fused(svtype_code, ref, alt, P, min_support, e, order):
    """(gt, PLs) as geno_row_pairs would give them if the compiler fused one product of every pair into geno_lik's two_sum
    (tests/lik_model.py: FUSED_ORDERS[order]): the g whose value (hi + lo, the one product at 2 g = P) alone is largest; the double-double
    steps behind the sums are taken as exact, the sums are not rounded to 28 digits"""
    from fractions import Fraction
    two_sum = lik_model.FUSED_ORDERS[order]
    c1, c2, rc1, rc2 = normalised(svtype_code, ref, alt)
    lik = []
    for g in range(P + 1):
        lr, la, single = log_pair(P, g, e)
        if single:
            lik.append(Fraction((c1 + c2) * lr))
        else:
            hi, lo = two_sum(float(c1), lr, float(c2), la)
            lik.append(Fraction(hi) + Fraction(lo))
    top = max(lik)
    best = [g for g, x in enumerate(lik) if x == top]
    gt = best[0] if len(best) == 1 and c1 + c2 >= min_support else None
    comb = Fraction(_log10_comb(rc1 + rc2, rc1))
    return gt, [int(-10 * (x + comb)) for x in lik]


def pl_fractions(svtype_code, ref, alt, P, e):
    """(distance of each -10 * (lik_g + comb) from the nearest integer at 80 digits, log10 comb as a float)"""
    _, _, rc1, rc2 = normalised(svtype_code, ref, alt)
    with mpmath.workdps(lik_model.DPS):
        lc = _log10_comb(rc1 + rc2, rc1)
        comb = mpmath.mpf(lc)
        out = []
        for t in products(svtype_code, ref, alt, P, e):
            v = -10 * (sum((mpmath.mpf(x) for x in t), mpmath.mpf(0)) + comb)
            out.append(float(abs(v - mpmath.nint(v))))
        return out, lc


def check_against_model(rows, want, settings_of, gt, pl, flagged):
    """what the CPU and the GPU test ask of a result: GT equal on every row; PLs equal on every row that is not flagged, zeros beyond the
    ploidy; every row with a PL within 6e-7 of an integer (80 digits, binomial term non-zero) IS flagged; every flagged row has one within
    2e-6; flagged rows equal the model after exact_pl_ploidy.  -> number of flagged rows"""
    from svjg import genotype
    n_flagged = 0
    for r, (t, a, b, p) in enumerate(rows.tolist()):
        e, _ = settings_of(r)
        w_gt, w_pl = want[r]
        assert int(gt[r]) == (0xFF if w_gt is None else w_gt), (r, rows[r], gt[r], w_gt)
        assert not pl[r, p + 1:].any(), (r, rows[r], pl[r])
        fr, lc = pl_fractions(t, a, b, p, e)
        if lc != 0.0 and min(fr) < 6e-7:
            assert flagged[r], (r, rows[r], fr)
        if flagged[r]:
            n_flagged += 1
            assert min(fr) < 2e-6, (r, rows[r], fr)
            assert genotype.exact_pl_ploidy(t, a, b, p, e) == w_pl, (r, rows[r])
        else:
            assert pl[r, :p + 1].tolist() == w_pl, (r, rows[r], pl[r], w_pl)
    return n_flagged


def random_rows(n, seed=20240607):
    """the random set of the any-ploidy tests: (type, ref, alt, ploidy) int64[n, 4]; ploidy 1..8 mixed, all four types, counts 0..60 and a
    tenth of the rows up to 10^6"""
    import numpy as np
    rng = np.random.default_rng(seed)
    t = rng.integers(0, 4, n)
    p = rng.integers(1, 9, n)
    deep = rng.random(n) < 0.1
    hi = np.where(deep, 10**6, 60)
    ref = rng.integers(0, hi + 1)
    alt = rng.integers(0, hi + 1)
    return np.stack([t, ref, alt, p], axis=1).astype(np.int64)


SETTINGS = [(5e-5, 0), (5e-5, 3), (1e-2, 0), (1e-2, 3), (0.3, 0), (0.3, 3)]       # (err, min_support): row r of the random set runs under SETTINGS[r % 6]
