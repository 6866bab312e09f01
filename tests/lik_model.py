"""A high-precision model of the reference's likelihood() (predict-genotype.py:281-325), for counts the reference cannot finish.

The reference's arithmetic line for line — the allele normalisation round(x / 2, 1), int(round(c, 0)), double products, Decimal at
precision 28, truncation — with one change: math.log10(math.comb(n, k)) is not computed from the big integer.  The model emulates
CPython's loghelper (mathmodule.c) on ln comb(n, k) known to 80 digits (mpmath):

  - comb < 2^1024 after rounding to a double: log10 of comb correctly rounded to a double (what PyLong_AsDouble returns);
  - otherwise: x = comb / 2^e, e = bit length, x rounded half to even to 53 bits (a carry gives (0.5, e + 1), as _PyLong_Frexp
    does) -> math.log10(x) + math.log10(2.0) * e in Python floats.

Where the 80-digit value lies within 1e-40 of a rounding point the model raises (Undecided) instead of guessing.
Test infrastructure only: the product's own recomputation is svjg.genotype.exact_pl (stdlib decimal, no mpmath).
"""
import math
from decimal import Decimal, localcontext

import mpmath

DPS = 80
TOL = mpmath.mpf("1e-40")
_GT = ("0/0", "0/1", "1/1")


class Undecided(Exception):
    """the 80-digit value cannot decide a rounding"""


def _round53(m, tol=TOL):
    """m in [2^52, 2^53] (an mpf or an int) -> the integer nearest to m, ties to even; raises where m is within tol of a tie"""
    if isinstance(m, int):
        return m
    mi = int(mpmath.floor(m))
    fr = m - mi
    if abs(fr - mpmath.mpf("0.5")) < tol:
        raise Undecided(str(m))
    return mi + 1 if fr > 0.5 else mi


def loghelper(mant, e):
    """CPython's math.log10 of an int N = mant * 2^(e - 53), 2^52 <= mant < 2^53 (mant: an exact int, or an mpf close to one)"""
    mi = _round53(mant)
    if mi == 1 << 53:                                    # the rounding carried
        mi, e = 1 << 52, e + 1
    if e <= 1024:                                        # PyLong_AsDouble: the int rounded to a double
        return math.log10(math.ldexp(float(mi), e - 53))
    return math.log10(math.ldexp(float(mi), -53)) + math.log10(2.0) * e      # _PyLong_Frexp: (x, e)


def log10_int(c):
    """math.log10(c) of a positive int c, through the emulation with c known exactly (checks the emulation itself)"""
    e = c.bit_length()
    if e <= 53:
        return loghelper(c << (53 - e), e)
    sh = e - 53
    top, rest = c >> sh, c & ((1 << sh) - 1)
    half = 1 << (sh - 1)
    mi = top + (1 if rest > half or (rest == half and top & 1) else 0)
    return loghelper(mi, e)


def log10_of_ln(lnc):
    """math.log10(C) of the int C whose natural log is lnc (an mpf of DPS digits)"""
    with mpmath.workdps(DPS):
        t = lnc / mpmath.log(2)
        fl = mpmath.floor(t)
        if t - fl < TOL or fl + 1 - t < TOL:
            raise Undecided("bit length")
        e = int(fl) + 1
        return loghelper(mpmath.exp(lnc - (e - 53) * mpmath.log(2)), e)


def log10_comb(n, k):
    """math.log10(math.comb(n, k)) without the big integer"""
    if k < 0 or k > n:
        raise ValueError
    if min(k, n - k) <= 64:                              # the integer is cheap: the emulation on the exact value
        return log10_int(math.comb(n, k))
    with mpmath.workdps(DPS):
        lnc = mpmath.loggamma(n + 1) - mpmath.loggamma(k + 1) - mpmath.loggamma(n - k + 1)
        return log10_of_ln(lnc)


def likelihood(all_count, svtype, min_support, e):
    """predict-genotype.py likelihood() -> (GT text, [PL0, PL1, PL2] as str); all_count is normalised in place like the reference"""
    with localcontext() as ctx:
        ctx.prec = 28
        if svtype in ("DEL", "INS"):
            i = 0 if svtype == "DEL" else 1
            if all_count[i] > 0:
                all_count[i] = round(all_count[i] / 2, 1)
        c1, c2 = all_count
        rc1 = int(round(c1, 0))
        rc2 = int(round(c2, 0))
        lik0 = Decimal(c1 * math.log10(1 - e)) + Decimal(c2 * math.log10(e))
        lik1 = Decimal((c1 + c2) * math.log10(1 / 2))
        lik2 = Decimal(c2 * math.log10(1 - e)) + Decimal(c1 * math.log10(e))
        L = [lik0, lik1, lik2]
        best = [i for i, x in enumerate(L) if x == max(L)]
        geno = _GT[best[0]] if len(best) == 1 else "./."
        if not sum(all_count) >= min_support:
            geno = "./."
        combination = Decimal(log10_comb(rc1 + rc2, rc1))
        prob = [str(int(-10 * (x + combination))) for x in L]
        return geno, prob


def fused_two_sum(x1, y1, x2, y2):
    """What k_genotype's device code computed for two_sum(x1 * y1, x2 * y2) while geno_row was compiled with fused multiply-adds (before
    it carried `fp contract(off)`): only the SECOND product is rounded to a double, the first one enters every operation exactly.
    The five instructions in Fraction, float() for each rounding, then the add of the two tail halves -> (hi, lo).  Used by the
    generators of lik_products.npz (tests/golden/make_golden.py) and site_products.npz (tests/golden/make_site_products.py) to find items on
    which that differs from the plain C++, and by the CPU tests that count such items in every set the device tests run
    (tests/products_items.py: sensitive_*)."""
    from fractions import Fraction
    p1 = Fraction(x1) * Fraction(y1)
    p2 = Fraction(x2) * Fraction(y2)
    b = float(p2)                                        # v_mul_f64   b  = fl(x2 * y2)
    s = float(p1 + Fraction(b))                          # v_fmac_f64  s  = fl(x1 * y1 + b)
    bb = float(Fraction(s) - p1)                         # v_fma_f64   bb = fl(s - x1 * y1)
    t2 = float(p2 - Fraction(bb))                        # v_fma_f64   fl(x2 * y2 - bb)
    t1 = float(p1 - Fraction(s - bb))                    # v_fma_f64   fl(x1 * y1 - fl(s - bb))
    return s, t1 + t2


def fused_two_sum_second(x1, y1, x2, y2):
    """The other order a compiler that fuses wherever it can may choose for two_sum(x1 * y1, x2 * y2): in s = a + b the SECOND product is the
    one multiplied inside the instruction and the first its rounded addend; every other operation reads its product exactly, as in
    fused_two_sum (there s is fl(x1 * y1 + fl(x2 * y2)), and the other four lines are the same).  -> (hi, lo)"""
    from fractions import Fraction
    p1 = Fraction(x1) * Fraction(y1)
    p2 = Fraction(x2) * Fraction(y2)
    a = float(p1)                                        # v_mul_f64   a  = fl(x1 * y1)
    s = float(Fraction(a) + p2)                          # v_fmac_f64  s  = fl(a + x2 * y2)
    bb = float(Fraction(s) - p1)                         # v_fma_f64   bb = fl(s - x1 * y1)
    t2 = float(p2 - Fraction(bb))                        # v_fma_f64   fl(x2 * y2 - bb)
    t1 = float(p1 - Fraction(s - bb))                    # v_fma_f64   fl(x1 * y1 - fl(s - bb))
    return s, t1 + t2


FUSED_ORDERS = {"first": fused_two_sum, "second": fused_two_sum_second}      # the product that is multiplied inside s = a + b


def pl_fractions(svtype_code, ref, alt, e):
    """distance of each -10 * (lik + comb) from the nearest integer, at 80 digits (for the boundary searches)"""
    types = ("DEL", "INS", "INV", "BND")
    c = [ref, alt]
    if types[svtype_code] == "DEL" and ref > 0:
        c[0] = round(ref / 2, 1)
    if types[svtype_code] == "INS" and alt > 0:
        c[1] = round(alt / 2, 1)
    c1, c2 = c
    r1, r2 = int(round(c1, 0)), int(round(c2, 0))
    with mpmath.workdps(DPS):
        comb = mpmath.mpf(log10_comb(r1 + r2, r1))
        mp = mpmath.mpf
        liks = (mp(c1 * math.log10(1 - e)) + mp(c2 * math.log10(e)), mp((c1 + c2) * math.log10(1 / 2)),
                mp(c2 * math.log10(1 - e)) + mp(c1 * math.log10(e)))
        out = []
        for x in liks:
            v = -10 * (x + comb)
            out.append(float(abs(v - mpmath.nint(v))))
        return out
