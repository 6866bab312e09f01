"""The model of the cohort site quality (svjg_cohort_qual, DESIGN.md 4.3 "Site quality"), in Python's decimal at 60 digits from the raw counts.
Shared by tests/test_cohort_qual.py (CPU), tests/test_cohort_qual_gpu.py and tests/golden/make_cohort_qual.py.

An item (r, s) takes part iff the gate passed it (done, ploidy P >= 1) and c1 + c2 > 0.  Its coefficients a_g = C(P, g) w_g, w_g = 10^d_g as
tests/cohort_prior_model.weights gives them (d_g = l_g - max l, exact and then rounded to one double, as the device collapses it); beside them
d_0 = l_0 - max l EXACT.  y_0 = 1 at M' = 0; per item, with M = M' + P:
    y_k <- sum_(g = 0..min(P, k), k - g <= M') a_g y_(k-g) (k)_g (M - k)_(P-g) / (M)_P,   k = 0..M
(falling factorials as exact integers).  No rescaling: a Decimal's exponent has room.  Prior phi_k = theta / k, phi_0 = 1 - theta H_M with H_M the
DOUBLE that summing 1 / k in increasing k gives (the model's text says so; theta is the double the caller passes).  chroms = M; mlac = the
smallest k at max phi_k y_k; qual = max(0, -10 (log10 phi_0 + D_0 - log10 T)), T = sum_k phi_k y_k, D_0 = sum_s d_(s,0)."""
import math
from decimal import Decimal, localcontext
from fractions import Fraction

import numpy as np

from tests import cohort_prior_model as PM

PREC = 60
THETA = 1e-3
_COMB = [[math.comb(P, g) for g in range(P + 1)] for P in range(9)]
_D0_CACHE = {}


def d0_exact(c1, c2, P, err):
    """l_0 - max_g l_g as a Fraction (the l_g as cohort_prior_model.weights forms them)"""
    key = (c1, c2, P, err)
    got = _D0_CACHE.get(key)
    if got is None:
        ls = []
        for g, (lr, la) in enumerate(PM.log_pairs(P, err)):
            ls.append(Fraction((c1 + c2) * lr) if g != 0 and 2 * g == P else Fraction(c1 * lr) + Fraction(c2 * la))
        got = _D0_CACHE[key] = ls[0] - max(ls)
    return got


def row_items(t, raw, done, ploidy, err):
    """the items of one row that take part, in sample order: [(P, [a_g as Decimal], d_0 as Fraction)]; raw[S, 2], done[S], ploidy[S] or None.
    Inside a 60-digit context"""
    out = []
    for s in range(len(done)):
        P = (2 if ploidy is None else int(ploidy[s])) if done[s] else 0
        if P == 0:
            continue
        c1, c2 = PM.norm_counts(t, int(raw[s, 0]), int(raw[s, 1]))
        if c1 + c2 > 0:
            w, _ = PM.weights(c1, c2, P, err)
            out.append((P, [_COMB[P][g] * w[g] for g in range(P + 1)], d0_exact(c1, c2, P, err)))
    return out


def falling(x, n):
    out = 1
    for i in range(n):
        out *= x - i
    return out


def fold(y, P, a):
    """one step of the recurrence: y of M' = len(y) - 1 chromosomes -> y of M' + P"""
    M0 = len(y) - 1
    M = M0 + P
    den = falling(M, P)
    out = []
    for k in range(M + 1):
        up, dn = [1], [1]                                        # (k)_g and (M - k)_j for g, j = 0..P
        for i in range(P):
            up.append(up[-1] * (k - i))
            dn.append(dn[-1] * (M - k - i))
        acc = 0
        for g in range(max(0, k - M0), min(P, k) + 1):
            acc += a[g] * y[k - g] * (up[g] * dn[P - g])
        out.append(acc / den)
    return out


def recurrence(items):
    """-> y_0..y_M (Decimal) over the items in order"""
    y = [Decimal(1)]
    for P, a, _ in items:
        y = fold(y, P, a)
    return y


def harmonic(M):
    """H_M as the double the device's table holds"""
    h = 0.0
    for k in range(1, M + 1):
        h = h + 1.0 / k
    return h


def prior(theta, M):
    """[phi_0..phi_M] as Decimals"""
    th = Decimal(float(theta))
    return [1 - th * Decimal(harmonic(M))] + [th / k for k in range(1, M + 1)]


def posterior_terms(items, theta):
    """-> [phi_k y_k]"""
    y = recurrence(items)
    return [p * v for p, v in zip(prior(theta, len(y) - 1), y)]


def row(items, theta):
    """-> (chroms, mlac, qual as Decimal or None, relative gap of the two largest phi_k y_k or None)"""
    if not items:
        return 0, 0, None, None
    t = posterior_terms(items, theta)
    M = len(t) - 1
    top = max(t)
    mlac = t.index(top)
    second = max(v for k, v in enumerate(t) if k != mlac)
    D0 = sum((d for _, _, d in items), Fraction(0))
    phi0 = prior(theta, M)[0]
    q = -10 * (phi0.log10() + Decimal(D0.numerator) / Decimal(D0.denominator) - sum(t).log10())
    return M, mlac, q if q > 0 else Decimal(0), (top - second) / top


def run(sv_type, raw, done, ploidy, err, theta=THETA, rows=None):
    """sv_type[R]; raw[R, S, 2], done[R, S] as the gate leaves them; ploidy[R, S] or None (2 everywhere).  rows: only these (None: all).
    -> dict: chroms, mlac (uint32[R]), qual (float64[R]: the model's value rounded; NaN: no item took part), qual_lo (the rest, float64), gap
    (float64[R], NaN without an item), half (|100 qual - nearest half-integer|, NaN without an item)"""
    raw, done = np.asarray(raw), np.asarray(done)
    R = done.shape[0]
    out = {"chroms": np.zeros(R, np.uint32), "mlac": np.zeros(R, np.uint32), "qual": np.full(R, np.nan), "qual_lo": np.zeros(R),
           "gap": np.full(R, np.nan), "half": np.full(R, np.nan)}
    with localcontext() as ctx:
        ctx.prec = PREC
        for r in (range(R) if rows is None else rows):
            items = row_items(int(sv_type[r]), raw[r], done[r], None if ploidy is None else ploidy[r], err)
            M, mlac, q, gap = row(items, theta)
            out["chroms"][r], out["mlac"][r] = M, mlac
            if q is not None:
                out["qual"][r], out["gap"][r] = float(q), float(gap)
                out["qual_lo"][r] = float(q - Decimal(float(q)))
                x = q * 100 - Decimal("0.5")
                out["half"][r] = float(abs(x - x.to_integral_value()))
    return out
