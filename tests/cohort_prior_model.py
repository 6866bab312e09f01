"""The model of the cohort call with an allele-frequency prior (svjg_genotype_cohort_prior), in Python's decimal at 60 digits
from the raw counts.  Shared by tests/test_cohort_prior.py (CPU), tests/test_cohort_prior_gpu.py and tests/golden/make_cohort_prior.py.

An item (r, s) takes part iff it was genotyped (done, ploidy P >= 1) and c1 + c2 > 0.  Its l_g, g = 0..P, are the EXACT sums of the two double
products, or the one product at 2 g = P, formed as svjg.genotype.exact_pl_ploidy forms them (the same doubles the device has, so both sides
share them exactly); d_g = l_g - max l_g, exact and then rounded to one double (the device subtracts in double-double and collapses);
w_g = 10^d_g.  Prior pi_g(f; P) = C(P, g) f^g (1 - f)^(P - g); posterior q_g = pi_g w_g / sum; x = sum g q_g; f_0 = 1/2, f_(k+1) = sum x /
sum P; stop after the first step with |f_(k+1) - f_k| <= EM_TOL, or after EM_MAX_IT steps (then: not converged).  Calls under the final f:
GT = argmax q_g, an exact tie at the maximum = no call, c1 + c2 < min_support = no call; GQ = min(99, int(-10 log10(sum of the other q_g))).
10^d, every product, sum and quotient and the stopping rule are evaluated at 60 digits."""
import math
from decimal import Decimal, localcontext
from fractions import Fraction

import numpy as np

PREC = 60
EM_TOL = Decimal("1e-9")
EM_MAX_IT = 128
NO_CALL = 0xFF
_COMB = [[math.comb(P, g) for g in range(P + 1)] for P in range(9)]


def norm_counts(svtype_code, ref, alt):
    """(c1, c2) as doubles: svjg.genotype._norm_counts (halves are exact)"""
    c1, c2 = float(ref), float(alt)
    if svtype_code == 0 and ref > 0:
        c1 = ref / 2
    if svtype_code == 1 and alt > 0:
        c2 = alt / 2
    return c1, c2


def log_pairs(P, err):
    """[(Lr, La)] for g = 0..P, the doubles of exact_pl_ploidy / ploidy_log_table; the middle genotype of an even ploidy: log10(1/2) twice"""
    out = []
    for g in range(P + 1):
        if g == 0:
            out.append((math.log10(1 - err), math.log10(err)))
        elif g == P:
            out.append((math.log10(err), math.log10(1 - err)))
        elif 2 * g == P:
            out.append((math.log10(1 / 2),) * 2)
        else:
            out.append((math.log10(((P - g) * (1 - err) + g * err) / P), math.log10((g * (1 - err) + (P - g) * err) / P)))
    return out


_W_CACHE = {}


def weights(c1, c2, P, err):
    """-> ([w_g as Decimal], the first g with the largest l_g); inside a 60-digit context"""
    key = (c1, c2, P, err)
    got = _W_CACHE.get(key)
    if got is None:
        ls = []
        for g, (lr, la) in enumerate(log_pairs(P, err)):
            if g != 0 and 2 * g == P:
                ls.append(Fraction((c1 + c2) * lr))              # ONE product
            else:
                ls.append(Fraction(c1 * lr) + Fraction(c2 * la))  # each product rounded to a double, the sum exact
        top = max(ls)
        ten = Decimal(10)
        got = ([ten ** Decimal(float(l - top)) for l in ls], ls.index(top))
        _W_CACHE[key] = got
    return got


def prior(f, P):
    """[pi_g(f; P)]: integer powers by repeated multiplication (0^0 = 1)"""
    q = 1 - f
    up, down = [Decimal(1)], [Decimal(1)]
    for _ in range(P):
        up.append(up[-1] * f)
        down.append(down[-1] * q)
    return [_COMB[P][g] * up[g] * down[P - g] for g in range(P + 1)]


def _expected(pi, w, gmax):
    t = [a * b for a, b in zip(pi, w)]
    z = sum(t)
    if z == 0:
        return Decimal(gmax)
    return sum(g * v for g, v in enumerate(t)) / z


def row_em(items):
    """items: [(P, [w_g], gmax)] of the row's items that take part -> (f or None, steps, not_converged, ratio): ratio = |f_(k+1) - f_k| /
    EM_TOL of the deciding step — the last one, or an earlier one if that came closer to 1 (a device that differs there stops elsewhere)"""
    if not items:
        return None, 0, False, None
    sum_p = sum(P for P, _, _ in items)
    ploidies = sorted({P for P, _, _ in items})
    f, ratio, steps, conv = Decimal("0.5"), None, 0, False
    while steps < EM_MAX_IT and not conv:
        pis = {P: prior(f, P) for P in ploidies}
        fn = sum(_expected(pis[P], w, gmax) for P, w, gmax in items) / sum_p
        r = abs(fn - f) / EM_TOL
        if ratio is None or abs(r - 1) < abs(ratio - 1):
            ratio = r
        f, steps, conv = fn, steps + 1, r <= 1
    return f, steps, not conv, ratio


def call(f, P, w, gmax):
    """-> (GT, GQ, distance of -10 log10(rest) from an integer (1: beyond 99.5, nothing to decide), relative gap of the two largest q); GT =
    NO_CALL, GQ = NO_CALL for an exact tie at the maximum"""
    t = [a * b for a, b in zip(prior(f, P), w)]
    z = sum(t)
    q = [v / z for v in t] if z != 0 else [Decimal(int(g == gmax)) for g in range(P + 1)]
    top = max(q)
    best = q.index(top)
    second = max(v for g, v in enumerate(q) if g != best)
    gap = (top - second) / top
    rest = sum(v for g, v in enumerate(q) if g != best)
    if rest < Decimal("1e-10"):
        gq, margin = 99, Decimal(1)
    else:
        v = -10 * rest.log10()
        gq = min(99, int(v))
        margin = abs(v - v.to_integral_value()) if v < Decimal("99.5") else Decimal(1)
    if second == top:
        return NO_CALL, NO_CALL, margin, gap
    return best, gq, margin, gap


def run(sv_type, raw, done, ploidy, err, min_support, rows=None):
    """sv_type[R]; raw[R, S, 2], done[R, S] as the cohort call returns them; ploidy[R, S] or None (2 everywhere).  rows: only these (None:
    all).  -> dict: f (Decimal or None per row), f_hi / f_lo (float64: f = f_hi + f_lo to ~32 digits, NaN / 0 without an estimate), steps,
    flag, ratio (float64, NaN without an estimate), gt, gq (uint8[R, S], NO_CALL: none), gq_margin, gap (float64[R, S], NaN where the item
    takes no part)"""
    raw, done = np.asarray(raw), np.asarray(done)
    R, S = done.shape
    out = {"f": [None] * R, "f_hi": np.full(R, np.nan), "f_lo": np.zeros(R), "steps": np.zeros(R, np.uint32), "flag": np.zeros(R, bool),
           "ratio": np.full(R, np.nan), "gt": np.full((R, S), NO_CALL, np.uint8), "gq": np.full((R, S), NO_CALL, np.uint8),
           "gq_margin": np.full((R, S), np.nan), "gap": np.full((R, S), np.nan)}
    with localcontext() as ctx:
        ctx.prec = PREC
        for r in (range(R) if rows is None else rows):
            t = int(sv_type[r])
            items = []
            for s in range(S):
                P = (2 if ploidy is None else int(ploidy[r, s])) if done[r, s] else 0
                if P == 0:
                    continue
                c1, c2 = norm_counts(t, int(raw[r, s, 0]), int(raw[r, s, 1]))
                if c1 + c2 > 0:
                    items.append((s, c1 + c2, P) + weights(c1, c2, P, err))
            f, steps, flag, ratio = row_em([it[2:] for it in items])
            out["steps"][r], out["flag"][r] = steps, flag
            if f is None:
                continue
            out["f"][r], out["f_hi"][r], out["ratio"][r] = f, float(f), float(ratio)
            out["f_lo"][r] = float(f - Decimal(float(f)))
            for s, c_sum, P, w, gmax in items:
                gt, gq, margin, gap = call(f, P, w, gmax)
                out["gq_margin"][r, s], out["gap"][r, s] = float(margin), float(gap)
                if c_sum >= min_support:
                    out["gt"][r, s], out["gq"][r, s] = gt, gq
    return out


def site_of(gt, ploidy):
    """NS, AN, AC of every row from its posterior calls (ploidy None: 2 everywhere)"""
    gt = np.asarray(gt)
    called = gt != NO_CALL
    P = np.full(gt.shape, 2, np.int64) if ploidy is None else np.asarray(ploidy, np.int64)
    return np.stack([called.sum(axis=1), np.where(called, P, 0).sum(axis=1), np.where(called, gt, 0).sum(axis=1, dtype=np.int64)], axis=1).astype(np.uint32)
