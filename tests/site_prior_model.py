"""The model of the cohort site call with an allele-frequency prior (svjg_genotype_cohort_sites_prior), in Python's decimal at 60
digits (as tests/cohort_prior_model.py), written from the issue's statement and independent of svjg_geno.h.  Shared by
tests/test_cohort_site_prior.py, tests/test_cohort_site_prior_gpu.py and tests/golden/make_cohort_site_prior.py.

A site has C candidates; allele 0 is the reference, allele j candidate j.  Item (k, s) takes part iff K' >= 2 candidates are present for s and it
has a read.  From what the first kernel leaves (raw = the ref maximum and the members' alt counts, members = the presence bits): c_0 = ref,
c_j = alt_j / 2, N their sum; l_AB over the genotypes on {0} + members is the EXACT sum of the two double products (own * L, rest * L_x with that
K''s logarithms, the same doubles the device has); d = l - max l, exact and then rounded to one double; w = 10^d, NOT flushed to zero however small
(the exponent range is widened: a weight the device's doubles lose is below 1e-308 of the largest and moves nothing that is compared).  Prior
pi_AB = p_A^2 or 2 p_A p_B, posterior over the item's own genotypes, x_j = sum copies_j q; p_j <- sum x_j / (2 n) from p_j = 1 / (C + 1); stop
after the first step with max_j |p_j' - p_j| <= EM_TOL or after EM_MAX_IT steps.  Calls under the final p: argmax q, a tie = no call, N <
min_support = no call; SGQ = min(99, int(-10 log10(sum of the other q))).

The margins are the model's own: a site whose deciding step lies within RATIO_BAND of EM_TOL is `site_out` (a device that differs there stops
elsewhere); an item whose two largest posteriors lie within TOP_GAP (relative) or whose -10 log10 lies within GQ_MARGIN of an integer is
undecided (`item_out`)."""
import math
from decimal import Decimal, localcontext
from fractions import Fraction

import numpy as np

PREC = 60
EM_TOL = Decimal("1e-9")
EM_MAX_IT = 128
NO_CALL = 0xFF
MAX_ALTS, ALLELES, NPL = 6, 7, 28
RATIO_BAND, GQ_MARGIN, TOP_GAP, CAP = 1e-6, 1e-6, 1e-9, 0.01


def site_logs(err, K):
    """(L_ok, L_x, L_he) of a site of K members, as svjg.genotype forms them with math.log10"""
    x, ok = err / K, 1.0 - err
    return math.log10(ok), math.log10(x), math.log10((ok + x) / 2.0)


_W_CACHE = {}


def candidates_of(members):
    return [j + 1 for j in range(MAX_ALTS) if (members >> j) & 1]


def weights(raw, members, err):
    """-> None (the item takes no part) or (N, [(A, B)] in increasing slot order, [w as Decimal], index of the first largest l); inside a 60-digit context"""
    cand = candidates_of(members)
    K = len(cand)
    key = (tuple(int(v) for v in raw[:K + 1]), members, err)
    if key in _W_CACHE:
        return _W_CACHE[key]
    got = None
    if K >= 2:
        c = {0: float(raw[0])}
        for t, j in enumerate(cand):
            c[j] = int(raw[1 + t]) / 2
        N = sum(c.values())
        if N > 0:
            l_ok, l_x, l_he = site_logs(err, K)
            alleles = [0] + cand
            pairs = sorted(((a, b) for i, a in enumerate(alleles) for b in alleles[i:]), key=lambda ab: ab[1] * (ab[1] + 1) // 2 + ab[0])
            ls = []
            for a, b in pairs:
                own = c[a] if a == b else c[a] + c[b]
                rest = N - c[a] if a == b else N - c[a] - c[b]
                ls.append(Fraction(own * (l_ok if a == b else l_he)) + Fraction(rest * l_x))
            top = max(ls)
            ten = Decimal(10)
            got = (N, pairs, [ten ** Decimal(float(l - top)) for l in ls], ls.index(top))
    _W_CACHE[key] = got
    return got


def _terms(p, pairs, w):
    return [(p[a] * p[a] if a == b else 2 * p[a] * p[b]) * v for (a, b), v in zip(pairs, w)]


def site_em(C, items):
    """items: [(N, pairs, w, top)] of the site's items that take part -> (p[7] or None, steps, not_converged, ratio of the deciding step)"""
    if not items:
        return None, 0, False, None
    n = len(items)
    p = [Decimal(1) / (C + 1) if j <= C else Decimal(0) for j in range(ALLELES)]
    ratio, steps, conv = None, 0, False
    while steps < EM_MAX_IT and not conv:
        x = [Decimal(0)] * ALLELES
        for _, pairs, w, top in items:
            t = _terms(p, pairs, w)
            z = sum(t)
            if z == 0:
                t = [Decimal(int(i == top)) for i in range(len(pairs))]
                z = Decimal(1)
            for (a, b), v in zip(pairs, t):
                x[a] += v / z
                x[b] += v / z
        pn = [v / (2 * n) for v in x]
        r = max(abs(a - b) for a, b in zip(pn, p)) / EM_TOL
        if ratio is None or abs(r - 1) < abs(ratio - 1):
            ratio = r
        p, steps, conv = pn, steps + 1, r <= 1
    return p, steps, not conv, ratio


def call(p, members, pairs, w, top):
    """-> ((a, b) in the item's member numbering or (NO_CALL, NO_CALL), SGQ, distance of -10 log10(rest) from an integer (1: nothing to decide),
    relative gap of the two largest q)"""
    t = _terms(p, pairs, w)
    z = sum(t)
    q = [v / z for v in t] if z != 0 else [Decimal(int(i == top)) for i in range(len(pairs))]
    hi = max(q)
    best = q.index(hi)
    second = max(v for i, v in enumerate(q) if i != best)
    gap = (hi - second) / hi
    rest = sum(v for i, v in enumerate(q) if i != best)
    if rest < Decimal("1e-10"):
        gq, margin = 99, Decimal(1)
    else:
        v = -10 * rest.log10()
        gq = min(99, int(v))
        margin = abs(v - v.to_integral_value()) if v < Decimal("99.5") else Decimal(1)
    if second == hi:
        return (NO_CALL, NO_CALL), NO_CALL, margin, gap
    number = {0: 0}
    number.update({j: t + 1 for t, j in enumerate(candidates_of(members))})
    a, b = pairs[best]
    return (number[a], number[b]), gq, margin, gap


def run(raw, members, C, err, min_support, sites=None):
    """raw[n, S, 7], members[n, S] as svjg_genotype_cohort_sites returns them, C[n] -> dict: p (7 Decimals or None per site), p_hi / p_lo
    (float64[n, 7]: p = hi + lo to ~32 digits; NaN / 0 without an estimate), steps, flag, ratio (NaN without an estimate), sgt uint8[n, S, 2],
    sgq uint8[n, S] (NO_CALL: none), gq_margin, gap (NaN where the item takes no part).  sites: only these (None: all)"""
    raw, members = np.asarray(raw), np.asarray(members)
    n, S = members.shape
    out = {"p": [None] * n, "p_hi": np.full((n, ALLELES), np.nan), "p_lo": np.zeros((n, ALLELES)), "steps": np.zeros(n, np.uint32), "flag": np.zeros(n, bool),
           "ratio": np.full(n, np.nan), "sgt": np.full((n, S, 2), NO_CALL, np.uint8), "sgq": np.full((n, S), NO_CALL, np.uint8),
           "gq_margin": np.full((n, S), np.nan), "gap": np.full((n, S), np.nan)}
    with localcontext() as ctx:
        ctx.prec = PREC
        ctx.Emin, ctx.Emax = -10 ** 12, 10 ** 12                  # no weight is flushed to zero
        for k in (range(n) if sites is None else sites):
            items = []
            for s in range(S):
                got = weights(raw[k, s], int(members[k, s]), err)
                if got is not None:
                    items.append((s,) + got)
            p, steps, flag, ratio = site_em(int(C[k]), [it[1:] for it in items])
            out["steps"][k], out["flag"][k] = steps, flag
            if p is None:
                continue
            out["p"][k], out["ratio"][k] = p, float(ratio)
            for j in range(ALLELES):
                out["p_hi"][k, j] = float(p[j])
                out["p_lo"][k, j] = float(p[j] - Decimal(float(p[j])))
            for s, N, pairs, w, top in items:
                gt, gq, margin, gap = call(p, int(members[k, s]), pairs, w, top)
                out["gq_margin"][k, s], out["gap"][k, s] = float(margin), float(gap)
                if N >= min_support:
                    out["sgt"][k, s], out["sgq"][k, s] = gt, gq
    return out


def outside(res):
    """-> (site_out[n], item_out[n, S]): what the margins leave undecided; the items of a site that is out are all out"""
    site_out = np.abs(res["ratio"] - 1) < RATIO_BAND
    item_out = (res["gq_margin"] < GQ_MARGIN) | (res["gap"] < TOP_GAP) | site_out[:, None]
    return site_out, item_out


def psite_of(sgt, members):
    """NS_j, AC_j of every site from its calls in member numbering: uint32[n, 6, 2]"""
    sgt, members = np.asarray(sgt), np.asarray(members)
    n, S = members.shape
    out = np.zeros((n, MAX_ALTS, 2), np.uint32)
    called = sgt[:, :, 0] != NO_CALL
    for j in range(MAX_ALTS):
        member = ((members >> j) & 1).astype(bool) & called
        number = 1 + np.bitwise_count(members & ((1 << j) - 1)).astype(np.int64) if hasattr(np, "bitwise_count") else \
            1 + np.array([[bin(int(m) & ((1 << j) - 1)).count("1") for m in row] for row in members], np.int64).reshape(n, S)
        copies = (sgt[:, :, 0] == number).astype(np.int64) + (sgt[:, :, 1] == number)
        out[:, j, 0] = member.sum(axis=1)
        out[:, j, 1] = np.where(member, copies, 0).sum(axis=1)
    return out
