"""The joint model for insertions that share a position, as the issue defines it: independent of the product (svjg.genotype.exact_pl_site) and of
the kernel.  Decimal at precision 28, Python floats for the products and logarithms, the chain's binomial terms from tests/lik_model.

A site has K insertions; allele 0 is the reference, allele j the j-th insertion.  c_0 = ref (the members' largest raw ref count),
c_j = round(alt_j / 2, 1) if alt_j > 0 else 0, r_j = int(round(c_j, 0)), N = sum c_j.  For the genotypes {a, b}, 0 <= a <= b <= K, in VCF order
b (b + 1) / 2 + a:

    a == b   lik = Decimal(c_a * L_ok) + Decimal((N - c_a) * L_x)                     L_ok = log10(1 - e), L_x = log10(e / K)
    a <  b   lik = Decimal((c_a + c_b) * L_he) + Decimal((N - c_a - c_b) * L_x)       L_he = log10(((1 - e) + e / K) / 2); at K = 1: log10(1 / 2)

s_0 = r_0, s_j = s_(j-1) + r_j, T = sum over j = 1..K of Decimal(log10 comb(s_j, r_j)); PL_ab = int(-10 * (lik_ab + T)).  The call is the genotype
that alone attains the maximum (None: a tie, or not N >= min_support).
"""
import functools
import math
from decimal import Decimal, localcontext

import mpmath

from tests import lik_model

SITE_PL_GUARD = 2.5e-6                       # svjg_geno.h
NO_CALL = 0xFF
_log10_comb = functools.lru_cache(maxsize=None)(lik_model.log10_comb)


def genotypes(K):
    return [(a, b) for b in range(K + 1) for a in range(b + 1)]


def counts(ref, alts):
    c = [ref] + [round(x / 2, 1) if x > 0 else 0 for x in alts]
    return c, [int(round(x, 0)) for x in c]


def logs(K, e):
    l_he = math.log10(1 / 2) if K == 1 else math.log10(((1 - e) + e / K) / 2)
    return math.log10(1 - e), math.log10(e / K), l_he


def products(ref, alts, e):
    """per genotype: the two double products whose exact sum is its lik"""
    K = len(alts)
    c, _ = counts(ref, alts)
    N = sum(c)
    l_ok, l_x, l_he = logs(K, e)
    out = []
    for a, b in genotypes(K):
        if a == b:
            out.append((c[a] * l_ok, (N - c[a]) * l_x))
        else:
            out.append(((c[a] + c[b]) * l_he, (N - c[a] - c[b]) * l_x))
    return out


def chain(ref, alts):
    """the K doubles log10 comb(s_j, r_j)"""
    _, r = counts(ref, alts)
    s, out = r[0], []
    for x in r[1:]:
        s += x
        out.append(_log10_comb(s, x))
    return out


def genotype(ref, alts, min_support, e):
    """-> (the pair (a, b) or None, the (K + 1)(K + 2) / 2 PLs in VCF order)"""
    K = len(alts)
    assert 1 <= K <= 6
    c, _ = counts(ref, alts)
    with localcontext() as ctx:
        ctx.prec = 28
        lik = [Decimal(p) + Decimal(q) for p, q in products(ref, alts, e)]
        top = max(lik)
        best = [g for g, x in zip(genotypes(K), lik) if x == top]
        call = best[0] if len(best) == 1 else None
        if not (sum(c) >= min_support):
            call = None
        T = Decimal(0)
        for t in chain(ref, alts):
            T += Decimal(t)
        return call, [int(-10 * (x + T)) for x in lik]


def factors(ref, alts, e):
    """per genotype: (own, L_own, rest, L_x), the factors of products()' two doubles"""
    K = len(alts)
    c, _ = counts(ref, alts)
    N = sum(c)
    l_ok, l_x, l_he = logs(K, e)
    return [(c[a], l_ok, N - c[a], l_x) if a == b else (c[a] + c[b], l_he, N - c[a] - c[b], l_x) for a, b in genotypes(K)]


def fused_pls(ref, alts, e, order):
    """the PLs geno_site would give for a site whose chain term T is 0 if the compiler fused one product of every pair into two_sum
    (tests/lik_model.py: FUSED_ORDERS[order]); the double-double steps behind the sum are taken as exact"""
    from fractions import Fraction
    assert not any(chain(ref, alts))
    fused = lik_model.FUSED_ORDERS[order]
    out = []
    for own, l_own, rest, l_x in factors(ref, alts, e):
        hi, lo = fused(float(own), l_own, float(rest), l_x)
        out.append(int(-10 * (Fraction(hi) + Fraction(lo))))
    return out


def pl_fractions(ref, alts, e):
    """(distance of each -10 * (lik + T) from the nearest integer at 80 digits, whether T is non-zero)"""
    with mpmath.workdps(lik_model.DPS):
        terms = chain(ref, alts)
        T = sum((mpmath.mpf(t) for t in terms), mpmath.mpf(0))
        out = []
        for p, q in products(ref, alts, e):
            v = -10 * (mpmath.mpf(p) + mpmath.mpf(q) + T)
            out.append(float(abs(v - mpmath.nint(v))))
        return out, any(t != 0.0 for t in terms)


def project(K, i, call, pls):
    """member i of a site called `call` -> (its copies 0..2 or None, [PL_0, PL_1, PL_2]: the smallest site PL over the genotypes with that many
    copies of allele i)"""
    g = None if call is None else (call[0] == i) + (call[1] == i)
    by = [[], [], []]
    for (a, b), v in zip(genotypes(K), pls):
        by[(a == i) + (b == i)].append(v)
    return g, [min(x) for x in by]


def random_sites(n, seed=20241018):
    """the random set of the joint-insertion tests: [(ref, [alt_1 .. alt_K])]; K mixed over 2..6, raw counts 0..60, a tenth of the sites up to
    20 000"""
    import numpy as np
    rng = np.random.default_rng(seed)
    K = rng.integers(2, 7, n)
    deep = rng.random(n) < 0.1
    out = []
    for k, d in zip(K.tolist(), deep.tolist()):
        v = rng.integers(0, (20_000 if d else 60) + 1, k + 1).tolist()
        out.append((v[0], v[1:]))
    return out


def check_against_model(sites, want, settings_of, gt, pl, flagged):
    """what the CPU and the GPU test ask of a result: the GT pair equal on every site; PLs equal on every site that is not flagged, zeros beyond
    the site's genotypes; every site with a PL within 0.6 x SITE_PL_GUARD of an integer (80 digits, T non-zero) IS flagged; every flagged site has
    one within 2 x SITE_PL_GUARD; flagged sites equal the model after exact_pl_site.  -> number of flagged sites"""
    from svjg import genotype as product
    n_flagged = 0
    for s, (ref, alts) in enumerate(sites):
        e, _ = settings_of(s)
        w_call, w_pl = want[s]
        G = len(w_pl)
        assert (int(gt[s, 0]), int(gt[s, 1])) == ((NO_CALL, NO_CALL) if w_call is None else w_call), (s, sites[s], gt[s], w_call)
        assert not pl[s, G:].any(), (s, sites[s], pl[s])
        fr, nonzero = pl_fractions(ref, alts, e)
        if nonzero and min(fr) < 0.6 * SITE_PL_GUARD:
            assert flagged[s], (s, sites[s], fr)
        if flagged[s]:
            n_flagged += 1
            assert min(fr) < 2 * SITE_PL_GUARD, (s, sites[s], fr)
            assert product.exact_pl_site(ref, alts, e) == w_pl, (s, sites[s])
        else:
            assert pl[s, :G].tolist() == w_pl, (s, sites[s], pl[s], w_pl)
    return n_flagged
