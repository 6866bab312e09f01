// The per-row arithmetic of k_genotype (svjg_kernels.h): the reference's likelihood() (predict-genotype.py:281-338) in fp64 /
// double-double.  Plain C++ so that tests/hostsim compiles the same code with g++ and checks it against known answers of the
// reference on a machine without a GPU (and under -fsanitize=address,undefined, tools/asan.sh).
#pragma once
#include <math.h>
#include <stdint.h>
#include <string.h>
#include "svjg_pass.h"

#ifndef SVJG_HD
#define SVJG_HD __host__ __device__ inline __attribute__((always_inline))
#endif

namespace svjg {

struct dd { double hi, lo; };

SVJG_HD dd two_sum(double a, double b) {
    double s = a + b, bb = s - a;
    return dd{s, (a - (s - bb)) + (b - bb)};
}
SVJG_HD dd dd_add(dd a, dd b) {
    dd s = two_sum(a.hi, b.hi);
    dd t = two_sum(a.lo, b.lo);
    s.lo += t.hi;
    s = two_sum(s.hi, s.lo);          // quick renormalisation (|lo| << |hi| here)
    s.lo += t.lo;
    return two_sum(s.hi, s.lo);
}
SVJG_HD dd dd_neg(dd a) { return dd{-a.hi, -a.lo}; }
SVJG_HD int dd_cmp(dd a, dd b) { return a.hi < b.hi ? -1 : a.hi > b.hi ? 1 : a.lo < b.lo ? -1 : a.lo > b.lo ? 1 : 0; }

SVJG_HD int64_t trunc_dd(dd v) {                         // int(Decimal): toward zero
    double t = trunc(v.hi);
    if (t == v.hi) {                                     // hi is integral: the tail decides
        if (v.hi > 0 && v.lo < 0) t -= 1.0;
        else if (v.hi < 0 && v.lo > 0) t += 1.0;
    }
    return (int64_t)t;
}

// The log10(i!) table (k_logfact_*) never grows beyond LOGFACT_CAP entries (256 MB).  A row whose binomial term would need more
// (n = r1 + r2 >= LOGFACT_CAP, both r1 and r2 > 0) is not computed from the table: the kernel flags it like a row next to an
// integer boundary, and the host recomputes it with the reference's arithmetic (svjg/genotype.py: exact_pl).
constexpr uint32_t LOGFACT_CAP = 1u << 24;

// A row is flagged for the host when one of its -10 * (lik + comb) lies within PL_GUARD of an integer.  The budget, for
// n < LOGFACT_CAP: every table entry is a sum of at most n values log10(i) < 7.3, each within 1 ulp (2^-50) of the true value,
// summed in double-double: |table error| <= 2^24 * 2^-50 = 1.5e-8 per entry, and comb takes one
// entry of n terms and two of n terms together: <= 3e-8.  The reference's log10 of a big integer goes through CPython's frexp
// path, log10(x) + log10(2) * e: a few ulps of L = log10(comb) <= 5.1e6 (ulp 9.3e-10): <= 4e-9.  Both sides round L to a
// double (1 ulp each).  The likelihood sums are exact here and at 28 digits in the reference BECAUSE each product c * L is rounded to a double
// before it is added, as the reference's Decimal(c * L) is: geno_row_pairs and geno_site form them under `fp contract(off)`
// (measured on the device where fused products would change the answer: tests/test_genotype_products_gpu.py).  Times ten: < 3.6e-7 < 1e-6.
// The "1 ulp" of the device's log10 is measured, not assumed (2026-10-18, one MI355X, ROCm 7.2.0; the table at the cap read back through
// svjg_logfact_read and held against 60-digit values, tests/test_logfact_gpu.py asserts each bound on every run): all 2^24 - 2 increments
// table[i] - table[i-1] lie within 0.504 * 2^-50 of log10(i) (worst at i = 5 638 997: the device's log10 is correctly rounded or next to
// it), the worst entry of 5 450 sampled is 7.6e-12 off (i = 16 344 492; the roundings cancel, they do not add up: 1/2000 of the 1.5e-8),
// and 10 * |comb from the table - the reference's double| is at most 4.7e-9 over 8 846 pairs (n, k) = (13 266 267, 1 927 482): one ulp of
// L, against the 3.6e-7 above.  The table the CPU stand-ins build with the host's libm (tests/hostsim) differs from the device's in
// 16 777 051 of 2^24 entries, by at most 2.2e-11 (i = 11 186 418).
constexpr double PL_GUARD = 1e-6;

// normalised counts (predict-genotype.py:327-338) and the rounded ones fed to comb()
SVJG_HD void geno_counts(uint32_t type, uint32_t ref, uint32_t alt, double &c1, double &c2, uint32_t &r1, uint32_t &r2) {
    c1 = (double)ref; c2 = (double)alt;
    if (type == 0 && ref) c1 = (double)ref * 0.5;       // round(x/2, 1) is exact for halves
    if (type == 1 && alt) c2 = (double)alt * 0.5;
    r1 = (uint32_t)rint(c1); r2 = (uint32_t)rint(c2);   // int(round(c, 0)): half to even
}

// n = r1 + r2 of a row, computed in 64 bits (ref + alt reaches 2^33 - 2)
SVJG_HD uint64_t geno_n(uint32_t r1, uint32_t r2) { return (uint64_t)r1 + r2; }

enum : uint32_t { GENO_ROW_OK = 0, GENO_ROW_GROW = 1, GENO_ROW_HOST = 2 };

// log10 comb(n, k) = log10 n! - log10 (n - k)! - log10 k! from the table, in double-double (n below the table's entries)
SVJG_HD dd logfact_comb(const dd *logfact, uint32_t n, uint32_t k) { return dd_add(dd_add(logfact[n], dd_neg(logfact[n - k])), dd_neg(logfact[k])); }

// The binomial term of a row with the rounded counts r1, r2, rounded to a double first like the reference (:313), and n = r1 + r2.
// -> GENO_ROW_OK, GENO_ROW_GROW (the table is too short for n < LOGFACT_CAP: the host grows it and runs the rows again; the term is 0) or
// GENO_ROW_HOST (n >= LOGFACT_CAP: the row is flagged for the host, the term is 0).
SVJG_HD uint32_t geno_comb(uint32_t r1, uint32_t r2, const dd *logfact, uint32_t logfact_n, dd &comb, uint64_t &n) {
    n = geno_n(r1, r2);                                  // (never a wrapped sum: no index comes from one)
    comb = dd{0.0, 0.0};                                 // comb(n, 0) = comb(n, n) = 1: no table needed
    if (!(r1 && r2)) return GENO_ROW_OK;
    if (n >= logfact_n) return n < LOGFACT_CAP ? GENO_ROW_GROW : GENO_ROW_HOST;
    comb = dd{logfact_comb(logfact, (uint32_t)n, r1).hi, 0.0};
    return GENO_ROW_OK;
}

// One PL integer: int(-10 (lik + term)), and whether -10 (lik + term) lies within `guard` of an integer.  The reference adds
// Decimal(math.log10(math.comb(n, k))) (:313): libm's log10 of a big integer rounded to a double, which need not be the correctly rounded
// value the table holds.  The two can differ in the last places; times ten, next to an integer, that could turn a PL by one.  Values that
// close are flagged and recomputed on the host (svjg/genotype.py).  The fraction is taken from hi AND lo: above |p| ~ 2^33 hi alone cannot
// resolve the guard.  term = log10(1) = 0 on both sides: nothing to disagree about, never inside.
SVJG_HD int64_t geno_pl(dd lik, dd term, double guard, bool &inside) {
    const dd s = dd_add(lik, term);
    dd p = dd_add(dd_add(dd_add(s, s), dd_add(s, s)), s);                     // 5 s
    p = dd_add(p, p);                                                         // 10 s
    inside = fabs((p.hi - rint(p.hi)) + p.lo) < guard && term.hi != 0.0;
    return trunc_dd(dd_neg(p));
}

// ---- one row at any ploidy from 1 to MAX_PLOIDY (k_genotype_ploidy; k_genotype at P = 2) ----
// A row of ploidy P has P + 1 genotypes, g = 0..P alt copies.  A read shows the alt allele with probability (g (1 - e) + (P - g) e) / P,
// the ref allele with ((P - g) (1 - e) + g e) / P: lik_g = c1 * Lr[P][g] + c2 * La[P][g].  g = 0 and g = P are the reference's lik0 and
// lik2 (log10(1 - e), log10(e)), 2 g = P its lik1, ONE product (c1 + c2) * log10(1/2).
constexpr uint32_t MAX_PLOIDY = 8;
#ifdef __clang__
#define SVJG_UNROLL _Pragma("unroll")
#else
#define SVJG_UNROLL
#endif
constexpr uint32_t PLOIDY_TAB = 45;                      // entries of Lr (and of La): [P (P + 1) / 2 + g], P = 1..8, g = 0..P; entry 0 unused
SVJG_HD uint32_t ploidy_tab_at(uint32_t P, uint32_t g) { return P * (P + 1) / 2 + g; }

// The logarithms of a call, by the host's libm like geno_args' three (the kernel computes none): tab[0..44] = Lr, tab[45..89] = La.
// The quotients are formed in doubles in exactly the order the model is written in.
inline void ploidy_log_table(double err, double *tab) {
    const double l_ok = log10(1.0 - err), l_err = log10(err), l_half = log10(1.0 / 2.0);
    tab[0] = tab[PLOIDY_TAB] = 0.0;
    for (uint32_t P = 1; P <= MAX_PLOIDY; ++P)
        for (uint32_t g = 0; g <= P; ++g) {
            double lr, la;
            if (g == 0) { lr = l_ok; la = l_err; }
            else if (g == P) { lr = l_err; la = l_ok; }
            else if (2 * g == P) lr = la = l_half;
            else {
                const double pg = (double)(P - g), gg = (double)g, pp = (double)P, ok = 1.0 - err;
                const double a = pg * ok, b = gg * err, c = gg * ok, d = pg * err;       // (each product rounded on its own: no fused multiply-add)
                lr = log10((a + b) / pp); la = log10((c + d) / pp);
            }
            tab[ploidy_tab_at(P, g)] = lr; tab[PLOIDY_TAB + ploidy_tab_at(P, g)] = la;
        }
}

struct GenoRowPloidy {
    int64_t pl[MAX_PLOIDY + 1];   // PL_g for g = 0..P, 0 beyond
    uint8_t gt;                   // alt copies of the call, 0xFF: no call
    bool near;                    // one of the P + 1 PLs lies within PL_GUARD of an integer, or the row is beyond the table's cap: the host recomputes it
    uint64_t n;                   // r1 + r2
};

// The reference's lik0 and lik2 are SUMS of two Decimals, rounded to the context's 28 significant digits (half to even); its lik1 is ONE
// Decimal, the exact image of a double, which no operation ever rounds.  Where the exact sum of the two products IS the double h of lik1
// (every row at e = 0.5, where log10(1 - e) = log10(e) = log10(1 / 2), whenever the two roundings cancel), the reference therefore compares
// round28(h) with h itself, and the 29th digit of h decides its GT.  -> the sign of round28(h) - h, 0: h has at most 28 digits.
// h = (c1 + c2) * log10(1 / 2) with c1 + c2 in [0.5, 2^33]: 0.15 <= |h| < 2^32, so 10^s |h| with s = 27 - floor(log10 |h|) in 18..28 is
// m * 5^s / 2^r (m: the 53 bits of |h| = m * 2^(ex - 53), r = 53 - ex - s in 1..27; r < 1: an integer): the fraction and the parity of the
// 28th digit are the low r + 1 bits of m * 5^s, and a 64-bit product that wraps holds them.  (Differences of less than one unit of the 28th digit that are not zero cannot occur: they are
// multiples of an ulp of the smallest product, > 2^-86 of the largest.)
#ifdef __clang__
#define SVJG_NOUNROLL _Pragma("nounroll")
#else
#define SVJG_NOUNROLL
#endif
SVJG_HD int dec28_round_dir(double h) {
    const double x = fabs(h);
    const bool inside = x >= 0.125 && x < 4294967296.0;  // (outside: 0, the row without reads; nothing else)
    int ex; const double f = frexp(inside ? x : 1.0, &ex);
    int p10 = -1; double ten = 1.0;
    SVJG_NOUNROLL                                        // (unrolled, the ten powers would sit in twenty scalar registers of every kernel that inlines this)
    for (int k = 0; k < 10; ++k) { if (x >= ten) p10 = k; ten *= 10.0; }      // (powers of ten up to 10^9: exact doubles)
    const int s = 27 - p10, r = 53 - ex - s;             // |h| 10^s = m 5^s / 2^r, s in 18..28
    uint64_t N = (uint64_t)ldexp(f, 53) * 3814697265625ull;                   // m * 5^18 mod 2^64
    for (int i = 18; i < 28; ++i) N *= i < s ? 5u : 1u;                       // m * 5^s mod 2^64 (no branch: the lanes of a wave differ in s)
    const int rr = r < 1 ? 1 : r;
    const uint64_t frac = N & ((1ull << rr) - 1), half = 1ull << (rr - 1);
    const bool up = frac > half || (frac == half && ((N >> rr) & 1));         // the magnitude grows (half to even)
    if (!inside || r < 1 || frac == 0) return 0;         // (r < 1: an integer of 28 digits)
    return (up == (h > 0)) ? 1 : -1;
}

// lik_g of a row of ploidy P as every caller compares it: the exact sum of the two ROUNDED products, the one product at 2 g = P.  (its own
// pragma: the caller's does not reach into an inlined callee)
SVJG_HD dd geno_lik(double c1, double c2, uint32_t P, uint32_t g, const double *lr, const double *la) {
#ifdef __clang__
#pragma clang fp contract(off)                           // the products are rounded to doubles before the exact sums
#endif
    const double a = c1 * lr[g], b = c2 * la[g], h = (c1 + c2) * lr[g];
    return (g != 0 && 2 * g == P) ? dd{h, 0.0} : two_sum(a, b);
}

// One genotyped row of ploidy P in 1..MAX_PLOIDY; lr / la: the row's own P + 1 logarithms (geno_row_ploidy and geno_row below say which).
// Status as geno_comb (the PLs of a row that is not GENO_ROW_OK are without the binomial term).  The loop over g is unrolled with a predicate
// so that pl[] is only ever indexed by constants (registers on the device, no scratch).
SVJG_HD uint32_t geno_row_pairs(uint32_t type, uint32_t ref, uint32_t alt, uint32_t P, uint32_t min_support, const double *lr, const double *la,
                                 const dd *logfact, uint32_t logfact_n, GenoRowPloidy &o) {
#ifdef __clang__
#pragma clang fp contract(off)                           // the products are rounded to doubles before the exact sums
#endif
    double c1, c2; uint32_t r1, r2;
    geno_counts(type, ref, alt, c1, c2, r1, r2);
    dd comb;
    const uint32_t st = geno_comb(r1, r2, logfact, logfact_n, comb, o.n);
    // The one product of an even ploidy, g = P / 2, is never rounded to 28 digits, the sums are: where a sum IS that double, the 29th digit
    // decides (above).  Looked for ahead of the loop, so that the digits are worked out at one place and only for such a row.
    int dir = 0;
    if ((P & 1) == 0) {
        const double h = (c1 + c2) * lr[P / 2];
        bool same = false;
        SVJG_UNROLL
        for (uint32_t g = 0; g <= MAX_PLOIDY; ++g) {
            if (g > P || 2 * g == P) continue;
            const dd l = geno_lik(c1, c2, P, g, lr, la);
            if (l.hi == h && l.lo == 0.0) same = true;
        }
        if (same) dir = dec28_round_dir(h);
    }
    dd best{0.0, 0.0}; uint8_t g_best = 0xFF; bool tie = false, near = false, best_single = false;
    SVJG_UNROLL
    for (uint32_t g = 0; g <= MAX_PLOIDY; ++g) {
        o.pl[g] = 0;
        if (g > P) continue;
        // products in double, sums exact (the reference adds Decimal images of the doubles, :295-297): each product is ROUNDED before two_sum sees it
        const bool single = g != 0 && 2 * g == P;
        const dd l = geno_lik(c1, c2, P, g, lr, la);
        int c = g ? dd_cmp(l, best) : 1;
        if (c == 0 && single != best_single) c = single ? -dir : dir;      // sign of (the rounded sum - the product) seen from l
        if (c > 0) { best = l; g_best = (uint8_t)g; best_single = single; tie = false; } else if (c == 0) tie = true;
        bool inside;
        o.pl[g] = geno_pl(l, comb, PL_GUARD, inside);
        near |= inside;
    }
    if (tie || !(c1 + c2 >= (double)min_support)) g_best = 0xFF;
    o.gt = g_best;
    o.near = near || st == GENO_ROW_HOST;
    return st;
}

// The row of ploidy P on a call's table (k_genotype_ploidy, k_genotype_cohort_ploidy); lr / la: the two halves of ploidy_log_table, the row's
// own entries start at ploidy_tab_at(P, 0) of either.
SVJG_HD uint32_t geno_row_ploidy(uint32_t type, uint32_t ref, uint32_t alt, uint32_t P, uint32_t min_support, const double *lr, const double *la,
                                 const dd *logfact, uint32_t logfact_n, GenoRowPloidy &o) {
    return geno_row_pairs(type, ref, alt, P, min_support, lr + ploidy_tab_at(P, 0), la + ploidy_tab_at(P, 0), logfact, logfact_n, o);
}

// The diploid row (k_genotype, k_genotype_cohort): geno_row_pairs at the literal ploidy 2, the reference's three likelihoods as the row's
// three pairs, no table.  gt: 0 / 1 / 2 alt copies, 3: no call.
struct GenoRow {
    int64_t pl[3];
    uint8_t gt;
    bool near;       // as GenoRowPloidy::near
    uint64_t n;      // r1 + r2
};
SVJG_HD uint32_t geno_row(uint32_t type, uint32_t ref, uint32_t alt, uint32_t min_support, double l_ok, double l_err, double l_half,
                          const dd *logfact, uint32_t logfact_n, GenoRow &o) {
    const double lr[3] = {l_ok, l_half, l_err}, la[3] = {l_err, l_half, l_ok};
    GenoRowPloidy w;
    const uint32_t st = geno_row_pairs(type, ref, alt, 2, min_support, lr, la, logfact, logfact_n, w);
    o.pl[0] = w.pl[0]; o.pl[1] = w.pl[1]; o.pl[2] = w.pl[2];
    o.gt = w.gt == 0xFF ? 3 : w.gt; o.near = w.near; o.n = w.n;
    return st;
}

// ---- insertions that share a position, genotyped together (k_genotype_sites; diploid) ----
// A site has K = 2..MAX_SITE_ALTS insertions at one CHROM and POS; allele 0 is the reference, allele j the j-th insertion.  Counts: c_0 = the
// largest raw ref count of the members (they share the one reference link), c_j = alt_j / 2 (the reference's INS normalisation), N their sum.
// Genotypes {a, b}, 0 <= a <= b <= K, in VCF order b (b + 1) / 2 + a.  A read shows an allele with probability q(.|a) / 2 + q(.|b) / 2, q = 1 - e
// for the haplotype's own allele and e / K for every other one:
//     a == b   lik = c_a * L_ok + (N - c_a) * L_x                      L_ok = log10(1 - e), L_x = log10(e / K)
//     a <  b   lik = (c_a + c_b) * L_he + (N - c_a - c_b) * L_x        L_he = log10(((1 - e) + e / K) / 2)
// two double products and one exact sum each, like lik0 / lik2.  The coefficient term is a chain of the reference's binomial terms over the
// rounded counts r_j: s_0 = r_0, s_j = s_(j-1) + r_j, T = sum of log10 comb(s_j, r_j), each term rounded to a double before it is added (the
// host model adds Decimal(math.log10(math.comb(s_j, r_j)))).  PL_ab = int(-10 (lik_ab + T)).
constexpr uint32_t MAX_SITE_ALTS = 6;
constexpr uint32_t SITE_GENOTYPES = (MAX_SITE_ALTS + 1) * (MAX_SITE_ALTS + 2) / 2;       // 28
constexpr uint8_t SITE_NO_CALL = 0xFF;

// A site is flagged when one of its -10 (lik + T) lies within SITE_PL_GUARD of an integer.  PL_GUARD's budget above bounds what ONE binomial
// term can disagree by between the table and the reference's log10 of the big integer, times ten: 3.6e-7.  T has up to MAX_SITE_ALTS such terms
// (every index is at most s_K < LOGFACT_CAP, so each term is within that budget), their roundings to doubles are part of it, and the sums are
// exact on both sides: 6 x 3.6e-7 = 2.16e-6 < 2.5e-6.
constexpr double SITE_PL_GUARD = 2.5e-6;

// The logarithms of a call by the host's libm, in exactly the written order: tab[0] = L_ok, tab[K] = L_x[K], tab[8 + K] = L_he[K], K = 1..6
constexpr uint32_t SITE_LOGS = 16;
inline void site_log_table(double err, double *tab) {
    for (uint32_t i = 0; i < SITE_LOGS; ++i) tab[i] = 0.0;
    tab[0] = log10(1.0 - err);
    for (uint32_t K = 1; K <= MAX_SITE_ALTS; ++K) {
        const double k = (double)K, x = err / k, ok = 1.0 - err;
        tab[K] = log10(x);
        tab[8 + K] = log10((ok + x) / 2.0);
    }
}

// lik_ab of a site as every caller compares it (geno_site, and site_prior_load below): the exact sum of the two ROUNDED products.  c: the site's
// normalised counts, indexed by the caller's unrolled constants, N their sum.  (its own pragma: the caller's does not reach into an inlined callee)
SVJG_HD dd site_lik(const double *c, double N, uint32_t a, uint32_t b, double l_ok, double l_x, double l_he) {
#ifdef __clang__
#pragma clang fp contract(off)                           // the products are rounded to doubles before the exact sum
#endif
    const double own = a == b ? c[a] : c[a] + c[b];
    const double rest = a == b ? N - c[a] : N - c[a] - c[b];
    const double p1 = own * (a == b ? l_ok : l_he), p2 = rest * l_x;
    return two_sum(p1, p2);
}

struct GenoSite {
    uint8_t a, b;    // the call, a <= b; SITE_NO_CALL, SITE_NO_CALL: a tie or below min_support
    bool near;       // one of the site's values lies within SITE_PL_GUARD of an integer, or the site is beyond the table's cap: the host recomputes it
    uint64_t n;      // s_K
};

// One site of K in 2..MAX_SITE_ALTS members: ref = the raw ref maximum, alt[0..K) the raw alt counts (entries beyond K are not read).  pl:
// SITE_GENOTYPES integers, written as they are produced (the kernel hands in the site's place in global memory), 0 beyond the site's
// (K + 1)(K + 2) / 2.  Status and flag as geno_row_pairs.  Both loops are unrolled under a predicate: c[] and r[] are only ever indexed by constants.
SVJG_HD uint32_t geno_site(uint32_t K, uint32_t ref, const uint32_t *alt, uint32_t min_support, double l_ok, double l_x, double l_he,
                           const dd *logfact, uint32_t logfact_n, int64_t *pl, GenoSite &o) {
#ifdef __clang__
#pragma clang fp contract(off)                           // the products are rounded to doubles before the exact sums
#endif
    double c[MAX_SITE_ALTS + 1]; uint32_t r[MAX_SITE_ALTS + 1];
    c[0] = (double)ref; r[0] = ref;
    double N = c[0];
    uint64_t s_K = ref;
    bool table = false;                                  // a chain term is not log10(1)
    SVJG_UNROLL
    for (uint32_t j = 1; j <= MAX_SITE_ALTS; ++j) {
        c[j] = 0.0; r[j] = 0;
        if (j > K) continue;
        const uint32_t v = alt[j - 1];
        c[j] = (double)v * 0.5;                          // round(x / 2, 1) is exact for halves (0 stays 0)
        r[j] = (uint32_t)rint(c[j]);                     // int(round(c, 0)): half to even
        N += c[j];                                       // (halves below 2^36: exact)
        if (r[j] && s_K) table = true;
        s_K += r[j];
    }
    o.n = s_K;
    uint32_t st = GENO_ROW_OK;
    dd T{0.0, 0.0};
    if (table) {
        if (s_K < logfact_n) {
            uint32_t s = r[0];
            SVJG_UNROLL
            for (uint32_t j = 1; j <= MAX_SITE_ALTS; ++j) {
                if (j > K) continue;
                const uint32_t t = s + r[j];             // <= s_K < logfact_n: every index below is inside the table
                if (r[j] && s) {
                    T = dd_add(T, dd{logfact_comb(logfact, t, r[j]).hi, 0.0});    // each term rounded to a double first, like the model's Decimal(math.log10(...))
                }
                s = t;
            }
        } else st = s_K < LOGFACT_CAP ? GENO_ROW_GROW : GENO_ROW_HOST;
    }
    dd best{0.0, 0.0}; uint8_t best_a = SITE_NO_CALL, best_b = SITE_NO_CALL; bool tie = false, near = false;
    SVJG_UNROLL
    for (uint32_t b = 0; b <= MAX_SITE_ALTS; ++b) {
        SVJG_UNROLL
        for (uint32_t a = 0; a <= b; ++a) {
            const uint32_t at = b * (b + 1) / 2 + a;
            if (b > K) { pl[at] = 0; continue; }
            const dd l = site_lik(c, N, a, b, l_ok, l_x, l_he);
            const int cmp = at ? dd_cmp(l, best) : 1;
            if (cmp > 0) { best = l; best_a = (uint8_t)a; best_b = (uint8_t)b; tie = false; } else if (cmp == 0) tie = true;
            bool inside;
            pl[at] = geno_pl(l, T, SITE_PL_GUARD, inside);
            near |= inside;
        }
    }
    if (tie || !(N >= (double)min_support)) best_a = best_b = SITE_NO_CALL;
    o.a = best_a; o.b = best_b;
    o.near = near || st == GENO_ROW_HOST;
    return st;
}

// ---- many samples, one row set (k_genotype_cohort; diploid) ----
// Items are flattened as i = r * S + s (row r, sample s) and walked a wave of 64 consecutive items at a time, so the samples of one row are
// consecutive lanes.  The lanes of a wave that hold the SAME row as lane `lane` (item i, sample s = i % S of S) form one segment:
// it starts s lanes below (cut at lane 0) and ends S - 1 - s lanes above (cut at lane 63).  A row of R x S items ends at an item below
// R * S, so no segment reaches beyond the last item; a lane whose item is at or beyond n_items belongs to no segment (mask 0, no leader).
// The leader is the segment's first lane: it alone adds the segment's sums to the row's site word, so a row that straddles two waves
// receives two additions.
struct CohortSeg { uint64_t mask; bool leader; };
SVJG_HD CohortSeg cohort_segment(uint64_t i, uint64_t s, uint64_t S, uint32_t lane, uint64_t n_items) {
    if (i >= n_items) return CohortSeg{0, false};
    const uint32_t lo = s > lane ? 0u : lane - (uint32_t)s;
    const uint64_t above = S - 1 - s;
    const uint32_t hi = above > 63u - lane ? 63u : lane + (uint32_t)above;
    const uint64_t upto = hi == 63u ? ~0ull : (1ull << (hi + 1)) - 1;          // lanes 0..hi
    return CohortSeg{upto & ~((1ull << lo) - 1), lane == lo};
}

// ---- many samples at per-sample ploidy (k_genotype_cohort_ploidy) ----
// With the ploidy differing from item to item a row's site tags are three sums over its called items: NS = their number, AN = the sum of their
// ploidies, AC = the sum of their alt copies.  Both summands are at most MAX_PLOIDY = 8, four bits: the wave takes one ballot for "called" and
// one per bit plane of gt and of the ploidy, and a sum over a segment is sum_b 2^b * popcount(plane_b & called & mask).  The planes are taken
// under `called` here, so a lane that is not called may vote anything (gt = 0xFF, whatever ploidy its item has).
struct CohortBallots { uint64_t called, gt[4], ploidy[4]; };
struct CohortSums { uint32_t ns, an, ac; };
SVJG_HD CohortSums cohort_ploidy_sums(const CohortBallots &b, uint64_t mask) {
    const uint64_t m = b.called & mask;
    CohortSums o{(uint32_t)__builtin_popcountll(m), 0, 0};
    SVJG_UNROLL
    for (uint32_t k = 0; k < 4; ++k) {
        o.ac += (uint32_t)__builtin_popcountll(b.gt[k] & m) << k;
        o.an += (uint32_t)__builtin_popcountll(b.ploidy[k] & m) << k;
    }
    return o;
}
// k_genotype_cohort's sums of a segment, every item diploid, from its three ballots (called: gt != 3, het: gt == 1, hom: gt == 2): NS, AC = het + 2 hom
// (AN = 2 NS: the kernel leaves it to the host)
SVJG_HD CohortSums cohort_diploid_sums(uint64_t called, uint64_t het, uint64_t hom, uint64_t mask) {
    const uint32_t ns = (uint32_t)__builtin_popcountll(called & mask);
    return CohortSums{ns, 2 * ns, (uint32_t)__builtin_popcountll(het & mask) + 2 * (uint32_t)__builtin_popcountll(hom & mask)};
}
// the row's two site words: NS | AC << 32 (k_genotype_cohort's word) and AN.  (AC, AN <= 8 S: they fit 32 bits for S < 2^28)
SVJG_HD uint64_t cohort_site_word(const CohortSums &s) { return (uint64_t)s.ns | ((uint64_t)s.ac << 32); }

// ---- many samples, insertions that share a position (k_genotype_cohort_sites; diploid) ----
// An item is (site k, sample s), i = k * S + s, walked like k_genotype_cohort's: the samples of one site are consecutive lanes, cohort_segment gives
// the site's lanes.  A site has up to MAX_SITE_ALTS CANDIDATES (the rows of the merged catalogue at one CHROM and POS); sample s's site consists of
// the candidates whose presence byte is set for s, in candidate order, numbered 1..K' — what form_sites makes of that sample's `done` bytes in a
// single-sample run.  K' < 2: the item has no site call.

// The present candidates (bit j of `bits`: candidate j is present, cref[j] / calt[j] its raw counts) compacted into alt[0..K): the reference count is
// the largest raw ref count over the PRESENT candidates only.  Both loops are unrolled and every array is indexed by constants only (the k-th place
// is chosen by selects), so that the kernel keeps cref, calt and alt in registers.  alt beyond K: 0.
struct SiteMembers { uint32_t K, ref, alt[MAX_SITE_ALTS]; };
SVJG_HD void site_compact(uint32_t bits, const uint32_t *cref, const uint32_t *calt, SiteMembers &m) {
    m.K = 0; m.ref = 0;
    SVJG_UNROLL
    for (uint32_t t = 0; t < MAX_SITE_ALTS; ++t) m.alt[t] = 0;
    SVJG_UNROLL
    for (uint32_t j = 0; j < MAX_SITE_ALTS; ++j) {
        const bool in = (bits >> j) & 1u;
        SVJG_UNROLL
        for (uint32_t t = 0; t <= j; ++t) m.alt[t] = in && t == m.K ? calt[j] : m.alt[t];      // (K <= j here: the place is one of 0..j)
        m.ref = in && cref[j] > m.ref ? cref[j] : m.ref;
        m.K += in;
    }
}

// Copies of candidate j's allele in an item's call (a, b), 0..2; SITE_NO_CALL: the item has no site call (a == SITE_NO_CALL: K' < 2, a tie, below
// min_support, or a lane beyond the last item) or candidate j is no member.  The candidate's allele number is 1 + the members in front of it.
SVJG_HD uint32_t site_candidate_copies(uint32_t members, uint32_t a, uint32_t b, uint32_t j) {
    if (a == SITE_NO_CALL || !((members >> j) & 1u)) return SITE_NO_CALL;
    const uint32_t al = 1u + (uint32_t)__builtin_popcount(members & ((1u << j) - 1u));
    return (uint32_t)(a == al) + (uint32_t)(b == al);
}

// Per candidate j three ballots of the wave: in = the lane's copies are not SITE_NO_CALL, one / two = they are 1 / 2.  The sums of a segment for
// candidate j: NS_j = the site-called items where j is a member, AC_j = the copies of its allele in those calls; the word the segment's first lane
// adds to site[k][j] is NS_j | AC_j << 32 (cohort_site_word).
struct SiteBallots { uint64_t in[MAX_SITE_ALTS], one[MAX_SITE_ALTS], two[MAX_SITE_ALTS]; };
SVJG_HD CohortSums cohort_site_member_sums(const SiteBallots &b, uint32_t j, uint64_t mask) {
    const uint32_t ns = (uint32_t)__builtin_popcountll(b.in[j] & mask);
    return CohortSums{ns, 2 * ns, (uint32_t)__builtin_popcountll(b.one[j] & mask) + 2 * (uint32_t)__builtin_popcountll(b.two[j] & mask)};
}

// ---- what both site kernels do per item (k_genotype_sites, k_genotype_cohort_sites; tests/geno_sim runs the same code on the CPU) ----
// The ONE place that reads a site's slots (the named ones first, SITE_NO_SLOT behind them), into sample s of a slot-major count matrix of S samples
// and n_slots slots (counts[slot * S + s], present[slot * S + s]); the count vector is the matrix of S = 1, s = 0, and present == nullptr says every
// named slot is a member (the single-sample call).  members: bit j = candidate j is present, cref[j] / calt[j] its raw counts (0 where it is not).
// bad: a slot behind a hole, or at or beyond n_slots — never, behind the host's checks; NOTHING is read through such a slot.  Unrolled, every array
// indexed by constants only (registers on the device, no scratch).
constexpr uint32_t SITE_NO_SLOT = 0xFFFFFFFFu;          // (svjg_line.h: NONE32)
struct SiteGather { uint32_t members, cref[MAX_SITE_ALTS], calt[MAX_SITE_ALTS]; bool bad; };
SVJG_HD void site_gather(const unsigned long long *counts, const uint8_t *present, uint64_t S, uint64_t s, uint32_t n_slots, const uint32_t *slots, SiteGather &g) {
    g.members = 0; g.bad = false;
    bool open = true;
    uint32_t named[MAX_SITE_ALTS];                       // (all six ahead of the first count: one round trip to the site's 24 bytes, not one per slot between the counts')
    SVJG_UNROLL
    for (uint32_t j = 0; j < MAX_SITE_ALTS; ++j) named[j] = slots[j];
    SVJG_UNROLL
    for (uint32_t j = 0; j < MAX_SITE_ALTS; ++j) {
        const uint32_t sl = named[j];
        g.cref[j] = g.calt[j] = 0;
        if (sl == SITE_NO_SLOT) open = false;
        else if (!open || sl >= n_slots) g.bad = true;
        else {
            const uint64_t at = (uint64_t)sl * S + s;
            if (!present || present[at]) {
                const unsigned long long c = counts[at];
                g.cref[j] = (uint32_t)c; g.calt[j] = (uint32_t)(c >> 32); g.members |= 1u << j;
            }
        }
    }
}

// One item behind the gather: the members compacted into alt[0..K') (site_compact), `call` = K' >= 2 and not bad, raw[1 + MAX_SITE_ALTS] = the ref
// maximum and the members' alt counts, geno_site into the item's SITE_GENOTYPES PLs or zeros, the two gt bytes, the boundary byte.  logs:
// site_log_table of the call's err.  dense (a literal at both calls): the single-sample call, present == nullptr — every named slot is a member and
// the host has refused holes, so the compaction is the identity, alt[j] = calt[j] and K = popcount(members), and is not run (through site_compact
// k_genotype_sites is 90 instructions longer and ran 1.914 .. 1.949 ms, 64 calls summed, against 1.910 .. 1.914 without it in the same job:
// profiles/r18/experiments/one_sites_leg.txt); K < 2 counts as bad there.  -> status as geno_site (GENO_ROW_OK without a call), n = s_K, members
// (0 for a bad item), the pair, bad.  What a kernel adds to max_n for it stays in the kernel: this is plain C++.
struct SiteItem { uint32_t status; uint64_t n; uint32_t members; uint8_t a, b; bool bad; };
SVJG_HD SiteItem site_item(const unsigned long long *counts, const uint8_t *present, bool dense, uint64_t S, uint64_t s, uint32_t n_slots, const uint32_t *slots,
                           uint32_t min_support, const double *logs, const dd *logfact, uint32_t logfact_n,
                           uint32_t *raw, int64_t *pl, uint8_t *gt, uint8_t *boundary) {
    const double l_ok = logs[0];                         // (ahead of the gather: the kernels' LDS read travels beside the global ones)
    SiteGather g;
    site_gather(counts, dense ? nullptr : present, S, s, n_slots, slots, g);
    if (g.bad) g.members = 0;
    SiteMembers m;
    if (dense) {
        m.K = (uint32_t)__builtin_popcount(g.members); m.ref = 0;
        SVJG_UNROLL
        for (uint32_t j = 0; j < MAX_SITE_ALTS; ++j) { m.alt[j] = g.calt[j]; m.ref = g.cref[j] > m.ref ? g.cref[j] : m.ref; }     // (a bad item: K = 0, neither is looked at)
    } else site_compact(g.members, g.cref, g.calt, m);
    const bool bad = g.bad || (dense && m.K < 2), call = m.K >= 2;
    raw[0] = call ? m.ref : 0;
    SVJG_UNROLL
    for (uint32_t j = 0; j < MAX_SITE_ALTS; ++j) raw[1 + j] = call ? m.alt[j] : 0;
    GenoSite o{SITE_NO_CALL, SITE_NO_CALL, false, 0};
    uint32_t st = GENO_ROW_OK;
    if (call) st = geno_site(m.K, m.ref, m.alt, min_support, l_ok, logs[m.K], logs[8 + m.K], logfact, logfact_n, pl, o);
    else {
        SVJG_UNROLL
        for (uint32_t i = 0; i < SITE_GENOTYPES; ++i) pl[i] = 0;
    }
    gt[0] = o.a; gt[1] = o.b; *boundary = o.near;
    return SiteItem{st, o.n, g.members, o.a, o.b, bad};
}

// ---- cohort with an allele-frequency prior (k_cohort_prior) ----
// The row's alt-allele frequency f is estimated from all its samples' likelihoods by EM under Hardy-Weinberg, each item is then called at
// the maximum of likelihood x prior.  An item (r, s) takes part iff the cohort call genotyped it and c1 + c2 > 0.  Its weights: l_g = geno_lik,
// what geno_row_pairs compares, d_g = l_g - max l_g subtracted in
// double-double and collapsed to one double, w_g = 10^d_g (the binomial term is the same for every g and cancels).  The prior is
// pi_g(f; P) = C(P, g) f^g (1 - f)^(P - g), powers by repeated multiplication (0^0 = 1); posterior q_g = pi_g w_g / sum_g pi_g w_g, one-hot at
// the item's largest w_g where that sum is 0; expected copies x = sum_g g q_g.  f_0 = 0.5, f_(k+1) = sum_s x_s / sum_s P_s over the row's items
// that take part; the row stops after the first step with |f_(k+1) - f_k| <= EM_TOL, or after EM_MAX_IT steps without one ("not converged").
// Every routine below is compiled without fused multiply-adds, so the host harness (tests/geno_sim: prior) and the kernel differ in exp10,
// log10 and nothing else.
constexpr double EM_TOL = 1e-9;
constexpr uint32_t EM_MAX_IT = 128;
constexpr uint32_t EM_NOT_CONVERGED = 1u << 31;          // top bit of a row's step word
// |f_device - f_model|, the model being tests/cohort_prior_model.py at 60 digits, is measured, not assumed (2026-10-19, one MI355X, ROCm 7.2.0,
// tests/test_cohort_prior_gpu.py: 25 cases of 400 or 1 500 rows x 1..130 samples, 30 133 rows with an estimate): at most 3.668e-16 absolute
// (1 sample a row, ploidies 0..8) and 1.187e-14 relative among the rows with f > 1e-6 (the same case; 3.7e-16 relative at 31 samples and more).
// At the shapes that only the kernel's body knows (2026-10-20, the same device: 22 further cases of 200 or 300 rows x 2, 8, 9, 16, 17, 192, 193,
// 256, 257 and 320 samples, 5 384 rows with an estimate): at most 1.957e-16 absolute and 6.123e-15 relative (mixed_2: 2 samples a row, ploidies
// 0..8), at 192 samples and more 1.755e-16 (mixed_193) and 4.942e-16 (mixed_256); the maximum over all 47 cases stays the 3.668e-16 of mixed_1.
// The tests assert 8 x the absolute maximum: the margin is for other seeds, not for other arithmetic.
constexpr double EM_F_BOUND = 8 * 3.668e-16;

// What an item keeps across the EM steps: w[g] = C(P, g) * 10^d_g for g = 0..P (0 beyond), the binomial coefficient folded in once (an exact
// integer <= 70 times a double: one rounding, and 0 iff 10^d_g is 0).  P = 0: the item takes no part.  gmax: the first g with d_g = 0.
struct PriorItem { double w[MAX_PLOIDY + 1]; uint32_t P, gmax; };

SVJG_HD double prior_exp10(double d) {
#if defined(__HIP_DEVICE_COMPILE__)
    return exp10(d);
#else
    return pow(10.0, d);                                 // (glibc's pow is correctly rounded in nearly every case; the harness compares against 60 digits)
#endif
}

// lr / la: the item's own P + 1 logarithms, as for geno_row_pairs.  Both loops under a predicate: w[] is only ever indexed by constants.
SVJG_HD void prior_item(uint32_t type, uint32_t ref, uint32_t alt, uint32_t P, const double *lr, const double *la, double &c_sum, PriorItem &o) {
#ifdef __clang__
#pragma clang fp contract(off)                           // the products are rounded to doubles before the exact sums
#endif
    double c1, c2; uint32_t r1, r2;
    geno_counts(type, ref, alt, c1, c2, r1, r2);
    c_sum = c1 + c2;
    o.P = c_sum > 0.0 ? P : 0u; o.gmax = 0;
    dd best{0.0, 0.0};
    SVJG_UNROLL
    for (uint32_t g = 0; g <= MAX_PLOIDY; ++g) {
        if (g > o.P || o.P == 0) continue;
        const dd l = geno_lik(c1, c2, P, g, lr, la);
        if (g == 0 || dd_cmp(l, best) > 0) { best = l; o.gmax = g; }
    }
    uint32_t comb = 1;                                   // C(P, g), exact in integers
    SVJG_UNROLL
    for (uint32_t g = 0; g <= MAX_PLOIDY; ++g) {
        o.w[g] = 0.0;
        if (g > o.P || o.P == 0) continue;
        if (g) comb = comb * (P - g + 1) / g;
        const dd d = dd_add(geno_lik(c1, c2, P, g, lr, la), dd_neg(best));
        o.w[g] = (double)comb * prior_exp10(d.hi + d.lo);
    }
}

// Item i as the EM sees it (k_cohort_prior and tests/geno_sim), from what the first kernel left: raw[i][2], genotyped[i], and the call's
// ploidy[i] (nullptr: 2 everywhere), the row's type byte and tab = ploidy_log_table.  The item takes no part (it.P = 0) unless the first kernel
// genotyped it and it has a read; the type is read only for an item that does (a pointer, so that the kernel's load stays behind that test).
SVJG_HD void prior_load(const uint8_t *type, const uint32_t *raw, const uint8_t *genotyped, const uint8_t *ploidy, uint64_t i, const double *tab, double &c_sum, PriorItem &it) {
    const uint32_t P = genotyped[i] ? (ploidy ? ploidy[i] : 2u) : 0u;
    it.P = 0; it.gmax = 0; c_sum = 0.0;
    SVJG_UNROLL
    for (uint32_t g = 0; g <= MAX_PLOIDY; ++g) it.w[g] = 0.0;
    if (P >= 1 && P <= MAX_PLOIDY) prior_item(*type, raw[i * 2], raw[i * 2 + 1], P, tab + ploidy_tab_at(P, 0), tab + PLOIDY_TAB + ploidy_tab_at(P, 0), c_sum, it);
}

// t[g] = pi_g(f; P) w_g for g = 0..P (0 beyond): (1 - f)^(P - g) from the top down, f^g from the bottom up.  P = 0: all 0, f is not looked at.
SVJG_HD void prior_terms(const PriorItem &it, double f, double *t) {
#ifdef __clang__
#pragma clang fp contract(off)
#endif
    const double q = 1.0 - f;
    double b = 1.0;
    SVJG_UNROLL
    for (int g = (int)MAX_PLOIDY; g >= 0; --g) {
        t[g] = 0.0;
        if ((uint32_t)g > it.P || it.P == 0) continue;
        if ((uint32_t)g < it.P) b *= q;
        t[g] = it.w[g] * b;
    }
    double a = 1.0;
    SVJG_UNROLL
    for (uint32_t g = 1; g <= MAX_PLOIDY; ++g) {
        if (g > it.P) continue;
        a *= f;
        t[g] *= a;
    }
}

// x = sum_g g q_g of one item under f (0 for an item that takes no part); both sums in increasing g
SVJG_HD double prior_expected(const PriorItem &it, double f) {
#ifdef __clang__
#pragma clang fp contract(off)
#endif
    double t[MAX_PLOIDY + 1];
    prior_terms(it, f, t);
    double z = 0.0, x = 0.0;
    SVJG_UNROLL
    for (uint32_t g = 0; g <= MAX_PLOIDY; ++g) { z += t[g]; x += (double)g * t[g]; }
    if (it.P == 0) return 0.0;
    return z > 0.0 ? x / z : (double)it.gmax;
}

// The call of one item under the row's final f: gt = argmax q_g (0xFF: a tie at the maximum, below min_support, or the item takes no part),
// gq = min(99, int(-10 log10(sum of the other q_g, in increasing g))), 99 where that sum is 0, 0xFF without a call.
struct PriorCall { uint8_t gt, gq; };
SVJG_HD PriorCall prior_call(const PriorItem &it, double f, double c_sum, uint32_t min_support) {
#ifdef __clang__
#pragma clang fp contract(off)
#endif
    double t[MAX_PLOIDY + 1];
    prior_terms(it, f, t);
    double z = 0.0, top = 0.0; uint32_t best = 0; bool tie = false;
    SVJG_UNROLL
    for (uint32_t g = 0; g <= MAX_PLOIDY; ++g) {
        if (g > it.P) continue;
        z += t[g];
        if (g == 0 || t[g] > top) { top = t[g]; best = g; tie = false; } else if (t[g] == top) tie = true;
    }
    if (it.P == 0) return PriorCall{0xFF, 0xFF};
    double rest = 0.0;
    SVJG_UNROLL
    for (uint32_t g = 0; g <= MAX_PLOIDY; ++g) if (g <= it.P && g != best) rest += t[g];
    if (z > 0.0) rest /= z; else { best = it.gmax; tie = false; rest = 0.0; }
    if (tie || !(c_sum >= (double)min_support)) return PriorCall{0xFF, 0xFF};
    double v = rest > 0.0 ? -10.0 * log10(rest) : 99.0;
    if (!(v < 99.0)) v = 99.0;
    return PriorCall{(uint8_t)best, (uint8_t)(v > 0.0 ? (uint32_t)v : 0u)};
}

// One EM step's outcome for a row: sum_x over sum_p against the f it was computed under; r.done: the row has stopped.
struct PriorRow { double f; uint32_t steps; bool done; };
SVJG_HD void prior_step(PriorRow &r, double sum_x, uint32_t sum_p) {
    if (r.done) return;                                  // a converged row keeps its f while its wave goes on
    const double fn = sum_x / (double)sum_p;
    const bool conv = fabs(fn - r.f) <= EM_TOL;
    r.f = fn; ++r.steps;
    if (conv) r.done = true;
    else if (r.steps == EM_MAX_IT) { r.done = true; r.steps |= EM_NOT_CONVERGED; }
}
// a row before its first step: no item takes part (sum_p = 0): no estimate (NaN), 0 steps
SVJG_HD PriorRow prior_row_start(uint32_t sum_p) { return PriorRow{sum_p ? 0.5 : NAN, 0u, sum_p == 0}; }

// The lanes a row takes in k_cohort_prior: the next power of two >= min(S, 64); 64 / width rows share a wave, a row never spans two.
SVJG_HD uint32_t prior_segment_width(uint64_t S) {
    const uint32_t m = S < 64 ? (uint32_t)S : 64u;
    uint32_t w = 1;
    while (w < m) w <<= 1;
    return w;
}
// The grid of a kernel that gives every row such a segment (k_cohort_prior, k_cohort_sites_prior, k_cohort_hwe), in blocks of tpb lanes: as many as
// hold the waves of n_rows rows, at most blocks_per_cu on each of n_cu units; the kernel takes the rest in strides of the grid.
SVJG_HD uint32_t segment_grid(uint64_t n_rows, uint64_t S, uint32_t tpb, uint32_t n_cu, uint32_t blocks_per_cu) {
    const uint64_t rows_per_wave = 64u / prior_segment_width(S), waves = (n_rows + rows_per_wave - 1) / rows_per_wave;
    const uint64_t blocks = (waves * 64 + tpb - 1) / tpb, cap = (uint64_t)n_cu * blocks_per_cu;
    return (uint32_t)(blocks < cap ? blocks : cap);
}
// the blocks a unit gets at the most, by launch
constexpr uint32_t PRIOR_BLOCKS_PER_CU = 8;              // k_cohort_prior: blocks of four waves
constexpr uint32_t SITES_PRIOR_BLOCKS_PER_CU = 2;        // k_cohort_sites_prior: a block's 57 472 bytes of LDS let two share a unit's 160 KiB
constexpr uint32_t HWE_BLOCKS_PER_CU = 8;                // k_cohort_hwe: blocks of four waves
constexpr uint32_t QC_BLOCKS_PER_CU = 4;                 // k_qc_planes, k_qc_pairs: the pair kernel's 36 864 bytes of LDS and 4 waves a block admit that many

// ---- cohort sites with an allele-frequency prior (k_cohort_sites_prior behind k_genotype_cohort_sites) ----
// The samples of a SITE inform each other: the frequencies p = (p_0..p_C) of the site's alleles are estimated by EM under Hardy-Weinberg, each item
// is then called at the maximum of likelihood x prior.  Alleles: a site has C = 2..MAX_SITE_ALTS candidates (its named slots); allele 0 is the
// reference, allele j candidate j, the same numbering for every sample of the site.  An item (k, s) takes part iff the first kernel gave it a site
// (K' >= 2 members present: `members` and the raw counts as site_item left them) and it has a read, N = sum c_j > 0; support gates calls, not
// likelihoods.  Weights: l_AB = site_lik on the item's own members with its own K' (logs[K'], logs[8 + K']) — with the counts expanded to
// candidate order (0 for an absent candidate) these are bit for bit the values geno_site compares in member numbering —, d_AB = l_AB - max l
// subtracted in double-double and collapsed to one double, w_AB = 10^d_AB (the chain term T is the same for every genotype and cancels).  The
// item keeps its SITE_GENOTYPES weights in CANDIDATE order, slot B (B + 1) / 2 + A for A <= B over 0..6; a genotype that names a candidate absent
// for this sample, or one beyond C, has weight 0: K' does not occur behind site_prior_load.  Prior pi_AB(p) = p_A^2 (A = B), 2 p_A p_B (A < B);
// t_AB = pi_AB w_AB, z = sum t, posterior q_AB = t_AB / z over the genotypes on {0} + the sample's members, one-hot at the item's first largest w
// where z is 0.  Expected copies x_j = (sum_AB copies_j(A, B) t_AB) / z for j = 0..C, numerator and z summed in increasing slot order.  Step:
// p_j <- sum_s x_(s,j) / (2 n), n the number of items taking part (an integer, reduced once); start p_j = 1 / (C + 1); the site stops after the
// first step with max_j |p_j' - p_j| <= EM_TOL or after EM_MAX_IT steps (bit 31 of the step word: not converged, as prior_step); n = 0: all p NaN,
// 0 steps.  p_j beyond C is 0 wherever there is an estimate.  Calls under the final p: argmax q, an exact tie or N < min_support is a no-call;
// SGQ = min(99, int(-10 log10(sum of the other q, in increasing slot order))), 99 where that sum is 0.
// This is a stated fixed-point iteration: a sample with a proper subset of the candidates conditions on that subset.  It is not claimed to be the
// maximum-likelihood estimate of a model in which an absent candidate counts as zero alt reads.
// Compiled without fused multiply-adds, so the host harness (tests/geno_sim, topic site_prior) and the kernel differ in exp10 and log10 only.
constexpr uint32_t SITE_ALLELES = MAX_SITE_ALTS + 1;    // 7: the reference and the candidates
// max_j |p_j(device) - p_j(model)|, the model being tests/site_prior_model.py at 60 digits, is measured, not assumed (2026-10-21, one MI355X, ROCm
// 7.2.0, tests/test_cohort_site_prior_gpu.py: 46 cases of 200 sites (one of 77) x 1..130 samples, the 37 of them with an estimate): at most
// 2.322e-16 absolute (rare_3: one carrier among 3 samples) and 8.230e-16 relative among the p_j > 1e-6 (mixed_3_odd).  The host harness in the
// kernel's order of the sums, glibc's pow and log10 in place of the device's exp10 and log10, measures the same two figures in the same two cases
// (tests/test_cohort_site_prior.py): the constant is the DEVICE reading, which the CPU tests assert as well.
// The tests assert 8 x the absolute maximum: the margin is for other seeds, not for other arithmetic.
constexpr double SITE_EM_P_BOUND = 8 * 2.322e-16;

// what an item keeps beside its weights: members (bit j = candidate j present), top = the slot of its first largest w, N, and whether it takes part
struct SitePriorMeta { uint32_t members, top; double N; bool part; };

SVJG_HD bool site_prior_valid(uint32_t members, uint32_t A, uint32_t B) {
    return (A == 0 || ((members >> (A - 1)) & 1u)) && (B == 0 || ((members >> (B - 1)) & 1u));
}

// One item from what the first kernel left: raw[1 + MAX_SITE_ALTS] = the ref maximum and the MEMBERS' alt counts (compacted), members.  The counts
// are expanded to candidate order ONCE, by unrolled selects under constant indices (site_compact's reverse); the weights go to w[slot * stride]
// (the kernel: slot-major in LDS, stride = the block's lanes; the harness: stride 1).  An item that takes no part: zeros.
SVJG_HD void site_prior_load(const uint32_t *raw, uint32_t members, const double *logs, double *w, uint32_t stride, SitePriorMeta &m) {
#ifdef __clang__
#pragma clang fp contract(off)
#endif
    uint32_t v[SITE_ALLELES];
    SVJG_UNROLL
    for (uint32_t t = 0; t < SITE_ALLELES; ++t) v[t] = raw[t];
    members &= (1u << MAX_SITE_ALTS) - 1u;
    const uint32_t K = (uint32_t)__builtin_popcount(members);
    double c[SITE_ALLELES];
    c[0] = (double)v[0];
    double N = c[0];
    SVJG_UNROLL
    for (uint32_t j = 0; j < MAX_SITE_ALTS; ++j) {
        const bool in = (members >> j) & 1u;
        const uint32_t at = (uint32_t)__builtin_popcount(members & ((1u << j) - 1u));       // the members in front of candidate j: its place in raw
        uint32_t a = 0;
        SVJG_UNROLL
        for (uint32_t t = 0; t <= j; ++t) a = in && t == at ? v[1 + t] : a;
        c[1 + j] = (double)a * 0.5;                      // the INS normalisation, exact for halves (0 stays 0)
        N += c[1 + j];                                   // (halves below 2^36: exact in any order)
    }
    m.members = members; m.top = 0; m.N = N; m.part = K >= 2 && N > 0.0;
    const uint32_t Kc = K < 2 ? 2u : K;                  // (an item that takes no part reads two logarithms it does not use)
    const double l_ok = logs[0], l_x = logs[Kc], l_he = logs[8 + Kc];
    dd best{0.0, 0.0};
    SVJG_UNROLL
    for (uint32_t B = 0; B <= MAX_SITE_ALTS; ++B) {
        SVJG_UNROLL
        for (uint32_t A = 0; A <= B; ++A) {
            const uint32_t at = B * (B + 1) / 2 + A;
            const dd l = site_lik(c, N, A, B, l_ok, l_x, l_he);
            if (site_prior_valid(members, A, B) && (at == 0 || dd_cmp(l, best) > 0)) { best = l; m.top = at; }
        }
    }
    SVJG_UNROLL
    for (uint32_t B = 0; B <= MAX_SITE_ALTS; ++B) {
        SVJG_UNROLL
        for (uint32_t A = 0; A <= B; ++A) {
            const uint32_t at = B * (B + 1) / 2 + A;
            const dd d = dd_add(site_lik(c, N, A, B, l_ok, l_x, l_he), dd_neg(best));
            w[at * stride] = m.part && site_prior_valid(members, A, B) ? prior_exp10(d.hi + d.lo) : 0.0;
        }
    }
}

// t_AB = pi_AB(p) w_AB of one slot (A, B: the callers' unrolled constants)
SVJG_HD double site_prior_term(const double *w, uint32_t stride, const double *p, uint32_t A, uint32_t B) {
#ifdef __clang__
#pragma clang fp contract(off)
#endif
    const double pi = A == B ? p[A] * p[A] : (2.0 * p[A]) * p[B];
    return pi * w[(B * (B + 1) / 2 + A) * stride];
}

// x[j] += the item's expected copies of allele j under p, j = 0..6 (nothing for an item that takes no part)
SVJG_HD void site_prior_expected(const double *w, uint32_t stride, const SitePriorMeta &m, const double *p, double *x) {
#ifdef __clang__
#pragma clang fp contract(off)
#endif
    double z = 0.0, u[SITE_ALLELES];
    SVJG_UNROLL
    for (uint32_t j = 0; j < SITE_ALLELES; ++j) u[j] = 0.0;
    SVJG_UNROLL
    for (uint32_t B = 0; B <= MAX_SITE_ALTS; ++B) {
        SVJG_UNROLL
        for (uint32_t A = 0; A <= B; ++A) {
            const double t = site_prior_term(w, stride, p, A, B);
            z += t;
            if (A == B) u[A] += 2.0 * t; else { u[A] += t; u[B] += t; }
        }
    }
    if (!m.part) return;
    SVJG_UNROLL
    for (uint32_t B = 0; B <= MAX_SITE_ALTS; ++B) {
        SVJG_UNROLL
        for (uint32_t A = 0; A <= B; ++A) {
            const uint32_t at = B * (B + 1) / 2 + A;
            if (!(z > 0.0) && at == m.top) { u[A] = u[A] + 1.0; u[B] = u[B] + 1.0; }     // one-hot at the first largest w (every u is 0 here)
        }
    }
    SVJG_UNROLL
    for (uint32_t j = 0; j < SITE_ALLELES; ++j) x[j] += z > 0.0 ? u[j] / z : u[j];
}

// The call of one item under the site's final p, in the ITEM's member numbering (gt's convention: project_cohort_sites serves both): a <= b, 0 the
// reference, t the t-th present candidate; SITE_NO_CALL twice and gq = 0xFF: a tie at the maximum, below min_support, or the item takes no part.
struct SitePriorCall { uint8_t a, b, gq; };
SVJG_HD SitePriorCall site_prior_call(const double *w, uint32_t stride, const SitePriorMeta &m, const double *p, uint32_t min_support) {
#ifdef __clang__
#pragma clang fp contract(off)
#endif
    double z = 0.0, top = 0.0; uint32_t best = 0; bool tie = false;
    SVJG_UNROLL
    for (uint32_t B = 0; B <= MAX_SITE_ALTS; ++B) {
        SVJG_UNROLL
        for (uint32_t A = 0; A <= B; ++A) {
            const uint32_t at = B * (B + 1) / 2 + A;
            const double t = site_prior_term(w, stride, p, A, B);
            z += t;
            if (at == 0 || t > top) { top = t; best = at; tie = false; } else if (t == top) tie = true;
        }
    }
    if (!m.part) return SitePriorCall{SITE_NO_CALL, SITE_NO_CALL, 0xFF};
    if (!(z > 0.0)) { best = m.top; tie = false; }
    double rest = 0.0; uint32_t bA = 0, bB = 0;
    SVJG_UNROLL
    for (uint32_t B = 0; B <= MAX_SITE_ALTS; ++B) {
        SVJG_UNROLL
        for (uint32_t A = 0; A <= B; ++A) {
            const uint32_t at = B * (B + 1) / 2 + A;
            if (at != best) rest += site_prior_term(w, stride, p, A, B); else { bA = A; bB = B; }     // (formed again, the same bits: 28 terms are not kept in registers)
        }
    }
    rest = z > 0.0 ? rest / z : 0.0;
    if (tie || !(m.N >= (double)min_support)) return SitePriorCall{SITE_NO_CALL, SITE_NO_CALL, 0xFF};
    double v = rest > 0.0 ? -10.0 * log10(rest) : 99.0;
    if (!(v < 99.0)) v = 99.0;
    const uint32_t a = bA ? 1u + (uint32_t)__builtin_popcount(m.members & ((1u << (bA - 1)) - 1u)) : 0u;
    const uint32_t b = bB ? 1u + (uint32_t)__builtin_popcount(m.members & ((1u << (bB - 1)) - 1u)) : 0u;
    return SitePriorCall{(uint8_t)a, (uint8_t)b, (uint8_t)(v > 0.0 ? (uint32_t)v : 0u)};
}

// A site across its EM steps.  C: its candidates (the named slots of its MAX_SITE_ALTS), n: its items that take part.
struct SitePriorSite { double p[SITE_ALLELES]; uint32_t steps; bool done; };
SVJG_HD uint32_t site_candidates(const uint32_t *slots) {
    uint32_t C = 0;
    SVJG_UNROLL
    for (uint32_t j = 0; j < MAX_SITE_ALTS; ++j) C += slots[j] != SITE_NO_SLOT;
    return C;
}
SVJG_HD SitePriorSite site_prior_start(uint32_t C, uint32_t n) {
    SitePriorSite s;
    const double p0 = 1.0 / (double)(C + 1u);
    SVJG_UNROLL
    for (uint32_t j = 0; j < SITE_ALLELES; ++j) s.p[j] = n ? (j <= C ? p0 : 0.0) : NAN;
    s.steps = 0; s.done = n == 0;
    return s;
}
// one step's outcome: the sums x[0..6] over the site's items against the p they were computed under
SVJG_HD void site_prior_step(SitePriorSite &s, const double *x, uint32_t n) {
    if (s.done) return;                                  // a stopped site keeps its p while its wave goes on
    const double den = 2.0 * (double)n;
    double far = 0.0;
    SVJG_UNROLL
    for (uint32_t j = 0; j < SITE_ALLELES; ++j) {
        const double pn = x[j] / den, d = fabs(pn - s.p[j]);
        far = d > far ? d : far;
        s.p[j] = pn;
    }
    ++s.steps;
    if (far <= EM_TOL) s.done = true;
    else if (s.steps == EM_MAX_IT) { s.done = true; s.steps |= EM_NOT_CONVERGED; }
}

// ---- cohort site quality: the exact allele-count posterior (k_cohort_qual) ----
// "Is there at least one alt copy in this cohort": the exact model of Li 2011 (the QUAL of samtools / bcftools), at any ploidy.  An item (r, s)
// takes part under the rule of the EM above: cohort_gate passes (ok & 1, a slot, presence), its ploidy P is in 1..max_ploidy (2 everywhere
// without a ploidy array) and c1 + c2 > 0.  Its coefficients are a_g = C(P, g) 10^(d_g), g = 0..P: exactly PriorItem::w of prior_item; beside
// them d_0 = l_0 - max l is kept in double-double (qual_item).  With M' the chromosomes of the items folded in so far and M = M' + P,
// y_k = z_k / C(M, k) is the likelihood of "k alt copies among M chromosomes", averaged over which chromosomes carry them: y_0 = 1 at M' = 0,
// and the items are folded in in sample order by
//     y_k <- sum_(g = 0..min(P, k)) a_g y_(k-g) (k)_g (M - k)_(P-g) / (M)_P      for k = 0..M,
// (x)_n the falling factorial x (x - 1) ... (x - n + 1), (x)_0 = 1; a term with k - g > M' is absent.  The factor is a hypergeometric
// probability (times C(P, g), which a_g carries); at P = 2 this is Li's recurrence term for term.  The normalised form is used on purpose: the
// plain convolution z_k with one division by C(M, k) at the end fails at scale — with a thousand shallow samples the posterior's mass sits at
// k where z_k / max z underflows while C(M, k_max) / C(M, k) overflows (tests/test_cohort_qual.py shows the case).
// Rescaling: 10^(d_g) <= 1 and the hypergeometric probabilities of a k add up to at most 1, so the row's maximum never grows; the item's
// largest coefficient is C(P, gmax) 10^0 >= 1 and the hypergeometric probability that goes with it is at least 1 / C(M, P), so one step
// shrinks the maximum by at most 1 / C(M, P) > 1 / M^P > 2^-(P bits), bits = the binary digits of the call's largest M (13 at 4096: one step
// is always safe, 1 / C(4096, 8) > 2^-82).  Every qual_rescale_every(M_max, max_ploidy) = max(1, 512 / (max_ploidy bits)) steps the row is
// multiplied by 2^(-ilogb(max y)) — exact, so harness and kernel see the same bits — and -ilogb(max y) is added to the integer E: behind a
// rescaling the maximum lies in [1, 2), so between two of them it cannot fall below 2^-512, and what then underflows is below 2^-510 of it.
// Prior over the allele count: phi_k = theta / k for k = 1..M, phi_0 = 1 - theta H_M, H_M = sum_(k = 1..M) 1 / k summed in increasing k in
// double (qual_harmonic: the host makes the table of a call, the kernel reads entry M).  Per row: chroms = M; without an item that takes part
// M = 0, qual = NaN, mlac = 0; mlac = the smallest k that attains max_k phi_k y_k; qual = max(0, -10 (log10 phi_0 + D_0 - log10 T + E log10 2)),
// T = sum_k phi_k y_k over the scaled y, D_0 = sum_s d_(s,0) in double-double in sample order: the log of the TRUE y_0, which may have
// underflowed in the scaled array.  Every sum over k is fixed once: lane-strided partials in increasing k (lane j: k = j, j + 64, ...), then the
// xor butterfly over 64 lanes.  Compiled without fused multiply-adds (the one fma() in qual_finish is an exact product, written out): the
// harness (tests/geno_sim: qual) and the kernel differ in exp10 and log10 only.
constexpr uint32_t QUAL_MAX_CHROMS = 4096;               // 2 x 4097 doubles = 65.6 KB of LDS a block: 2 048 diploid samples
constexpr double QUAL_THETA_MAX = 0.05;                  // 0.05 H_4096 = 0.445 < 1: phi_0 > 0 for every accepted call
constexpr double QUAL_LOG10_2_HI = 0.3010299956639812, QUAL_LOG10_2_LO = -2.8037281277851704e-18;   // log10 2 as a double-double
// |qual - model|, the model being tests/cohort_qual_model.py at 60 digits, is measured, not assumed (2026-10-20, one MI355X, ROCm 7.2.0,
// tests/test_cohort_qual_gpu.py: the 16 cases of tests/cohort_qual_cases.py, 3 235 rows with a quality, 1..2 048 samples): at most 3.769e-15
// absolute among the rows whose model value is below 1 and 1.993e-15 relative among the others, both at shallow_600 (600 samples of one read;
// every other case stays below 1.2e-15 and 9.8e-16).  The host harness on the same cases (tests/geno_sim, glibc's pow and log10):
// 8.210e-15 and 1.993e-15 with the sums in the kernel's order, 1.043e-14 and 1.993e-15 sequentially.  The tests assert
// |qual - model| <= QUAL_ABS + QUAL_REL * model with 8 x the device's maximum of each (the EM_F_BOUND convention: the margin is for other
// seeds, not for other arithmetic).
// Measured again over the enlarged set (2026-10-20, one MI355X, ROCm 7.2.0: 34 cases, 5 517 rows with a quality, the 18 new ones at max_ploidy
// 1..7, on the chrX / chrY shape, at mixed ploidy up to M = 560 and in the shallow regime up to 512 samples of ploidy 8, M = 4 096), with
// qual_finish normalising T: 8.592e-15 absolute among the rows whose model value is below 1 and 8.299e-15 relative among the others, both at
// shallow_hap_600 (600 haploid samples of one read; the relative one on a row whose model value is 3.4, 2.85e-14 absolute: 0.34 of the bound
// there, the largest share of any row); shallow_600 3.075e-15 and 2.515e-15, shallow_poly_512 5.369e-15, every case outside the shallow regime
// below 8.7e-16 and 3.9e-16.  The host harness: 1.029e-14 (shallow_600, sequentially) and 8.557e-15 (shallow_hap_600, sequentially; 8.428e-15
// in the kernel's order).  The two constants stay the first measurement's: the sum of the two terms is what is asserted, and it holds with the
// margin above.  One ploidy array gives equal bytes under every max_ploidy from its largest value to 8, on the harness (14 cases) and on the
// device (5 of them).
constexpr double QUAL_ABS_MEASURED = 3.769e-15, QUAL_REL_MEASURED = 1.993e-15;
constexpr double QUAL_ABS = 8 * QUAL_ABS_MEASURED, QUAL_REL = 8 * QUAL_REL_MEASURED;

struct QualItem { PriorItem it; dd d0; };                // it: prior_item's, unchanged; d0 = l_0 - l_gmax (0 for an item that takes no part)

// prior_item and, beside it, d_0 (l_gmax is prior_item's `best`: gmax is the first g with the largest l_g)
SVJG_HD void qual_item(uint32_t type, uint32_t ref, uint32_t alt, uint32_t P, const double *lr, const double *la, QualItem &o) {
    double c_sum;
    prior_item(type, ref, alt, P, lr, la, c_sum, o.it);
    o.d0 = dd{0.0, 0.0};
    if (o.it.P) {
        double c1, c2; uint32_t r1, r2;
        geno_counts(type, ref, alt, c1, c2, r1, r2);
        o.d0 = dd_add(geno_lik(c1, c2, P, 0, lr, la), dd_neg(geno_lik(c1, c2, P, o.it.gmax, lr, la)));
    }
}

// The item of ploidy P (0: the gate or the ploidy keeps it out) with the raw counts ref / alt on the call's table tab = ploidy_log_table
SVJG_HD void qual_load(uint32_t type, uint32_t ref, uint32_t alt, uint32_t P, const double *tab, QualItem &o) {
    o.it.P = 0; o.it.gmax = 0; o.d0 = dd{0.0, 0.0};
    SVJG_UNROLL
    for (uint32_t g = 0; g <= MAX_PLOIDY; ++g) o.it.w[g] = 0.0;
    if (P >= 1 && P <= MAX_PLOIDY) qual_item(type, ref, alt, P, tab + ploidy_tab_at(P, 0), tab + PLOIDY_TAB + ploidy_tab_at(P, 0), o);
}

// steps between two rescalings of a row (above)
SVJG_HD uint32_t qual_rescale_every(uint32_t m_max, uint32_t max_ploidy) {
    uint32_t bits = 0;
    while ((m_max >> bits) != 0) ++bits;
    const uint32_t n = 512u / (max_ploidy * (bits ? bits : 1u));
    return n < 1 ? 1u : n;
}

// (M)_P, the recurrence's denominator, from the top factor down
SVJG_HD double qual_den(uint32_t M, uint32_t P) {
#ifdef __clang__
#pragma clang fp contract(off)
#endif
    double d = 1.0;
    SVJG_UNROLL
    for (uint32_t i = 0; i < MAX_PLOIDY; ++i) if (i < P) d *= (double)(M - i);
    return d;
}

// y_k of M = M0 + P chromosomes from the row y of M0 (entries 0..M0), den = qual_den(M, P).  t_g = (a_g (M - k)_(P-g)) (k)_g: the first factorial
// from the top genotype down, the second from the bottom up, as prior_terms forms its powers; the sum over g in increasing g, then ONE division.
// A factorial that runs through 0 makes its term 0 (g > k, or k - g > M0): nothing is read for such a term.  t[] is only ever indexed by constants.
SVJG_HD double qual_fold(const PriorItem &it, const double *y, uint32_t M0, uint32_t M, uint32_t k, double den) {
#ifdef __clang__
#pragma clang fp contract(off)
#endif
    double t[MAX_PLOIDY + 1];
    const double rest = (double)(M - k), kk = (double)k;
    double b = 1.0;
    SVJG_UNROLL
    for (int g = (int)MAX_PLOIDY; g >= 0; --g) {
        t[g] = 0.0;
        if ((uint32_t)g > it.P) continue;
        if ((uint32_t)g < it.P) b *= rest - (double)(it.P - (uint32_t)g - 1u);
        t[g] = it.w[g] * b;
    }
    double a = 1.0;
    SVJG_UNROLL
    for (uint32_t g = 1; g <= MAX_PLOIDY; ++g) {
        if (g > it.P) continue;
        a *= kk - (double)(g - 1u);
        t[g] *= a;
    }
    double acc = 0.0;
    SVJG_UNROLL
    for (uint32_t g = 0; g <= MAX_PLOIDY; ++g) {
        if (g > it.P) continue;
        const bool in = g <= k && k - g <= M0;
        const double v = in ? y[in ? k - g : 0u] : 0.0;
        acc += t[g] * v;
    }
    return acc / den;
}

// H_0..H_m of a call, each the one before plus 1 / k in double
inline void qual_harmonic(uint32_t m, double *h) {
    h[0] = 0.0;
    for (uint32_t k = 1; k <= m; ++k) h[k] = h[k - 1] + 1.0 / (double)k;
}
SVJG_HD double qual_phi0(double theta, double h_m) {
#ifdef __clang__
#pragma clang fp contract(off)
#endif
    return 1.0 - theta * h_m;
}
// phi_k y_k
SVJG_HD double qual_term(double theta, double phi0, uint32_t k, double y) {
#ifdef __clang__
#pragma clang fp contract(off)
#endif
    return (k ? theta / (double)k : phi0) * y;
}
// The larger of two (phi_k y_k, k), the smaller k at equal values: what a lane keeps over its k and what the butterfly's partners exchange
struct QualBest { double v; uint32_t k; };
SVJG_HD QualBest qual_best(QualBest a, QualBest b) { return (b.v > a.v || (b.v == a.v && b.k < a.k)) ? b : a; }

// qual of a row with M > 0 (above): the sum in double-double, E log10 2 as an exact product of the integer and the constant's head plus the tail.
// T's own binary exponent goes to E first (exact), so that log10 sees a value in [1, 2) whatever scale the row was left at: which steps were
// followed by a rescaling (the cadence, and with it max_ploidy) then changes no bit of the answer, and log10's rounding is that of a value
// below 0.31 instead of one of up to 154
SVJG_HD double qual_finish(double phi0, dd D0, double T, int64_t E) {
#ifdef __clang__
#pragma clang fp contract(off)
#endif
    if (T > 0.0) {                                                             // (always: phi_k > 0 and the row's maximum is positive)
        const int x = ilogb(T);
        T = ldexp(T, -x);
        E -= x;
    }
    dd s = dd_add(dd{log10(phi0), 0.0}, D0);
    s = dd_add(s, dd{-log10(T), 0.0});
    const double e = (double)E, p = e * QUAL_LOG10_2_HI, pe = fma(e, QUAL_LOG10_2_HI, -p);
    s = dd_add(s, two_sum(p, pe + e * QUAL_LOG10_2_LO));
    dd v = dd_add(dd_add(dd_add(s, s), dd_add(s, s)), s);                      // 5 s
    v = dd_add(v, v);                                                          // 10 s
    const double q = -(v.hi + v.lo);
    return q > 0.0 ? q : 0.0;                                                  // (never -0.0)
}

// ---- cohort sample QC: per-sample sums and pairwise kinship counts (k_qc_planes, k_qc_pairs) ----
// Integers only.  Item (r, s) has the call g = gt[r][s] and the ploidy P = ploidy[r][s] (2 without an array); both no-call codes of the library are
// "g > P" (3 in the diploid calls, 0xFF elsewhere).  Six predicates an item, one bit each (QC_*): eligible P >= 1; called: eligible and g <= P;
// carrier: called and g >= 1; dip: called and P = 2; het: dip and g = 1; homalt: dip and g = 2 (homref = dip & ~het & ~homalt).  Per sample the six
// sums over the rows; per pair i < j, at k = i S - i (i + 1) / 2 + (j - i - 1), five sums over the rows: both = dip_i dip_j, het1 = het_i dip_j,
// het2 = dip_i het_j, hethet = het_i het_j, ibs0 = homref_i homalt_j + homalt_i homref_j.  A sample's predicates over 64 consecutive rows are one
// 64-bit word a predicate (row 64 w + b is bit b of word w; the bits behind the call's last row are 0), a pair's sums popcounts of ANDs of them.
enum : uint32_t { QC_ELIGIBLE, QC_CALLED, QC_CARRIER, QC_DIP, QC_HET, QC_HOMALT, QC_CLASSES };       // the order of sample[s][6]
constexpr uint32_t QC_PAIR_COUNTS = 5;                   // both, het1, het2, hethet, ibs0: the order of pair[k][5]
constexpr uint32_t QC_MAX_SAMPLES = 2048;                // 2 096 128 pairs, 42 MB of them
SVJG_HD uint32_t qc_class(uint32_t g, uint32_t P) {      // -> bit QC_x set: the predicate holds
    const uint32_t eligible = P >= 1, called = eligible & (g <= P), carrier = called & (g >= 1), dip = called & (P == 2);
    return eligible << QC_ELIGIBLE | called << QC_CALLED | carrier << QC_CARRIER | dip << QC_DIP | (dip & (g == 1)) << QC_HET | (dip & (g == 2)) << QC_HOMALT;
}
constexpr uint64_t qc_words(uint64_t n_rows) { return (n_rows + 63) / 64; }
constexpr uint64_t qc_pairs(uint64_t S) { return S * (S - 1) / 2; }
SVJG_HD uint32_t qc_pair_at(uint32_t i, uint32_t j, uint32_t S) { return i * S - i * (i + 1) / 2 + (j - i - 1); }      // i < j < S <= QC_MAX_SAMPLES: below 2^21

// the six words of sample s over the rows 64 w .. 64 w + 63 of a call of n_rows rows x S samples (k_qc_planes: one lane a sample, so a wave reads
// consecutive bytes of a row); word[] is indexed by unrolled constants only
SVJG_HD void qc_plane_words(const uint8_t *gt, const uint8_t *ploidy, uint64_t n_rows, uint64_t S, uint64_t w, uint64_t s, uint64_t *word) {
    SVJG_UNROLL
    for (uint32_t q = 0; q < QC_CLASSES; ++q) word[q] = 0;
    const uint64_t r0 = w * 64, left = n_rows - r0;
    const uint32_t n = left < 64 ? (uint32_t)left : 64u;
    for (uint32_t b = 0; b < n; ++b) {
        const uint64_t at = (r0 + b) * S + s;
        const uint32_t c = qc_class(gt[at], ploidy ? ploidy[at] : 2u);
        SVJG_UNROLL
        for (uint32_t q = 0; q < QC_CLASSES; ++q) word[q] |= (uint64_t)((c >> q) & 1u) << b;
    }
}

// one 64-row word of a pair: the five counts added to c[] (di / hi / ai: dip, het and homalt of sample i)
SVJG_HD void qc_pair_word(uint64_t di, uint64_t hi, uint64_t ai, uint64_t dj, uint64_t hj, uint64_t aj, uint32_t *c) {
    const uint64_t ri = di & ~hi & ~ai, rj = dj & ~hj & ~aj;
    c[0] += (uint32_t)__builtin_popcountll(di & dj);
    c[1] += (uint32_t)__builtin_popcountll(hi & dj);
    c[2] += (uint32_t)__builtin_popcountll(di & hj);
    c[3] += (uint32_t)__builtin_popcountll(hi & hj);
    c[4] += (uint32_t)__builtin_popcountll((ri & aj) | (ai & rj));
}

// k_qc_planes keeps the three planes k_qc_pairs reads (dip, het, homalt; plane p of QC_DIP + p), word-major: planes[(p * n_words + w) * S + s], so
// that the lanes of a wave (consecutive samples) write, and the pair kernel's staging reads, consecutive words.
constexpr uint32_t QC_PLANES = 3;
SVJG_HD uint64_t qc_plane_at(uint32_t p, uint64_t w, uint64_t s, uint64_t n_words, uint64_t S) { return ((uint64_t)p * n_words + w) * S + s; }
// a lane of k_qc_planes takes QC_PLANE_WORDS consecutive words of one sample (a "unit": unit u = chunk u / S, sample u % S) and adds its six
// popcounts to sample[] once per unit
constexpr uint32_t QC_PLANE_WORDS = 2;
constexpr uint64_t qc_plane_units(uint64_t n_words, uint64_t S) { return (n_words + QC_PLANE_WORDS - 1) / QC_PLANE_WORDS * S; }

// k_qc_pairs: a block of four waves takes a tile of QC_TI x QC_TJ samples (i x j) of the upper triangle.  Lane l of wave v owns the QC_RI pairs
// (i0 + v QC_RI + a, j0 + l), a = 0..QC_RI - 1: a register tile of QC_RI x 5 counters.  The row words go through LDS QC_STAGE_WORDS at a time, as
// uint64 slot e of [ i-side: plane p, word w, sample x of QC_TI | j-side: the same of QC_TJ ], sample fastest: a wave's 64-bit reads of the j-side
// are 64 consecutive slots (banks 2 l, 2 l + 1 within a 32-lane group: no conflict), its reads of the i-side one slot (a broadcast).
constexpr uint32_t QC_TI = 32, QC_TJ = 64, QC_WAVES = 4, QC_RI = QC_TI / QC_WAVES, QC_STAGE_WORDS = 16;
constexpr uint32_t QC_LDS_I = QC_PLANES * QC_STAGE_WORDS * QC_TI, QC_LDS_SLOTS = QC_LDS_I + QC_PLANES * QC_STAGE_WORDS * QC_TJ;    // 36 864 bytes
SVJG_HD uint32_t qc_lds_i(uint32_t p, uint32_t w, uint32_t x) { return (p * QC_STAGE_WORDS + w) * QC_TI + x; }
SVJG_HD uint32_t qc_lds_j(uint32_t p, uint32_t w, uint32_t x) { return QC_LDS_I + (p * QC_STAGE_WORDS + w) * QC_TJ + x; }
// what slot e holds in the stage that begins at word w0 of the tile at samples i0, j0: 0 for a sample at or beyond S or a word at or beyond n_words
SVJG_HD uint64_t qc_stage_word(const uint64_t *planes, uint32_t e, uint32_t i0, uint32_t j0, uint64_t w0, uint64_t n_words, uint32_t S) {
    const bool jside = e >= QC_LDS_I;
    const uint32_t f = jside ? e - QC_LDS_I : e, width = jside ? QC_TJ : QC_TI;
    const uint32_t x = f % width, pw = f / width, w = pw % QC_STAGE_WORDS, p = pw / QC_STAGE_WORDS;
    const uint32_t s = (jside ? j0 : i0) + x;
    return s < S && w0 + w < n_words ? planes[qc_plane_at(p, w0 + w, s, n_words, S)] : 0ull;
}
// The tiles of the upper triangle, i-tile by i-tile: i runs over 0..S - 2, so there are ceil((S - 1) / QC_TI) i-tiles, and the i-tile at i0 needs the
// j-tiles that hold a j > i0: from (i0 + 1) / QC_TJ on.  Tile t -> (ti, tj) by walking the i-tiles (at most 64 steps: bounded by S alone).
SVJG_HD uint32_t qc_tiles_i(uint32_t S) { return S < 2 ? 0u : (S - 1 + QC_TI - 1) / QC_TI; }
SVJG_HD uint32_t qc_tiles_j(uint32_t S) { return (S + QC_TJ - 1) / QC_TJ; }
SVJG_HD uint32_t qc_tile_first_j(uint32_t ti) { return (ti * QC_TI + 1) / QC_TJ; }
SVJG_HD uint32_t qc_tiles(uint32_t S) {
    uint32_t n = 0;
    for (uint32_t ti = 0; ti < qc_tiles_i(S); ++ti) n += qc_tiles_j(S) - qc_tile_first_j(ti);
    return n;
}
SVJG_HD void qc_tile_at(uint32_t t, uint32_t S, uint32_t &ti, uint32_t &tj) {         // t < qc_tiles(S)
    const uint32_t ni = qc_tiles_i(S), nj = qc_tiles_j(S);
    for (ti = 0; ti + 1 < ni; ++ti) {
        const uint32_t n = nj - qc_tile_first_j(ti);
        if (t < n) break;
        t -= n;
    }
    tj = qc_tile_first_j(ti) + t;
}

// ---- cohort site test for Hardy-Weinberg equilibrium (k_cohort_hwe) ----
// Item (r, s) enters iff it is a called diploid item (the dip predicate of qc_class).  Per row n_ref, n_het, n_alt = the entering items with g = 0,
// 1, 2 and n their sum; nA = 2 n_alt + n_het, nB = 2 n_ref + n_het, m = min(nA, nB).  For every h = m mod 2, + 2, .., m with a = (m - h) / 2 and
// b = (2 n - m - h) / 2 the weight is w(h) = 2^h n! / (a! h! b!) (Wigginton et al. 2005).  HWE = sum of w(h) over the h with
// w(h) <= (1 + 1e-7) w(n_het), over the sum of all; EXCHET = the same with h >= n_het.  m = 0: both 1.0; n = 0: both NaN.  On the device
// u(h) = log10 w(h) - log10 n! = h log10 2 - log10 a! - log10 h! - log10 b! in double-double from the log10(i!) table (entries 0..n), every term is
// 10^(u(h) - u(h0)) with h0 = the h of right parity next to nA nB / (2 n - 1), the mean of h: near the mode, so one pass is enough and a term that
// underflows against it is 0, rightly.  The tie rule is decided on the double-double u(h) - u(n_het) against log10(1 + 1e-7).  Compiled without
// fused multiply-adds, so the host harness (tests/geno_sim, topic hwe) and the kernel differ in exp10 and in the table's log10 only.
constexpr uint32_t HWE_MAX_SAMPLES = 65536;
// log10 2 = HWE_L2_0 + HWE_L2_1 + HWE_L2_2, the first two of 30 and 29 significant bits: h times either is exact for every h <= 2^17
constexpr double HWE_L2_0 = 0x1.34413508p-2, HWE_L2_1 = 0x1.f79fef3p-34, HWE_L2_2 = 0x1.1f12b35816f92p-66;
constexpr double HWE_TIE_HI = 0x1.750e5c9d09872p-25, HWE_TIE_LO = 0x1.ea2bc03de8dp-80;       // log10(1 + 1e-7)

// the three counts of an item added to a lane's (integer registers)
SVJG_HD void hwe_count(uint32_t g, uint32_t P, uint32_t &n_ref, uint32_t &n_het, uint32_t &n_alt) {
    const uint32_t c = qc_class(g, P), dip = (c >> QC_DIP) & 1u, het = (c >> QC_HET) & 1u, alt = (c >> QC_HOMALT) & 1u;
    n_het += het; n_alt += alt; n_ref += dip - het - alt;
}

// what the test of a row needs of its counts: terms = the number of h (0: no test, n = 0 or m = 0), h = par + 2 t for t < terms
struct HweRow { uint32_t n, m, par, het, h0, terms; };
SVJG_HD HweRow hwe_row(uint32_t n_ref, uint32_t n_het, uint32_t n_alt) {
    HweRow r{};
    r.n = n_ref + n_het + n_alt; r.het = n_het;
    const uint32_t nA = 2 * n_alt + n_het, nB = 2 * n_ref + n_het;
    r.m = nA < nB ? nA : nB; r.par = r.m & 1u;
    if (r.m == 0) return r;                              // (n = 0 too)
    uint32_t h0 = (uint32_t)((uint64_t)nA * nB / (2ull * r.n - 1));      // <= m, as max(nA, nB) <= 2 n - 1 where m >= 1
    if ((h0 ^ r.m) & 1u) ++h0;                           // (h0 = m has m's parity: never beyond m)
    r.h0 = h0; r.terms = (r.m - r.par) / 2 + 1;
    return r;
}

SVJG_HD dd hwe_h_log2(uint32_t h) {                      // h log10 2, h <= 2^17
#ifdef __clang__
#pragma clang fp contract(off)                           // the two exact products are rounded (not at all) before the exact sum
#endif
    const double x = (double)h, p0 = x * HWE_L2_0, p1 = x * HWE_L2_1, p2 = x * HWE_L2_2;
    dd s = two_sum(p0, p1);
    s.lo += p2;
    return two_sum(s.hi, s.lo);
}
// u(h) of a row; h has m's parity and h <= m: a, h, b <= n index the table
SVJG_HD dd hwe_log_weight(const dd *logfact, uint32_t n, uint32_t m, uint32_t h) {
    const uint32_t a = (m - h) / 2, b = n - h - a;
    return dd_add(hwe_h_log2(h), dd_neg(dd_add(dd_add(logfact[a], logfact[h]), logfact[b])));
}
// term t of a row added to a lane's three sums: all, selected by the tie rule, h >= n_het; u0 = u(h0), uhet = u(n_het)
struct HweSums { double all, sel, exc; };
SVJG_HD void hwe_term(const dd *logfact, const HweRow &r, dd u0, dd uhet, uint32_t t, HweSums &s) {
#ifdef __clang__
#pragma clang fp contract(off)
#endif
    const uint32_t h = r.par + 2 * t;
    const dd u = hwe_log_weight(logfact, r.n, r.m, h), d = dd_add(u, dd_neg(u0));
    const double x = prior_exp10(d.hi + d.lo);
    s.all += x;
    if (dd_cmp(dd_add(u, dd_neg(uhet)), dd{HWE_TIE_HI, HWE_TIE_LO}) <= 0) s.sel += x;
    if (h >= r.het) s.exc += x;
}
// a row's HWE or EXCHET from its reduced sums: min(1, part / all) (all >= 1: the term of h0 is 10^0); 1.0 where m = 0, NaN where n = 0
SVJG_HD double hwe_p(const HweRow &r, double part, double all) {
    if (r.n == 0) return NAN;
    if (r.m == 0) return 1.0;
    const double p = part / all;
    return p < 1.0 ? p : 1.0;
}

// ---- host side of a k_genotype launch: the table's size and where a call's rows lie, in plain integers (pinned without a GPU: tests/test_rows_layout.py) ----

// entries of the log10(i!) table: the first one built; the one that holds max_n (the largest n the kernel met beyond the table, < LOGFACT_CAP) with room to spare
constexpr uint32_t logfact_first() { return 65536; }
constexpr uint32_t logfact_grow_to(uint32_t max_n) { return max_n < LOGFACT_CAP - 1024 ? max_n + 1 + 1024 : LOGFACT_CAP; }
// entries a build for `upto` makes: capped, then whole blocks of the table kernels (LOGFACT_BLOCK = LF_BLOCK of svjg_kernels.h)
constexpr uint32_t LOGFACT_BLOCK = 1024;
constexpr uint32_t logfact_built(uint32_t upto) { return ((upto > LOGFACT_CAP ? LOGFACT_CAP : upto) + LOGFACT_BLOCK - 1) / LOGFACT_BLOCK * LOGFACT_BLOCK; }
// svjg_logfact_reserve: the table has `have` entries (0: none yet) and `entries` are asked for -> the size to build, 0: nothing to do (never a smaller table)
constexpr uint32_t logfact_reserve_to(uint32_t have, uint32_t entries) { return logfact_built(entries) > have ? logfact_built(entries) : 0; }

// the three input arrays of n rows, back to back from byte `at` of a block: [ slot 4 | type 1 | ok 1 ] x n
struct RowsIn { uint64_t slot, type, ok, bytes; };
inline RowsIn rows_in(uint64_t n, uint64_t at = 0) { return RowsIn{at, at + n * 4, at + n * 5, n * 6}; }
// the input arrays of a call that takes the run's calls (svjg_cohort_qc, svjg_cohort_hwe), back to back from byte `at` of a block: [ gt 1 ] x n_rows * S and, per_item, as many
// ploidy bytes (ploidy 0: no array); such a call's layout IS a CallsIn as it is a LegSpan.  stage_calls: the call's arrays, n bytes each, into the block (host; tests/geno_sim too)
struct CallsIn { uint64_t gt, ploidy, bytes; };
inline CallsIn calls_in(uint64_t n_rows, uint64_t S, bool per_item, uint64_t at = 0) { const uint64_t n = n_rows * S; return CallsIn{at, per_item ? at + n : 0, per_item ? 2 * n : n}; }
inline void stage_calls(uint8_t *hb, const CallsIn &I, const uint8_t *gt, const uint8_t *ploidy, uint64_t n) { memcpy(hb + I.gt, gt, n); if (ploidy) memcpy(hb + I.ploidy, ploidy, n); }

// The eleven step-by-step calls (svjg_genotype / _view, _ploidy, _sites, _cohort, _cohort_ploidy, _cohort_prior, _cohort_sites, _cohort_sites_prior, svjg_cohort_qual, svjg_cohort_qc, svjg_cohort_hwe) each own one device block and its pinned host twin, all of ONE
// shape: the outputs (they end at out_end), the max_n pair 8-aligned, ONE contiguous input region right behind the pair, 64 spare bytes -> ONE copy
// in (in_bytes from in_at), ONE copy out (maxn + 8 bytes from 0).  A layout below IS a LegSpan and adds only what is its own: its outputs and where its inputs lie.
struct LegSpan { uint64_t maxn, in_at, in_bytes, total; };
inline void leg_span(LegSpan &S, uint64_t out_end, uint64_t in_bytes) {
    S.maxn = (out_end + 7) & ~7ull; S.in_at = S.maxn + 8; S.in_bytes = in_bytes; S.total = S.in_at + in_bytes + 64;
}

// svjg_genotype, svjg_genotype_view, svjg_genotype_boundary: [ pl 24 | raw 8 | gt 1 | flags 1 | boundary 1 ] x n of output (flags: a row's
// `genotyped` byte); in: rows_in(n)
struct RowsLayout : LegSpan { uint64_t pl, raw, gt, flags, boundary;  RowsIn in; };
inline RowsLayout rows_layout(uint64_t n) {
    RowsLayout L; uint64_t o = 0;
    L.pl = o; o += n * 24; L.raw = o; o += n * 8; L.gt = o; o += n; L.flags = o; o += n; L.boundary = o; o += n;
    leg_span(L, o, n * 6); L.in = rows_in(n, L.in_at);
    return L;
}

// svjg_genotype_ploidy: [ pl 72 | raw 8 | gt 1 | flags 1 | boundary 1 ] x n; in: the call's logarithms (ploidy_log_table), rows_in(n) and the
// ploidy bytes
struct PloidyLayout : LegSpan { uint64_t pl, raw, gt, flags, boundary, logtab;  RowsIn in;  uint64_t ploidy; };
inline PloidyLayout ploidy_layout(uint64_t n) {
    PloidyLayout L; uint64_t o = 0;
    L.pl = o; o += n * 8 * (MAX_PLOIDY + 1); L.raw = o; o += n * 8; L.gt = o; o += n; L.flags = o; o += n; L.boundary = o; o += n;
    leg_span(L, o, 2 * PLOIDY_TAB * 8 + n * 7);
    L.logtab = L.in_at; L.in = rows_in(n, L.logtab + 2 * PLOIDY_TAB * 8); L.ploidy = L.in.slot + L.in.bytes;
    return L;
}

// svjg_genotype_sites (S = 1, not cohort): [ pl 224 | raw 28 | gt 2 | boundary 1 ] x n_sites.  svjg_genotype_cohort_sites (cohort): [ pl 224 | raw 28 |
// gt 2 | members 1 | boundary 1 ] x (n_sites * S items, site-major: 256 bytes an item), then the site words, 8-aligned, as the LAST output:
// MAX_SITE_ALTS words a site, NS_j | AC_j << 32; the max_n pair lies right behind them, and ONE memset zeroes both in front of every launch (as
// cohort_layout).  svjg_genotype_cohort_sites_prior (cohort and prior): k_cohort_sites_prior's own outputs [ sgt 2 | sgq 1 ] x items behind the
// boundary bytes and, 8-aligned, [ af 56 | psite 48 (NS_j, AC_j) | steps 4 ] x sites in front of the first kernel's site words, which stay the
// LAST output.  in, all: the call's logarithms (site_log_table) and the sites' slots.  A field the call does not have is 0.
struct SitesLayout : LegSpan { uint64_t pl, raw, gt, members, boundary, site, logs, slots, sgt, sgq, af, psite, steps; };
inline SitesLayout sites_layout(uint64_t n_sites, uint64_t S = 1, bool cohort = false, bool prior = false) {
    SitesLayout L{}; uint64_t o = 0; const uint64_t n = n_sites * S;
    L.pl = o; o += n * 8 * SITE_GENOTYPES; L.raw = o; o += n * 4 * (MAX_SITE_ALTS + 1); L.gt = o; o += n * 2;
    if (cohort) { L.members = o; o += n; }
    L.boundary = o; o += n;
    if (cohort && prior) { L.sgt = o; o += n * 2; L.sgq = o; o += n; }
    if (cohort) o = (o + 7) & ~7ull;
    if (cohort && prior) { L.af = o; o += n_sites * 8 * SITE_ALLELES; L.psite = o; o += n_sites * 8 * MAX_SITE_ALTS; L.steps = o; o += n_sites * 4; o = (o + 7) & ~7ull; }
    if (cohort) { L.site = o; o += n_sites * 8 * MAX_SITE_ALTS; }
    leg_span(L, o, SITE_LOGS * 8 + n_sites * 4 * MAX_SITE_ALTS);
    L.logs = L.in_at; L.slots = L.logs + SITE_LOGS * 8;
    return L;
}

// svjg_genotype_cohort (max_ploidy 2, neither switch), _cohort_ploidy (per_item) and _cohort_prior (prior; per_item iff it has a ploidy array):
// [ pl 8 (max_ploidy + 1) | raw 8 | gt 1 | flags 1 | boundary 1 ] x (n_rows * S items, row-major) — the PL stride is the CALL's, not MAX_PLOIDY + 1:
// a human cohort moves 24 bytes of PLs per item —; prior: k_cohort_prior's own outputs [ gq 1 ] x items and, 8-aligned, [ af 8 | psite 12 (NS, AN,
// AC) | steps 4 ] x rows (it writes the posterior call over gt); then the first kernel's site words, 8-aligned, as the LAST output: NS | AC << 32
// per row, per_item a second one, AN.  The max_n pair lies right behind them (a multiple of 8: leg_span pads nothing), and ONE memset zeroes both
// in front of every launch.  in: the call's logarithms (ploidy_log_table) iff per_item or prior, rows_in(n_rows), per_item the n_rows * S ploidy
// bytes.  A field the call does not have is 0 (ploidy: where the bytes would begin).
struct CohortLayout : LegSpan { uint64_t pl, raw, gt, flags, boundary, gq, af, psite, steps, site, logtab;  RowsIn in;  uint64_t ploidy; };
inline CohortLayout cohort_layout(uint64_t n_rows, uint64_t S, uint32_t max_ploidy = 2, bool per_item = false, bool prior = false) {
    CohortLayout L{}; uint64_t o = 0; const uint64_t n = n_rows * S, logs = per_item || prior ? 2 * PLOIDY_TAB * 8 : 0;
    L.pl = o; o += n * 8 * (max_ploidy + 1); L.raw = o; o += n * 8; L.gt = o; o += n; L.flags = o; o += n; L.boundary = o; o += n;
    if (prior) { L.gq = o; o += n; }
    o = (o + 7) & ~7ull;
    if (prior) { L.af = o; o += n_rows * 8; L.psite = o; o += n_rows * 12; L.steps = o; o += n_rows * 4; }
    L.site = o; o += n_rows * (per_item ? 16 : 8);
    leg_span(L, o, logs + n_rows * 6 + (per_item ? n : 0));
    L.logtab = logs ? L.in_at : 0; L.in = rows_in(n_rows, L.in_at + logs); L.ploidy = L.in.slot + L.in.bytes;
    return L;
}

// svjg_cohort_qual: [ qual 8 | mlac 4 | chroms 4 ] x n_rows of output; in: the call's logarithms (ploidy_log_table), H_0..H_m_max
// (qual_harmonic), rows_in(n_rows) and, per_item, the n_rows * S ploidy bytes
struct QualLayout : LegSpan { uint64_t qual, mlac, chroms, logtab, harm;  RowsIn in;  uint64_t ploidy; };
inline QualLayout qual_layout(uint64_t n_rows, uint64_t S, uint32_t m_max, bool per_item) {
    QualLayout L{}; uint64_t o = 0; const uint64_t logs = 2 * PLOIDY_TAB * 8, harm = ((uint64_t)m_max + 1) * 8;
    L.qual = o; o += n_rows * 8; L.mlac = o; o += n_rows * 4; L.chroms = o; o += n_rows * 4;
    leg_span(L, o, logs + harm + n_rows * 6 + (per_item ? n_rows * S : 0));
    L.logtab = L.in_at; L.harm = L.logtab + logs; L.in = rows_in(n_rows, L.harm + harm); L.ploidy = L.in.slot + L.in.bytes;
    return L;
}

// svjg_cohort_qc: [ pair 20 ] x S (S - 1) / 2 of output, then, 8-aligned, [ sample 24 ] x S as the LAST output: the max_n pair lies right behind
// it (a multiple of 8: leg_span pads nothing), and ONE memset zeroes both in front of every launch (k_qc_planes adds to sample[]; the pair is never
// written: the call reads no table and names no slot).  in: calls_in(n_rows, S, per_item).  Behind the inputs,
// 8-aligned and never copied: the QC_PLANES planes of qc_words(n_rows) * S words, written by k_qc_planes and read by k_qc_pairs.
struct QcLayout : LegSpan, CallsIn { uint64_t pair, sample, planes; };
inline QcLayout qc_layout(uint64_t n_rows, uint64_t S, bool per_item) {
    QcLayout L{}; uint64_t o = 0;
    L.pair = o; o += qc_pairs(S) * 4 * QC_PAIR_COUNTS; o = (o + 7) & ~7ull;
    L.sample = o; o += S * 4 * QC_CLASSES;
    leg_span(L, o, calls_in(n_rows, S, per_item).bytes); static_cast<CallsIn &>(L) = calls_in(n_rows, S, per_item, L.in_at);
    L.planes = (L.in_at + L.in_bytes + 7) & ~7ull;
    L.total = L.planes + QC_PLANES * qc_words(n_rows) * S * 8 + 64;
    return L;
}

// svjg_cohort_hwe: [ p 16 ] x n_rows (HWE, EXCHET), then [ counts 12 ] x n_rows (n_ref, n_het, n_alt) of output; the max_n pair is zeroed in front
// of every launch and never written (the call reserves the table entries it reads before it launches).  in: calls_in(n_rows, S, per_item).
struct HweLayout : LegSpan, CallsIn { uint64_t p, counts; };
inline HweLayout hwe_layout(uint64_t n_rows, uint64_t S, bool per_item) {
    HweLayout L{}; L.p = 0; L.counts = n_rows * 16;
    leg_span(L, L.counts + n_rows * 12, calls_in(n_rows, S, per_item).bytes); static_cast<CallsIn &>(L) = calls_in(n_rows, S, per_item, L.in_at);
    return L;
}

// fused pass (svjg_set_rows, svjg_run_begin, svjg_run_end), per slot.  Host block (pinned, mapped into the device: the genotype kernel
// writes its results straight into it — they cross PCIe as they are produced, no copy kernel competes with the next pass —): pl32, raw,
// gt, flags, boundary, then the tail; device block: the tail (max_n, the pass's status block, the guard words: written by atomics, copied
// to the host block's tail in one small copy), pl64.  The inputs: one rows_in(n) at offset 0 of a block all slots share.
struct RunLayout { uint64_t pl32, raw, gt, flags, boundary, h_tail, out_bytes;  uint64_t maxn, status, guard, tail_bytes, pl64, total; };
inline RunLayout run_layout(uint64_t n) {
    RunLayout L; uint64_t o = 0;
    L.pl32 = o; o += n * 12; L.raw = o; o += n * 8; L.gt = o; o += n; L.flags = o; o += n; L.boundary = o; o += n; o = (o + 63) & ~63ull; L.h_tail = o;
    uint64_t d = 0;
    L.maxn = d; d += 8; L.status = d; d += (sizeof(DevStatus) + 7) & ~7ull; L.guard = d; d += GUARD_WORDS * 8; L.tail_bytes = d;
    L.out_bytes = L.h_tail + L.tail_bytes;
    d = (d + 63) & ~63ull; L.pl64 = d; d += n * 24; L.total = d + 64;
    return L;
}

}  // namespace svjg
