// TEST HARNESS ONLY (never shipped, never loaded by the product): the joint arithmetic for insertions that share a position (svjg_geno.h:
// geno_site, what k_genotype_sites runs per lane) compiled with g++ and driven site by site.  With -DSITE_SIM_MAIN it is a stand-alone
// program (for -fsanitize=address,undefined) that runs a seeded random set.
#define SVJG_HD inline
#include "../../svjedi-graph_amd/csrc/svjg_geno.h"
#include <math.h>
#include <stdio.h>
#include <vector>

using namespace svjg;

// log10(i!) for i < n with the HOST libm's log10, summed in order in double-double (as tests/hostsim does)
extern "C" void sitesim_logfact(dd *tab, uint32_t n) {
    dd run{0.0, 0.0};
    for (uint32_t i = 0; i < n; ++i) { if (i >= 2) run = dd_add(run, dd{log10((double)i), 0.0}); tab[i] = run; }
}

// the SITE_LOGS logarithms of a call (svjg_geno.h: site_log_table)
extern "C" void sitesim_log_table(double err, double *tab) { site_log_table(err, tab); }

// geno_site over sites of (K in 2..6, ref, alt[6]) -> gt[n * 2] (0xFF, 0xFF: no call), pl[n * 28], near, status (GENO_ROW_*), n = s_K
extern "C" void sitesim_genotype(const uint8_t *K, const uint32_t *ref, const uint32_t *alt, uint64_t n_sites, uint32_t min_support, double err,
                                 const dd *tab, uint32_t tab_n, uint8_t *gt, int64_t *pl, uint8_t *near, uint8_t *status, uint64_t *n_out) {
    double lt[SITE_LOGS];
    site_log_table(err, lt);
    for (uint64_t s = 0; s < n_sites; ++s) {
        GenoSite o;
        status[s] = (uint8_t)geno_site(K[s], ref[s], alt + s * MAX_SITE_ALTS, min_support, lt[0], lt[K[s]], lt[8 + K[s]], tab, tab_n,
                                       pl + s * SITE_GENOTYPES, o);
        gt[s * 2] = o.a; gt[s * 2 + 1] = o.b; near[s] = o.near; n_out[s] = o.n;
    }
}

#ifdef SITE_SIM_MAIN
int main() {
    const uint32_t tab_n = 1u << 20;                     // beyond it: sites answer GENO_ROW_GROW / GENO_ROW_HOST and touch no entry
    std::vector<dd> tab(tab_n);
    sitesim_logfact(tab.data(), tab_n);
    const uint64_t n = 200000;
    std::vector<uint8_t> K(n), gt(n * 2), near(n), st(n);
    std::vector<uint32_t> ref(n), alt(n * MAX_SITE_ALTS);
    std::vector<int64_t> pl(n * SITE_GENOTYPES);
    std::vector<uint64_t> nn(n);
    uint64_t x = 0x9E3779B97F4A7C15ull;
    auto rnd = [&x]() { x ^= x << 13; x ^= x >> 7; x ^= x << 17; return x; };
    for (uint64_t s = 0; s < n; ++s) {
        K[s] = (uint8_t)(2 + rnd() % (MAX_SITE_ALTS - 1));
        const uint64_t k = rnd() % 20;
        const uint32_t top = k == 0 ? 0xFFFFFFFFu : k < 3 ? 1000000u : 60u;
        ref[s] = (uint32_t)(rnd() % ((uint64_t)top + 1));
        for (uint32_t j = 0; j < MAX_SITE_ALTS; ++j) alt[s * MAX_SITE_ALTS + j] = (uint32_t)(rnd() % ((uint64_t)top + 1));
    }
    uint64_t sum = 0, flagged = 0, grow = 0, host = 0;
    const double errs[3] = {5e-5, 1e-2, 0.3};
    for (double e : errs)
        for (uint32_t ms : {0u, 3u}) {
            sitesim_genotype(K.data(), ref.data(), alt.data(), n, ms, e, tab.data(), tab_n, gt.data(), pl.data(), near.data(), st.data(), nn.data());
            for (uint64_t s = 0; s < n; ++s) {
                sum += gt[s * 2] + gt[s * 2 + 1]; flagged += near[s]; grow += st[s] == GENO_ROW_GROW; host += st[s] == GENO_ROW_HOST;
                for (uint32_t i = 0; i < SITE_GENOTYPES; ++i) sum += (uint64_t)pl[s * SITE_GENOTYPES + i];
            }
        }
    printf("site_sim ok: %llu sites x 6 settings, checksum %llx, %llu flagged, %llu beyond the table, %llu for the host\n",
           (unsigned long long)n, (unsigned long long)sum, (unsigned long long)flagged, (unsigned long long)grow, (unsigned long long)host);
    return 0;
}
#endif
