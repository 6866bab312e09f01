// The genotype row arithmetic at any ploidy (svjg_geno.h: geno_row_ploidy, what k_genotype_ploidy runs per lane) driven row by row.  Topic
// `ploidy` of the stand-alone program runs a seeded random set through it, beside geno_row for the diploid comparison.

// the 2 x 45 logarithms of a call (svjg_geno.h: ploidy_log_table)
extern "C" void genosim_ploidy_log_table(double err, double *tab) { ploidy_log_table(err, tab); }

// geno_row_ploidy over rows of (type, ref, alt, ploidy in 1..8) -> gt (alt copies, 0xFF no call), pl[n * 9], near, status (GENO_ROW_*)
extern "C" void genosim_ploidy_rows(const uint8_t *type, const uint32_t *cnt, const uint8_t *ploidy, uint64_t n_rows, uint32_t min_support, double err,
                                    const dd *tab, uint32_t tab_n, uint8_t *gt, int64_t *pl, uint8_t *near, uint8_t *status) {
    double lt[2 * PLOIDY_TAB];
    ploidy_log_table(err, lt);
    for (uint64_t r = 0; r < n_rows; ++r) {
        GenoRowPloidy o;
        status[r] = (uint8_t)geno_row_ploidy(type[r], cnt[r * 2], cnt[r * 2 + 1], ploidy[r], min_support, lt, lt + PLOIDY_TAB, tab, tab_n, o);
        gt[r] = o.gt; near[r] = o.near;
        for (uint32_t i = 0; i <= MAX_PLOIDY; ++i) pl[r * (MAX_PLOIDY + 1) + i] = o.pl[i];
    }
}

#ifdef GENO_SIM_MAIN
static int main_ploidy() {
    const uint32_t tab_n = 1u << 21;                     // beyond it: rows answer GENO_ROW_GROW and touch no entry
    std::vector<dd> tab(tab_n);
    genosim_logfact(tab.data(), tab_n);
    const uint64_t n = 200000;
    std::vector<uint8_t> type(n), ploidy(n), gt(n), near(n), st(n);
    std::vector<uint32_t> cnt(n * 2);
    std::vector<int64_t> pl(n * (MAX_PLOIDY + 1)), pl3(n * 3);
    uint64_t x = 0x9E3779B97F4A7C15ull;
    auto rnd = [&x]() { x ^= x << 13; x ^= x >> 7; x ^= x << 17; return x; };
    for (uint64_t r = 0; r < n; ++r) {
        type[r] = (uint8_t)(rnd() % 4); ploidy[r] = (uint8_t)(1 + rnd() % MAX_PLOIDY);
        const uint64_t k = rnd() % 20;
        const uint32_t top = k == 0 ? 0xFFFFFFFFu : k < 3 ? 1000000u : 60u;
        cnt[r * 2] = (uint32_t)(rnd() % ((uint64_t)top + 1)); cnt[r * 2 + 1] = (uint32_t)(rnd() % ((uint64_t)top + 1));
    }
    uint64_t sum = 0, flagged = 0, grow = 0, host = 0;
    const double errs[3] = {5e-5, 1e-2, 0.3};
    for (double e : errs)
        for (uint32_t ms : {0u, 3u}) {
            genosim_ploidy_rows(type.data(), cnt.data(), ploidy.data(), n, ms, e, tab.data(), tab_n, gt.data(), pl.data(), near.data(), st.data());
            for (uint64_t r = 0; r < n; ++r) { sum += gt[r]; flagged += near[r]; grow += st[r] == GENO_ROW_GROW; host += st[r] == GENO_ROW_HOST; for (uint32_t i = 0; i <= MAX_PLOIDY; ++i) sum += (uint64_t)pl[r * 9 + i]; }
            const double l_ok = log10(1.0 - e), l_err = log10(e), l_half = log10(1.0 / 2.0);
            for (uint64_t r = 0; r < n; ++r) {                                     // geno_row (the diploid routine) over the same rows
                GenoRow o;
                st[r] = (uint8_t)geno_row(type[r], cnt[r * 2], cnt[r * 2 + 1], ms, l_ok, l_err, l_half, tab.data(), tab_n, o);
                gt[r] = o.gt; near[r] = o.near;
                for (int i = 0; i < 3; ++i) pl3[r * 3 + i] = o.pl[i];
            }
            for (uint64_t r = 0; r < n; ++r) sum += gt[r] + (uint64_t)pl3[r * 3];
        }
    printf("ploidy_sim ok: %llu rows x 6 settings, checksum %llx, %llu flagged, %llu beyond the table, %llu for the host\n",
           (unsigned long long)n, (unsigned long long)sum, (unsigned long long)flagged, (unsigned long long)grow, (unsigned long long)host);
    return 0;
}
#endif
