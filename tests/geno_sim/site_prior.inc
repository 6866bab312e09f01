// The routines of svjg_geno.h behind k_cohort_sites_prior (site_prior_load, site_prior_expected, site_prior_step, site_prior_call).  A site's EM
// runs sequentially over its samples (wave = 0) or with every step's sums in the kernel's order (wave = 1: geno_sim.cpp: wave_sum).  Topic
// `site_prior` of the stand-alone program runs seeded sites with every array at exactly its size.

// One site of S samples: raw[S][7], members[S] as the first kernel left them, slots[6] (only which are named matters) -> p[7] (NaN: no estimate),
// *steps (the kernel's word), sgt[S][2] (member numbering), sgq[S], psite[6][2] = NS_j, AC_j.
extern "C" void genosim_site_prior_site(int wave, const uint32_t *raw, const uint8_t *members, const uint32_t *slots, uint64_t S, double err, uint32_t min_support,
                                        double *p, uint32_t *steps, uint8_t *sgt, uint8_t *sgq, uint32_t *psite) {
    double logs[SITE_LOGS];
    site_log_table(err, logs);
    const uint32_t C = site_candidates(slots);
    std::vector<double> w(S * SITE_GENOTYPES);
    std::vector<SitePriorMeta> meta(S);
    uint32_t n = 0;
    for (uint64_t s = 0; s < S; ++s) {
        site_prior_load(raw + s * SITE_ALLELES, members[s], logs, w.data() + s * SITE_GENOTYPES, 1, meta[s]);
        n += meta[s].part;
    }
    SitePriorSite st = site_prior_start(C, n);
    while (!st.done) {
        double x[SITE_ALLELES];
        if (wave)
            wave_sum<SITE_ALLELES>(S, [&](uint64_t s, double *v) { site_prior_expected(w.data() + s * SITE_GENOTYPES, 1, meta[s], st.p, v); }, x);
        else {
            for (uint32_t a = 0; a < SITE_ALLELES; ++a) x[a] = 0.0;
            for (uint64_t s = 0; s < S; ++s) site_prior_expected(w.data() + s * SITE_GENOTYPES, 1, meta[s], st.p, x);
        }
        site_prior_step(st, x, n);
    }
    for (uint32_t j = 0; j < 2 * MAX_SITE_ALTS; ++j) psite[j] = 0;
    for (uint64_t s = 0; s < S; ++s) {
        const SitePriorCall k = site_prior_call(w.data() + s * SITE_GENOTYPES, 1, meta[s], st.p, min_support);
        sgt[s * 2] = k.a; sgt[s * 2 + 1] = k.b; sgq[s] = k.gq;
        for (uint32_t j = 0; j < MAX_SITE_ALTS; ++j) {
            const uint32_t c = site_candidate_copies(meta[s].members, k.a, k.b, j);
            if (c != SITE_NO_CALL) { ++psite[j * 2]; psite[j * 2 + 1] += c; }
        }
    }
    for (uint32_t a = 0; a < SITE_ALLELES; ++a) p[a] = st.p[a];
    *steps = st.steps;
}

// n sites of S samples each, back to back
extern "C" void genosim_site_prior_sites(int wave, const uint32_t *raw, const uint8_t *members, const uint32_t *slots, uint64_t n, uint64_t S, double err, uint32_t min_support,
                                         double *p, uint32_t *steps, uint8_t *sgt, uint8_t *sgq, uint32_t *psite) {
    for (uint64_t k = 0; k < n; ++k)
        genosim_site_prior_site(wave, raw + k * S * SITE_ALLELES, members + k * S, slots + k * MAX_SITE_ALTS, S, err, min_support,
                                p + k * SITE_ALLELES, steps + k, sgt + k * S * 2, sgq + k * S, psite + k * 2 * MAX_SITE_ALTS);
}

// the weights of one item in candidate order: w[28] at the given stride (a test may hand in a strided array), -> takes part; *top, *N
extern "C" uint32_t genosim_site_prior_item(const uint32_t *raw, uint32_t members, double err, double *w, uint32_t stride, uint32_t *top, double *N) {
    double logs[SITE_LOGS];
    site_log_table(err, logs);
    SitePriorMeta m;
    site_prior_load(raw, members, logs, w, stride, m);
    *top = m.top; *N = m.N;
    return m.part;
}

// geno_site's likelihoods in member numbering (what the factored site_lik returns for a site of K members): hi[28], lo[28], 0 beyond the site's
extern "C" void genosim_site_prior_lik(uint32_t K, uint32_t ref, const uint32_t *alt, double err, double *hi, double *lo) {
    double logs[SITE_LOGS], c[SITE_ALLELES];
    site_log_table(err, logs);
    c[0] = (double)ref; double N = c[0];
    for (uint32_t j = 1; j <= MAX_SITE_ALTS; ++j) { c[j] = j <= K ? (double)alt[j - 1] * 0.5 : 0.0; N += c[j]; }
    for (uint32_t b = 0; b <= MAX_SITE_ALTS; ++b)
        for (uint32_t a = 0; a <= b; ++a) {
            const dd l = b <= K ? site_lik(c, N, a, b, logs[0], logs[K], logs[8 + K]) : dd{0.0, 0.0};
            hi[b * (b + 1) / 2 + a] = l.hi; lo[b * (b + 1) / 2 + a] = l.lo;
        }
}

#ifdef GENO_SIM_MAIN
static int main_site_prior() {
    const uint64_t sizes[] = {1, 2, 3, 8, 9, 63, 64, 65, 130};
    uint64_t sites = 0, bad = 0, x = 88172645463325252ull;
    auto next = [&] { x ^= x << 13; x ^= x >> 7; x ^= x << 17; return x; };
    for (uint64_t S : sizes)
        for (int mode = 0; mode < 3; ++mode)                                          // shallow, deep (weights underflow), sparse presence
            for (int k = 0; k < 30; ++k) {
                const uint32_t C = 2 + (uint32_t)(next() % 5);
                std::vector<uint32_t> raw(S * SITE_ALLELES), slots(MAX_SITE_ALTS);
                std::vector<uint8_t> members(S), sgt(S * 2), sgq(S), sgt2(S * 2), sgq2(S);
                for (uint32_t j = 0; j < MAX_SITE_ALTS; ++j) slots[j] = j < C ? j : SITE_NO_SLOT;
                for (uint64_t s = 0; s < S; ++s) {
                    uint32_t m = 0;
                    for (uint32_t j = 0; j < C; ++j) if (next() % 10 < (mode == 2 ? 4u : 9u)) m |= 1u << j;
                    const uint32_t K = (uint32_t)__builtin_popcount(m);
                    members[s] = (uint8_t)m;
                    for (uint32_t t = 0; t < SITE_ALLELES; ++t) raw[s * SITE_ALLELES + t] = K >= 2 && t <= K ? (uint32_t)(next() % (mode == 1 ? 60001 : next() % 3 ? 61 : 3)) : 0u;
                }
                double p[SITE_ALLELES], p2[SITE_ALLELES]; uint32_t steps, steps2, ps[2 * MAX_SITE_ALTS], ps2[2 * MAX_SITE_ALTS];
                const uint32_t ms = k & 1 ? 3 : 0;
                genosim_site_prior_site(0, raw.data(), members.data(), slots.data(), S, 5e-5, ms, p, &steps, sgt.data(), sgq.data(), ps);
                genosim_site_prior_site(1, raw.data(), members.data(), slots.data(), S, 5e-5, ms, p2, &steps2, sgt2.data(), sgq2.data(), ps2);
                ++sites;
                uint32_t part = 0, ns[MAX_SITE_ALTS] = {0}, ac[MAX_SITE_ALTS] = {0};
                for (uint64_t s = 0; s < S; ++s) {
                    const uint32_t K = (uint32_t)__builtin_popcount(members[s]);
                    bool reads = false;
                    for (uint32_t t = 0; t < SITE_ALLELES; ++t) reads |= raw[s * SITE_ALLELES + t] != 0;
                    if (K >= 2 && reads) ++part;
                    const uint8_t a = sgt2[s * 2], b = sgt2[s * 2 + 1];
                    if (a == SITE_NO_CALL) { if (b != SITE_NO_CALL || sgq2[s] != 0xFF) ++bad; }
                    else if (!(a <= b && b <= K && sgq2[s] <= 99 && K >= 2 && reads)) ++bad;
                    for (uint32_t j = 0; j < MAX_SITE_ALTS; ++j) { const uint32_t c = site_candidate_copies(members[s], a, b, j); if (c != SITE_NO_CALL) { ++ns[j]; ac[j] += c; } }
                }
                for (uint32_t j = 0; j < MAX_SITE_ALTS; ++j) if (ns[j] != ps2[j * 2] || ac[j] != ps2[j * 2 + 1]) ++bad;
                double sum = 0.0, sum2 = 0.0;
                for (uint32_t a = 0; a < SITE_ALLELES; ++a) {
                    sum += p[a]; sum2 += p2[a];
                    if (part ? !(p[a] >= 0.0 && p[a] <= 1.0 && p2[a] >= 0.0 && p2[a] <= 1.0 && fabs(p[a] - p2[a]) < 1e-9 && (a <= C || (p[a] == 0.0 && p2[a] == 0.0))) : !(p[a] != p[a] && p2[a] != p2[a])) ++bad;
                }
                if (part ? !(fabs(sum - 1.0) < 1e-12 && fabs(sum2 - 1.0) < 1e-12 && (steps & ~EM_NOT_CONVERGED) >= 1 && (steps & ~EM_NOT_CONVERGED) <= EM_MAX_IT && (steps2 & ~EM_NOT_CONVERGED) >= 1)
                         : (steps || steps2)) ++bad;
            }
    for (uint64_t n : {1, 7, 1000}) for (uint64_t S : {1, 3, 64, 65}) {
        uint64_t a[17], b[17];
        layout_at(LAYOUT_SITES, n, S, 0, 1 | 4, a); layout_at(LAYOUT_SITES, n, S, 0, 1 | 8, b);
        if (a[7] % 8 || a[8] % 8 || a[10] % 8 || a[11] != a[10] + n * 48 || a[5] != b[4] + n * S || b[5] || b[7] || a[12] != a[11] + 8) ++bad;
    }
    printf("site_prior_sim %s: %llu sites, %llu checks failed\n", bad ? "FAILED" : "ok", (unsigned long long)sites, (unsigned long long)bad);
    return bad ? 1 : 0;
}
#endif
