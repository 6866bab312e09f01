// The per-item routines of the cohort call with an allele-frequency prior (svjg_geno.h: prior_load, prior_expected, prior_call, prior_step,
// prior_segment_width), and a row's EM run sequentially over its samples (genosim_prior_row) or with every step's sum in the kernel's order
// (genosim_prior_row_wave: lanes, strides, butterfly).  Topic `prior` of the stand-alone program runs random rows and checks what holds without a
// model.

// One row of S samples: raw[S][2], done[S], ploidy[S] or NULL (2 everywhere) -> *f (NaN: no estimate), *steps (the kernel's word: bit 31 = not
// converged), gt[S], gq[S], site[3] = NS, AN, AC.  wave: a step's x are summed in k_cohort_prior's order (genosim_prior_row_wave), else sample after sample
static void row_em(bool wave, uint32_t sv_type, const uint32_t *raw, const uint8_t *done, const uint8_t *ploidy, uint64_t S, double err, uint32_t min_support,
                   double *f, uint32_t *steps, uint8_t *gt, uint8_t *gq, uint32_t *site) {
    double tab[2 * PLOIDY_TAB];
    ploidy_log_table(err, tab);
    const uint8_t t8 = (uint8_t)sv_type, *type = &t8;
    uint32_t sum_p = 0;
    for (uint64_t s = 0; s < S; ++s) { PriorItem it; double c; prior_load(type, raw, done, ploidy, s, tab, c, it); sum_p += it.P; }
    PriorRow row = prior_row_start(sum_p);
    while (!row.done) {
        double x = 0.0;
        if (wave)
            wave_sum<1>(S, [&](uint64_t s, double *v) { PriorItem it; double c; prior_load(type, raw, done, ploidy, s, tab, c, it); *v += prior_expected(it, row.f); }, &x);
        else
            for (uint64_t s = 0; s < S; ++s) { PriorItem it; double c; prior_load(type, raw, done, ploidy, s, tab, c, it); x += prior_expected(it, row.f); }
        prior_step(row, x, sum_p);
    }
    site[0] = site[1] = site[2] = 0;
    for (uint64_t s = 0; s < S; ++s) {
        PriorItem it; double c;
        prior_load(type, raw, done, ploidy, s, tab, c, it);
        const PriorCall k = prior_call(it, row.f, c, min_support);
        gt[s] = k.gt; gq[s] = k.gq;
        if (k.gt != 0xFF) { ++site[0]; site[1] += it.P; site[2] += k.gt; }
    }
    *f = row.f; *steps = row.steps;
}

extern "C" void genosim_prior_row(uint32_t sv_type, const uint32_t *raw, const uint8_t *done, const uint8_t *ploidy, uint64_t S, double err, uint32_t min_support,
                                  double *f, uint32_t *steps, uint8_t *gt, uint8_t *gq, uint32_t *site) {
    row_em(false, sv_type, raw, done, ploidy, S, err, min_support, f, steps, gt, gq, site);
}

// The same row with every step's sum in the kernel's order (geno_sim.cpp: wave_sum).  The kernel differs from this in exp10 and log10 only.
extern "C" void genosim_prior_row_wave(uint32_t sv_type, const uint32_t *raw, const uint8_t *done, const uint8_t *ploidy, uint64_t S, double err, uint32_t min_support,
                                       double *f, uint32_t *steps, uint8_t *gt, uint8_t *gq, uint32_t *site) {
    row_em(true, sv_type, raw, done, ploidy, S, err, min_support, f, steps, gt, gq, site);
}

// the weights of one item: w[9] = C(P, g) 10^d_g, -> the item's ploidy as the EM sees it (0: it takes no part); *gmax
extern "C" uint32_t genosim_prior_item(uint32_t sv_type, uint32_t ref, uint32_t alt, uint32_t P, double err, double *w, uint32_t *gmax) {
    double tab[2 * PLOIDY_TAB];
    ploidy_log_table(err, tab);
    const uint32_t raw[2] = {ref, alt}; const uint8_t done = 1, p = (uint8_t)P, t8 = (uint8_t)sv_type, *type = &t8;
    PriorItem it; double c;
    prior_load(type, raw, &done, &p, 0, tab, c, it);
    for (uint32_t g = 0; g <= MAX_PLOIDY; ++g) w[g] = it.w[g];
    *gmax = it.gmax;
    return it.P;
}

extern "C" uint32_t genosim_prior_width(uint64_t S) { return prior_segment_width(S); }
extern "C" uint32_t genosim_segment_grid(uint64_t n_rows, uint64_t S, uint32_t tpb, uint32_t n_cu, uint32_t blocks_per_cu) { return segment_grid(n_rows, S, tpb, n_cu, blocks_per_cu); }
// the EM's constants, those of the site prior (site_prior.inc) among them
extern "C" void genosim_prior_constants(double *tol, uint32_t *max_it, uint32_t *flag_bit, double *f_bound, double *p_bound) {
    *tol = EM_TOL; *max_it = EM_MAX_IT; *flag_bit = EM_NOT_CONVERGED; *f_bound = EM_F_BOUND; *p_bound = SITE_EM_P_BOUND;
}

#ifdef GENO_SIM_MAIN
static int main_prior() {
    const uint64_t sizes[21] = {1, 2, 3, 4, 5, 8, 9, 16, 17, 31, 32, 33, 63, 64, 65, 130, 192, 193, 256, 257, 320};
    uint64_t rows = 0, bad = 0, x = 88172645463325252ull;
    auto next = [&] { x ^= x << 13; x ^= x >> 7; x ^= x << 17; return x; };
    for (uint64_t S : sizes)
        for (int mode = 0; mode < 3; ++mode)                                          // diploid, mixed ploidy 0..8, deep counts
            for (int k = 0; k < 40; ++k) {
                std::vector<uint32_t> raw(S * 2); std::vector<uint8_t> done(S), pld(S), gt(S), gq(S), gt2(S), gq2(S);
                for (uint64_t s = 0; s < S; ++s) {
                    const uint64_t v = next();
                    raw[s * 2] = (uint32_t)(v % (mode == 2 ? 5001 : (v >> 40) % 3 ? 61 : 5)); raw[s * 2 + 1] = (uint32_t)((v >> 16) % ((v >> 44) % 3 ? 61 : 5));
                    done[s] = (v >> 32) % 5 != 0; pld[s] = (uint8_t)((v >> 36) % 9);
                }
                double f, f2; uint32_t steps, steps2, site[3], site2[3];
                const uint32_t type = (uint32_t)(next() % 4), ms = k & 1 ? 3 : 0;
                genosim_prior_row(type, raw.data(), done.data(), mode == 1 ? pld.data() : nullptr, S, 5e-5, ms, &f, &steps, gt.data(), gq.data(), site);
                genosim_prior_row(type, raw.data(), done.data(), mode == 1 ? pld.data() : nullptr, S, 5e-5, ms, &f2, &steps2, gt2.data(), gq2.data(), site2);
                // the kernel's order of the sums: what holds of any order (the model decides the rest: tests/test_cohort_prior.py)
                std::vector<uint8_t> gt3(S), gq3(S); double f3; uint32_t steps3, site3[3];
                genosim_prior_row_wave(type, raw.data(), done.data(), mode == 1 ? pld.data() : nullptr, S, 5e-5, ms, &f3, &steps3, gt3.data(), gq3.data(), site3);
                uint32_t ns3 = 0, ac3 = 0;
                for (uint64_t s = 0; s < S; ++s) { if (gt3[s] != 0xFF) { ++ns3; ac3 += gt3[s]; if (gq3[s] > 99) ++bad; } else if (gq3[s] != 0xFF) ++bad; }
                if (ns3 != site3[0] || ac3 != site3[2] || (f != f) != (f3 != f3) || (f3 == f3 && !(f3 >= 0.0 && f3 <= 1.0 && steps3 && (steps3 & ~EM_NOT_CONVERGED) <= EM_MAX_IT))
                    || (f3 != f3 && steps3)) ++bad;
                ++rows;
                uint32_t ns = 0, an = 0, ac = 0, part = 0;
                for (uint64_t s = 0; s < S; ++s) {
                    const uint32_t P = done[s] ? (mode == 1 ? pld[s] : 2u) : 0u;
                    if (P && raw[s * 2] + raw[s * 2 + 1]) ++part;
                    if (gt[s] != 0xFF) { ++ns; an += P; ac += gt[s]; if (gt[s] > P || gq[s] > 99 || !P) ++bad; } else if (gq[s] != 0xFF) ++bad;
                    if (gt[s] != gt2[s] || gq[s] != gq2[s]) ++bad;
                }
                if (ns != site[0] || an != site[1] || ac != site[2] || steps != steps2 || site[0] != site2[0]) ++bad;
                if (part ? !(f >= 0.0 && f <= 1.0 && f == f2 && (steps & ~EM_NOT_CONVERGED) >= 1 && (steps & ~EM_NOT_CONVERGED) <= EM_MAX_IT) : !(f != f && steps == 0)) ++bad;
            }
    for (uint64_t n_rows : {1, 7, 1000}) for (uint64_t S : {1, 3, 64, 65}) for (uint32_t mp : {1u, 2u, 8u}) for (int per : {0, 1}) {
        uint64_t L[19];
        layout_at(LAYOUT_COHORT, n_rows, S, mp, per | 2, L);
        if (L[9] % 8 || L[6] % 8 || L[10] != L[9] + (per ? 16 : 8) * n_rows || L[11] != L[10] + 8 || L[13] + 6 * n_rows + (per ? n_rows * S : 0) != L[11] + L[18]) ++bad;
    }
    for (uint64_t S : sizes) { const uint32_t w = genosim_prior_width(S); if (w < (S < 64 ? S : 64) || w > 64 || (w & (w - 1)) || (w > 1 && w / 2 >= (S < 64 ? S : 64))) ++bad; }
    printf("cohort_prior_sim %s: %llu rows, %llu checks failed\n", bad ? "FAILED" : "ok", (unsigned long long)rows, (unsigned long long)bad);
    return bad ? 1 : 0;
}
#endif
