// The cohort site test for Hardy-Weinberg equilibrium (svjg_geno.h: hwe_count, hwe_row, hwe_log_weight, hwe_term, hwe_p are the kernel's own code)
// inside a plain C++ restatement of k_cohort_hwe's loops over blocks, waves, segments and lanes (svjg_kernels.h), the lane order of the xor
// butterfly included (geno_sim.cpp: butterfly), in a block laid out by hwe_layout, with the log10(i!) table of the host's libm.  Topic `hwe` of the
// stand-alone program runs seeded random calls against a brute-force count and a recurrence in long double.

extern "C" void genosim_hwe_constants(uint32_t *out) {
    const uint32_t v[3] = {HWE_MAX_SAMPLES, SIM_TPB, HWE_BLOCKS_PER_CU};
    memcpy(out, v, sizeof v);
}
extern "C" void genosim_hwe_row(uint32_t n_ref, uint32_t n_het, uint32_t n_alt, uint32_t *out) {
    const HweRow r = hwe_row(n_ref, n_het, n_alt);
    const uint32_t v[6] = {r.n, r.m, r.par, r.het, r.h0, r.terms};
    memcpy(out, v, sizeof v);
}

// The kernel over a call with a grid of `grid` blocks (0: what launch_cohort_hwe takes on n_cu units).  -> 0, or a code: 1 a store outside its
// field, 2 an output word written twice or never, 3 a table entry read beyond the reserved ones, 4 the lanes of a segment disagree.
extern "C" int genosim_hwe_run(const uint8_t *gt, const uint8_t *ploidy, uint64_t n_rows, uint32_t S32, uint32_t grid, uint32_t n_cu, uint32_t *counts, double *p) {
    const uint64_t S = S32, n = n_rows * S;
    const HweLayout L = hwe_layout(n_rows, S, ploidy != nullptr);
    std::vector<uint64_t> block = poisoned_block(L.total);
    uint8_t *base = (uint8_t *)block.data();
    stage_calls(base, L, gt, ploidy, n);
    memset(base + L.maxn, 0, 8);                                               // the launch's memset
    const uint8_t *d_gt = base + L.gt, *d_ploidy = ploidy ? base + L.ploidy : nullptr;
    uint32_t *d_counts = (uint32_t *)(base + L.counts);
    double *d_p = (double *)(base + L.p);
    if (L.p != 0 || L.counts != n_rows * 16 || L.counts + n_rows * 12 > L.maxn || L.in_at != L.maxn + 8 || L.in_at + L.in_bytes + 64 != L.total) return 1;
    const uint32_t tab_n = 2 * S32 + 1;                                         // what svjg_cohort_hwe reserves
    std::vector<dd> tab(tab_n);
    host_logfact(tab.data(), tab_n);
    std::vector<uint8_t> written(n_rows * 5, 0);                                // 3 count words and 2 doubles a row

    const uint32_t W = prior_segment_width(S), rows_per_wave = 64u / W;
    const uint64_t n_waves = (n_rows + rows_per_wave - 1) / rows_per_wave;
    const uint64_t blocks = grid ? grid : segment_grid(n_rows, S, SIM_TPB, n_cu ? n_cu : 256, HWE_BLOCKS_PER_CU);
    const uint64_t grid_waves = blocks * SIM_TPB / 64;
    for (uint64_t first = 0; first < grid_waves; ++first)
        for (uint64_t wv = first; wv < n_waves; wv += grid_waves) {
            uint32_t c[3][64]; double s[3][64]; HweRow row[64];
            for (uint32_t lane = 0; lane < 64; ++lane) {
                const uint32_t j = lane & (W - 1), sub = lane / W;
                const uint64_t r = wv * rows_per_wave + sub;
                c[0][lane] = c[1][lane] = c[2][lane] = 0;
                if (r < n_rows)
                    for (uint64_t at = j; at < S; at += W) hwe_count(d_gt[r * S + at], d_ploidy ? d_ploidy[r * S + at] : 2u, c[0][lane], c[1][lane], c[2][lane]);
            }
            for (auto &x : c) butterfly<1>(x, 64, W);
            for (uint32_t lane = 0; lane < 64; ++lane) {
                const uint32_t j = lane & (W - 1);
                row[lane] = hwe_row(c[0][lane], c[1][lane], c[2][lane]);
                HweSums sum{0.0, 0.0, 0.0};
                if (row[lane].terms) {
                    if (row[lane].n >= tab_n) return 3;
                    const dd u0 = hwe_log_weight(tab.data(), row[lane].n, row[lane].m, row[lane].h0), uhet = hwe_log_weight(tab.data(), row[lane].n, row[lane].m, row[lane].het);
                    for (uint32_t t = j; t < row[lane].terms; t += W) hwe_term(tab.data(), row[lane], u0, uhet, t, sum);
                }
                s[0][lane] = sum.all; s[1][lane] = sum.sel; s[2][lane] = sum.exc;
            }
            for (auto &x : s) butterfly<1>(x, 64, W);
            for (uint32_t lane = 0; lane < 64; ++lane) {
                const uint32_t j = lane & (W - 1), sub = lane / W, l0 = lane - j;
                const uint64_t r = wv * rows_per_wave + sub;
                if (memcmp(&s[0][lane], &s[0][l0], 8) || memcmp(&s[1][lane], &s[1][l0], 8) || memcmp(&s[2][lane], &s[2][l0], 8) || c[0][lane] != c[0][l0]) return 4;
                if (!(r < n_rows && j == 0)) continue;
                for (uint32_t k = 0; k < 5; ++k) if (written[r * 5 + k]++) return 2;
                for (uint32_t k = 0; k < 3; ++k) d_counts[r * 3 + k] = c[k][lane];
                d_p[r * 2] = hwe_p(row[lane], s[1][lane], s[0][lane]); d_p[r * 2 + 1] = hwe_p(row[lane], s[2][lane], s[0][lane]);
            }
        }
    for (uint8_t w : written) if (w != 1) return 2;
    if (!maxn_stayed_zero(base, L.maxn)) return 1;
    memcpy(counts, d_counts, n_rows * 12);
    memcpy(p, d_p, n_rows * 16);
    return 0;
}

#ifdef GENO_SIM_MAIN
// the definitions item by item, and the weights by their recurrence in long double from the largest one down and up (Wigginton's own order)
static int hwe_brute(const std::vector<uint8_t> &gt, const uint8_t *ploidy, uint64_t R, uint32_t S, const std::vector<uint32_t> &counts, const std::vector<double> &p) {
    for (uint64_t r = 0; r < R; ++r) {
        uint32_t want[3] = {};
        for (uint32_t s = 0; s < S; ++s) {
            const uint32_t g = gt[r * S + s], P = ploidy ? ploidy[r * S + s] : 2u;
            if (P == 2 && g <= 2) ++want[g];
        }
        if (memcmp(want, &counts[r * 3], sizeof want)) return 1;
        const uint32_t n = want[0] + want[1] + want[2], nA = 2 * want[2] + want[1], nB = 2 * want[0] + want[1], m = nA < nB ? nA : nB;
        if (n == 0) { if (p[r * 2] == p[r * 2] || p[r * 2 + 1] == p[r * 2 + 1]) return 2; continue; }
        if (m == 0) { if (p[r * 2] != 1.0 || p[r * 2 + 1] != 1.0) return 2; continue; }
        std::vector<long double> w(m + 1, 0.0L);
        uint32_t mid = (uint32_t)((uint64_t)nA * nB / (2ull * n));
        if ((mid ^ m) & 1u) ++mid;
        if (mid > m) mid -= 2;
        w[mid] = 1.0L;
        for (uint32_t h = mid; h >= 2; h -= 2) {
            const long double a = (m - h) / 2, b = n - h - (m - h) / 2;
            w[h - 2] = w[h] * h * (h - 1.0L) / (4.0L * (a + 1.0L) * (b + 1.0L));
        }
        for (uint32_t h = mid; h + 2 <= m; h += 2) {
            const long double a = (m - h) / 2, b = n - h - (m - h) / 2;
            w[h + 2] = w[h] * 4.0L * a * b / ((h + 2.0L) * (h + 1.0L));
        }
        long double all = 0, sel = 0, exc = 0;
        bool edge = false;
        for (uint32_t h = m & 1u; h <= m; h += 2) {
            all += w[h];
            const long double ratio = w[h] / w[want[1]];
            if (ratio > 1.0L + 0.9e-7L && ratio < 1.0L + 1.1e-7L) edge = true;
            if (ratio <= 1.0L + 1e-7L) sel += w[h];
            if (h >= want[1]) exc += w[h];
        }
        const long double hw = sel / all < 1 ? sel / all : 1, ex = exc / all < 1 ? exc / all : 1;
        if (!edge && hw >= 1e-280L && !(fabsl(p[r * 2] - hw) <= 1e-9L * hw)) return 3;
        if (ex >= 1e-280L && !(fabsl(p[r * 2 + 1] - ex) <= 1e-9L * ex)) return 3;
    }
    return 0;
}

static int main_hwe() {
    const uint32_t sizes[] = {1, 2, 3, 5, 31, 32, 33, 63, 64, 65, 130, 193, 400};
    const uint64_t rows[] = {1, 3, 65, 130};
    int cases = 0;
    for (uint32_t S : sizes)
        for (uint64_t R : rows)
            for (int mode = 0; mode < 3; ++mode) {           // no ploidy array, all 2, mixed 0..8
                std::vector<uint8_t> gt(R * S), pl(R * S);
                for (uint64_t r = 0; r < R; ++r) {
                    const uint32_t f = 1 + rnd() % 50;       // a row's allele frequency in percent
                    for (uint32_t s = 0; s < S; ++s) {
                        const uint32_t v = rnd() % 40;
                        gt[r * S + s] = v == 0 ? 0xFF : v == 1 ? 3 : v == 2 ? 7 : (uint8_t)((rnd() % 100 < f) + (rnd() % 100 < f));
                    }
                }
                for (auto &q : pl) q = mode == 1 ? 2 : (uint8_t)(rnd() % 4 ? 2 : rnd() % 9);
                std::vector<uint32_t> counts(R * 3);
                std::vector<double> p(R * 2);
                const uint8_t *ploidy = mode ? pl.data() : nullptr;
                const int rc = genosim_hwe_run(gt.data(), ploidy, R, S, cases % 2 ? 1 : 0, 256, counts.data(), p.data());
                if (rc) { fprintf(stderr, "hwe_sim: code %d at S %u rows %llu mode %d\n", rc, S, (unsigned long long)R, mode); return 1; }
                const int bad = hwe_brute(gt, ploidy, R, S, counts, p);
                if (bad) { fprintf(stderr, "hwe_sim: %s at S %u rows %llu mode %d\n", bad == 1 ? "counts differ" : bad == 2 ? "a row without a test is wrong" : "p differs", S, (unsigned long long)R, mode); return 1; }
                ++cases;
            }
    printf("hwe_sim ok: %d cases\n", cases);
    return 0;
}
#endif
