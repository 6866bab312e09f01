// The pieces of the cohort genotype leg that are plain integers (svjg_geno.h: cohort_segment, what the cohort kernels mask their ballots with;
// cohort_diploid_sums and cohort_ploidy_sums, what k_genotype_cohort turns its three ballots into and k_genotype_cohort_ploidy its nine).  Topic
// `cohort` of the stand-alone program checks every wave of 3 * 64 * S items against the brute-force segments and sums, and the layouts.

// the 64 lanes of the wave whose first item is w0, for n_rows x S items: mask[lane], leader[lane]
extern "C" void genosim_cohort_wave(uint64_t w0, uint64_t S, uint64_t n_items, uint64_t *mask, uint8_t *leader) {
    for (uint32_t lane = 0; lane < 64; ++lane) {
        const uint64_t i = w0 + lane;
        const CohortSeg g = cohort_segment(i, i % S, S, lane, n_items);
        mask[lane] = g.mask; leader[lane] = g.leader;
    }
}

// The wave whose first item is w0, of n_items items of S samples a row; gt[i] (alt copies, 0xFF: no call) and ploidy[i] per ITEM, or ploidy == NULL:
// the diploid kernel (gt 0 / 1 / 2, 3: no call; its three ballots called / het / hom).  The ballots are formed as the kernel forms them (a lane
// beyond the last item votes "no call", ploidy 0), then for every lane: leader[lane], and the segment's sums ns / an /
// ac[lane] and the first site word as the leader would add them (0 where the lane is no leader).
extern "C" void genosim_cohort_sums(uint64_t w0, uint64_t S, uint64_t n_items, const uint8_t *gt, const uint8_t *ploidy,
                                    uint8_t *leader, uint32_t *ns, uint32_t *an, uint32_t *ac, uint64_t *word) {
    CohortBallots b{};
    uint64_t het = 0, hom = 0;
    for (uint32_t lane = 0; lane < 64; ++lane) {
        const uint64_t i = w0 + lane;
        const uint32_t g = i < n_items ? gt[i] : (ploidy ? 0xFF : 3), P = i < n_items && ploidy ? ploidy[i] : 0;
        if (g != (ploidy ? 0xFF : 3)) b.called |= 1ull << lane;
        if (g == 1) het |= 1ull << lane;
        if (g == 2) hom |= 1ull << lane;
        for (uint32_t k = 0; k < 4; ++k) {
            if ((g >> k) & 1u) b.gt[k] |= 1ull << lane;
            if ((P >> k) & 1u) b.ploidy[k] |= 1ull << lane;
        }
    }
    for (uint32_t lane = 0; lane < 64; ++lane) {
        const uint64_t i = w0 + lane;
        const CohortSeg seg = cohort_segment(i, i % S, S, lane, n_items);
        leader[lane] = seg.leader; ns[lane] = an[lane] = ac[lane] = 0; word[lane] = 0;
        if (!seg.leader) continue;
        const CohortSums t = ploidy ? cohort_ploidy_sums(b, seg.mask) : cohort_diploid_sums(b.called, het, hom, seg.mask);
        ns[lane] = t.ns; an[lane] = t.an; ac[lane] = t.ac; word[lane] = cohort_site_word(t);
    }
}

#ifdef GENO_SIM_MAIN
static int main_cohort() {
    const uint64_t sizes[8] = {1, 2, 3, 31, 63, 64, 65, 130};
    uint64_t waves = 0, bad = 0, x = 88172645463325252ull;
    for (uint64_t S : sizes) {
        const uint64_t full = 3 * 64 * S;
        // whole rows, ending inside a wave or not; the diploid kernel's three ballots, then the nine
        for (uint64_t n_items : {full, full - S, (full / S / 2) * S + S}) for (int per_item = 0; per_item < 2; ++per_item) {
            const uint8_t no_call = per_item ? 0xFF : 3;
            std::vector<uint8_t> gt(n_items), pld(n_items);
            for (uint64_t i = 0; i < n_items; ++i) {
                x ^= x << 13; x ^= x >> 7; x ^= x << 17;
                pld[i] = per_item ? (uint8_t)(x % 9) : 2;
                const uint32_t g = (uint32_t)((x >> 20) % (per_item ? 10 : 4));
                gt[i] = per_item && g == 9 ? 0xFF : (uint8_t)g;                   // (gt above the ploidy is fine here: the sums are plain sums)
            }
            std::vector<uint64_t> row_ns(n_items / S, 0), row_an(n_items / S, 0), row_ac(n_items / S, 0), row_word(n_items / S, 0);
            for (uint64_t w0 = 0; w0 < n_items; w0 += 64) {
                uint64_t mask[64]; uint8_t seg_leader[64];
                genosim_cohort_wave(w0, S, n_items, mask, seg_leader);
                uint8_t leader[64]; uint32_t ns[64], an[64], ac[64]; uint64_t word[64];
                genosim_cohort_sums(w0, S, n_items, gt.data(), per_item ? pld.data() : nullptr, leader, ns, an, ac, word);
                ++waves;
                for (uint32_t lane = 0; lane < 64; ++lane) {
                    const uint64_t i = w0 + lane;
                    uint64_t want = 0; uint32_t first = 64;
                    if (i < n_items)
                        for (uint32_t l = 0; l < 64; ++l)
                            if (w0 + l < n_items && (w0 + l) / S == i / S) { want |= 1ull << l; if (first == 64) first = l; }
                    if (mask[lane] != want || seg_leader[lane] != (i < n_items && first == lane) || leader[lane] != seg_leader[lane]) ++bad;
                    if (leader[lane]) { const uint64_t r = i / S; row_ns[r] += ns[lane]; row_an[r] += an[lane]; row_ac[r] += ac[lane]; row_word[r] += word[lane]; }
                }
            }
            for (uint64_t r = 0; r < n_items / S; ++r) {
                uint64_t wn = 0, wa = 0, wc = 0;
                for (uint64_t s = 0; s < S; ++s)
                    if (gt[r * S + s] != no_call) { ++wn; wa += pld[r * S + s]; wc += gt[r * S + s]; }
                if (wn != row_ns[r] || wa != row_an[r] || wc != row_ac[r] || row_word[r] != (wn | wc << 32)) ++bad;
            }
        }
    }
    for (uint64_t n_rows : {1, 7, 1000}) for (uint64_t S : {1, 3, 64, 65}) for (uint32_t mp : {1u, 2u, 8u}) for (int per : {0, 1}) for (int prior : {0, 1}) {
        uint64_t L[19];
        layout_at(LAYOUT_COHORT, n_rows, S, mp, per | prior << 1, L);
        const uint64_t logs = per || prior ? 720 : 0;
        if (L[9] % 8 || L[6] % 8 || L[10] != L[9] + (per ? 16 : 8) * n_rows || L[11] != L[10] + 8 || L[13] != L[11] + logs ||
            L[16] != L[13] + 6 * n_rows || L[18] != logs + 6 * n_rows + (per ? n_rows * S : 0)) ++bad;
    }
    printf("cohort_sim %s: %llu waves, %llu lanes, rows or layouts differ\n", bad ? "FAILED" : "ok", (unsigned long long)waves, (unsigned long long)bad);
    return bad ? 1 : 0;
}
#endif
