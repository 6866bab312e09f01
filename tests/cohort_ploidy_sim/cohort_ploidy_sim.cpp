// TEST HARNESS ONLY (never shipped, never loaded by the product): the integer pieces of the cohort-at-per-sample-ploidy leg (svjg_geno.h:
// cohort_ploidy_sums, what k_genotype_cohort_ploidy turns its nine ballots into under cohort_segment's masks, and cohort_ploidy_layout) compiled
// with g++.  With -DCOHORT_PLOIDY_SIM_MAIN it is a stand-alone program (for -fsanitize=address,undefined) that checks every wave of 3 * 64 * S
// items against brute-force sums.
#define SVJG_HD inline
#include "../../svjedi-graph_amd/csrc/svjg_geno.h"
#include <stdio.h>
#include <initializer_list>

using namespace svjg;

// The wave whose first item is w0, of n_items items of S samples a row; gt[i] (alt copies, 0xFF: no call) and ploidy[i] per ITEM.  The ballots are
// formed as the kernel forms them (a lane beyond the last item votes gt = 0xFF, ploidy 0), then for every lane: leader[lane], and the segment's
// sums ns / an / ac[lane] and the first site word as the leader would add them (0 where the lane is no leader).
extern "C" void cpsim_wave(uint64_t w0, uint64_t S, uint64_t n_items, const uint8_t *gt, const uint8_t *ploidy,
                           uint8_t *leader, uint32_t *ns, uint32_t *an, uint32_t *ac, uint64_t *word) {
    CohortBallots b{};
    for (uint32_t lane = 0; lane < 64; ++lane) {
        const uint64_t i = w0 + lane;
        const uint32_t g = i < n_items ? gt[i] : 0xFF, P = i < n_items ? ploidy[i] : 0;
        if (g != 0xFF) b.called |= 1ull << lane;
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
        const CohortSums t = cohort_ploidy_sums(b, seg.mask);
        ns[lane] = t.ns; an[lane] = t.an; ac[lane] = t.ac; word[lane] = cohort_site_word(t);
    }
}

// cohort_ploidy_layout(n_rows, S, max_ploidy) -> out[14]: pl, raw, gt, flags, boundary, site, maxn, in_at, logtab, slot, type, ok, ploidy, total; out[14] = in_bytes
extern "C" void cpsim_layout(uint64_t n_rows, uint64_t S, uint32_t max_ploidy, uint64_t *out) {
    const CohortPloidyLayout L = cohort_ploidy_layout(n_rows, S, max_ploidy);
    const uint64_t v[15] = {L.pl, L.raw, L.gt, L.flags, L.boundary, L.site, L.maxn, L.in_at, L.logtab, L.in.slot, L.in.type, L.in.ok, L.ploidy, L.total, L.in_bytes};
    for (int i = 0; i < 15; ++i) out[i] = v[i];
}

#ifdef COHORT_PLOIDY_SIM_MAIN
#include <vector>
int main() {
    const uint64_t sizes[8] = {1, 2, 3, 31, 63, 64, 65, 130};
    uint64_t waves = 0, bad = 0, x = 88172645463325252ull;
    for (uint64_t S : sizes) {
        const uint64_t full = 3 * 64 * S;
        for (uint64_t n_items : {full, full - S, (full / S / 2) * S + S}) {           // whole rows, ending inside a wave or not
            std::vector<uint8_t> gt(n_items), pld(n_items);
            for (uint64_t i = 0; i < n_items; ++i) {
                x ^= x << 13; x ^= x >> 7; x ^= x << 17;
                pld[i] = (uint8_t)(x % 9);
                const uint32_t g = (uint32_t)((x >> 20) % 10);
                gt[i] = g == 9 ? 0xFF : (uint8_t)g;                                   // (gt above the ploidy is fine here: the sums are plain sums)
            }
            std::vector<uint64_t> row_ns(n_items / S, 0), row_an(n_items / S, 0), row_ac(n_items / S, 0);
            for (uint64_t w0 = 0; w0 < n_items; w0 += 64) {
                uint8_t leader[64]; uint32_t ns[64], an[64], ac[64]; uint64_t word[64];
                cpsim_wave(w0, S, n_items, gt.data(), pld.data(), leader, ns, an, ac, word);
                ++waves;
                for (uint32_t lane = 0; lane < 64; ++lane)
                    if (leader[lane]) { const uint64_t r = (w0 + lane) / S; row_ns[r] += ns[lane]; row_an[r] += an[lane]; row_ac[r] += ac[lane]; }
            }
            for (uint64_t r = 0; r < n_items / S; ++r) {
                uint64_t wn = 0, wa = 0, wc = 0;
                for (uint64_t s = 0; s < S; ++s)
                    if (gt[r * S + s] != 0xFF) { ++wn; wa += pld[r * S + s]; wc += gt[r * S + s]; }
                if (wn != row_ns[r] || wa != row_an[r] || wc != row_ac[r]) ++bad;
            }
        }
    }
    for (uint64_t n_rows : {1, 7, 1000}) for (uint64_t S : {1, 3, 64, 65}) for (uint32_t mp : {1u, 2u, 8u}) {
        uint64_t L[15];
        cpsim_layout(n_rows, S, mp, L);
        if (L[5] % 8 || L[6] != L[5] + 16 * n_rows || L[7] != L[6] + 8 || L[12] + n_rows * S != L[7] + L[14]) ++bad;
    }
    printf("cohort_ploidy_sim %s: %llu waves, %llu rows or layouts differ\n", bad ? "FAILED" : "ok", (unsigned long long)waves, (unsigned long long)bad);
    return bad ? 1 : 0;
}
#endif
