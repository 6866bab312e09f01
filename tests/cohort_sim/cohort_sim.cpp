// TEST HARNESS ONLY (never shipped, never loaded by the product): the two pieces of the cohort genotype leg that are plain integers
// (svjg_geno.h: cohort_segment, what k_genotype_cohort masks its ballots with, and cohort_layout) compiled with g++.  With
// -DCOHORT_SIM_MAIN it is a stand-alone program (for -fsanitize=address,undefined) that checks every wave of the first 3 * 64 * S items
// against the brute-force segments.
#define SVJG_HD inline
#include "../../svjedi-graph_amd/csrc/svjg_geno.h"
#include <stdio.h>
#include <initializer_list>

using namespace svjg;

// the 64 lanes of the wave whose first item is w0, for n_rows x S items: mask[lane], leader[lane]
extern "C" void cohortsim_wave(uint64_t w0, uint64_t S, uint64_t n_items, uint64_t *mask, uint8_t *leader) {
    for (uint32_t lane = 0; lane < 64; ++lane) {
        const uint64_t i = w0 + lane;
        const CohortSeg g = cohort_segment(i, i % S, S, lane, n_items);
        mask[lane] = g.mask; leader[lane] = g.leader;
    }
}

// cohort_layout(n_rows, S) -> out[12]: pl, raw, gt, flags, boundary, site, maxn, slot, type, ok, in_bytes, total
extern "C" void cohortsim_layout(uint64_t n_rows, uint64_t S, uint64_t *out) {
    const CohortLayout L = cohort_layout(n_rows, S);
    const uint64_t v[12] = {L.pl, L.raw, L.gt, L.flags, L.boundary, L.site, L.maxn, L.in.slot, L.in.type, L.in.ok, L.in.bytes, L.total};
    for (int i = 0; i < 12; ++i) out[i] = v[i];
}

#ifdef COHORT_SIM_MAIN
int main() {
    const uint64_t sizes[8] = {1, 2, 3, 31, 63, 64, 65, 130};
    uint64_t waves = 0, bad = 0;
    for (uint64_t S : sizes) {
        const uint64_t full = 3 * 64 * S;
        for (uint64_t n_items : {full, full - S, (full / S / 2) * S + S}) {           // whole rows, ending inside a wave or not
            for (uint64_t w0 = 0; w0 < n_items; w0 += 64) {
                uint64_t mask[64]; uint8_t leader[64];
                cohortsim_wave(w0, S, n_items, mask, leader);
                ++waves;
                for (uint32_t lane = 0; lane < 64; ++lane) {
                    const uint64_t i = w0 + lane;
                    uint64_t want = 0; uint32_t first = 64;
                    if (i < n_items)
                        for (uint32_t l = 0; l < 64; ++l)
                            if (w0 + l < n_items && (w0 + l) / S == i / S) { want |= 1ull << l; if (first == 64) first = l; }
                    if (mask[lane] != want || leader[lane] != (i < n_items && first == lane)) ++bad;
                }
            }
        }
    }
    printf("cohort_sim %s: %llu waves, %llu lanes differ\n", bad ? "FAILED" : "ok", (unsigned long long)waves, (unsigned long long)bad);
    return bad ? 1 : 0;
}
#endif
