// TEST HARNESS ONLY (never shipped, never loaded by the product): the plain pieces of the cohort call for insertions that share a position
// (svjg_geno.h: site_compact, site_candidate_copies, cohort_site_member_sums under cohort_segment's masks, cohort_sites_layout, and geno_site behind
// the compaction, item by item as k_genotype_cohort_sites runs it per lane) compiled with g++.  With -DCOHORT_SITES_SIM_MAIN it is a stand-alone
// program (for -fsanitize=address,undefined) that checks the compaction of every presence pattern, every wave of 3 * 64 * S items against
// brute-force sums, and the layouts.
#define SVJG_HD inline
#include "../../svjedi-graph_amd/csrc/svjg_geno.h"
#include <stdio.h>
#include <initializer_list>

using namespace svjg;

// site_compact: bits, cref[6], calt[6] -> out[8] = K, ref, alt[0..6)
extern "C" void csitesim_compact(uint32_t bits, const uint32_t *cref, const uint32_t *calt, uint32_t *out) {
    SiteMembers m;
    site_compact(bits, cref, calt, m);
    out[0] = m.K; out[1] = m.ref;
    for (uint32_t t = 0; t < MAX_SITE_ALTS; ++t) out[2 + t] = m.alt[t];
}

// The wave whose first item is w0, of n_items items of S samples a site; members[i] and gt[i * 2..] per ITEM as the kernel leaves them (gt 0xFF,
// 0xFF: no site call).  The ballots are formed as the kernel forms them (a lane beyond the last item votes members 0, no call), then for every
// lane: leader[lane] and, per candidate j, ns / ac / word[lane * 6 + j] as the leader would add them (0 where the lane is no leader).
extern "C" void csitesim_sums(uint64_t w0, uint64_t S, uint64_t n_items, const uint8_t *members, const uint8_t *gt,
                              uint8_t *leader, uint32_t *ns, uint32_t *ac, uint64_t *word) {
    SiteBallots b{};
    for (uint32_t lane = 0; lane < 64; ++lane) {
        const uint64_t i = w0 + lane;
        const uint32_t mem = i < n_items ? members[i] : 0u, ga = i < n_items ? gt[i * 2] : SITE_NO_CALL, gb = i < n_items ? gt[i * 2 + 1] : SITE_NO_CALL;
        for (uint32_t j = 0; j < MAX_SITE_ALTS; ++j) {
            const uint32_t c = site_candidate_copies(mem, ga, gb, j);
            if (c != SITE_NO_CALL) b.in[j] |= 1ull << lane;
            if (c == 1u) b.one[j] |= 1ull << lane;
            if (c == 2u) b.two[j] |= 1ull << lane;
        }
    }
    for (uint32_t lane = 0; lane < 64; ++lane) {
        const uint64_t i = w0 + lane;
        const CohortSeg seg = cohort_segment(i, i % S, S, lane, n_items);
        leader[lane] = seg.leader;
        for (uint32_t j = 0; j < MAX_SITE_ALTS; ++j) {
            ns[lane * MAX_SITE_ALTS + j] = ac[lane * MAX_SITE_ALTS + j] = 0; word[lane * MAX_SITE_ALTS + j] = 0;
            if (!seg.leader) continue;
            const CohortSums t = cohort_site_member_sums(b, j, seg.mask);
            ns[lane * MAX_SITE_ALTS + j] = t.ns; ac[lane * MAX_SITE_ALTS + j] = t.ac; word[lane * MAX_SITE_ALTS + j] = cohort_site_word(t);
        }
    }
}

// Items as a lane of k_genotype_cohort_sites runs them: bits[i], cref / calt[i * 6..] (the candidates' raw counts; those of an absent candidate are
// not looked at) -> gt[i * 2..], pl[i * 28..], raw[i * 7..], near, status (GENO_ROW_*), n = s_K; K' < 2: 0xFF, 0xFF and zeros
extern "C" void csitesim_items(uint64_t n_items, const uint8_t *bits, const uint32_t *cref, const uint32_t *calt, uint32_t min_support, double err,
                               const dd *tab, uint32_t tab_n, uint8_t *gt, int64_t *pl, uint32_t *raw, uint8_t *near, uint8_t *status, uint64_t *n_out) {
    double lt[SITE_LOGS];
    site_log_table(err, lt);
    for (uint64_t i = 0; i < n_items; ++i) {
        SiteMembers m;
        site_compact(bits[i], cref + i * MAX_SITE_ALTS, calt + i * MAX_SITE_ALTS, m);
        const bool call = m.K >= 2;
        raw[i * 7] = call ? m.ref : 0;
        for (uint32_t j = 0; j < MAX_SITE_ALTS; ++j) raw[i * 7 + 1 + j] = call ? m.alt[j] : 0;
        GenoSite o{SITE_NO_CALL, SITE_NO_CALL, false, 0};
        status[i] = 0;
        if (call) status[i] = (uint8_t)geno_site(m.K, m.ref, m.alt, min_support, lt[0], lt[m.K], lt[8 + m.K], tab, tab_n, pl + i * SITE_GENOTYPES, o);
        else for (uint32_t g = 0; g < SITE_GENOTYPES; ++g) pl[i * SITE_GENOTYPES + g] = 0;
        gt[i * 2] = o.a; gt[i * 2 + 1] = o.b; near[i] = o.near; n_out[i] = o.n;
    }
}

// cohort_sites_layout(n_sites, S) -> out[13]: pl, raw, gt, members, boundary, site, maxn, in_at, logs, slots, in_bytes, total, (unused)
extern "C" void csitesim_layout(uint64_t n_sites, uint64_t S, uint64_t *out) {
    const CohortSitesLayout L = cohort_sites_layout(n_sites, S);
    const uint64_t v[12] = {L.pl, L.raw, L.gt, L.members, L.boundary, L.site, L.maxn, L.in_at, L.logs, L.slots, L.in_bytes, L.total};
    for (int i = 0; i < 12; ++i) out[i] = v[i];
}

#ifdef COHORT_SITES_SIM_MAIN
#include <vector>
int main() {
    uint64_t bad = 0, waves = 0, x = 88172645463325252ull;
    auto rnd = [&x]() { x ^= x << 13; x ^= x >> 7; x ^= x << 17; return x; };
    // the compaction: every presence pattern, against the members picked out one by one
    for (uint32_t bits = 0; bits < 64; ++bits) for (int rep = 0; rep < 8; ++rep) {
        uint32_t cref[6], calt[6], out[8], want[8] = {0, 0, 0, 0, 0, 0, 0, 0};
        for (uint32_t j = 0; j < 6; ++j) { cref[j] = (uint32_t)(rnd() % 1000); calt[j] = (uint32_t)(rnd() % 1000) + 1; }
        for (uint32_t j = 0; j < 6; ++j) if ((bits >> j) & 1u) { want[2 + want[0]++] = calt[j]; if (cref[j] > want[1]) want[1] = cref[j]; }
        csitesim_compact(bits, cref, calt, out);
        for (int t = 0; t < 8; ++t) if (out[t] != want[t]) ++bad;
    }
    const uint64_t sizes[8] = {1, 2, 3, 31, 63, 64, 65, 130};
    for (uint64_t S : sizes) {
        const uint64_t full = 3 * 64 * S;
        for (uint64_t n_items : {full, full - S, (full / S / 2) * S + S}) {
            std::vector<uint8_t> members(n_items), gt(n_items * 2);
            for (uint64_t i = 0; i < n_items; ++i) {
                uint32_t mem = 0;
                const uint32_t cand = 2 + (uint32_t)((i / S) % 5);                     // the site's candidates: 2..6
                for (uint32_t j = 0; j < cand; ++j) if (rnd() % 10 < 7) mem |= 1u << j;
                const uint32_t K = (uint32_t)__builtin_popcount(mem);
                members[i] = (uint8_t)mem;
                uint32_t a = SITE_NO_CALL, b = SITE_NO_CALL;
                if (K >= 2 && rnd() % 8) { a = (uint32_t)(rnd() % (K + 1)); b = a + (uint32_t)(rnd() % (K + 1 - a)); }
                gt[i * 2] = (uint8_t)a; gt[i * 2 + 1] = (uint8_t)b;
            }
            const uint64_t n_sites = n_items / S;
            std::vector<uint64_t> got_ns(n_sites * 6, 0), got_ac(n_sites * 6, 0), got_word(n_sites * 6, 0);
            for (uint64_t w0 = 0; w0 < n_items; w0 += 64) {
                uint8_t leader[64]; uint32_t ns[64 * 6], ac[64 * 6]; uint64_t word[64 * 6];
                csitesim_sums(w0, S, n_items, members.data(), gt.data(), leader, ns, ac, word);
                ++waves;
                for (uint32_t lane = 0; lane < 64; ++lane) {
                    const uint64_t i = w0 + lane;
                    const bool first = i < n_items && (lane == 0 || (i - 1) / S != i / S);
                    if ((leader[lane] != 0) != first) ++bad;
                    for (uint32_t j = 0; j < 6; ++j) {
                        if (!leader[lane]) { if (ns[lane * 6 + j] || ac[lane * 6 + j] || word[lane * 6 + j]) ++bad; continue; }
                        got_ns[i / S * 6 + j] += ns[lane * 6 + j]; got_ac[i / S * 6 + j] += ac[lane * 6 + j]; got_word[i / S * 6 + j] += word[lane * 6 + j];
                    }
                }
            }
            for (uint64_t k = 0; k < n_sites; ++k) for (uint32_t j = 0; j < 6; ++j) {
                uint64_t wn = 0, wc = 0;
                for (uint64_t s = 0; s < S; ++s) {
                    const uint64_t i = k * S + s;
                    if (gt[i * 2] == SITE_NO_CALL || !((members[i] >> j) & 1u)) continue;
                    uint32_t al = 1;
                    for (uint32_t t = 0; t < j; ++t) al += (members[i] >> t) & 1u;
                    ++wn; wc += (gt[i * 2] == al) + (gt[i * 2 + 1] == al);
                }
                if (wn != got_ns[k * 6 + j] || wc != got_ac[k * 6 + j] || got_word[k * 6 + j] != (wn | wc << 32)) ++bad;
            }
        }
    }
    for (uint64_t n_sites : {1, 7, 1000}) for (uint64_t S : {1, 3, 64, 65}) {
        uint64_t L[12];
        csitesim_layout(n_sites, S, L);
        const uint64_t n = n_sites * S;
        if (L[0] != 0 || L[1] != 224 * n || L[2] != 252 * n || L[3] != 254 * n || L[4] != 255 * n || L[5] != ((256 * n + 7) & ~7ull) || L[5] % 8 ||
            L[6] != L[5] + 48 * n_sites || L[7] != L[6] + 8 || L[8] != L[7] || L[9] != L[8] + 128 || L[10] != 128 + 24 * n_sites || L[11] != L[7] + L[10] + 64) ++bad;
    }
    printf("cohort_sites_sim %s: %llu waves, %llu lanes, sites, compactions or layouts differ\n", bad ? "FAILED" : "ok", (unsigned long long)waves,
           (unsigned long long)bad);
    return bad ? 1 : 0;
}
#endif
