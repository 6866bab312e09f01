// What the two site kernels run per lane (svjg_geno.h) — the joint arithmetic for insertions that share a position (geno_site), the slot gather and
// the item behind it (site_gather, site_item: what k_genotype_sites and k_genotype_cohort_sites do per item), and the plain pieces of the cohort
// call (site_compact, site_candidate_copies, cohort_site_member_sums under cohort_segment's masks).  Topic `site` of the stand-alone program runs
// the compaction of every presence pattern, every wave of 3 * 64 * S items against brute-force sums, the layouts, and the gather and the item over
// count and presence arrays allocated at exactly their size, bad slots and counts of every depth among them.

// the SITE_LOGS logarithms of a call (svjg_geno.h: site_log_table)
extern "C" void genosim_site_log_table(double err, double *tab) { site_log_table(err, tab); }

// geno_site over sites of (K in 2..6, ref, alt[6]) -> gt[n * 2] (0xFF, 0xFF: no call), pl[n * 28], near, status (GENO_ROW_*), n = s_K
extern "C" void genosim_site_genotype(const uint8_t *K, const uint32_t *ref, const uint32_t *alt, uint64_t n_sites, uint32_t min_support, double err,
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

// site_gather as the lane of sample s does it: counts[n_slots * S] slot-major (ref | alt << 32), present[n_slots * S] or nullptr, the site's six
// slots -> out[14] = members, bad, cref[6], calt[6]
extern "C" void genosim_site_gather(const unsigned long long *counts, const uint8_t *present, uint64_t S, uint64_t s, uint32_t n_slots, const uint32_t *slots,
                                    uint32_t *out) {
    SiteGather g;
    site_gather(counts, present, S, s, n_slots, slots, g);
    out[0] = g.members; out[1] = g.bad;
    for (uint32_t j = 0; j < MAX_SITE_ALTS; ++j) { out[2 + j] = g.cref[j]; out[8 + j] = g.calt[j]; }
}

// site_item over all (site k, sample s) items, i = k * S + s, as the lanes do: slots[n_sites * 6] -> gt[i * 2..], pl[i * 28..], raw[i * 7..],
// boundary[i], and what the routine returns: members, status (GENO_ROW_*), n = s_K, bad
extern "C" void genosim_site_items(const unsigned long long *counts, const uint8_t *present, uint64_t S, uint32_t n_slots, const uint32_t *slots,
                                   uint64_t n_sites, uint32_t min_support, double err, const dd *tab, uint32_t tab_n, uint8_t *gt, int64_t *pl,
                                   uint32_t *raw, uint8_t *boundary, uint8_t *members, uint8_t *status, uint64_t *n_out, uint8_t *bad) {
    double lt[SITE_LOGS];
    site_log_table(err, lt);
    for (uint64_t i = 0; i < n_sites * S; ++i) {
        const uint64_t k = i / S, s = i - k * S;
        const SiteItem t = site_item(counts, present, present == nullptr, S, s, n_slots, slots + k * MAX_SITE_ALTS, min_support, lt, tab, tab_n,
                                     raw + i * (MAX_SITE_ALTS + 1), pl + i * SITE_GENOTYPES, gt + i * 2, boundary + i);
        members[i] = (uint8_t)t.members; status[i] = (uint8_t)t.status; n_out[i] = t.n; bad[i] = t.bad;
        if (t.a != gt[i * 2] || t.b != gt[i * 2 + 1]) bad[i] |= 0x80;         // (the returned pair is the stored one: never)
    }
}

// site_compact: bits, cref[6], calt[6] -> out[8] = K, ref, alt[0..6)
extern "C" void genosim_site_compact(uint32_t bits, const uint32_t *cref, const uint32_t *calt, uint32_t *out) {
    SiteMembers m;
    site_compact(bits, cref, calt, m);
    out[0] = m.K; out[1] = m.ref;
    for (uint32_t t = 0; t < MAX_SITE_ALTS; ++t) out[2 + t] = m.alt[t];
}

// The wave whose first item is w0, of n_items items of S samples a site; members[i] and gt[i * 2..] per ITEM as the kernel leaves them (gt 0xFF,
// 0xFF: no site call).  The ballots are formed as the kernel forms them (a lane beyond the last item votes members 0, no call), then for every
// lane: leader[lane] and, per candidate j, ns / ac / word[lane * 6 + j] as the leader would add them (0 where the lane is no leader).
extern "C" void genosim_site_sums(uint64_t w0, uint64_t S, uint64_t n_items, const uint8_t *members, const uint8_t *gt,
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

// Items from the gathered (bits, cref, calt), the compaction and geno_site written out step by step — the second opinion on site_item: bits[i],
// cref / calt[i * 6..] (those of an absent candidate are not looked at) -> gt[i * 2..], pl[i * 28..], raw[i * 7..], near, status (GENO_ROW_*),
// n = s_K; K' < 2: 0xFF, 0xFF and zeros
extern "C" void genosim_site_items_by_steps(uint64_t n_items, const uint8_t *bits, const uint32_t *cref, const uint32_t *calt, uint32_t min_support, double err,
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

#ifdef GENO_SIM_MAIN
// The gather and the item at S samples (S = 1 also with present == nullptr) over arrays of EXACTLY n_slots * S entries: a read through a slot
// behind a hole or at or beyond n_slots would be a read beyond the allocation.  Every eighth site is bad in one of four ways.  -> what differs
static uint64_t beyond = 0;
static uint64_t run_gather_and_items(uint64_t S, bool vector_call, const std::vector<dd> &tab) {
    const uint32_t n_slots = 97;
    const uint64_t n_sites = 200, n = n_sites * S;
    uint64_t bad = 0;
    std::vector<unsigned long long> counts(n_slots * S);
    std::vector<uint8_t> present(n_slots * S);
    for (auto &c : counts) {                             // shallow, deep and full-range counts: sites beyond the table and beyond its cap among them
        const uint64_t k = rnd() % 20, top = k == 0 ? 0xFFFFFFFFull : k < 3 ? 1000000 : 60;
        c = (rnd() % (top + 1)) | ((rnd() % (top + 1)) << 32);
    }
    for (auto &p : present) p = rnd() % 10 < 8;
    const uint8_t *pres = vector_call ? nullptr : present.data();
    std::vector<uint32_t> slots(n_sites * MAX_SITE_ALTS, SITE_NO_SLOT);
    std::vector<uint8_t> want_bad(n_sites, 0);
    for (uint64_t k = 0; k < n_sites; ++k) {
        uint32_t *m = slots.data() + k * MAX_SITE_ALTS;
        const uint32_t K = 2 + (uint32_t)(rnd() % 5);
        for (uint32_t j = 0; j < K; ++j) m[j] = (uint32_t)(rnd() % n_slots);
        if (k % 8 != 7) continue;
        want_bad[k] = 1;
        switch ((k / 8) % 4) {
            case 0: m[rnd() % K] = n_slots; break;                            // the first slot beyond the counts
            case 1: m[rnd() % K] = 0xFFFFFFFEu; break;                        // far beyond
            case 2: m[0] = SITE_NO_SLOT; m[1] = 0x7FFFFFFFu; break;           // a hole in front, an impossible slot behind it
            default: m[K - 1] = SITE_NO_SLOT; if (K < MAX_SITE_ALTS) m[K] = 5; else m[K - 2] = n_slots + 1; break;   // a hole in the middle
        }
    }
    for (uint64_t i = 0; i < n; ++i) {
        const uint64_t k = i / S, s = i % S;
        const uint32_t *m = slots.data() + k * MAX_SITE_ALTS;
        uint32_t out[14], members = 0, cref[6] = {0}, calt[6] = {0};
        genosim_site_gather(counts.data(), pres, S, s, n_slots, m, out);
        if ((out[1] != 0) != (want_bad[k] != 0)) ++bad;
        bool open = true;
        for (uint32_t j = 0; j < MAX_SITE_ALTS; ++j) {                         // the candidates picked out one by one
            if (m[j] == SITE_NO_SLOT) { open = false; continue; }
            if (!open || m[j] >= n_slots) continue;
            const uint64_t at = (uint64_t)m[j] * S + s;
            if (pres && !pres[at]) continue;
            members |= 1u << j; cref[j] = (uint32_t)counts[at]; calt[j] = (uint32_t)(counts[at] >> 32);
        }
        if (out[0] != members) ++bad;
        for (uint32_t j = 0; j < MAX_SITE_ALTS; ++j) if (out[2 + j] != cref[j] || out[8 + j] != calt[j]) ++bad;
    }
    // the items: site_item against the compaction and geno_site step by step on the gathered counts (a bad item: no members)
    std::vector<uint8_t> gt(n * 2), boundary(n), members(n), st(n), isbad(n), bits(n), gt2(n * 2), near2(n), st2(n);
    std::vector<int64_t> pl(n * SITE_GENOTYPES), pl2(n * SITE_GENOTYPES);
    std::vector<uint32_t> raw(n * 7), raw2(n * 7), cref(n * 6), calt(n * 6);
    std::vector<uint64_t> nn(n), nn2(n);
    genosim_site_items(counts.data(), pres, S, n_slots, slots.data(), n_sites, 3, 5e-5, tab.data(), (uint32_t)tab.size(), gt.data(), pl.data(), raw.data(),
                       boundary.data(), members.data(), st.data(), nn.data(), isbad.data());
    for (uint64_t i = 0; i < n; ++i) {
        uint32_t out[14];
        genosim_site_gather(counts.data(), pres, S, i % S, n_slots, slots.data() + i / S * MAX_SITE_ALTS, out);
        bits[i] = out[1] ? 0 : (uint8_t)out[0];
        for (uint32_t j = 0; j < 6; ++j) { cref[i * 6 + j] = out[2 + j]; calt[i * 6 + j] = out[8 + j]; }
    }
    genosim_site_items_by_steps(n, bits.data(), cref.data(), calt.data(), 3, 5e-5, tab.data(), (uint32_t)tab.size(), gt2.data(), pl2.data(), raw2.data(), near2.data(), st2.data(), nn2.data());
    if (gt != gt2 || pl != pl2 || raw != raw2 || boundary != near2 || st != st2 || nn != nn2 || members != bits) ++bad;
    for (uint64_t i = 0; i < n; ++i) {
        const bool few = __builtin_popcount(bits[i]) < 2;
        if (isbad[i] != (want_bad[i / S] || (vector_call && few))) ++bad;
        if (few && (gt[i * 2] != SITE_NO_CALL || gt[i * 2 + 1] != SITE_NO_CALL || boundary[i] || raw[i * 7])) ++bad;
    }
    for (uint64_t i = 0; i < n; ++i) beyond += st[i] != GENO_ROW_OK;
    return bad;
}

static int main_site() {
    const uint32_t tab_n = 1u << 20;                     // beyond it: sites answer GENO_ROW_GROW / GENO_ROW_HOST and touch no entry
    std::vector<dd> tab(tab_n);
    genosim_logfact(tab.data(), tab_n);
    uint64_t bad = 0, waves = 0;
    bad += run_gather_and_items(1, true, tab) + run_gather_and_items(1, false, tab) + run_gather_and_items(3, false, tab) + run_gather_and_items(65, false, tab);
    // the compaction: every presence pattern, against the members picked out one by one
    for (uint32_t bits = 0; bits < 64; ++bits) for (int rep = 0; rep < 8; ++rep) {
        uint32_t cref[6], calt[6], out[8], want[8] = {0, 0, 0, 0, 0, 0, 0, 0};
        for (uint32_t j = 0; j < 6; ++j) { cref[j] = (uint32_t)(rnd() % 1000); calt[j] = (uint32_t)(rnd() % 1000) + 1; }
        for (uint32_t j = 0; j < 6; ++j) if ((bits >> j) & 1u) { want[2 + want[0]++] = calt[j]; if (cref[j] > want[1]) want[1] = cref[j]; }
        genosim_site_compact(bits, cref, calt, out);
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
                genosim_site_sums(w0, S, n_items, members.data(), gt.data(), leader, ns, ac, word);
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
        layout_at(LAYOUT_SITES, n_sites, S, 0, 1, L);
        const uint64_t n = n_sites * S;
        if (L[0] != 0 || L[1] != 224 * n || L[2] != 252 * n || L[3] != 254 * n || L[4] != 255 * n || L[5] != ((256 * n + 7) & ~7ull) || L[5] % 8 ||
            L[6] != L[5] + 48 * n_sites || L[7] != L[6] + 8 || L[8] != L[7] || L[9] != L[8] + 128 || L[10] != 128 + 24 * n_sites || L[11] != L[7] + L[10] + 64) ++bad;
        layout_at(LAYOUT_SITES, n_sites, 1, 0, 0, L);
        if (L[0] != 0 || L[1] != 224 * n_sites || L[2] != 252 * n_sites || L[3] != 0 || L[4] != 254 * n_sites || L[5] != 0 || L[6] != ((255 * n_sites + 7) & ~7ull) ||
            L[7] != L[6] + 8 || L[8] != L[7] || L[9] != L[8] + 128 || L[10] != 128 + 24 * n_sites || L[11] != L[7] + L[10] + 64) ++bad;
    }
    printf("site_sim %s: %llu waves, %llu items beyond the table; %llu gathers, items, lanes, sites, compactions or layouts differ\n", bad ? "FAILED" : "ok",
           (unsigned long long)waves, (unsigned long long)beyond, (unsigned long long)bad);
    return bad ? 1 : 0;
}
#endif
