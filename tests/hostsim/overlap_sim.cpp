// Host harness of the fused pass's host decisions and of a classify launch's plan (tests only): the functions of svjg_pass.h exactly as
// libsvjg_hip.so compiles them.  -DOVERLAP_SIM_MAIN: a stand-alone program that runs the plan and the list sizes over a sweep of sizes
// (for a build under AddressSanitizer / UBSan: nothing is preloaded into anything).
#include "../../svjedi-graph_amd/csrc/svjg_pass.h"

using namespace svjg;

extern "C" int overlapsim_pass_overlaps(int has_comm, int all_slow, int timed_by_events, int last_pass_deferred) {
    return pass_overlaps(has_comm != 0, all_slow != 0, timed_by_events != 0, last_pass_deferred != 0) ? 1 : 0;
}
extern "C" int overlapsim_pass_settles_exact(int has_comm, int all_slow, int overlapped, uint32_t own_overflow_bits, uint64_t n_deferred) {
    return pass_settles_exact(has_comm != 0, all_slow != 0, overlapped != 0, own_overflow_bits, n_deferred) ? 1 : 0;
}
extern "C" uint64_t overlapsim_pass_main_ticks(uint64_t t_first, uint64_t t_last, uint64_t prev_t_last) { return pass_main_ticks(t_first, t_last, prev_t_last); }
extern "C" int overlapsim_pass_repeats(int has_comm, uint32_t own_overflow_bits, uint64_t guard_repeat_sum) { return pass_repeats(has_comm != 0, own_overflow_bits, guard_repeat_sum) ? 1 : 0; }

// out3: region, small, grid
extern "C" void overlapsim_main_plan(uint64_t n_bytes, uint64_t workers, uint64_t stripe, uint64_t small_chunk, double first_share, uint64_t *out3) {
    const MainPlan p = main_plan(n_bytes, workers, stripe, small_chunk, first_share);
    out3[0] = p.region; out3[1] = p.small; out3[2] = p.grid;
}
extern "C" int overlapsim_main_occupancy(int api, uint64_t lds, uint64_t granule) { return main_occupancy(api, lds, granule); }

static DevStatus status_of(uint64_t n_recs, uint64_t n_host, uint32_t overflow) {
    DevStatus s{};
    s.n_recs = n_recs; s.n_host = n_host; s.overflow = overflow;
    return s;
}
// out3: deferred, recs, host
extern "C" void overlapsim_lists_first(int all_slow, int want_hits, uint64_t n, uint64_t n_recs, uint64_t n_host, uint64_t *out3) {
    const ListSizes s = lists_first(all_slow != 0, want_hits != 0, n, status_of(n_recs, n_host, 0));
    out3[0] = s.deferred; out3[1] = s.recs; out3[2] = s.host;
}
extern "C" void overlapsim_lists_grown(const uint64_t *in3, uint64_t n, uint64_t recs_before, uint64_t host_before, uint64_t recs_after, uint32_t overflow, uint64_t *out3) {
    const ListSizes s = lists_grown(ListSizes{in3[0], in3[1], in3[2]}, n, status_of(recs_before, host_before, 0), status_of(recs_after, host_before, overflow));
    out3[0] = s.deferred; out3[1] = s.recs; out3[2] = s.host;
}
extern "C" void overlapsim_lists_fused(int all_slow, uint64_t n, uint64_t *out3) {
    const ListSizes s = lists_fused(all_slow != 0, n);
    out3[0] = s.deferred; out3[1] = s.recs; out3[2] = s.host;
}

#ifdef OVERLAP_SIM_MAIN
#include <stdio.h>

// what k_classify_main relies on (tests/test_main_plan.py holds the same against a restatement of the formulas)
static int plan_holds(uint64_t n, uint64_t workers, uint64_t stripe, uint64_t small_chunk, double first_share) {
    const MainPlan p = main_plan(n, workers, stripe, small_chunk, first_share);
    const uint64_t share = (n + workers - 1) / workers;
    bool ok = p.region % 16 == 0 && p.region >= stripe && p.grid >= 1 && p.grid <= workers && (p.small == 0 || p.small == small_chunk);
    if (p.small == 0) ok = ok && (uint64_t)p.grid * p.region >= n;
    else ok = ok && p.grid == workers && p.region <= share && (double)p.region >= 0.84 * (double)share;
    if (!ok) fprintf(stderr, "main_plan(%llu, %llu): region %llu small %llu grid %u\n", (unsigned long long)n, (unsigned long long)workers,
                     (unsigned long long)p.region, (unsigned long long)p.small, p.grid);
    return ok ? 0 : 1;
}

int main() {
    const uint64_t stripe = 8192, small_chunk = 65536;
    const double first_share = 0.85;
    const uint64_t workers[4] = {1, 14, 3584, 4096};
    uint64_t cases = 0, sum = 0;
    int bad = 0;
    uint64_t x = 0x9E3779B97F4A7C15ull;                            // (xorshift64: the sizes need no quality, only a seed)
    for (const uint64_t w : workers) {
        const uint64_t fixed[] = {1, stripe - 1, stripe, stripe + 1, w * stripe - 1, w * stripe + 1, 8 * small_chunk * w - 1, 8 * small_chunk * w,
                                  8 * small_chunk * w + 1, (8 * small_chunk - 1) * w, (8 * small_chunk - 1) * w + 1, (1ull << 32) - 1, (1ull << 32) + 1,
                                  2133165175ull, 21621759346ull, 1ull << 36};
        for (const uint64_t n : fixed) { bad += plan_holds(n, w, stripe, small_chunk, first_share); ++cases; }
        for (int i = 0; i < 4000; ++i) {
            x ^= x << 13; x ^= x >> 7; x ^= x << 17;
            const uint64_t n = 1 + (x >> (28 + i % 36)) % (1ull << 36);
            bad += plan_holds(n, w, stripe, small_chunk, first_share); ++cases;
            for (int all_slow = 0; all_slow < 2; ++all_slow) {
                const DevStatus before = status_of(x & 0xFFFFF, x >> 50, 0);
                ListSizes s = lists_first(all_slow != 0, (i & 1) != 0, n, before);
                for (uint32_t bits = 0; bits < 8; ++bits) {
                    const ListSizes g = lists_grown(s, n, before, status_of(before.n_recs + (x >> 40), before.n_host, bits));
                    if (g.deferred < s.deferred && !(bits & 1u)) ++bad;
                    sum += g.deferred + g.recs + g.host;
                }
                const ListSizes f = lists_fused(all_slow != 0, n);
                if (f.deferred != s.deferred || f.recs != 0) ++bad;
            }
        }
    }
    const MainPlan k = main_plan(2133165175ull, 3584, stripe, small_chunk, first_share);
    if (k.region != 505920 || k.small != 65536 || k.grid != 3584) ++bad;
    if (main_occupancy(16, 15568, 1280) != 9 || main_occupancy(8, 15568, 1280) != 8) ++bad;
    if (bad) { printf("overlap_sim FAILED: %d of %llu cases\n", bad, (unsigned long long)cases); return 1; }
    printf("overlap_sim ok: %llu plans (checksum %llu)\n", (unsigned long long)cases, (unsigned long long)sum);
    return 0;
}
#endif
