// What a finished fused pass (svjg_run_begin / svjg_run_end) means for the ranks of a job — host logic shared by libsvjg_hip.so
// and the CPU harness (tests/hostsim), so that the decision the ranks must take TOGETHER is tested where there is no GPU.  Further down, in
// the same spirit: how one k_classify_main launch divides the text among its workers and how long its lists are (main_plan, ListSizes).
//
// A pass enqueues, with no host round trip: k_classify_main, k_classify_exact (the exact path: it reads the number of deferred
// lines on the device and takes its wave role, one wave per line, up to `wave_limit` lines, its lane role, one lane per line,
// beyond it; the same launch resets what the next pass starts from), the guard kernel, the all-reduce of [ counts | guard words ], the genotypes.  The only thing the device cannot repair by itself
// is a list that overflowed (deferred lines, lines for the host): such a pass has to be repeated with larger lists.  Under a
// communicator that decision is COLLECTIVE: every rank puts "I must repeat" into guard word 2, the words travel through the
// pass's own all-reduce, and every rank repeats (classify step by step + ONE more all-reduce) iff the sum is not zero — so all
// ranks issue the same number of collectives in the same order and none hands out a sum that lacks a rank's deferred lines.
//
// A ONE-GPU pass (no communicator, a graph whose lines are not all the exact path's, the kernels timed by their stamps) runs in the
// OVERLAPPED form: consecutive passes alternate between two compute streams, so that the workers of pass k + 1 move into the slots
// those of pass k vacate, and nothing sits on a compute stream between two k_classify_main — no k_classify_exact either.  Such a
// pass has a SECOND thing the host settles at svjg_run_end: lines that were deferred.  n_deferred comes back in the pass's status
// block; if it is not zero the host launches k_classify_exact on the pass's own deferred list into the pass's own count vector,
// runs the genotypes again and waits once more (pass_settles_exact; the pass is not repeated; whoever asks for the pass's counts before
// svjg_run_end settles it there and then; overflow bits the exact path sets repeat the pass like the main kernel's: pass_repeats).  A context whose last finished pass
// deferred lines runs its next pass in the former form, exact path on the stream (pass_overlaps), until a pass defers nothing.
#pragma once
#include <stdint.h>

namespace svjg {

constexpr uint32_t GUARD_WORDS = 3;          // behind the count vector: largest ref field, largest alt field, ranks that must repeat the pass
constexpr uint32_t GUARD_MAX_REF = 0, GUARD_MAX_ALT = 1, GUARD_REPEAT = 2;

// status words (device); here because a fused pass's row block holds one (svjg_geno.h: run_layout)
struct DevStatus {
    unsigned long long n_lines;
    unsigned long long n_deferred;       // entries appended to the deferred list
    unsigned long long n_recs;           // hit records appended
    unsigned long long err;              // min over (file offset << 3 | exception class); ~0 = none
    unsigned int non_ascii;
    unsigned int overflow;               // bit 0: deferred list, bit 1: hit-record buffer, bit 2: list of lines for the host
    unsigned long long next_chunk;       // k_classify_main: small chunks handed out so far (zero at launch)
    unsigned long long n_host;           // lines set aside for the host (SVJG_EXC_ASK_HOST)
    unsigned long long cause[8];         // deferred lines by cause (DC_*)
    unsigned long long t_first, t_last;  // k_classify_main: wall_clock64() when its first worker started / its last worker ended (zero at launch)
    unsigned long long t_exact;          // k_classify_exact: when the last block that had lines to work off ended
};

// what this rank contributes to guard word 2 (computed on the device by k_counts_guard from the pass's status block)
inline
#ifdef __HIPCC__
__host__ __device__
#endif
uint64_t pass_repeat_word(uint32_t overflow_bits) { return overflow_bits ? 1u : 0u; }

// does the pass have to be repeated?  has_comm: the guard words went through the all-reduce (their sum over the ranks is at hand);
// otherwise the rank is alone and its own status decides.
inline bool pass_repeats(bool has_comm, uint32_t own_overflow_bits, uint64_t guard_repeat_sum) {
    return has_comm ? guard_repeat_sum != 0 : own_overflow_bits != 0;
}

// the form of the next pass (svjg_run_begin).  Overlapped — two compute streams, no exact-path launch on them — unless the pass's
// all-reduce needs the exact path's hits first (has_comm), every line is the exact path's (all_slow), the kernels are timed by event
// pairs on the stream (timed_by_events), or the last pass that finished on this context deferred lines: a settle step waits for the
// NEXT pass's main kernel to drain, which a stream of deferring passes would pay every time.
inline bool pass_overlaps(bool has_comm, bool all_slow, bool timed_by_events, bool last_pass_deferred) {
    return !has_comm && !all_slow && !timed_by_events && !last_pass_deferred;
}

// does svjg_run_end owe the pass its exact path (the settle step)?  Only a pass in the overlapped form, which has none on its stream
// (has_comm / all_slow: never overlapped; given so that the rule stands by itself); a list that overflowed repeats the pass instead.
inline bool pass_settles_exact(bool has_comm, bool all_slow, bool overlapped, uint32_t own_overflow_bits, uint64_t n_deferred) {
    return overlapped && !has_comm && !all_slow && !own_overflow_bits && n_deferred != 0;
}

// kernel_ms()[0] of a fused pass, in ticks of the stamps' clock: its first worker's start to its last worker's end — but where the
// pass before (prev_t_last != 0: it ran on this context with no host synchronisation in between) was still running when this one's
// first worker started, only from that pass's end: the interval two overlapped launches share is counted once, in the earlier one.
inline uint64_t pass_main_ticks(uint64_t t_first, uint64_t t_last, uint64_t prev_t_last) {
    const uint64_t from = prev_t_last > t_first ? prev_t_last : t_first;
    return t_last > from ? t_last - from : 0;
}

// ---- one k_classify_main launch: how the text is divided among its workers, how long its lists are ----
// (the kernel's constants come in as arguments: this header knows no kernel)

// Workgroups of k_classify_main one CU holds: what the occupancy API says, capped by the LDS.  LDS is handed out in units of `granule`
// bytes (measured: a 15 568-byte workgroup is admitted 9 times per CU where the API says 10); a worker too many would run in a second
// round behind the others.
inline int main_occupancy(int api, uint64_t lds, uint64_t granule) {
    const int by_lds = (int)((160u * 1024u) / ((lds + granule - 1) / granule * granule));
    return by_lds >= 1 && api > by_lds ? by_lds : api;
}

// One worker (wave) per resident slot, `workers` = CUs x main_occupancy of them; every worker owns the lines starting in its region of
// the text.  A worker's first chunk is most of an even share (`first_share` of it), fixed; what is left goes in chunks of `small_chunk`
// bytes to whoever is free next (svjg_kernels.h: the workers of a CU do not run equally fast).  Inputs too small for that — an even
// share below 8 chunks —: even shares, small = 0.  Smaller still: regions of one `stripe`, fewer workers.
struct MainPlan { uint64_t region, small; uint32_t grid; };
inline MainPlan main_plan(uint64_t n_bytes, uint64_t workers, uint64_t stripe, uint64_t small_chunk, double first_share) {
    MainPlan p;
    const uint64_t share = (n_bytes + workers - 1) / workers;
    p.region = (share + 15) & ~15ull;
    p.small = 0;
    if (share >= 8 * small_chunk) { p.region = ((uint64_t)(share * first_share) + 15) & ~15ull; p.small = small_chunk; }
    if (p.region < stripe) p.region = stripe;
    const uint64_t want_grid = (n_bytes + p.region - 1) / p.region;
    p.grid = (uint32_t)(want_grid < workers ? want_grid : workers);
    return p;
}

// Entries of the three lists a launch over n bytes of text appends to: deferred lines, hit records, lines for the host.
struct ListSizes { uint64_t deferred, recs, host; };
inline uint64_t deferred_want(bool all_slow, uint64_t n) { return all_slow ? n / 24 + 64 : (n / 4096 + 65536); }
// a step-by-step call's first attempt; `now`: the status before it (hit records and host lines add up over the calls)
inline ListSizes lists_first(bool all_slow, bool want_hits, uint64_t n, const DevStatus &now) {
    return ListSizes{deferred_want(all_slow, n),
                     want_hits ? now.n_recs + n / 40 + 65536 : 0,      // (the synthetic workloads: one hit per 60 bytes of text)
                     now.n_host + 4096};
}
// ... and what an attempt that ended with overflow bits is repeated with: worst-case lists (before, after: the status around the attempt)
inline ListSizes lists_grown(ListSizes s, uint64_t n, const DevStatus &before, const DevStatus &after) {
    if (after.overflow & 1u) s.deferred = n / 24 + 64;
    if (after.overflow & 2u) s.recs = before.n_recs + (after.n_recs - before.n_recs) * 2 + n / 24 + 64;
    if (after.overflow & 4u) s.host = before.n_host + n / 24 + 64;
    return s;
}
// a fused pass's own lists: no hit records, a fixed list of lines for the host (one that overflows repeats the pass step by step)
inline ListSizes lists_fused(bool all_slow, uint64_t n) { return ListSizes{deferred_want(all_slow, n), 0, 4096}; }

// 32-bit halves of the packed ref | alt << 32 counters cannot have carried into each other iff the SUMS of the ranks' maxima fit
inline bool pass_counts_overflowed(uint64_t guard_max_ref_sum, uint64_t guard_max_alt_sum) {
    return guard_max_ref_sum >= (1ull << 32) || guard_max_alt_sum >= (1ull << 32);
}

}  // namespace svjg
