// Host harness of the overlapped fused pass's decisions (tests only): the functions of svjg_pass.h exactly as libsvjg_hip.so compiles them.
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
