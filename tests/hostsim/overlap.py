"""Build + call the host harness of the fused pass's decisions and of a classify launch's plan (svjedi-graph_amd/csrc/svjg_pass.h; tests only)."""
import ctypes
import os

from tests import sim_build

HERE = os.path.dirname(os.path.abspath(__file__))
SO = os.path.join(HERE, "_overlapsim.so")
MAIN = os.path.join(HERE, "_overlapsim_main")
SRC = os.path.join(HERE, "overlap_sim.cpp")
DEPS = [os.path.join(HERE, "..", "..", "svjedi-graph_amd", "csrc", "svjg_pass.h")]


def build():
    sim_build.shared(SO, SRC, DEPS)
    return SO


def build_main():
    """the stand-alone program under AddressSanitizer and UBSan (its own main: nothing is preloaded into anything)"""
    return sim_build.program(MAIN, SRC, DEPS, ["OVERLAP_SIM_MAIN"])


def plan_logic():
    """-> (main_plan(n, workers, stripe, small_chunk, first_share) -> (region, small, grid), main_occupancy(api, lds, granule),
    lists_first(all_slow, want_hits, n, n_recs, n_host) -> (deferred, recs, host),
    lists_grown((deferred, recs, host), n, recs_before, host_before, recs_after, overflow) -> the same,
    lists_fused(all_slow, n) -> the same)"""
    lib = sim_build.shared(SO, SRC, DEPS)
    u64, out3 = ctypes.c_uint64, ctypes.c_uint64 * 3
    lib.overlapsim_main_plan.restype = None
    lib.overlapsim_main_plan.argtypes = [u64] * 4 + [ctypes.c_double, ctypes.POINTER(u64)]
    lib.overlapsim_main_occupancy.restype = ctypes.c_int
    lib.overlapsim_main_occupancy.argtypes = [ctypes.c_int, u64, u64]
    lib.overlapsim_lists_first.restype = None
    lib.overlapsim_lists_first.argtypes = [ctypes.c_int, ctypes.c_int, u64, u64, u64, ctypes.POINTER(u64)]
    lib.overlapsim_lists_grown.restype = None
    lib.overlapsim_lists_grown.argtypes = [ctypes.POINTER(u64)] + [u64] * 4 + [ctypes.c_uint32, ctypes.POINTER(u64)]
    lib.overlapsim_lists_fused.restype = None
    lib.overlapsim_lists_fused.argtypes = [ctypes.c_int, u64, ctypes.POINTER(u64)]

    def call(fn, *args):
        o = out3()
        fn(*args, o)
        return tuple(int(v) for v in o)

    return (lambda n, w, stripe, small, share: call(lib.overlapsim_main_plan, n, w, stripe, small, share),
            lambda api, lds, granule: int(lib.overlapsim_main_occupancy(api, lds, granule)),
            lambda slow, hits, n, recs, host: call(lib.overlapsim_lists_first, int(slow), int(hits), n, recs, host),
            lambda s, n, rb, hb, ra, bits: call(lib.overlapsim_lists_grown, out3(*s), n, rb, hb, ra, bits),
            lambda slow, n: call(lib.overlapsim_lists_fused, int(slow), n))


def overlap_logic():
    """-> (overlaps(has_comm, all_slow, timed_by_events, last_pass_deferred), settles_exact(has_comm, all_slow, overlapped, overflow, n_deferred),
    main_ticks(t_first, t_last, prev_t_last), repeats(has_comm, overflow, guard_sum))"""
    lib = sim_build.shared(SO, SRC, DEPS)
    lib.overlapsim_pass_overlaps.restype = ctypes.c_int
    lib.overlapsim_pass_overlaps.argtypes = [ctypes.c_int] * 4
    lib.overlapsim_pass_settles_exact.restype = ctypes.c_int
    lib.overlapsim_pass_settles_exact.argtypes = [ctypes.c_int] * 3 + [ctypes.c_uint32, ctypes.c_uint64]
    lib.overlapsim_pass_main_ticks.restype = ctypes.c_uint64
    lib.overlapsim_pass_main_ticks.argtypes = [ctypes.c_uint64] * 3
    lib.overlapsim_pass_repeats.restype = ctypes.c_int
    lib.overlapsim_pass_repeats.argtypes = [ctypes.c_int, ctypes.c_uint32, ctypes.c_uint64]
    return (lambda c, s, e, d: bool(lib.overlapsim_pass_overlaps(int(c), int(s), int(e), int(d))),
            lambda c, s, o, v, n: bool(lib.overlapsim_pass_settles_exact(int(c), int(s), int(o), v, n)),
            lambda a, b, p: int(lib.overlapsim_pass_main_ticks(a, b, p)),
            lambda c, o, s: bool(lib.overlapsim_pass_repeats(int(c), o, s)))
