"""Build + call the host harness of the overlapped fused pass's decisions (svjedi-graph_amd/csrc/svjg_pass.h; tests only)."""
import ctypes
import os
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
SO = os.path.join(HERE, "_overlapsim.so")


def build():
    src = [os.path.join(HERE, "overlap_sim.cpp"), os.path.join(HERE, "..", "..", "svjedi-graph_amd", "csrc", "svjg_pass.h")]
    if not os.path.exists(SO) or os.path.getmtime(SO) < max(os.path.getmtime(s) for s in src):
        subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-shared", "-fPIC", "-o", SO, src[0]], check=True)
    return SO


def overlap_logic():
    """-> (overlaps(has_comm, all_slow, timed_by_events, last_pass_deferred), settles_exact(has_comm, all_slow, overlapped, overflow, n_deferred),
    main_ticks(t_first, t_last, prev_t_last), repeats(has_comm, overflow, guard_sum))"""
    lib = ctypes.CDLL(build())
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
