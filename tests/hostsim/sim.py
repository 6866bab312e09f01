"""Build + call the host harness of the per-line device routines (tests only)."""
import ctypes
import os

import numpy as np

from tests import geno_sim, sim_build

HERE = os.path.dirname(os.path.abspath(__file__))
SO = os.path.join(HERE, "_hostsim.so")
CSRC = os.path.join(HERE, "..", "..", "svjedi-graph_amd", "csrc")
DEPS = [os.path.join(CSRC, h) for h in ("svjg_line.h", "svjg_host_tables.h", "svjg_planes.h", "svjg_pass.h", "svjg_geno.h")] + [
    os.path.join(HERE, "..", "host_logfact.h"), os.path.join(HERE, "..", "..", "include", "svjg.h")]
class HostLine(Exception):
    """the exact routine's "the host decides" (svjg.h: SVJG_EXC_ASK_HOST): a decimal column with non-ASCII bytes"""


EXC = {1: ValueError, 2: IndexError, 3: KeyError, 4: ZeroDivisionError, 5: HostLine, 6: TypeError}


def _so():
    return sim_build.shared(SO, os.path.join(HERE, "hostsim.cpp"), DEPS)


def build():
    _so()
    return SO


def _lib():
    from svjg import capi
    lib = _so()
    lib.hostsim_classify.restype = ctypes.c_int
    lib.hostsim_classify.argtypes = [ctypes.POINTER(capi.CGraph), ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p] + [ctypes.c_void_p] * 3
    lib.hostsim_check_tables.restype = ctypes.c_uint64
    lib.hostsim_check_tables.argtypes = [ctypes.POINTER(capi.CGraph)]
    return lib, capi


def classify(graph, gaf, tables=True, wave=False):
    """Every line through svjg::slow_line (the exact path the kernels defer to).  tables=False: node names are resolved
    through the sorted node table only (what the device does for names the node-name hash table cannot hold)."""
    lib, capi = _lib()
    cg = capi.cgraph_of(graph)
    if not tables:
        cg.flags |= 2
    if wave:
        # 2 = the two-phase routine of the wave role of k_classify_exact (64 lanes), 1 = its fallback for very long paths (64 lanes), 3 = one lane with its
        # per-node results kept (the lane role of k_classify_exact), 4 = the two-phase routine without the table of the pieces' colons (every offset of every piece is tried)
        # 5 = the two-phase routine with every node resolved first and the strands taken by id where the line allows it (the wave role of k_classify_exact since r05)
        cg.flags |= {1: 4, 2: 8, 3: 32, 4: 8 | 64, 5: 8 | 128}[wave]
    buf = np.frombuffer(gaf, dtype=np.uint8) if not isinstance(gaf, np.ndarray) else gaf
    counts = np.zeros((max(graph.n_slots, 1), 2), dtype=np.uint32)
    nl, eo = ctypes.c_uint64(0), ctypes.c_uint64(0)
    ex = ctypes.c_int(0)
    rc = lib.hostsim_classify(ctypes.byref(cg), buf.ctypes.data if buf.size else None, buf.size, counts.ctypes.data,
                              ctypes.addressof(nl), ctypes.addressof(ex), ctypes.addressof(eo))
    if rc:
        raise EXC[ex.value](f"offset {eo.value}")
    return counts[: graph.n_slots], nl.value


_WAVE_FLAGS = {0: 0, 1: 4, 2: 8, 3: 32, 4: 8 | 64, 5: 8 | 128}


def classify_cases(graph, frags, tables=True, wave=0):
    """Many small GAF fragments (list of bytes), each on its own -> (counts uint32[n, n_slots, 2], exception class or None per fragment)"""
    lib, capi = _lib()
    cg = capi.cgraph_of(graph)
    if not tables:
        cg.flags |= 2
    cg.flags |= _WAVE_FLAGS[int(wave)]
    offs = np.zeros(len(frags) + 1, np.uint64)
    np.cumsum([len(f) for f in frags], out=offs[1:])
    buf = np.frombuffer(b"".join(frags) + b"\0", dtype=np.uint8)
    counts = np.zeros((len(frags), max(graph.n_slots, 1), 2), dtype=np.uint32)
    exc = np.zeros(len(frags), np.int32)
    lib.hostsim_classify_cases.restype = None
    lib.hostsim_classify_cases.argtypes = [ctypes.POINTER(capi.CGraph)] + [ctypes.c_void_p] * 2 + [ctypes.c_uint64] + [ctypes.c_void_p] * 2
    lib.hostsim_classify_cases(ctypes.byref(cg), buf.ctypes.data, offs.ctypes.data, len(frags), counts.ctypes.data, exc.ctypes.data)
    return counts[:, : graph.n_slots], [EXC.get(int(x)) if x else None for x in exc]


def check_tables(graph):
    lib, capi = _lib()
    cg = capi.cgraph_of(graph)
    return lib.hostsim_check_tables(ctypes.byref(cg))


def table_stats(graph):
    """(names left out, names skipped, links left out, name slots, name buckets, link slots, inline hit words, max displacement)"""
    lib, capi = _lib()
    cg = capi.cgraph_of(graph)
    out = (ctypes.c_uint64 * 8)()
    lib.hostsim_table_stats.restype = None
    lib.hostsim_table_stats(ctypes.byref(cg), out)
    return tuple(int(x) for x in out)


def span_classes(text):
    """Byte-class masks of the 64-byte spans of text (len % 64 == 0) by the main kernel's bit-plane routine:
    uint64[n_spans, 8] = nl, cr, tab, ori, nd, dee, colon, high."""
    lib = _so()
    buf = np.frombuffer(bytes(text), dtype=np.uint8)
    assert buf.size % 64 == 0
    out = np.zeros((buf.size // 64, 8), np.uint64)
    lib.hostsim_span_classes.restype = None
    lib.hostsim_span_classes.argtypes = [ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p]
    lib.hostsim_span_classes(buf.ctypes.data, buf.size // 64, out.ctypes.data)
    return out


def pass_logic():
    """the fused pass's host decisions (svjedi-graph_amd/csrc/svjg_pass.h) -> (repeat_word(overflow), repeats(has_comm, overflow, guard_sum),
    counts_overflowed(max_ref_sum, max_alt_sum), number of guard words)"""
    lib = _so()
    lib.hostsim_pass_repeat_word.restype = ctypes.c_uint64
    lib.hostsim_pass_repeat_word.argtypes = [ctypes.c_uint32]
    lib.hostsim_pass_repeats.restype = ctypes.c_int
    lib.hostsim_pass_repeats.argtypes = [ctypes.c_int, ctypes.c_uint32, ctypes.c_uint64]
    lib.hostsim_pass_counts_overflowed.restype = ctypes.c_int
    lib.hostsim_pass_counts_overflowed.argtypes = [ctypes.c_uint64, ctypes.c_uint64]
    lib.hostsim_guard_words.restype = ctypes.c_uint32
    return (lambda o: int(lib.hostsim_pass_repeat_word(o)), lambda c, o, s: bool(lib.hostsim_pass_repeats(int(c), o, s)),
            lambda a, b: bool(lib.hostsim_pass_counts_overflowed(a, b)), int(lib.hostsim_guard_words()))


FUSED_FIELDS = ("pl32", "raw", "gt", "flags", "boundary", "h_tail", "out_bytes", "maxn", "status", "guard", "tail_bytes", "pl64", "total",
                "slot", "type", "ok", "in_bytes")


def rows_layout(n, fused=False):
    """byte offsets of the row block(s) of k_genotype's calls over n rows (svjg_geno.h: rows_layout / run_layout + rows_in), by field name (the
    blocks of the other calls: tests/geno_sim).  The step-by-step block is exported by both libraries: the names are geno_sim's, the values must agree"""
    out = np.zeros(32, np.uint64)
    count = sim_build.call(_so(), "hostsim_rows_layout", ctypes.c_int, [ctypes.c_uint64, ctypes.c_int, ctypes.c_void_p], n, int(fused), out)
    if fused:
        assert count == len(FUSED_FIELDS)
        return {k: int(out[i]) for i, k in enumerate(FUSED_FIELDS)}
    L = geno_sim.layout(geno_sim.ROWS, n)
    assert list(L.values()) == [int(v) for v in out[:count]]
    return L


def geno_constants():
    """(sizeof(DevStatus), logfact_first(), LOGFACT_CAP, logfact_grow_to) of the library's headers"""
    lib = _so()
    lib.hostsim_sizeof_devstatus.restype = ctypes.c_uint64
    for f in (lib.hostsim_logfact_first, lib.hostsim_logfact_grow_to, lib.hostsim_logfact_cap):
        f.restype = ctypes.c_uint32
    lib.hostsim_logfact_grow_to.argtypes = [ctypes.c_uint32]
    return (int(lib.hostsim_sizeof_devstatus()), int(lib.hostsim_logfact_first()), int(lib.hostsim_logfact_cap()),
            lambda m: int(lib.hostsim_logfact_grow_to(m)))


def logfact_sizes():
    """(logfact_built(upto): the entries a build for `upto` makes, logfact_reserve_to(have, entries): the size svjg_logfact_reserve builds or 0)
    of svjg_geno.h"""
    lib = _so()
    lib.hostsim_logfact_built.restype = lib.hostsim_logfact_reserve_to.restype = ctypes.c_uint32
    lib.hostsim_logfact_built.argtypes = [ctypes.c_uint32]
    lib.hostsim_logfact_reserve_to.argtypes = [ctypes.c_uint32, ctypes.c_uint32]
    return (lambda u: int(lib.hostsim_logfact_built(u))), (lambda h, e: int(lib.hostsim_logfact_reserve_to(h, e)))


def logfact_table(n):
    """log10(i!) for i < n in double-double (float64[n, 2]), built with the host libm's log10 — not the device's"""
    tab = np.zeros((n, 2), np.float64)
    sim_build.call(_so(), "hostsim_logfact", None, [ctypes.c_void_p, ctypes.c_uint32], tab, n)
    return tab


def genotype_rows(sv_type, counts, min_support, err, tab):
    """k_genotype's per-row arithmetic (svjg_geno.h: geno_row) -> (gt, pl[n, 3], near, status: 0 ok, 1 table too short, 2 beyond the cap)"""
    sv_type, counts, tab = np.ascontiguousarray(sv_type, np.uint8), np.ascontiguousarray(counts, np.uint32), np.ascontiguousarray(tab, np.float64)
    n = len(sv_type)
    gt, pl, near, st = np.zeros(n, np.uint8), np.zeros((n, 3), np.int64), np.zeros(n, np.uint8), np.zeros(n, np.uint8)
    sim_build.call(_so(), "hostsim_genotype", None, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_uint32, ctypes.c_double, ctypes.c_void_p,
                                                     ctypes.c_uint32] + [ctypes.c_void_p] * 4,
                   sv_type, counts, n, int(min_support), float(err), tab, len(tab), gt, pl, near, st)
    return gt, pl, near, st
