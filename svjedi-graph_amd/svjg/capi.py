"""ctypes binding of libsvjg_hip.so (include/svjg.h).

There is no fallback: if the shared library is missing, or no MI355X is visible, the calls raise.
"""
import ctypes
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(os.path.dirname(HERE), "csrc", "libsvjg_hip.so")
HOST_LIB_PATH = os.path.join(os.path.dirname(HERE), "csrc", "libsvjg_host.so")

HITREC_DT = np.dtype([("line_start", "<u8"), ("slot", "<u4"), ("n_ref", "<u2"), ("n_alt", "<u2")])

EXC_CLASS = {1: ValueError, 2: IndexError, 3: KeyError, 4: ZeroDivisionError, 6: TypeError}
LINE_ERRORS = (ValueError, IndexError, KeyError, ZeroDivisionError, TypeError)      # what a GAF line can make the reference die with
DOVER_TYPE_ERROR = "'>=' not supported between instances of 'int' and 'list'"       # filter-alignments.py:269 under -O (svjg.h: SVJG_EXC_TYPE_ERROR)


class SvjgError(RuntimeError):
    pass


class CGraph(ctypes.Structure):
    _fields_ = [
        ("nodes", ctypes.c_void_p), ("n_nodes", ctypes.c_uint64),
        ("edges", ctypes.c_void_p), ("n_edges", ctypes.c_uint64),
        ("hits", ctypes.c_void_p), ("n_hits", ctypes.c_uint64),
        ("chrom_names", ctypes.c_char_p), ("chrom_off", ctypes.c_void_p), ("chrom_node_lo", ctypes.c_void_p),
        ("n_chrom", ctypes.c_uint32),
        ("n_slots", ctypes.c_uint32), ("d_over", ctypes.c_uint32), ("flags", ctypes.c_uint32),
    ]


class CStats(ctypes.Structure):
    _fields_ = [("n_lines", ctypes.c_uint64), ("n_deferred", ctypes.c_uint64), ("n_hitrecs", ctypes.c_uint64),
                ("non_ascii", ctypes.c_uint64)]


def cgraph_of(g):
    """ctypes view of a svjg.graph.Graph (the Graph must stay alive while the struct is in use)."""
    return CGraph(
        g.nodes.ctypes.data, g.n_nodes, g.edges.ctypes.data, g.n_edges, g.hits.ctypes.data, g.n_hits,
        g.chrom_names, g.chrom_off.ctypes.data, g.chrom_lo.ctypes.data, len(g.chroms),
        g.n_slots, g.d_over, g.flags)


_SIGS = {
    "svjg_abi_version": (ctypes.c_int, []),
    "svjg_device_count": (ctypes.c_int, []),
    "svjg_init": (ctypes.c_int, [ctypes.c_int, ctypes.POINTER(ctypes.c_void_p)]),
    "svjg_destroy": (None, [ctypes.c_void_p]),
    "svjg_last_error": (ctypes.c_char_p, [ctypes.c_void_p]),
    "svjg_load_graph": (ctypes.c_int, [ctypes.c_void_p, ctypes.POINTER(CGraph)]),
    "svjg_release_host_tables": (None, []),
    "svjg_gaf_upload": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64]),
    "svjg_gaf_upload_part": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_uint64, ctypes.c_uint64, ctypes.c_int]),
    "svjg_comm_set_stream": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int]),
    "svjg_copy_rate": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_uint64, ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_double)]),
    "svjg_classify_resident": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_uint64, ctypes.c_int]),
    "svjg_classify": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_uint64, ctypes.c_int]),
    "svjg_gaf_upload_file": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_char_p, ctypes.c_uint64, ctypes.c_uint64]),
    "svjg_classify_file": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_char_p, ctypes.c_uint64, ctypes.c_uint64, ctypes.c_int]),
    "svjg_reset_counts": (ctypes.c_int, [ctypes.c_void_p]),
    "svjg_get_stats": (ctypes.c_int, [ctypes.c_void_p, ctypes.POINTER(CStats)]),
    "svjg_get_defer_causes": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p]),
    "svjg_input_error": (ctypes.c_int, [ctypes.c_void_p, ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_uint64)]),
    "svjg_get_counts": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint32]),
    "svjg_set_counts": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint32]),
    "svjg_alloc_counts": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_uint32]),
    "svjg_get_hits": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64, ctypes.POINTER(ctypes.c_uint64)]),
    "svjg_get_host_lines": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64, ctypes.POINTER(ctypes.c_uint64)]),
    "svjg_comm_unique_id": (ctypes.c_int, [ctypes.c_char_p]),
    "svjg_comm_init": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_char_p, ctypes.c_int, ctypes.c_int]),
    "svjg_allreduce_counts": (ctypes.c_int, [ctypes.c_void_p]),
    "svjg_comm_init_all": (ctypes.c_int, [ctypes.POINTER(ctypes.c_void_p), ctypes.c_int]),
    "svjg_comm_error": (ctypes.c_int, [ctypes.c_char_p, ctypes.c_uint64]),
    "svjg_allreduce_counts_all": (ctypes.c_int, [ctypes.POINTER(ctypes.c_void_p), ctypes.c_int]),
    "svjg_genotype": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64,
                                     ctypes.c_uint32, ctypes.c_double, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                                     ctypes.c_void_p]),
    "svjg_genotype_view": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64,
                                          ctypes.c_uint32, ctypes.c_double] + [ctypes.POINTER(ctypes.c_void_p)] * 4),
    "svjg_genotype_ploidy": (ctypes.c_int, [ctypes.c_void_p] * 5 + [ctypes.c_uint64, ctypes.c_uint32, ctypes.c_double] + [ctypes.c_void_p] * 5),
    "svjg_genotype_sites": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_uint32, ctypes.c_double] + [ctypes.c_void_p] * 4),
    "svjg_cohort_alloc": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint32]),
    "svjg_cohort_set_counts": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_uint32, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64]),
    "svjg_cohort_store_counts": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_uint32]),
    "svjg_cohort_get_counts": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_uint32, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint32]),
    "svjg_genotype_cohort": (ctypes.c_int, [ctypes.c_void_p] * 4 + [ctypes.c_uint64, ctypes.c_uint32, ctypes.c_double] + [ctypes.c_void_p] * 6),
    "svjg_genotype_cohort_ploidy": (ctypes.c_int, [ctypes.c_void_p] * 5 + [ctypes.c_uint32, ctypes.c_uint64, ctypes.c_uint32, ctypes.c_double] + [ctypes.c_void_p] * 6),
    "svjg_genotype_cohort_prior": (ctypes.c_int, [ctypes.c_void_p] * 5 + [ctypes.c_uint32, ctypes.c_uint64, ctypes.c_uint32, ctypes.c_double] + [ctypes.c_void_p] * 9),
    "svjg_genotype_cohort_sites": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_uint32, ctypes.c_double] + [ctypes.c_void_p] * 6),
    "svjg_genotype_cohort_sites_prior": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_uint32, ctypes.c_double] + [ctypes.c_void_p] * 11),
    "svjg_cohort_qual": (ctypes.c_int, [ctypes.c_void_p] * 5 + [ctypes.c_uint32, ctypes.c_uint64, ctypes.c_double, ctypes.c_double] + [ctypes.c_void_p] * 3),
    "svjg_cohort_qc": (ctypes.c_int, [ctypes.c_void_p] * 3 + [ctypes.c_uint64, ctypes.c_uint32] + [ctypes.c_void_p] * 2),
    "svjg_cohort_hwe": (ctypes.c_int, [ctypes.c_void_p] * 3 + [ctypes.c_uint64, ctypes.c_uint32] + [ctypes.c_void_p] * 2),
    "svjg_set_rows": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64]),
    "svjg_run_resident": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_uint64, ctypes.c_uint32, ctypes.c_double] + [ctypes.POINTER(ctypes.c_void_p)] * 5),
    "svjg_run_begin": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_uint64, ctypes.c_uint32, ctypes.c_double]),
    "svjg_run_end": (ctypes.c_int, [ctypes.c_void_p] + [ctypes.POINTER(ctypes.c_void_p)] * 5),
    "svjg_genotype_boundary": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64]),
    "svjg_logfact_reserve": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_uint32]),
    "svjg_logfact_read": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_void_p, ctypes.POINTER(ctypes.c_uint32)]),
    "svjg_last_kernel_ms": (ctypes.c_int, [ctypes.c_void_p, ctypes.POINTER(ctypes.c_float), ctypes.POINTER(ctypes.c_float),
                                           ctypes.POINTER(ctypes.c_float)]),
    "svjg_last_main_ms": (ctypes.c_int, [ctypes.c_void_p, ctypes.POINTER(ctypes.c_float), ctypes.POINTER(ctypes.c_float)]),
    "svjg_sync": (ctypes.c_int, [ctypes.c_void_p]),
    "svjg_set_main_workers": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_uint32]),
    "svjg_last_main_plan": (ctypes.c_int, [ctypes.c_void_p, ctypes.POINTER(ctypes.c_uint64), ctypes.POINTER(ctypes.c_uint64), ctypes.POINTER(ctypes.c_uint32),
                                           ctypes.POINTER(ctypes.c_uint64)]),
}

EXPORTS = tuple(_SIGS) + ("svjg_write_informative_json", "svjg_count_informative_json", "svjg_host_free",
                          "svjg_graph_load", "svjg_graph_view", "svjg_graph_info", "svjg_graph_free",
                          "svjg_vcf_load", "svjg_vcf_arrays", "svjg_vcf_write", "svjg_vcf_free")
MAX_PLOIDY = 8                      # svjg.h: SVJG_MAX_PLOIDY
MAX_SITE_ALTS = 6                   # svjg.h: SVJG_MAX_SITE_ALTS
SITE_GENOTYPES = 28                 # svjg.h: SVJG_SITE_GENOTYPES
QC_MAX_SAMPLES = 2048               # svjg.h: SVJG_QC_MAX_SAMPLES
HWE_MAX_SAMPLES = 65536             # svjg.h: SVJG_HWE_MAX_SAMPLES
QUAL_THETA = 1e-3                   # the default theta of the site quality (svjg_cohort_qual; the library takes a value in (0, 0.05])
_lib = None
_host_lib = None


def load_host_library():
    """libsvjg_host.so: the native JSON writer (plain C++, no GPU)."""
    global _host_lib
    if _host_lib is None:
        if not os.path.exists(HOST_LIB_PATH):
            raise SvjgError(f"{HOST_LIB_PATH} not found: build it first (python __graft_entry__.py build)")
        lib = ctypes.CDLL(HOST_LIB_PATH)
        lib.svjg_write_informative_json.restype = ctypes.c_int
        lib.svjg_write_informative_json.argtypes = [ctypes.c_char_p, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p, ctypes.c_uint64,
                                                    ctypes.POINTER(ctypes.c_char_p), ctypes.c_uint32, ctypes.c_int]
        lib.svjg_count_informative_json.restype = ctypes.c_int
        lib.svjg_count_informative_json.argtypes = [ctypes.c_char_p, ctypes.POINTER(ctypes.c_void_p), ctypes.POINTER(ctypes.c_uint64),
                                                    ctypes.POINTER(ctypes.c_void_p), ctypes.POINTER(ctypes.c_uint64)]
        lib.svjg_host_free.restype = None
        lib.svjg_host_free.argtypes = [ctypes.c_void_p]
        lib.svjg_graph_load.restype = ctypes.c_int
        lib.svjg_graph_load.argtypes = [ctypes.c_char_p, ctypes.c_char_p, ctypes.POINTER(ctypes.c_void_p)]
        lib.svjg_graph_view.restype = ctypes.POINTER(CGraph)
        lib.svjg_graph_view.argtypes = [ctypes.c_void_p]
        lib.svjg_graph_info.restype = ctypes.c_int
        lib.svjg_graph_info.argtypes = [ctypes.c_void_p, ctypes.POINTER(ctypes.c_void_p), ctypes.POINTER(ctypes.c_uint64), ctypes.POINTER(ctypes.c_uint32)]
        lib.svjg_graph_free.restype = None
        lib.svjg_graph_free.argtypes = [ctypes.c_void_p]
        lib.svjg_vcf_load.restype = ctypes.c_int
        lib.svjg_vcf_load.argtypes = [ctypes.c_char_p, ctypes.c_char_p, ctypes.c_uint64, ctypes.c_void_p, ctypes.c_uint32, ctypes.c_int,
                                      ctypes.POINTER(ctypes.c_void_p)]
        lib.svjg_vcf_arrays.restype = ctypes.c_int
        lib.svjg_vcf_arrays.argtypes = [ctypes.c_void_p] + [ctypes.POINTER(ctypes.c_void_p)] * 3 + [ctypes.POINTER(ctypes.c_uint64)]
        lib.svjg_vcf_write.restype = ctypes.c_int
        lib.svjg_vcf_write.argtypes = [ctypes.c_void_p, ctypes.c_char_p] + [ctypes.c_void_p] * 4 + [ctypes.POINTER(ctypes.c_uint64)]
        lib.svjg_vcf_free.restype = None
        lib.svjg_vcf_free.argtypes = [ctypes.c_void_p]
        _host_lib = lib
    return _host_lib


class NativeVcfRows:
    """Rows of a VCF held by libsvjg_host (svjg_vcf_*): the same three arrays as svjg.genotype.VcfRows, and the writer."""

    def __init__(self, lib, h):
        self.lib, self.h = lib, h
        p = [ctypes.c_void_p() for _ in range(3)]
        n = ctypes.c_uint64(0)
        lib.svjg_vcf_arrays(h, ctypes.byref(p[0]), ctypes.byref(p[1]), ctypes.byref(p[2]), ctypes.byref(n))
        n = n.value

        def arr(ptr, dt):
            return np.frombuffer(ctypes.string_at(ptr, n * np.dtype(dt).itemsize), dtype=dt).copy() if n else np.zeros(0, dtype=dt)
        self.sv_type, self.slot, self.ok = arr(p[0], np.uint8), arr(p[1], np.uint32), arr(p[2], np.uint8)

    def write(self, out_path, gt, pl, raw, done):
        gt = np.ascontiguousarray(gt, dtype=np.uint8); pl = np.ascontiguousarray(pl, dtype=np.int64)
        raw = np.ascontiguousarray(raw, dtype=np.uint32); done = np.ascontiguousarray(done, dtype=np.uint8)
        n = len(self.sv_type)
        if len(gt) != n or pl.shape != (n, 3) or raw.shape != (n, 2) or len(done) != n:
            raise ValueError("result arrays do not match the rows")
        nd = ctypes.c_uint64(0)
        rc = self.lib.svjg_vcf_write(self.h, os.fsencode(out_path), gt.ctypes.data, pl.ctypes.data, raw.ctypes.data, done.ctypes.data, ctypes.byref(nd))
        if rc:
            raise OSError(f"cannot write {out_path} ({rc})")
        return nd.value

    def close(self):
        if self.h:
            self.lib.svjg_vcf_free(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def vcf_load_native(vcf_path, keys, slots=None, slot_is_presence=False):
    """NativeVcfRows, or None when the native reader leaves the file to svjg.genotype.VcfRows.  keys: iterable of sv_id strings
    (slots: their count slots, default 0..n-1)."""
    lib = load_host_library()
    keys = list(keys)
    try:
        blob = ("\0".join(keys) + "\0").encode("ascii") if keys else b""
    except UnicodeEncodeError:
        return None
    if blob.count(b"\0") != len(keys):                          # a NUL inside a key
        return None
    sl = None if slots is None else np.ascontiguousarray(slots, dtype=np.uint32)
    h = ctypes.c_void_p()
    rc = lib.svjg_vcf_load(os.fsencode(vcf_path), blob, len(blob), None if sl is None else sl.ctypes.data, len(keys), int(slot_is_presence), ctypes.byref(h))
    if rc == -11:
        return None
    if rc:
        raise SvjgError(f"svjg_vcf_load failed ({rc})")
    return NativeVcfRows(lib, h)


def graph_load_native(edges_json, gfa):
    """Tables of a svjg.graph.Graph from the native loader, or None when it leaves the input to the Python loader.
    -> dict(nodes, edges, hits, n_edges, n_hits, chrom_names (bytes), chrom_off, chrom_lo, sv_ids (list), n_hazard)"""
    lib = load_host_library()
    h = ctypes.c_void_p()
    rc = lib.svjg_graph_load(os.fsencode(edges_json), os.fsencode(gfa), ctypes.byref(h))
    if rc == -11:
        return None
    if rc:
        raise OSError(f"cannot read {edges_json} / {gfa}")
    try:
        v = lib.svjg_graph_view(h).contents
        from .graph import NODE_DT, EDGE_DT

        def arr(ptr, n, dt):
            if n == 0:
                return np.zeros(0, dtype=dt)
            return np.frombuffer(ctypes.string_at(ptr, n * np.dtype(dt).itemsize), dtype=dt).copy()
        n_chrom = v.n_chrom
        # (the field is declared c_char_p for the callers that PASS names in; read as such it is a Python bytes object cut at the first
        #  NUL, and string_at() of that would run past its end: take the raw pointer)
        names_ptr = ctypes.c_void_p.from_buffer(v, type(v).chrom_names.offset).value
        chrom_off = arr(v.chrom_off, n_chrom + 1, np.uint32)
        blob, blen, nhz = ctypes.c_void_p(), ctypes.c_uint64(0), ctypes.c_uint32(0)
        lib.svjg_graph_info(h, ctypes.byref(blob), ctypes.byref(blen), ctypes.byref(nhz))
        sv = ctypes.string_at(blob, blen.value).decode("ascii").split("\0")[:-1] if blen.value else []
        return dict(
            nodes=arr(v.nodes, v.n_nodes + 1, NODE_DT), n_nodes=int(v.n_nodes),
            edges=arr(v.edges, max(1, v.n_edges), EDGE_DT), n_edges=int(v.n_edges),
            hits=arr(v.hits, max(1, v.n_hits), np.uint32), n_hits=int(v.n_hits),
            chrom_names=ctypes.string_at(names_ptr, int(chrom_off[-1]) + 4), chrom_off=chrom_off,
            chrom_lo=arr(v.chrom_node_lo, n_chrom + 1, np.uint32), sv_ids=sv, n_hazard=int(nhz.value))
    finally:
        lib.svjg_graph_free(h)


def count_informative_json(path):
    """-> (list of keys in file order, uint32 array [n, 2] of list lengths) of an _informative_aln.json."""
    lib = load_host_library()
    kp, cp = ctypes.c_void_p(), ctypes.c_void_p()
    kl, nk = ctypes.c_uint64(0), ctypes.c_uint64(0)
    rc = lib.svjg_count_informative_json(os.fsencode(path), ctypes.byref(kp), ctypes.byref(kl), ctypes.byref(cp), ctypes.byref(nk))
    if rc == -10:
        raise ValueError(f"{path}: not the JSON written by filter-alignments.py")
    if rc:
        raise OSError(f"cannot read {path}")
    try:
        blob = ctypes.string_at(kp, kl.value)
        keys = [k.decode("utf-8") for k in blob.split(b"\0")[:-1]] if kl.value else []
        if nk.value:
            cnt = np.ctypeslib.as_array(ctypes.cast(cp, ctypes.POINTER(ctypes.c_uint64)), shape=(nk.value * 2,)).copy()
        else:
            cnt = np.zeros(0, dtype=np.uint64)                      # (nothing to read: the buffer may be empty)
    finally:
        lib.svjg_host_free(kp); lib.svjg_host_free(cp)
    if (cnt >= 2 ** 32).any():
        raise ValueError("list too long")
    return keys, cnt.astype(np.uint32).reshape(-1, 2)


def write_informative_json(path, gaf, recs, sv_ids, n_threads=0):
    """<prefix>_informative_aln.json from hit records (filter-alignments.py:174-175)."""
    lib = load_host_library()
    a = _as_u8(gaf)
    n_threads = n_threads or int(os.environ.get("SVJG_JSON_THREADS", "0"))
    recs = np.ascontiguousarray(recs, dtype=HITREC_DT)
    keys = (ctypes.c_char_p * max(1, len(sv_ids)))(*[s.encode("utf-8") for s in sv_ids])
    rc = lib.svjg_write_informative_json(os.fsencode(path), a.ctypes.data if a.size else None, a.size,
                                         recs.ctypes.data if len(recs) else None, len(recs), keys, len(sv_ids), n_threads)
    if rc == -10:
        raise UnicodeDecodeError("utf-8", b"", 0, 1, "invalid UTF-8 in an informative alignment line")
    if rc:
        raise SvjgError(f"svjg_write_informative_json failed ({rc}) for {path}")


def load_library(path=None):
    """dlopen the HIP library and attach the prototypes.  Raises if it has not been built."""
    global _lib
    if _lib is not None and path is None:
        return _lib
    p = path or os.environ.get("SVJG_HIP_LIB") or LIB_PATH    # SVJG_HIP_LIB: a measurement build of the same library (tools/mkvariant.sh -> build/lib_<name>.so)
    if p != LIB_PATH and path is None:
        sys.stderr.write(f"[svjg] measurement build in use: {p}\n")
    if not os.path.exists(p):
        raise SvjgError(f"{p} not found: build it first (python __graft_entry__.py build, needs hipcc); there is no CPU fallback")
    # Copies by shader, not by the copy engines: the ROCm runtime creates the queue of a copy engine the first time a copy happens
    # to be handed to it (6-7 ms each, several engines, at unpredictable calls early in a process: one `svjg_genotype` call of
    # 6.4 ms among 0.13 ms ones).  Must be in the environment before the runtime starts, i.e. before the first HIP call of the
    # process; the price is a slower bulk upload (41 instead of 56 GB/s).  SVJG_SDMA=1 keeps the runtime's default.
    if os.environ.get("SVJG_SDMA", "0") != "1":
        os.environ.setdefault("HSA_ENABLE_SDMA", "0")
    lib = ctypes.CDLL(p)
    for name, (res, args) in _SIGS.items():
        fn = getattr(lib, name)
        fn.restype = res
        fn.argtypes = args
    if lib.svjg_abi_version() != 1:
        raise SvjgError("libsvjg_hip.so ABI mismatch")
    if path is None:
        _lib = lib
    return lib


def _row_inputs(sv_type, slot, ok):
    """the three per-row input arrays of a genotype call in the element types the library reads"""
    return np.ascontiguousarray(sv_type, dtype=np.uint8), np.ascontiguousarray(slot, dtype=np.uint32), np.ascontiguousarray(ok, dtype=np.uint8)


def _view(ptr, count, dtype):
    """`count` elements at the library's pointer as a read-only array: no copy"""
    a = np.frombuffer((ctypes.c_char * (count * np.dtype(dtype).itemsize)).from_address(ptr.value), dtype=dtype)
    a.flags.writeable = False
    return a


def _max_ploidy(max_ploidy):
    """a cohort call's max_ploidy as the library takes it (a value out of 1..MAX_PLOIDY is the library's to refuse: nothing is written then)"""
    if not 0 <= int(max_ploidy) <= 0xFFFFFFFF:
        raise SvjgError("max_ploidy: 1..%d" % MAX_PLOIDY)
    return int(max_ploidy)


def _ploidy_matrix(ploidy, n, S):
    """a cohort call's ploidy[n, S] in the element type the library reads"""
    ploidy = np.asarray(ploidy)
    if ploidy.shape != (n, S) or (ploidy.size and (int(ploidy.min()) < 0 or int(ploidy.max()) > 255)):
        raise SvjgError("ploidy: one value in 0..max_ploidy per (row, sample)")
    return np.ascontiguousarray(ploidy, dtype=np.uint8)


def _calls_in(gt, ploidy):
    """a run's calls as cohort_qc and cohort_hwe take them -> (gt[n, S] uint8, ploidy the same or None, n, S)"""
    gt = np.ascontiguousarray(gt, dtype=np.uint8)
    if gt.ndim != 2:
        raise ValueError("gt must be [n_rows, n_samples]")
    if ploidy is not None:
        ploidy = np.ascontiguousarray(ploidy, dtype=np.uint8)
        if ploidy.shape != gt.shape:
            raise ValueError("ploidy must have gt's shape")
    return (gt, ploidy) + gt.shape


class Context:
    """One GPU.  Thin, stateful wrapper over the C ABI."""

    def __init__(self, device=0):
        self.lib = load_library()
        h = ctypes.c_void_p()
        rc = self.lib.svjg_init(device, ctypes.byref(h))
        if rc:
            msg = self.lib.svjg_last_error(None)
            raise SvjgError(f"svjg_init failed ({rc}): {msg.decode() if msg else ''}")
        self.h = h
        self.graph = None
        self._cohort = (0, 0)                                   # (n_samples, n_slots) of the cohort matrix (cohort_alloc)

    def close(self):
        if getattr(self, "h", None):
            self.lib.svjg_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _chk(self, rc):
        if rc == -10:
            cls, off = ctypes.c_int(0), ctypes.c_uint64(0)
            self.lib.svjg_input_error(self.h, ctypes.byref(cls), ctypes.byref(off))
            e = TypeError(DOVER_TYPE_ERROR) if cls.value == 6 else EXC_CLASS.get(cls.value, ValueError)(f"malformed GAF line at byte offset {off.value}")
            e.svjg_offset = off.value                           # (svjg/filter.py: reference_error)
            raise e
        if rc == -12:
            raise OverflowError(self.lib.svjg_last_error(self.h).decode())
        if rc:
            raise SvjgError(f"libsvjg_hip error {rc}: {self.lib.svjg_last_error(self.h).decode()}")

    def load_graph(self, g):
        self.graph = g
        self.n_slots = g.n_slots
        cg = cgraph_of(g)
        self._chk(self.lib.svjg_load_graph(self.h, ctypes.byref(cg)))

    def alloc_counts(self, n_slots):
        self.graph = None
        self.n_slots = n_slots
        self._chk(self.lib.svjg_alloc_counts(self.h, n_slots))

    def upload(self, gaf):
        a = _as_u8(gaf)
        self._chk(self.lib.svjg_gaf_upload(self.h, a.ctypes.data if a.size else None, a.size))

    def upload_parts(self, parts, capacity_bytes):
        """the resident text from an iterable of pieces (ascending; at most `capacity_bytes` in all): a text the host never holds
        whole (svjg_gaf_upload_part).  -> bytes uploaded"""
        at, prev = 0, None
        for p in parts:
            if prev is not None:
                self._chk(self.lib.svjg_gaf_upload_part(self.h, prev.ctypes.data if prev.size else None, prev.size, at, capacity_bytes, 0))
                at += int(prev.size)
            prev = _as_u8(p)
        if prev is None:
            prev = np.zeros(0, dtype=np.uint8)
        self._chk(self.lib.svjg_gaf_upload_part(self.h, prev.ctypes.data if prev.size else None, prev.size, at, capacity_bytes, 1))
        return at + int(prev.size)

    def allreduce_on_second_stream(self, on):
        """where the fused pass puts its all-reduce (svjg_comm_set_stream): False = the compute stream (default)"""
        self._chk(self.lib.svjg_comm_set_stream(self.h, 1 if on else 0))

    def copy_rate(self, n_bytes=1 << 31):
        """-> (GB/s read + written by a plain device-to-device copy, GB/s of a kernel that only reads) on this GPU (svjg_copy_rate)"""
        v, r = ctypes.c_double(0), ctypes.c_double(0)
        self._chk(self.lib.svjg_copy_rate(self.h, n_bytes, ctypes.byref(v), ctypes.byref(r)))
        return v.value, r.value

    def classify_resident(self, base_offset=0, want_hits=False):
        self._chk(self.lib.svjg_classify_resident(self.h, base_offset, int(want_hits)))

    def classify(self, gaf, base_offset=0, want_hits=False):
        a = _as_u8(gaf)
        self._chk(self.lib.svjg_classify(self.h, a.ctypes.data if a.size else None, a.size, base_offset, int(want_hits)))

    def classify_file(self, path, offset, n_bytes, want_hits=False):
        """bytes [offset, offset + n_bytes) of the file, read by the library's feeder threads (no host copy here); a read
        error surfaces as OSError like the reference's own open()/read would"""
        rc = self.lib.svjg_classify_file(self.h, os.fsencode(path), offset, n_bytes, int(want_hits))
        if rc == -6:
            raise OSError(self.lib.svjg_last_error(self.h).decode())
        self._chk(rc)

    def reset_counts(self):
        self._chk(self.lib.svjg_reset_counts(self.h))

    def stats(self):
        s = CStats()
        self._chk(self.lib.svjg_get_stats(self.h, ctypes.byref(s)))
        return {"n_lines": s.n_lines, "n_deferred": s.n_deferred, "n_hitrecs": s.n_hitrecs, "non_ascii": s.non_ascii}

    def defer_causes(self):
        """why lines took the exact path (svjg_get_defer_causes)"""
        out = np.zeros(8, dtype=np.uint64)
        self._chk(self.lib.svjg_get_defer_causes(self.h, out.ctypes.data))
        return dict(zip(("columns", "id_tag_filter", "long_path", "node_name", "whole_stripe"), (int(x) for x in out[:5])))

    def counts(self):
        out = np.zeros((self.n_slots, 2), dtype=np.uint32)
        self._chk(self.lib.svjg_get_counts(self.h, out.ctypes.data, self.n_slots))
        return out

    def set_counts(self, c):
        c = np.ascontiguousarray(c, dtype=np.uint32)
        assert c.shape == (self.n_slots, 2)
        self._chk(self.lib.svjg_set_counts(self.h, c.ctypes.data, self.n_slots))

    def hits(self, out=None):
        """the hit records of this context -> a new array, or into `out` (a contiguous slice of HITREC_DT sized stats()["n_hitrecs"]:
        several contexts fill one array side by side, no concatenation afterwards)"""
        n = self.stats()["n_hitrecs"]
        if out is None:
            out = np.empty(n, dtype=HITREC_DT)
        assert out.dtype == HITREC_DT and out.flags["C_CONTIGUOUS"] and len(out) == n
        got = ctypes.c_uint64(0)
        self._chk(self.lib.svjg_get_hits(self.h, out.ctypes.data, n, ctypes.byref(got)))
        assert got.value == n
        return out

    def host_lines(self):
        """byte offsets of the lines the kernels set aside for the host (svjg.h: SVJG_EXC_ASK_HOST), in file order"""
        n = ctypes.c_uint64(0)
        self._chk(self.lib.svjg_get_host_lines(self.h, None, 0, ctypes.byref(n)))
        out = np.zeros(n.value, dtype=np.uint64)
        if n.value:
            self._chk(self.lib.svjg_get_host_lines(self.h, out.ctypes.data, n.value, ctypes.byref(n)))
        return np.sort(out)

    def comm_init(self, unique_id, n_ranks, rank):
        self._chk(self.lib.svjg_comm_init(self.h, unique_id, n_ranks, rank))

    def allreduce_counts(self):
        self._chk(self.lib.svjg_allreduce_counts(self.h))

    def genotype(self, sv_type, slot, ok, min_support, err, reuse_outputs=False):
        """-> (gt, pl[n, 3], raw[n, 2], genotyped).  reuse_outputs: the arrays are read-only views of the library's pinned
        result block (svjg_genotype_view: no copy); they are overwritten by the next call and die with the context, so copy
        what has to outlive either."""
        n = len(sv_type)
        sv_type, slot, ok = _row_inputs(sv_type, slot, ok)
        if reuse_outputs and n:
            p = [ctypes.c_void_p() for _ in range(4)]
            self._chk(self.lib.svjg_genotype_view(self.h, sv_type.ctypes.data, slot.ctypes.data, ok.ctypes.data, n, min_support,
                                                  float(err), *[ctypes.byref(x) for x in p]))
            return _view(p[0], n, np.uint8), _view(p[1], n * 3, np.int64).reshape(n, 3), _view(p[2], n * 2, np.uint32).reshape(n, 2), _view(p[3], n, np.uint8)
        gt = np.empty(n, dtype=np.uint8)
        pl = np.empty((n, 3), dtype=np.int64)
        raw = np.empty((n, 2), dtype=np.uint32)
        done = np.empty(n, dtype=np.uint8)
        self._chk(self.lib.svjg_genotype(self.h, sv_type.ctypes.data, slot.ctypes.data, ok.ctypes.data, n, min_support,
                                         float(err), gt.ctypes.data, pl.ctypes.data, raw.ctypes.data, done.ctypes.data))
        return gt, pl, raw, done

    def genotype_ploidy(self, sv_type, slot, ok, ploidy, min_support, err):
        """Any ploidy from 1 to MAX_PLOIDY per row (svjg_genotype_ploidy; ploidy 0: the row is never genotyped).
        -> (gt = alt copies or 0xFF, pl[n, 9] = PL_0..PL_P then zeros, raw[n, 2], genotyped, boundary = the rows to recompute with
        svjg.genotype.exact_pl_ploidy)"""
        n = len(sv_type)
        sv_type, slot, ok = _row_inputs(sv_type, slot, ok)
        ploidy = np.asarray(ploidy)
        if n and (len(ploidy) != n or int(ploidy.min()) < 0 or int(ploidy.max()) > 255):
            raise SvjgError("ploidy: one value in 0..%d per row" % MAX_PLOIDY)
        ploidy = np.ascontiguousarray(ploidy, dtype=np.uint8)
        gt = np.empty(n, dtype=np.uint8)
        pl = np.empty((n, MAX_PLOIDY + 1), dtype=np.int64)
        raw = np.empty((n, 2), dtype=np.uint32)
        done = np.empty(n, dtype=np.uint8)
        boundary = np.empty(n, dtype=np.uint8)
        self._chk(self.lib.svjg_genotype_ploidy(self.h, sv_type.ctypes.data, slot.ctypes.data, ok.ctypes.data, ploidy.ctypes.data, n,
                                                min_support, float(err), gt.ctypes.data, pl.ctypes.data, raw.ctypes.data,
                                                done.ctypes.data, boundary.ctypes.data))
        return gt, pl, raw, done, boundary

    def genotype_sites(self, slots, min_support, err):
        """Insertions that share a position, genotyped together (svjg_genotype_sites).  slots[n, 6]: the members' count slots first, 0xFFFFFFFF
        behind them.  -> (gt[n, 2] = the pair (a, b) or 0xFF, 0xFF, pl[n, 28] in VCF order then zeros, raw[n, 7] = ref maximum and alt_1..alt_6,
        boundary = the sites to recompute with svjg.genotype.exact_pl_site)"""
        return self._sites_call(self.lib.svjg_genotype_sites, slots, min_support, err)

    def _sites_call(self, fn, slots, min_support, err, cohort=False, prior=False):
        """The three site calls: the slot matrix's check, the output arrays (per site; cohort: per (site, sample) item, with members and the site
        words; prior: the posterior's five behind those) and the call of library function `fn`"""
        slots = np.ascontiguousarray(slots, dtype=np.uint32)
        if slots.ndim != 2 or slots.shape[1] != MAX_SITE_ALTS:
            raise SvjgError("slots: %d per site" % MAX_SITE_ALTS)
        n = len(slots)
        at = (n, self._cohort[0]) if cohort else (n,)
        out = (np.empty(at + (2,), np.uint8), np.empty(at + (SITE_GENOTYPES,), np.int64), np.empty(at + (MAX_SITE_ALTS + 1,), np.uint32), np.empty(at, np.uint8))
        if cohort:
            out = out[:3] + (np.empty(at, np.uint8), out[3], np.empty((n, MAX_SITE_ALTS, 2), np.uint32))
        if prior:
            out += (np.empty(at + (2,), np.uint8), np.empty(at, np.uint8), np.empty((n, MAX_SITE_ALTS + 1), np.float64), np.empty(n, np.uint32),
                    np.empty((n, MAX_SITE_ALTS, 2), np.uint32))
        self._chk(fn(self.h, slots.ctypes.data, n, min_support, float(err), *(a.ctypes.data for a in out)))
        return out

    def cohort_alloc(self, n_samples, n_slots):
        """a zeroed count matrix of n_samples x n_slots with its presence bytes (svjg_cohort_alloc); a second call replaces it"""
        self._chk(self.lib.svjg_cohort_alloc(self.h, int(n_samples), int(n_slots)))
        self._cohort = (int(n_samples), int(n_slots))

    def cohort_set_counts(self, sample, slots, counts):
        """the slots `sample` has as keys with their (ref, alt) counts[k]; every other slot of the sample becomes absent (svjg_cohort_set_counts)"""
        slots = np.ascontiguousarray(slots, dtype=np.uint32)
        counts = np.ascontiguousarray(counts, dtype=np.uint32).reshape(-1, 2)
        if len(slots) != len(counts) or slots.ndim != 1:
            raise SvjgError("cohort_set_counts: one (ref, alt) pair per slot")
        n = len(slots)
        self._chk(self.lib.svjg_cohort_set_counts(self.h, int(sample), slots.ctypes.data if n else None, counts.ctypes.data if n else None, n))

    def cohort_store_counts(self, sample):
        """the context's current count vector -> column `sample`, on the device; presence = a non-zero count (svjg_cohort_store_counts)"""
        self._chk(self.lib.svjg_cohort_store_counts(self.h, int(sample)))

    def cohort_get_counts(self, sample):
        """-> (counts[n_slots, 2], present[n_slots]) of one sample (svjg_cohort_get_counts)"""
        n_slots = self._cohort[1]
        out = np.zeros((n_slots, 2), dtype=np.uint32)
        present = np.zeros(n_slots, dtype=np.uint8)
        self._chk(self.lib.svjg_cohort_get_counts(self.h, int(sample), out.ctypes.data, present.ctypes.data, n_slots))
        return out, present

    def _cohort_call(self, fn, sv_type, slot, ok, ploidy, max_ploidy, min_support, err, ploidy_pair=True, need_ploidy=False, prior=False):
        """The three cohort calls: the checks, the output arrays and the call of library function `fn`.  ploidy_pair: fn takes (ploidy, max_ploidy)
        and gives site[n, 3], else site[n, 2]; need_ploidy: ploidy may not be None; prior: fn gives (gq[n, S], af[n], em_steps[n]) as well.
        -> (gt[n, S], pl[n, S, max_ploidy + 1], raw[n, S, 2], genotyped[n, S], boundary[n, S], site) and the prior's three"""
        n, S = len(sv_type), self._cohort[0]
        max_ploidy = _max_ploidy(max_ploidy)
        width = min(max_ploidy, MAX_PLOIDY) + 1
        sv_type, slot, ok = _row_inputs(sv_type, slot, ok)
        if ploidy is not None or need_ploidy:
            ploidy = _ploidy_matrix(ploidy, n, S)
        out = (np.empty((n, S), np.uint8), np.empty((n, S, width), np.int64), np.empty((n, S, 2), np.uint32), np.empty((n, S), np.uint8),
               np.empty((n, S), np.uint8), np.empty((n, 3 if ploidy_pair else 2), np.uint32))
        if prior:
            out += (np.empty((n, S), np.uint8), np.empty(n, np.float64), np.empty(n, np.uint32))
        kind = (None if ploidy is None else ploidy.ctypes.data, max_ploidy) if ploidy_pair else ()
        self._chk(fn(self.h, sv_type.ctypes.data, slot.ctypes.data, ok.ctypes.data, *kind, n, min_support, float(err), *(a.ctypes.data for a in out)))
        return out

    def genotype_cohort(self, sv_type, slot, ok, min_support, err):
        """Every row against every sample of the cohort matrix (svjg_genotype_cohort; ok bit 1 is ignored: the presence bytes decide).
        -> (gt[n, S], pl[n, S, 3], raw[n, S, 2], genotyped[n, S], boundary[n, S] = the items to recompute with svjg.genotype.exact_pl,
        site[n, 2] = NS and AC of each row)"""
        return self._cohort_call(self.lib.svjg_genotype_cohort, sv_type, slot, ok, None, 2, min_support, err, ploidy_pair=False)

    def genotype_cohort_ploidy(self, sv_type, slot, ok, ploidy, max_ploidy, min_support, err):
        """Every row against every sample of the cohort matrix at a ploidy per item (svjg_genotype_cohort_ploidy): ploidy[n, S] in 0..max_ploidy,
        0 = the item is never genotyped.  -> (gt[n, S] = alt copies or 0xFF, pl[n, S, max_ploidy + 1] = PL_0..PL_P then zeros, raw[n, S, 2],
        genotyped[n, S], boundary[n, S] = the items to recompute with svjg.genotype.exact_pl_ploidy, site[n, 3] = NS, AN and AC of each row)"""
        return self._cohort_call(self.lib.svjg_genotype_cohort_ploidy, sv_type, slot, ok, ploidy, max_ploidy, min_support, err, need_ploidy=True)

    def genotype_cohort_prior(self, sv_type, slot, ok, ploidy, max_ploidy, min_support, err):
        """The cohort call with an allele-frequency prior (svjg_genotype_cohort_prior).  ploidy: [n, S] in 0..max_ploidy, or None = every item
        diploid (max_ploidy must then be 2).  -> (gt[n, S] = alt copies of the POSTERIOR call or 0xFF, pl[n, S, max_ploidy + 1], raw[n, S, 2],
        genotyped[n, S], boundary[n, S] — pl, raw, genotyped and boundary as genotype_cohort / genotype_cohort_ploidy give them —, site[n, 3] =
        NS, AN, AC of the posterior calls, gq[n, S] (0xFF: none), af[n] (NaN: no estimate), em_steps[n] (bit 31: not converged))"""
        return self._cohort_call(self.lib.svjg_genotype_cohort_prior, sv_type, slot, ok, ploidy, max_ploidy, min_support, err, prior=True)

    def cohort_qual(self, sv_type, slot, ok, ploidy, max_ploidy, err, theta=QUAL_THETA):
        """The site quality of every row against the cohort matrix: the exact allele-count posterior (svjg_cohort_qual).  ploidy: [n, S] in
        0..max_ploidy, or None = every item diploid (max_ploidy must then be 2).  -> (qual[n] = -10 log10 of the posterior of "no alt copy in the
        cohort", NaN where no item took part; mlac[n] = the allele count at the posterior's maximum; chroms[n] = the chromosomes that took part)"""
        n = len(sv_type)
        max_ploidy = _max_ploidy(max_ploidy)
        sv_type, slot, ok = _row_inputs(sv_type, slot, ok)
        if ploidy is not None:
            ploidy = _ploidy_matrix(ploidy, n, self._cohort[0])
        out = (np.empty(n, np.float64), np.empty(n, np.uint32), np.empty(n, np.uint32))
        self._chk(self.lib.svjg_cohort_qual(self.h, sv_type.ctypes.data, slot.ctypes.data, ok.ctypes.data, None if ploidy is None else ploidy.ctypes.data,
                                            max_ploidy, n, float(err), float(theta), *(a.ctypes.data for a in out)))
        return out

    def cohort_qc(self, gt, ploidy=None):
        """The samples of a cohort from its calls (svjg_cohort_qc): gt[n, S] = alt copies, ploidy[n, S] or None (2 everywhere); an item with
        gt > ploidy (3, 0xFF) is not called, one with ploidy 0 not eligible.  It reads nothing of the context's matrix or counts.
        -> (sample[S, 6] = eligible, called, carrier, diploid, het, homalt; pair[S (S - 1) / 2, 5] = both, het1, het2, hethet, ibs0 of the pairs
        i < j at k = i S - i (i + 1) / 2 + (j - i - 1), over the items both diploid), uint32 sums over the rows"""
        gt, ploidy, n, S = _calls_in(gt, ploidy)
        sample, pair = np.empty((S, 6), np.uint32), np.empty((S * (S - 1) // 2 if S else 0, 5), np.uint32)
        self._chk(self.lib.svjg_cohort_qc(self.h, gt.ctypes.data, None if ploidy is None else ploidy.ctypes.data, n, S, sample.ctypes.data,
                                          pair.ctypes.data if len(pair) else None))
        return sample, pair

    def cohort_hwe(self, gt, ploidy=None):
        """The sites of a cohort from its calls (svjg_cohort_hwe): gt[n, S] = alt copies, ploidy[n, S] or None (2 everywhere); only the called
        diploid items of a row enter (ploidy 2 and gt <= 2).  It reads nothing of the context's matrix or counts.
        -> (counts[n, 3] = n_ref, n_het, n_alt, uint32; p[n, 2] = HWE, the two-sided exact test, and EXCHET, the one-sided one for excess
        heterozygotes, float64: 1.0 for a row without a minor allele, NaN for a row without an item)"""
        gt, ploidy, n, S = _calls_in(gt, ploidy)
        counts, p = np.empty((n, 3), np.uint32), np.empty((n, 2), np.float64)
        self._chk(self.lib.svjg_cohort_hwe(self.h, gt.ctypes.data, None if ploidy is None else ploidy.ctypes.data, n, S, counts.ctypes.data,
                                           p.ctypes.data))
        return counts, p

    def genotype_cohort_sites(self, slots, min_support, err):
        """genotype_sites for every sample of the cohort matrix in one launch (svjg_genotype_cohort_sites).  slots[n, 6]: the CANDIDATE slots of each
        site first, 0xFFFFFFFF behind them; sample s's site = the candidates present for s.  -> (gt[n, S, 2] = the pair or 0xFF, 0xFF, pl[n, S, 28],
        raw[n, S, 7], members[n, S] = bit j: candidate j took part (fewer than two: no site call), boundary[n, S] = the items to recompute with
        svjg.genotype.exact_pl_site, site[n, 6, 2] = NS_j and AC_j of every candidate over the items with a site call)"""
        return self._sites_call(self.lib.svjg_genotype_cohort_sites, slots, min_support, err, cohort=True)

    def genotype_cohort_sites_prior(self, slots, min_support, err):
        """genotype_cohort_sites with an allele-frequency prior over the samples of a site (svjg_genotype_cohort_sites_prior).  -> the six arrays of
        genotype_cohort_sites, bit for bit, and (sgt[n, S, 2] = the POSTERIOR call in the item's member numbering or 0xFF, 0xFF, sgq[n, S] (0xFF:
        none), af[n, 7] = the frequencies of the reference and the six candidates (NaN: no estimate), em_steps[n] (bit 31: not converged),
        psite[n, 6, 2] = NS_j and AC_j of the posterior calls)"""
        return self._sites_call(self.lib.svjg_genotype_cohort_sites_prior, slots, min_support, err, cohort=True, prior=True)

    def set_rows(self, sv_type, slot, ok):
        """the VCF rows' input arrays of genotype(), left on the device for run_resident()"""
        sv_type, slot, ok = _row_inputs(sv_type, slot, ok)
        self._n_rows = len(sv_type)
        self._chk(self.lib.svjg_set_rows(self.h, sv_type.ctypes.data, slot.ctypes.data, ok.ctypes.data, self._n_rows))

    def _run_views(self, p):
        n = self._n_rows
        if not n:
            self.last_boundary = np.zeros(0, np.uint8)
            return np.zeros(0, np.uint8), np.zeros((0, 3), np.int32), np.zeros((0, 2), np.uint32), np.zeros(0, np.uint8)
        self.last_boundary = _view(p[4], n, np.uint8)
        return _view(p[0], n, np.uint8), _view(p[1], n * 3, np.int32).reshape(n, 3), _view(p[2], n * 2, np.uint32).reshape(n, 2), _view(p[3], n, np.uint8)

    def run_resident(self, min_support, err, base_offset=0):
        """One whole pass with one host wait (svjg_run_resident): zero the counts, classify the uploaded text, all-reduce the
        counts if this context has a communicator, genotype the rows of set_rows().  -> (gt, pl[n, 3] int32, raw[n, 2], flags):
        read-only views of the library's pinned result block, overwritten by the second pass after this one; flags bit 0 =
        genotyped, bit 1 = the row's PLs need 64 bits (genotype() has them).  self.last_boundary: the rows to recompute like the
        reference (svjg_genotype_boundary)."""
        p = [ctypes.c_void_p() for _ in range(5)]
        self._chk(self.lib.svjg_run_resident(self.h, base_offset, min_support, float(err), *[ctypes.byref(x) for x in p]))
        return self._run_views(p)

    def run_begin(self, min_support, err, base_offset=0):
        """enqueue a pass (svjg_run_begin); at most two may be in flight"""
        self._chk(self.lib.svjg_run_begin(self.h, base_offset, min_support, float(err)))

    def run_end(self):
        """wait for the oldest pass in flight and return its results like run_resident() (svjg_run_end)"""
        p = [ctypes.c_void_p() for _ in range(5)]
        self._chk(self.lib.svjg_run_end(self.h, *[ctypes.byref(x) for x in p]))
        return self._run_views(p)

    def boundary_flags(self, n_rows):
        """rows of the last genotype() call whose PLs lie within 1e-6 of an integer boundary (to be recomputed by
        svjg.genotype.exact_pl, the reference's own arithmetic)"""
        out = np.zeros(n_rows, dtype=np.uint8)
        if n_rows:
            self._chk(self.lib.svjg_genotype_boundary(self.h, out.ctypes.data, n_rows))
        return out

    def logfact_reserve(self, n):
        """the log10(i!) table holds at least n entries afterwards (capped at 2^24, whole blocks of 1024; never smaller than it was): the table
        build taken out of a first genotype call (svjg_logfact_reserve)"""
        if not 0 <= int(n) < 2 ** 32:
            raise SvjgError("logfact_reserve: 0 <= n < 2^32")
        self._chk(self.lib.svjg_logfact_reserve(self.h, int(n)))

    def logfact_entries(self):
        """entries of the log10(i!) table right now, 0 before the context's first genotype call or reserve (svjg_logfact_read)"""
        n = ctypes.c_uint32(0)
        self._chk(self.lib.svjg_logfact_read(self.h, 0, 0, None, ctypes.byref(n)))
        return n.value

    def logfact_table(self, first=0, n=None):
        """entries first .. first + n of the device's log10(i!) table (n = None: all from `first`) -> float64[n, 2] = (hi, lo)
        (svjg_logfact_read); SvjgError beyond the table's end"""
        first = int(first)
        if n is None:
            n = self.logfact_entries() - first
        n = int(n)
        if first < 0 or n < 0 or first + n >= 2 ** 32:
            raise SvjgError("logfact_table: entries %d .. %d" % (first, first + n))
        out = np.empty((n, 2), dtype=np.float64)
        self._chk(self.lib.svjg_logfact_read(self.h, first, n, out.ctypes.data if n else None, None))
        return out

    def kernel_ms(self):
        a, b, c = ctypes.c_float(0), ctypes.c_float(0), ctypes.c_float(0)
        self._chk(self.lib.svjg_last_kernel_ms(self.h, ctypes.byref(a), ctypes.byref(b), ctypes.byref(c)))
        return a.value, b.value, c.value

    def main_ms_both(self):
        """k_classify_main of the last fused pass -> (ms by the device's clock, ms by the event pair or 0.0 without SVJG_KERNEL_MS=events)"""
        a, b = ctypes.c_float(0), ctypes.c_float(0)
        self._chk(self.lib.svjg_last_main_ms(self.h, ctypes.byref(a), ctypes.byref(b)))
        return a.value, b.value

    def sync(self):
        self._chk(self.lib.svjg_sync(self.h))

    def set_main_workers(self, workers):
        """a test hook (svjg_set_main_workers): k_classify_main's launch plan is made for at most `workers` workers on this context, so that
        its chunked regime begins at 8 x 65 536 x workers bytes of text; 0: no cap"""
        self._chk(self.lib.svjg_set_main_workers(self.h, int(workers)))

    def last_main_plan(self):
        """-> (region, small, grid, chunks_claimed) of the last k_classify_main launch that finished on this context — of a fused pass: the
        pass run_end() last returned — (svjg_last_main_plan)"""
        region, small, grid, claimed = ctypes.c_uint64(0), ctypes.c_uint64(0), ctypes.c_uint32(0), ctypes.c_uint64(0)
        self._chk(self.lib.svjg_last_main_plan(self.h, ctypes.byref(region), ctypes.byref(small), ctypes.byref(grid), ctypes.byref(claimed)))
        return region.value, small.value, grid.value, claimed.value


def release_host_tables():
    """drop the host copy of the kernels' lookup tables that load_graph keeps for the next context with the same graph"""
    load_library().svjg_release_host_tables()


def device_count():
    return int(load_library().svjg_device_count())


def _handles(ctxs):
    return (ctypes.c_void_p * len(ctxs))(*[c.h for c in ctxs])


def comm_init_all(ctxs):
    """One process, one Context per GPU: RCCL communicators for all of them (ncclCommInitAll inside the library)."""
    rc = ctxs[0].lib.svjg_comm_init_all(_handles(ctxs), len(ctxs))
    if rc:                                                       # (its own message buffer: the call may run beside others on these contexts)
        buf = ctypes.create_string_buffer(512)
        ctxs[0].lib.svjg_comm_error(buf, 512)
        raise SvjgError(f"libsvjg_hip error {rc}: {buf.value.decode(errors='replace')}")


def allreduce_counts_all(ctxs):
    """The path's one collective for a single-process run: afterwards every context holds the summed count vector.
    With one context only the overflow guard runs.  OverflowError if a per-SV count does not fit 32 bits."""
    ctxs[0]._chk(ctxs[0].lib.svjg_allreduce_counts_all(_handles(ctxs), len(ctxs)))


def unique_id():
    lib = load_library()
    buf = ctypes.create_string_buffer(128)
    rc = lib.svjg_comm_unique_id(buf)
    if rc:
        raise SvjgError(f"svjg_comm_unique_id failed ({rc})")
    return buf.raw


def _as_u8(x):
    if isinstance(x, np.ndarray):
        return np.ascontiguousarray(x.view(np.uint8))
    return np.frombuffer(x, dtype=np.uint8)
