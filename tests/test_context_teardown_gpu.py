"""A context owns its device and pinned blocks, events and streams through owners (svjedi-graph_amd/csrc/svjg_own.h) and gives all of them back in
svjg_destroy: contexts opened, used through every call that allocates, and closed over and over leave the device's free memory where it was and
compute the same bytes; buffers that grow with their contents kept (hit records, host lines) keep them; a graph reloaded over another gives a
fresh context's counts; a failed svjg_init returns its code.  (The owners' failure paths: tests/test_owners.py, on the CPU.  Graph after graph
on one context against the oracle: tests/test_gpu_parity.py, whose tests share a context.)  Needs an MI355X: run with -m gpu."""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

NONE = 0xFFFFFFFF
MS, ERR = 3, 5e-5
S = 3                                  # cohort samples
TEXT_BYTES = 8 << 20                   # the resident text of a cycle: the smallest large allocation a teardown could drop


def _host_line(line):
    """the line with its path length (column 7) in Arabic-Indic digits: the kernels set it aside for the host (svjg.h: SVJG_EXC_ASK_HOST)"""
    f = line.split(b"\t")
    f[6] = f[6].decode().translate({ord("0") + d: 0x0660 + d for d in range(10)}).encode()
    return b"\t".join(f)


@pytest.fixture(scope="module")
def kit(golden):
    from svjg import genotype
    from svjg.graph import Graph
    d = f"{golden}/testdir"
    g = Graph.from_files(f"{d}/test_svs_edges.json", f"{d}/test.gfa")
    gaf = open(f"{d}/test.gaf", "rb").read()
    assert gaf.endswith(b"\n")
    gaf_host = gaf + _host_line(gaf.split(b"\n", 1)[0]) + b"\n"   # (the fused pass refuses a text with a line for the host: the growth test's alone)
    rows = genotype.VcfRows(f"{d}/test.vcf", g.slot_of)
    R = len(rows.sv_type)
    sites = np.full((2, 6), NONE, np.uint32)
    sites[0, :2] = (0, 1)
    sites[1, :3] = (2, 3, 4)
    assert g.n_slots >= 5 and R >= 5
    return {"g": g, "gaf": np.frombuffer(gaf, np.uint8), "gaf_host": gaf_host, "text": np.frombuffer(gaf * (TEXT_BYTES // len(gaf) + 1), np.uint8), "rows": rows,
            "ploidy": np.resize(np.array([1, 2, 3, 8], np.uint8), R), "sites": sites}


def _sorted_hits(ctx):
    return np.sort(ctx.hits(), order=("line_start", "slot", "n_ref", "n_alt"))


def _hip_runtime():
    """the HIP runtime the library has brought into the process"""
    for line in open("/proc/self/maps"):
        if "libamdhip64.so" in line:
            return ctypes.CDLL(line.split()[-1])
    raise AssertionError("no HIP runtime in this process")


def _free_bytes(hip):
    free, total = ctypes.c_size_t(0), ctypes.c_size_t(0)
    assert hip.hipMemGetInfo(ctypes.byref(free), ctypes.byref(total)) == 0
    return free.value


def _cycle(kit):
    """one context through every call that allocates -> the bytes of everything it computed"""
    from svjg import capi
    g, rows = kit["g"], kit["rows"]
    out = []
    ctx = capi.Context(0)
    try:
        ctx.load_graph(g)
        ctx.upload(kit["text"])
        ctx.classify_resident(want_hits=True)
        st = ctx.stats()
        assert st["n_hitrecs"] > 1000 and st["n_lines"] > 10000
        out += [ctx.counts(), _sorted_hits(ctx)]
        ctx.set_rows(rows.sv_type, rows.slot, rows.ok)
        ctx.run_begin(MS, ERR); ctx.run_begin(MS, ERR)
        for _ in range(2):
            out += [np.array(x) for x in ctx.run_end()]
        out.append(ctx.counts())
        out += [np.array(x) for x in ctx.genotype(rows.sv_type, rows.slot, rows.ok, MS, ERR, reuse_outputs=True)]
        out += list(ctx.genotype_ploidy(rows.sv_type, rows.slot, rows.ok, kit["ploidy"], MS, ERR))
        out += list(ctx.genotype_sites(kit["sites"], MS, ERR))
        ctx.cohort_alloc(S, g.n_slots)
        for s in range(S):
            ctx.cohort_store_counts(s)
        out += list(ctx.genotype_cohort(rows.sv_type, rows.slot, rows.ok, MS, ERR))
        ctx.load_graph(g)                                          # over the graph that is there: svjg_capi.hip, free_graph
        ctx.classify(kit["gaf"])
        out.append(ctx.counts())
    finally:
        ctx.close()
    return [np.ascontiguousarray(a).tobytes() for a in out]


def test_contexts_opened_and_closed_leave_nothing_behind(kit):
    """One warm-up cycle, then eight: every cycle computes the first one's bytes, and the device's free memory after the eighth is not lower
    than after the first by the size of one text buffer or more (a context's leak before the owners: 256 bytes)."""
    from svjg import capi
    capi.load_library()
    _cycle(kit)
    hip = _hip_runtime()
    first, free_first = _cycle(kit), _free_bytes(hip)
    assert any(first[0]) and any(first[2]) and any(first[-1])
    for k in range(7):
        assert _cycle(kit) == first, f"cycle {k + 2}"
    free_last = _free_bytes(hip)
    print(f"free device memory after the first cycle {free_first} B, after the eighth {free_last} B")
    assert free_last > free_first - TEXT_BYTES


def test_lists_grow_with_their_contents_kept(kit):
    """Three line-aligned pieces of 1, 2 and 8 copies of the text on one context, none reset in between (svjg/filter.py: classify_stream adds
    pieces this way): hit records, host lines and counts equal those of three fresh contexts, concatenated or summed."""
    from svjg import capi
    gaf = kit["gaf_host"]
    pieces, at = [], 0
    for copies in (1, 2, 8):
        pieces.append((at, np.frombuffer(gaf * copies, np.uint8)))
        at += len(gaf) * copies
    alone = []
    for base, piece in pieces:
        c = capi.Context(0)
        try:
            c.load_graph(kit["g"])
            c.classify(piece, base_offset=base, want_hits=True)
            alone.append((c.counts(), c.hits(), c.host_lines()))
        finally:
            c.close()
    c = capi.Context(0)
    try:
        c.load_graph(kit["g"])
        n_recs = []
        for base, piece in pieces:
            c.classify(piece, base_offset=base, want_hits=True)
            n_recs.append(c.stats()["n_hitrecs"])
        assert n_recs[0] == len(alone[0][1]) > 0 and n_recs[2] > n_recs[1] > n_recs[0]     # the buffers grew past the first piece's, contents kept
        order = ("line_start", "slot", "n_ref", "n_alt")
        assert np.array_equal(_sorted_hits(c), np.sort(np.concatenate([a[1] for a in alone]), order=order))
        assert np.array_equal(c.host_lines(), np.sort(np.concatenate([a[2] for a in alone]))) and len(c.host_lines()) == 11
        assert np.array_equal(c.counts(), sum(a[0].astype(np.uint64) for a in alone).astype(np.uint32))
    finally:
        c.close()


def test_graph_reloaded_over_another(kit, tmp_path):
    """graph A, a graph with more slots, A again on one context: each time the counts of a fresh context"""
    import synth
    from svjg import capi
    from svjg.graph import Graph
    pre = str(tmp_path / "b")
    gaf_b = synth.generate(pre, 2000, 300, 2, "mixed", 5, write_gaf=False, return_gaf=True)["gaf"]
    b = Graph.from_files(pre + "_svs_edges.json", pre + ".gfa")
    assert b.n_slots > kit["g"].n_slots
    legs = [(kit["g"], kit["gaf"]), (b, gaf_b), (kit["g"], kit["gaf"])]
    want = []
    for g, gaf in legs[:2]:
        c = capi.Context(0)
        try:
            c.load_graph(g)
            c.classify(gaf)
            want.append(c.counts())
        finally:
            c.close()
    want.append(want[0])
    assert want[0].sum() > 0 and want[1].sum() > 0
    c = capi.Context(0)
    try:
        for (g, gaf), w in zip(legs, want):
            c.load_graph(g)
            c.classify(gaf)
            assert np.array_equal(c.counts(), w)
    finally:
        c.close()


def test_failed_init_returns_its_code():
    from svjg import capi
    lib = capi.load_library()
    n = capi.device_count()
    assert n >= 1
    for device in (n, -1):
        h = ctypes.c_void_p()
        assert lib.svjg_init(device, ctypes.byref(h)) == -3 and not h.value          # SVJG_E_ARG
        assert lib.svjg_last_error(None) == b"device index out of range"
