"""Overlapped fused passes (svjg_run_begin / svjg_run_end on a context alone on its GPU): consecutive passes alternate between two
compute streams, so that the next pass's k_classify_main moves into the slots the one in front vacates; no exact-path launch sits on
those streams — svjg_run_end settles a pass that deferred lines (k_classify_exact on the pass's own list, the genotypes again) and
the context then runs its next pass in the former form until a pass defers nothing.  Everything against classify + genotype done step
by step on the same context.  The host's decisions alone: tests/test_pass_overlap.py.  Needs an MI355X: run with -m gpu."""
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MS, ERR = 3, 0.00005
DEVICE_FILLING_BYTES = 3584 * 8192              # 256 CUs x 14 workers, a stripe of text each: the smallest text whose grid fills the device


class Rows:
    """one VCF row per count slot (the soup's graph comes without a VCF)"""

    def __init__(self, n_slots):
        self.sv_type = (np.arange(n_slots) % 4).astype(np.uint8)
        self.slot = np.arange(n_slots, dtype=np.uint32)
        self.ok = np.ones(n_slots, dtype=np.uint8)


def _step_by_step(c, gaf, rows):
    c.reset_counts()
    c.upload(gaf)
    c.classify_resident()
    gt, pl, raw, done = c.genotype(rows.sv_type, rows.slot, rows.ok, MS, ERR)
    return {"counts": c.counts(), "stats": c.stats(), "causes": c.defer_causes(), "gt": gt, "pl": pl, "raw": raw, "done": done}


def _check_pass(c, got, want):
    gt, pl, raw, flags = [np.array(x) for x in got]
    assert np.array_equal(gt, want["gt"]) and np.array_equal(pl, want["pl"]) and np.array_equal(raw, want["raw"])
    assert np.array_equal(flags & 1, want["done"]) and not (flags & 2).any()
    st = c.stats()
    assert st["n_lines"] == want["stats"]["n_lines"] and st["n_deferred"] == want["stats"]["n_deferred"]
    assert c.defer_causes() == want["causes"]
    assert (c.kernel_ms()[1] > 0) == (want["stats"]["n_deferred"] > 0)       # the exact path's own interval: exactly the passes that deferred


def _passes(c, n, want, counts_every=False):
    """n passes, two in flight, as bench.py drives them; every one against `want`.  counts_every: counts() after every run_end too — while
    a pass is in flight that is the NEWEST pass's vector, asked for before that pass has been ended"""
    c.run_begin(MS, ERR)
    for i in range(n):
        if i < n - 1:
            c.run_begin(MS, ERR)
        _check_pass(c, c.run_end(), want)
        if counts_every:
            assert np.array_equal(c.counts(), want["counts"])
    assert np.array_equal(c.counts(), want["counts"])


STRIPE = 8192                                   # a worker's region of a text that does not fill the device (svjg_kernels.h: TEXT)
CLEAN_STRIPES = 32                              # 3 584 = 112 x 32: the clean text tiled 112 times is EXACTLY a device-filling grid of one stripe a worker


@pytest.fixture(scope="module")
def soup():
    """tests/longpath_fuzz.py: make_soup on one graph -> (graph, rows, {name: text}):
    soup   the text as it is (some of its lines take the exact path);
    clean  exactly 32 stripes of its lines, in their order, of which the main kernel defers NONE: whether it defers a line depends on where the
           line lies in its worker's stripe, so the text is grown line by line (in runs, halved where a run defers) and a line is kept only if
           the text up to it still defers nothing; a last line with a plain tag fills the 32nd stripe to its last byte;
    tiled  clean x 112 = 3 584 stripes, the smallest text whose grid fills the device: every copy starts at a worker's region boundary, so every
           line lies in its stripe as it does in `clean`."""
    from tests import longpath_fuzz
    from svjg import capi
    from svjg.graph import Graph
    edges, alt, text = longpath_fuzz.make_soup(3100)
    some_node = next(iter(edges)).split("@")[0].encode()
    g = Graph(edges, alt)
    target = CLEAN_STRIPES * STRIPE
    lines = [l + b"\n" for l in text.split(b"\n")[:-1]]
    c = capi.Context(0)
    try:
        c.load_graph(g)

        def n_def(buf):
            c.reset_counts()
            c.upload(np.frombuffer(buf, dtype=np.uint8))
            c.classify_resident()
            return c.stats()["n_deferred"]

        kept = [b""]

        def add(run):
            run = [l for l in run]
            while run and len(kept[0]) + sum(map(len, run)) > target - 200:     # (room for the filling line)
                run.pop()
            if not run:
                return
            cand = kept[0] + b"".join(run)
            if n_def(cand) == 0:
                kept[0] = cand
            elif len(run) > 1:
                add(run[:len(run) // 2]); add(run[len(run) // 2:])

        for at in range(0, len(lines), 32):
            if len(kept[0]) >= target - 260:
                break
            add(lines[at:at + 32])
        head = b"fill\t9\t0\t9\t+\t>" + some_node + b"\t9\t0\t9\t9\t9\t0\tzz:Z:"
        room = target - len(kept[0])
        assert room > len(head) + 1
        clean = kept[0] + head + b"A" * (room - len(head) - 1) + b"\n"
        assert len(clean) == target and n_def(clean) == 0
    finally:
        c.close()
    assert sum(len(l) > 400 for l in clean.split(b"\n")) >= 8                  # long paths among them
    tiled = clean * (3584 // CLEAN_STRIPES)
    assert len(tiled) == 3584 * STRIPE
    as_array = lambda b: np.frombuffer(b, dtype=np.uint8)
    return g, Rows(g.n_slots), {"soup": as_array(text), "clean": as_array(clean), "tiled": as_array(tiled)}


@pytest.mark.parametrize("which", ["soup", "clean", "tiled"])
def test_long_lines_in_both_live_passes(soup, which):
    """Twenty passes, two in flight, over texts whose long paths (65 .. 216 nodes, hits held back until the line's last name is known)
    make the workers use their scratch words (ClassifyArgs::long_pre).  `clean` and `tiled` defer NOTHING (asserted), so all twenty
    passes run in the overlapped form, two main kernels alive at once: `clean` gives a grid of 32 workers, far below the device, so the
    two run fully side by side; `tiled` is the smallest text whose grid fills the device, so the next pass enters only through vacated
    slots.  `soup` keeps the lines that take the exact path: its first two passes are overlapped and settled, the rest run in the
    former form.  Every pass must equal the step-by-step result.  A scratch block or a list shared by the two live launches shows
    here only by chance — whether two workers with the same number touch the same words at the same time is up to the hardware's
    placing; the check that counts is the field-by-field walk through ClassifyArgs in profiles/r11/experiments/pass_overlap.txt
    (which pointers two concurrent launches may share)."""
    from svjg import capi
    g, rows, texts = soup
    c = capi.Context(0)
    try:
        c.load_graph(g)
        c.set_rows(rows.sv_type, rows.slot, rows.ok)
        want = _step_by_step(c, texts[which], rows)
        print(which, len(texts[which]), "bytes,", want["stats"]["n_lines"], "lines,", want["stats"]["n_deferred"], "deferred")
        assert want["counts"].sum() > 0
        assert (want["stats"]["n_deferred"] == 0) == (which != "soup")
        _passes(c, 20, want)
    finally:
        c.close()


@pytest.fixture(scope="module")
def tail_case(tmp_path_factory):
    """the texts of tests/test_fused_pass_tail.py: none deferred / a handful (the wave role) / 40 000 (the lane role)"""
    import synth
    from svjg import genotype
    from svjg.graph import Graph
    pre = str(tmp_path_factory.mktemp("overlap") / "c")
    inf = synth.generate(pre, 40000, 1500, 3, "mixed", 41, write_gaf=False, return_gaf=True)
    gaf = inf["gaf"]
    g = Graph.from_files(pre + "_svs_edges.json", pre + ".gfa")
    rows = genotype.VcfRows(pre + ".vcf", g.slot_of)
    few = np.frombuffer(bytes(gaf).replace(b"\tdv:f:", b"\tid:f:9e-1\tdv:f:", 7), dtype=np.uint8)
    many = np.frombuffer(bytes(gaf).replace(b"\tdv:f:", b"\tid:f:5e-1\tdv:f:"), dtype=np.uint8)
    return g, rows, {"none": gaf, "few": few, "many": many}


@pytest.fixture()
def ctx(tail_case):
    from svjg import capi
    g, rows, _ = tail_case
    c = capi.Context(0)
    c.load_graph(g)
    c.set_rows(rows.sv_type, rows.slot, rows.ok)
    yield c
    c.close()


def test_settle_step_and_form_switches(ctx, tail_case):
    """begin, begin, end, ... with the text changing whenever nothing is in flight.  Behind clean passes a text's first two passes are
    overlapped (enqueued before a deferring pass has finished): both are settled by svjg_run_end; the third runs in the former form
    behind an overlapped one still in flight; a clean text's first two passes behind deferring ones run in the former form, its
    third is overlapped behind one of those.  Three and four passes a text put either form on either stream.  So every pair of forms
    follows each other, a deferring pass directly ahead of a clean one and the reverse included (the texts only differ in the tags
    that defer).  Results, status, counts() after each pass; kernel_ms()[1] > 0 exactly for the passes that deferred."""
    _, rows, texts = tail_case
    want = {k: _step_by_step(ctx, texts[k], rows) for k in ("none", "few", "many")}
    assert want["none"]["stats"]["n_deferred"] == 0 < want["few"]["stats"]["n_deferred"] <= 16384 < want["many"]["stats"]["n_deferred"]
    order = ("none", "few", "none", "many", "none", "none", "few", "many", "few", "none")
    for n_passes in (3, 4, 1, 2):
        for name in order:
            ctx.upload(texts[name])
            _passes(ctx, n_passes, want[name], counts_every=True)
    # one pass at a time: deferring and clean passes alternate directly
    for name in order + order[::-1]:
        ctx.upload(texts[name])
        _check_pass(ctx, ctx.run_resident(MS, ERR), want[name])
        assert np.array_equal(ctx.counts(), want[name]["counts"])


def test_step_by_step_calls_behind_overlapped_passes(ctx, tail_case):
    """reset_counts / classify_resident / counts() straight after run_end of the last of several overlapped passes, no explicit sync:
    the step-by-step calls run on the first compute stream and must come behind what the second one holds; then passes again"""
    _, rows, texts = tail_case
    want = _step_by_step(ctx, texts["none"], rows)
    assert want["stats"]["n_deferred"] == 0
    for n_passes in (5, 4):                                       # (the last pass on the second / on the first stream)
        _passes(ctx, n_passes, want)
        ctx.reset_counts()
        assert ctx.counts().sum() == 0
        ctx.classify_resident()
        assert np.array_equal(ctx.counts(), want["counts"])
        ctx.classify_resident()                                   # (adds to the same vector)
        assert np.array_equal(ctx.counts(), want["counts"] * 2)
        # counts() of the newest pass while it is still in flight, then the step-by-step calls with a pass in flight on either stream
        ctx.run_begin(MS, ERR); ctx.run_begin(MS, ERR)
        _check_pass(ctx, ctx.run_end(), want)
        ctx.reset_counts()
        ctx.classify_resident()
        assert np.array_equal(ctx.counts(), want["counts"])
        _check_pass(ctx, ctx.run_end(), want)
        gt, pl, raw, done = ctx.genotype(rows.sv_type, rows.slot, rows.ok, MS, ERR)
        assert np.array_equal(gt, want["gt"]) and np.array_equal(pl, want["pl"])
    ctx.sync()
    _passes(ctx, 3, want)


@pytest.mark.parametrize("which", ["few", "many"])
def test_counts_of_a_deferring_pass_still_in_flight(ctx, tail_case, which):
    """counts() — and everything else that takes the newest pass's vector — asked for before svjg_run_end of an overlapped pass that
    deferred lines: the vector must already hold the exact path's hits (the pass is settled there and then; run_end finds it
    settled).  begin; counts(), and begin(0); begin(1); end(0); counts(), which reads pass 1's slot.  Behind a clean text, so that the
    deferring passes are overlapped ones.  (`many` defers every line: a vector without the exact path's hits would be empty.)"""
    _, rows, texts = tail_case
    clean = _step_by_step(ctx, texts["none"], rows)
    want = _step_by_step(ctx, texts[which], rows)
    assert want["stats"]["n_deferred"] > 0 and want["counts"].sum() > 0      # (a vector that lacks the deferred lines' hits differs from it)
    for second in (False, True):
        ctx.upload(texts["none"])
        _passes(ctx, 3, clean)                                     # (the context is back in the overlapped form)
        ctx.upload(texts[which])
        ctx.run_begin(MS, ERR)
        if second:
            ctx.run_begin(MS, ERR)
            _check_pass(ctx, ctx.run_end(), want)
        assert np.array_equal(ctx.counts(), want["counts"])
        _check_pass(ctx, ctx.run_end(), want)
        assert np.array_equal(ctx.counts(), want["counts"])
        # ... and the genotype call, which takes the same vector
        ctx.run_begin(MS, ERR)
        gt, pl, raw, done = ctx.genotype(rows.sv_type, rows.slot, rows.ok, MS, ERR)
        assert np.array_equal(gt, want["gt"]) and np.array_equal(pl, want["pl"]) and np.array_equal(raw, want["raw"])
        _check_pass(ctx, ctx.run_end(), want)


def test_more_host_lines_than_a_pass_list_holds(ctx, tail_case):
    """5 000 lines only the host can decide (non-ASCII digits in a decimal column) in an overlapped pass: the main kernel defers them, the
    settle step's exact path sets them aside — more than the 4 096 entries of the pass's list, so it sets the overflow bit, and
    svjg_run_end must see THAT and repeat the pass with a list that holds them all, as it did when the exact path ran ahead of it:
    run_end refuses the text (the caller has to know) and host_lines() hands out every offset, the step-by-step call's"""
    from svjg import capi
    _, rows, texts = tail_case
    lines = bytes(texts["none"]).split(b"\n")[:-1]
    digits = "\u0661\u0662\u0663".encode()
    out, offs, at = [], [], 0
    for i, l in enumerate(lines):
        if i % 8 == 0 and len(offs) < 5000:
            f = l.split(b"\t")
            f[1] = digits
            l = b"\t".join(f)
            offs.append(at)
        out.append(l)
        at += len(l) + 1
    text = np.frombuffer(b"\n".join(out) + b"\n", dtype=np.uint8)
    assert len(offs) == 5000
    clean = _step_by_step(ctx, texts["none"], rows)
    ctx.reset_counts()
    ctx.upload(text)
    ctx.classify_resident()
    want_counts, want_lines = ctx.counts(), np.sort(ctx.host_lines())
    assert np.array_equal(want_lines, np.array(offs, dtype=np.uint64))
    for _ in range(2):
        ctx.upload(texts["none"])
        _passes(ctx, 3, clean)
        ctx.upload(text)
        with pytest.raises(capi.SvjgError):
            ctx.run_resident(MS, ERR)
        assert np.array_equal(np.sort(ctx.host_lines()), want_lines)
        assert np.array_equal(ctx.counts(), want_counts)
