"""The tail of the fused pass (svjg_run_begin / svjg_run_end): ONE launch between two k_classify_main — k_classify_exact, whose blocks
pick their role (none / one wave per line / one lane per line) from the number of deferred lines they read on the device and zero
the NEXT pass's count vector and status block — three slots rotating under two passes in flight, and k_classify_main's time taken
from the device's clock instead of an event pair.  Everything against classify + genotype done step by step on the same context —
which launches the same k_classify_exact, so the counts of the texts that run its two roles are also pinned to the Python oracle.
Needs an MI355X: run with -m gpu."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MS, ERR = 3, 0.00005

# Stamp tolerance (ms), from the record (profiles/r07/experiments/pass_tail.txt).  The event pair's interval holds what the stamps do
# not: the two barrier packets' own handling and the kernel's launch and drain around its first worker's start and last worker's
# end.  Measured on the same launches (40 passes, two processes): events minus stamps 0.0030 .. 0.0102 ms a launch, mean 0.0048.
# The parent's run-to-run spread of kernel_ms in the A/B of the same record: 1.21321 .. 1.21832 ms = 0.0051 ms.
STAMP_EVENTS_DIFF_MS = 0.0048
KERNEL_MS_SPREAD_MS = 0.0051


def _synth_case(tmp_path, n_aln, n_sv, n_chrom, mix, seed):
    import synth
    from svjg.graph import Graph
    pre = str(tmp_path / "c")
    inf = synth.generate(pre, n_aln, n_sv, n_chrom, mix, seed, write_gaf=False, return_gaf=True)
    g = Graph.from_files(pre + "_svs_edges.json", pre + ".gfa")
    return pre, inf["gaf"], g


def _step_by_step(c, gaf, rows):
    c.reset_counts()
    c.upload(gaf)
    c.classify_resident()
    gt, pl, raw, done = c.genotype(rows.sv_type, rows.slot, rows.ok, MS, ERR)
    return {"counts": c.counts(), "stats": c.stats(), "causes": c.defer_causes(), "gt": gt, "pl": pl, "raw": raw, "done": done}


def _oracle_counts(pre, g, gaf):
    """the count vector of the text by oracle.oracle_py (the checker that shares no code with the library), in the graph's slot order"""
    from oracle import oracle_py
    d = oracle_py.classify([ln + "\n" for ln in bytes(gaf).decode().split("\n")[:-1]], oracle_py.load_edges(pre + "_svs_edges.json"), oracle_py.load_alt_node_len(pre + ".gfa"))
    out = np.zeros((g.n_slots, 2), dtype=np.uint32)
    for sv, n in oracle_py.counts_of(d).items():
        out[g.slot_of[sv]] = n
    return out


def _same_results(got, want):
    gt, pl, raw, flags = got
    assert np.array_equal(gt, want["gt"]) and np.array_equal(pl, want["pl"]) and np.array_equal(raw, want["raw"])
    assert np.array_equal(flags & 1, want["done"]) and not (flags & 2).any()


def _same_status(c, want):
    st = c.stats()
    assert st["n_lines"] == want["stats"]["n_lines"] and st["n_deferred"] == want["stats"]["n_deferred"]
    assert c.defer_causes() == want["causes"]


@pytest.fixture(scope="module")
def case(tmp_path_factory):
    from svjg import genotype
    pre, gaf, g = _synth_case(tmp_path_factory.mktemp("tail"), 40000, 1500, 3, "mixed", 41)
    rows = genotype.VcfRows(pre + ".vcf", g.slot_of)
    # (an id:f: value in exponent form: float() takes it, the main kernel leaves the line to the exact path)
    few = np.frombuffer(bytes(gaf).replace(b"\tdv:f:", b"\tid:f:9e-1\tdv:f:", 7), dtype=np.uint8)      # a handful: the wave role
    many = np.frombuffer(bytes(gaf).replace(b"\tdv:f:", b"\tid:f:5e-1\tdv:f:"), dtype=np.uint8)        # 40 000 > 64 x n_cu: the lane role
    texts = {"none": gaf, "few": few, "many": many}
    return g, rows, texts, {k: _oracle_counts(pre, g, texts[k]) for k in ("few", "many")}


@pytest.fixture()
def ctx(case):
    from svjg import capi
    g, rows, _, _ = case
    c = capi.Context(0)
    c.load_graph(g)
    c.set_rows(rows.sv_type, rows.slot, rows.ok)
    yield c
    c.close()


@pytest.mark.parametrize("which,least,most", [("few", 7, 16384), ("many", 16385 + 23615, 40000)])
def test_roles_of_the_exact_launch(ctx, case, which, least, most):
    """a pass that defers a handful of lines (one wave per line) and one that defers more than wave_limit = 64 x n_cu lines (one lane
    per line): counts, n_deferred, defer_causes and genotypes equal the step-by-step calls; the pass is not repeated for them (the
    list did not overflow), twice in a row and with two in flight.  Both sides run k_classify_exact, so the counts must also be
    the Python oracle's over the same text and graph"""
    _, rows, texts, oracle = case
    want = _step_by_step(ctx, texts[which], rows)
    assert least <= want["stats"]["n_deferred"] <= most and want["counts"].sum() > 0
    assert np.array_equal(want["counts"], oracle[which])
    for _ in range(2):
        got = [np.array(x) for x in ctx.run_resident(MS, ERR)]
        _same_results(got, want)
        _same_status(ctx, want)
        assert np.array_equal(ctx.counts(), want["counts"])
        assert ctx.kernel_ms()[1] > 0                                        # (the exact path's own interval)
    ctx.run_begin(MS, ERR); ctx.run_begin(MS, ERR)
    for _ in range(2):
        _same_results([np.array(x) for x in ctx.run_end()], want)
        _same_status(ctx, want)
    assert np.array_equal(ctx.counts(), want["counts"])


def test_five_passes_alternating_texts(ctx, case):
    """driven as bench.py drives them (begin, begin, end, begin, end, ...), the text changing between a deferring one and one that
    defers nothing whenever no pass is in flight: every pass equals its step-by-step twin — a vector zeroed too late or too early, or
    a status block shared by two passes, shows here"""
    _, rows, texts, _ = case
    want = {k: _step_by_step(ctx, texts[k], rows) for k in ("none", "few", "many")}
    assert want["none"]["stats"]["n_deferred"] < want["few"]["stats"]["n_deferred"] < want["many"]["stats"]["n_deferred"]
    for order in (("few", "none", "many", "none", "few"), ("none", "many", "none", "few", "none")):
        for name in order:
            # five passes of this text, two in flight
            ctx.upload(texts[name])
            ctx.run_begin(MS, ERR)
            for i in range(5):
                if i < 4:
                    ctx.run_begin(MS, ERR)
                _same_results([np.array(x) for x in ctx.run_end()], want[name])
                _same_status(ctx, want[name])
            assert np.array_equal(ctx.counts(), want[name]["counts"])
        # one pass per text, the text re-uploaded between them (no pass in flight)
        for name in order:
            ctx.upload(texts[name])
            _same_results([np.array(x) for x in ctx.run_resident(MS, ERR)], want[name])
            _same_status(ctx, want[name])
            assert np.array_equal(ctx.counts(), want[name]["counts"])


def test_counts_after_the_last_pass(ctx, case):
    """counts() after the last run_end is the last pass's vector; reset_counts / classify_resident behind fused passes work on a
    vector of their own and the next fused pass starts from zero again; the uploads still refuse while a pass is in flight"""
    from svjg import capi
    _, rows, texts, _ = case
    want = _step_by_step(ctx, texts["few"], rows)
    ctx.run_begin(MS, ERR); ctx.run_begin(MS, ERR)
    with pytest.raises(capi.SvjgError):
        ctx.run_begin(MS, ERR)
    for up in (lambda: ctx.upload(texts["none"]), lambda: ctx.upload_parts([texts["none"][:1000]], 4096)):
        with pytest.raises(capi.SvjgError):
            up()
    ctx.run_end(); ctx.run_end()
    assert np.array_equal(ctx.counts(), want["counts"])
    assert np.array_equal(ctx.counts(), want["counts"])                      # (asked twice: the copy out of the slot happens once)
    ctx.reset_counts()
    assert ctx.counts().sum() == 0
    ctx.classify_resident()
    assert np.array_equal(ctx.counts(), want["counts"])
    ctx.classify_resident()                                                  # (adds to the same vector)
    assert np.array_equal(ctx.counts(), want["counts"] * 2)
    for _ in range(3):
        _same_results([np.array(x) for x in ctx.run_resident(MS, ERR)], want)
    assert np.array_equal(ctx.counts(), want["counts"])
    # a new graph's rows behind fused passes: the slots are zeroed afresh
    ctx.set_rows(rows.sv_type, rows.slot, rows.ok)
    _same_results([np.array(x) for x in ctx.run_resident(MS, ERR)], want)
    assert np.array_equal(ctx.counts(), want["counts"])


_BOTH_CLOCKS = r"""
import json, sys
import numpy as np
import __graft_entry__                                   # (the package's paths)
import synth
from svjg import capi, genotype
from svjg.graph import Graph
pre = sys.argv[1]
inf = synth.generate(pre, 400000, 1500, 3, "mixed", 43, write_gaf=False, return_gaf=True)
g = Graph.from_files(pre + "_svs_edges.json", pre + ".gfa")
rows = genotype.VcfRows(pre + ".vcf", g.slot_of)
c = capi.Context(0)
c.load_graph(g); c.set_rows(rows.sv_type, rows.slot, rows.ok); c.upload(inf["gaf"])
out = []
c.run_begin(3, 0.00005)
for i in range(24):
    c.run_begin(3, 0.00005)
    c.run_end()
    if i >= 4:
        out.append(c.main_ms_both())
c.run_end()
c.close()
print("BOTH " + json.dumps(out))
"""


def measure_both_clocks(tmp_dir):
    """[(ms by the device's stamps, ms by the event pair)] of the same k_classify_main launches, in a process of its own (the
    measurement switch is read once per process)"""
    env = dict(os.environ, SVJG_KERNEL_MS="events")
    p = subprocess.run([sys.executable, "-c", _BOTH_CLOCKS, os.path.join(str(tmp_dir), "t")], cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-2000:]
    line = [l for l in p.stdout.splitlines() if l.startswith("BOTH ")][-1]
    return json.loads(line[5:])


def test_stamps_against_the_event_pair(tmp_path):
    """kernel_ms()[0] of a fused pass comes from the stamps k_classify_main leaves in the pass's status block; under
    SVJG_KERNEL_MS=events the same launches are also timed by the event pair of before.  The stamps read shorter (the events hold
    their own barrier packets and the kernel's launch and drain), on average by no more than the measured difference plus the spread of kernel_ms."""
    both = measure_both_clocks(tmp_path)
    diffs = [e - s for s, e in both]
    print("stamps, events, difference (ms):", [(round(s, 4), round(e, 4), round(e - s, 4)) for s, e in both])
    assert all(s > 0 and e > 0 for s, e in both)
    mean = sum(diffs) / len(diffs)
    assert 0 <= mean <= STAMP_EVENTS_DIFF_MS + KERNEL_MS_SPREAD_MS, (mean, diffs)      # over the passes: the measured difference + the spread
    assert all(d > -KERNEL_MS_SPREAD_MS for d in diffs), diffs                         # no single launch where the stamps read clearly LONGER
