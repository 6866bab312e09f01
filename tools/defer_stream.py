"""measurement only (GPU box): what a stream of fused passes costs when EVERY pass defers a handful of lines — the `few` text of
tests/test_fused_pass_tail.py (seven lines with an id:f: value in exponent form) at bench size, driven begin, begin, end, ... as
bench.py drives its passes — beside the same text with none deferred.
  python tools/defer_stream.py [steps] [rounds]"""
import os, sys, tempfile, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "svjedi-graph_amd"), os.path.join(ROOT, "tools")):
    sys.path.insert(0, p)
import synth
from svjg import capi, genotype
from svjg.graph import Graph
steps = int(sys.argv[1]) if len(sys.argv) > 1 else 200
rounds = int(sys.argv[2]) if len(sys.argv) > 2 else 5
pre = os.path.join(tempfile.mkdtemp(prefix="svjg_defer_"), "w")
inf = synth.generate(pre, 0, 100_000, 4, "mixed", 20260517, write_gaf=False)
gaf = synth.gaf_bytes(inf["tables"], 20260517, 0, 10_000_000, threads=16)
head = bytes(gaf[:1 << 20]).replace(b"\tdv:f:", b"\tid:f:9e-1\tdv:f:", 7)
few = np.concatenate([np.frombuffer(head, dtype=np.uint8), gaf[1 << 20:]])
g = Graph.from_files(pre + "_svs_edges.json", pre + ".gfa")
rows = genotype.VcfRows(pre + ".vcf", g.slot_of)
ctx = capi.Context(0); ctx.load_graph(g); ctx.set_rows(rows.sv_type, rows.slot, rows.ok)


def stream(n):
    ctx.run_begin(3, 0.00005)
    for _ in range(n - 1):
        ctx.run_begin(3, 0.00005)
        ctx.run_end()
    ctx.run_end()


for name, text in (("none", gaf), ("few", few), ("none", gaf), ("few", few)):
    ctx.upload(text)
    stream(300)
    ms = []
    for _ in range(rounds):
        t = time.perf_counter(); stream(steps); ms.append((time.perf_counter() - t) / steps * 1e3)
    print(f"{name}: {ctx.stats()['n_deferred']} deferred lines a pass; ms per step over {rounds} x {steps} steps: mean {np.mean(ms):.4f} min {min(ms):.4f} max {max(ms):.4f}; exact path ms {ctx.kernel_ms()[1]:.4f}")
