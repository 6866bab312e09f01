"""measurement only (GPU box): the end-time spread of k_classify_main's workers in ONE launch over the resident configs[2] text.
Needs build/lib_endtimes.so (tools/mkvariant.sh endtimes -DSVJG_ENDTIMES) named by SVJG_HIP_LIB: that build keeps, per launch, the sum and a
histogram of the workers' end times, and svjg_run_end prints how long before the last worker the others ended (stderr, one line a pass).
  SVJG_HIP_LIB=build/lib_endtimes.so python tools/end_times.py [passes]"""
import os, sys
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "svjedi-graph_amd"), os.path.join(ROOT, "tools")):
    sys.path.insert(0, p)
import synth
from svjg import capi, genotype
from svjg.graph import Graph
n = int(sys.argv[1]) if len(sys.argv) > 1 else 12
import tempfile
pre = os.path.join(tempfile.mkdtemp(prefix="svjg_endt_"), "w")
inf = synth.generate(pre, 0, 100_000, 4, "mixed", 20260517, write_gaf=False)
gaf = synth.gaf_bytes(inf["tables"], 20260517, 0, 10_000_000, threads=16)
g = Graph.from_files(pre + "_svs_edges.json", pre + ".gfa")
rows = genotype.VcfRows(pre + ".vcf", g.slot_of)
ctx = capi.Context(0); ctx.load_graph(g); ctx.set_rows(rows.sv_type, rows.slot, rows.ok); ctx.upload(gaf)
for i in range(300):                                          # (the clocks settle)
    ctx.run_resident(3, 0.00005)
sys.stderr.write("[end_times] settled; one launch at a time from here\n")
for i in range(n):
    ctx.run_resident(3, 0.00005)
    sys.stderr.write(f"[end_times] pass {i}: kernel_ms {ctx.kernel_ms()[0]:.4f}\n")
