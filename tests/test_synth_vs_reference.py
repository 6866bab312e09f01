"""tools/synth.py lays the graph out exactly like the reference's construct-graph.py.
The reference's graph files for each case are stored under tests/golden/graphlayout (tests/golden/make_golden.py: make_graphlayout)."""
import gzip
import os

import pytest


def _elide(path):
    """the GFA with the reference sequences elided (S lines of nodes without a '.' in the last ':' field): what the fixture holds"""
    out = []
    for ln in open(path):
        if ln.startswith("S"):
            c = ln.rstrip("\n").split("\t")
            if "." not in c[1].split(":")[-1]:
                ln = f"S\t{c[1]}\t*\n"
        out.append(ln)
    return out


@pytest.mark.parametrize("n_sv,n_chrom,mix,seed", [(300, 3, "mixed", 7), (200, 1, "del", 8)])
def test_graph_matches_construct_graph(tmp_path, golden, n_sv, n_chrom, mix, seed):
    import synth
    pre = str(tmp_path / "s")
    synth.generate(pre, 100, n_sv, n_chrom, mix, seed)
    ref = os.path.join(golden, "graphlayout", f"{n_sv}-{n_chrom}-{mix}-{seed}")
    assert open(pre + "_svs_edges.json").read() == gzip.open(ref + "_svs_edges.json.gz", "rt").read()
    assert _elide(pre + ".gfa") == gzip.open(ref + ".elided.gfa.gz", "rt").read().splitlines(True)
