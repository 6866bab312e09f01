"""The cohort fixtures of tests/golden/cohort/ (tests/golden/make_cohort.py: the reference run once per sample) as arrays, and the multi-sample
file assembled from the reference's per-sample outputs with the product's writer — what predict-genotype.py --cohort has to produce byte for
byte.  Shared by tests/test_cohort.py (CPU) and tests/test_cohort_gpu.py."""
import json
import os

import numpy as np

GT_CODE = {"0/0": 0, "0/1": 1, "1/1": 2, "./.": 3}


class Cohort:
    """which: "plain" (golden/cohort, over testdir/test.vcf) or "edited" (golden/cohort/edited, over edited.vcf)"""

    def __init__(self, golden, which):
        from svjg import genotype
        top = os.path.join(golden, "cohort")
        self.manifest = json.load(open(os.path.join(top, "manifest.json")))
        self.dir = top if which == "plain" else os.path.join(top, "edited")
        self.vcf = os.path.join(golden, "testdir", "test.vcf") if which == "plain" else os.path.join(self.dir, "edited.vcf")
        self.list = os.path.join(self.dir, "cohort.list")
        entries = self.manifest[which]
        self.names = sorted(entries)
        self.genotyped = [entries[n]["genotyped"] for n in self.names]
        self.jsons = [json.load(open(os.path.join(self.dir, entries[n]["json"]))) for n in self.names]
        self.ref_lines = [open(os.path.join(self.dir, entries[n]["ref_vcf"])).read().split("\n") for n in self.names]
        self.ref_data = [[ln.split("\t") for ln in lines if ln and not ln.startswith("#")] for lines in self.ref_lines]
        self.keys, _ = genotype.cohort_union([(list(d), np.zeros((len(d), 2), np.uint32)) for d in self.jsons])
        self.rows = genotype.VcfRows(self.vcf, {k: i for i, k in enumerate(self.keys)})
        n, S = len(self.rows.slot), len(self.names)
        assert all(len(d) == n for d in self.ref_data)
        self.gt, self.pl = np.full((n, S), 3, np.uint8), np.zeros((n, S, 3), np.int64)
        self.raw, self.done = np.zeros((n, S, 2), np.uint32), np.zeros((n, S), np.uint8)
        for s in range(S):
            for r in range(n):
                gt, _dp, _ad, pl = self.ref_data[s][r][9].split(":")
                self.gt[r, s] = GT_CODE[gt]
                if pl != ".,.,.":                                   # the reference genotyped the row for this sample
                    key = self.keys[self.rows.slot[r]]
                    self.done[r, s] = 1
                    self.pl[r, s] = [int(x) for x in pl.split(",")]
                    self.raw[r, s] = [len(self.jsons[s][key][0]), len(self.jsons[s][key][1])]
        called = self.gt != 3
        self.site = np.stack([called.sum(axis=1), np.where(called, self.gt, 0).sum(axis=1)], axis=1).astype(np.uint32)

    def assemble(self, out_path):
        """the merged file from the reference's columns -> the per-sample numbers of genotyped rows"""
        from svjg import genotype
        return genotype.write_vcf_cohort(out_path, self.rows, self.names, genotype.CohortCalls(self.gt, self.pl, self.raw, self.done, self.site))
