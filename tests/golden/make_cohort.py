#!/usr/bin/env python3
"""Generate tests/golden/cohort/ by RUNNING THE REFERENCE ITSELF, once per sample (like make_golden.py: only where the reference is at hand; no
GPU).  Nothing of the reference's source is copied: the fixtures are inputs and the VCFs its predict-genotype.py writes for them.

    python tests/golden/make_cohort.py

Two cohorts of four samples over golden/testdir/test.vcf:
  cohort/         the plain cohort.  s1..s4.json: the testdir's informative-alignment JSON with its lists thinned (fixed seed) to about 1.0,
                  0.5, 0.2 and 0.05 of their entries, every entry replaced by "" (the genotyper only takes len()); a key both of whose lists
                  end up empty is left out, as filter-alignments.py would.  sN.ref_genotype.vcf: what the reference writes for sample N alone.
  cohort/edited/  the same samples with three edits planted in the JSONs (one key deleted from sample 2, one key with two empty lists in
                  sample 3, one key present only in sample 4) over edited.vcf, a copy of test.vcf one of whose rows already carries AC= and AF=
                  in INFO.  eN.ref_genotype.vcf likewise.
manifest.json names the edits and holds the reference's `Genotyped svs` number of every sample.
"""
import contextlib
import importlib.util
import io
import json
import os

import numpy as np

REF = "/root/reference"
HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "cohort")
DEPTHS = (1.0, 0.5, 0.2, 0.05)
SEED = 20261018


def _load(name, path):
    spec = importlib.util.spec_from_file_location(name, path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


ref_geno = _load("ref_geno", f"{REF}/predict-genotype.py")


def run_ref(js, vcf, out):
    """the reference's main() without its argument parser: json.load, decision_vcf -> its `Genotyped svs` number"""
    with open(js) as fh:
        d = json.load(fh)
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf):
        ref_geno.decision_vcf(d, vcf, out, 3, 0.00005, [])
    return int(buf.getvalue().strip().split(": ")[1])


def thin(full, depth, rng):
    out = {}
    for key in sorted(full):
        lists = [[""] * (len(lst) if depth >= 1.0 else int((rng.random(len(lst)) < depth).sum())) for lst in full[key]]
        if lists[0] or lists[1]:
            out[key] = lists
    return out


def dump(d, path):
    with open(path, "w") as fh:
        fh.write(json.dumps(d, sort_keys=True, indent=None, separators=(",", ":")) + "\n")


def main():
    os.makedirs(f"{OUT}/edited", exist_ok=True)
    vcf = f"{HERE}/testdir/test.vcf"
    full = json.load(open(f"{HERE}/testdir/ref_informative_aln.json"))
    rng = np.random.default_rng(SEED)
    samples = [thin(full, d, rng) for d in DEPTHS]
    manifest = {"seed": SEED, "depths": list(DEPTHS), "vcf": "../testdir/test.vcf", "min_support": 3, "err": 0.00005, "plain": {}, "edited": {}}

    with open(f"{OUT}/cohort.list", "w") as fh:
        fh.write("# the plain cohort: NAME<TAB>PATH, paths relative to this file\n\n")
        for n in range(1, 5):
            fh.write(f"S{n}\ts{n}.json\n")
    for n, d in enumerate(samples, 1):
        dump(d, f"{OUT}/s{n}.json")
        manifest["plain"][f"S{n}"] = {"json": f"s{n}.json", "ref_vcf": f"s{n}.ref_genotype.vcf", "keys": len(d),
                                      "genotyped": run_ref(f"{OUT}/s{n}.json", vcf, f"{OUT}/s{n}.ref_genotype.vcf")}

    # the edited cohort
    common = [k for k in sorted(full) if all(k in s for s in samples)]
    deleted, emptied, only4 = common[3], common[7], common[11]
    edited = [json.loads(json.dumps(s)) for s in samples]
    del edited[1][deleted]
    edited[2][emptied] = [[], []]
    for s in edited[:3]:
        del s[only4]
    lines = open(vcf).read().split("\n")
    data = [i for i, ln in enumerate(lines) if ln and not ln.startswith("#")]
    at = data[5]
    cols = lines[at].split("\t")
    fields = cols[7].split(";")
    cols[7] = ";".join(fields[:2] + ["AC=7"] + fields[2:] + ["AF=0.4375"])
    lines[at] = "\t".join(cols)
    with open(f"{OUT}/edited/edited.vcf", "w") as fh:
        fh.write("\n".join(lines))
    with open(f"{OUT}/edited/cohort.list", "w") as fh:
        for n in range(1, 5):
            fh.write(f"E{n}\te{n}.json\n")
    manifest["edits"] = {"deleted_from_sample_2": deleted, "empty_lists_in_sample_3": emptied, "only_in_sample_4": only4,
                         "vcf_row_with_site_tags": {"id": cols[2], "info": cols[7]}}
    for n, d in enumerate(edited, 1):
        dump(d, f"{OUT}/edited/e{n}.json")
        manifest["edited"][f"E{n}"] = {"json": f"e{n}.json", "ref_vcf": f"e{n}.ref_genotype.vcf", "keys": len(d),
                                       "genotyped": run_ref(f"{OUT}/edited/e{n}.json", f"{OUT}/edited/edited.vcf", f"{OUT}/edited/e{n}.ref_genotype.vcf")}
    with open(f"{OUT}/manifest.json", "w") as fh:
        json.dump(manifest, fh, indent=1, sort_keys=True)
    size = sum(os.path.getsize(os.path.join(dp, f)) for dp, _, fs in os.walk(OUT) for f in fs)
    print(f"cohort: {json.dumps({k: v['genotyped'] for k, v in {**manifest['plain'], **manifest['edited']}.items()})}, {size} bytes")


if __name__ == "__main__":
    main()
