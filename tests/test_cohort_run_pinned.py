"""run_cohort's bytes, pinned: the eight accepted non-joint combinations ({plain, ploidy_file, prior, prior + ploidy_file} x {qual off, qual on})
through a stand-in context whose answers are fixed arrays, against the files under tests/golden/cohort_run/ (written by the commit before the
cohort host side was reshaped: the project's own output).  The arrays hold every branch of the writer at least once.  The two joint combinations
are pinned through the model contexts of tests/test_cohort_joint_ins.py and tests/test_cohort_site_prior.py.  CPU, milliseconds."""
import json
import os

import numpy as np
import pytest

from tests.test_joint_ins import _ROWS, KEYS

NONE, NO_CALL = 0xFFFFFFFF, 0xFF
E, MS = 5e-5, 3
NAMES = ("A", "B c", "C")                                                 # (a sample name may hold a blank)
S, N = len(NAMES), len(KEYS) + 1                                          # one answer per count slot, and one for the rows without a slot
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "cohort_run")

# the handmade rows of tests/test_joint_ins.py; row 1's INFO already holds fields the cohort writer owns; row 9's is a lone `.` once the writer has
# dropped its NS= field (an INFO that IS a lone `.` names no SVTYPE and no END: the rows die on it like the reference, test_a_lone_dot_info_...)
_INFO = {1: "SVTYPE=DEL;END=600;NS=9;AF=0.5;EMAF=0.1;EMNC;SVQ=3;MLAC=2;XNS=1", 9: ".;NS=SVTYPE=INS"}
VCF_TEXT = ("##fileformat=VCFv4.2\n"
            '##FORMAT=<ID=GT,Number=1,Type=String,Description="old">\n'
            "#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\tSAMPLE\n" +
            "".join("%s\t%s\t.\tN\t%s\t.\tPASS\t%s\n" % (r[0], r[1], r[2], _INFO.get(v, r[3])) for v, r in enumerate(_ROWS)))
# ploidy 1 (A on chr1), 0 (B on chr2), 3 (C on chr4, everyone at chr3:700, B at chr1:400-600), 2 elsewhere
PLOIDY_TEXT = "# sample\tcontig\t[from\tto]\tploidy\nA\tchr1\t1\nB c\tchr2\t0\nC\tchr4\t3\n*\tchr3\t700\t700\t3\nB c\tchr1\t400\t600\t3\n"
SLOT = {k: i for i, k in enumerate(KEYS)}
AT = {"hap": (SLOT["chr1:INS-100-1"], 0), "dip": (SLOT["chr1:DEL-500-600"], 2), "tri": (SLOT["chr4:INS-900-1"], 2),      # (slot, sample): boundary set
      "no_gq": (SLOT["chr1:INS-100-2"], 1), "no_call": (SLOT["chr2:INS-100-3"], 0), "not_done": (SLOT["chr2:INS-100-4"], 2)}


def _tables():
    """the fixed answers, one per (slot, sample) or slot; index N - 1: a row without a slot"""
    rng = np.random.default_rng(7)
    t = dict(done=(rng.random((N, S)) < 0.8).astype(np.uint8), raw=rng.integers(0, 40, (N, S, 2)).astype(np.uint32), pl=rng.integers(0, 400, (N, S, 9)).astype(np.int64),
             g=rng.integers(0, 9, (N, S)), no_call=rng.random((N, S)) < 0.15, gq=rng.integers(0, 100, (N, S)).astype(np.uint8), boundary=np.zeros((N, S), np.uint8),
             ns=rng.integers(0, 4, N), an=rng.integers(0, 10, N), ac=rng.integers(0, 7, N), af=rng.random(N), steps=rng.integers(1, 50, N).astype(np.uint32),
             qual=rng.random(N) * 80, mlac=rng.integers(0, 6, N).astype(np.uint32), chroms=rng.integers(1, 7, N).astype(np.uint32))
    for k in ("hap", "dip", "tri"):
        t["done"][AT[k]], t["boundary"][AT[k]], t["no_call"][AT[k]] = 1, 1, False
    t["done"][AT["no_gq"]], t["no_call"][AT["no_gq"]], t["gq"][AT["no_gq"]] = 1, False, NO_CALL
    t["done"][AT["no_call"]], t["no_call"][AT["no_call"]] = 1, True
    t["done"][AT["not_done"]] = 0
    t["ns"][0], t["an"][0] = 0, 0                                             # AN = 0: no AF
    t["af"][3], t["steps"][4] = np.nan, t["steps"][4] | (1 << 31)
    t["qual"][2], t["qual"][5], t["chroms"][7] = np.nan, -0.001, 0
    return t


class FixedCtx:
    """stands in for capi.Context in a cohort run.  A row's answer depends on nothing but the row handed in (its slot and, per sample, its
    ploidy), so any chunking gives the same arrays."""
    made = []

    def __init__(self, device=0):
        self.t, self.calls = _tables(), []
        FixedCtx.made.append(self)

    def cohort_alloc(self, n_samples, n_slots):
        assert (n_samples, n_slots) == (S, N - 1)

    def cohort_set_counts(self, sample, slots, counts):
        assert len(slots) == len(counts)

    def _items(self, name, slot, ploidy, width):
        self.calls.append((name, len(slot)))
        at = np.where(np.asarray(slot) == NONE, N - 1, slot).astype(np.int64)
        t = self.t
        P = np.full((len(at), S), 2) if ploidy is None else np.asarray(ploidy).astype(np.int64)
        done = t["done"][at] & (P != 0)
        gt = np.where(t["no_call"][at], NO_CALL, t["g"][at] % (P + 1)).astype(np.uint8)
        return at, gt, t["pl"][at][..., :width].copy(), t["raw"][at].copy(), done.astype(np.uint8), t["boundary"][at].copy()

    def _site(self, at, an):
        t = self.t
        return np.stack([t["ns"][at]] + ([t["an"][at]] if an else []) + [t["ac"][at]], axis=1).astype(np.uint32)

    def genotype_cohort(self, sv_type, slot, ok, min_support, err):
        at, gt, pl, raw, done, boundary = self._items("plain", slot, None, 3)
        return np.where(gt == NO_CALL, 3, gt).astype(np.uint8), pl, raw, done, boundary, self._site(at, False)

    def genotype_cohort_ploidy(self, sv_type, slot, ok, ploidy, max_ploidy, min_support, err):
        at, *items = self._items("ploidy", slot, ploidy, max_ploidy + 1)
        return (*items, self._site(at, True))

    def genotype_cohort_prior(self, sv_type, slot, ok, ploidy, max_ploidy, min_support, err):
        at, *items = self._items("prior", slot, ploidy, max_ploidy + 1)
        return (*items, self._site(at, True), self.t["gq"][at].copy(), self.t["af"][at].copy(), self.t["steps"][at].copy())

    def cohort_qual(self, sv_type, slot, ok, ploidy, max_ploidy, err, theta=1e-3):
        self.calls.append(("qual", len(slot), theta))
        at = np.where(np.asarray(slot) == NONE, N - 1, slot).astype(np.int64)
        return self.t["qual"][at].copy(), self.t["mlac"][at].copy(), self.t["chroms"][at].copy()

    def close(self):
        pass


@pytest.fixture()
def cohort(tmp_path, monkeypatch):
    return make_inputs(tmp_path, monkeypatch)


def make_inputs(tmp_path, monkeypatch):
    """the input files and the patches -> tmp_path"""
    from svjg import capi, filter as flt
    counts = np.arange(2 * len(KEYS), dtype=np.uint32).reshape(-1, 2)
    per = {"a.json": (list(KEYS), counts), "b.json": (KEYS[2:9], counts[2:9]), "c.json": (KEYS[::-2], counts[::-2])}       # (A first: slot = index in KEYS)
    monkeypatch.setattr(capi, "Context", FixedCtx)
    monkeypatch.setattr(flt, "read_handoff", lambda path: per[os.path.basename(path)])
    (tmp_path / "in.vcf").write_text(VCF_TEXT)
    (tmp_path / "ploidy.tsv").write_text(PLOIDY_TEXT)
    (tmp_path / "cohort.list").write_text("".join("%s\t%s.json\n" % (name, name[0].lower()) for name in NAMES))
    return tmp_path


MODES = {"plain": {}, "ploidy": {"ploidy_file": True}, "prior": {"prior": True}, "prior_ploidy": {"prior": True, "ploidy_file": True}}
RUNS = [(m + q, dict(kw, **qkw)) for m, kw in MODES.items() for q, qkw in (("", {}), ("_qual", {"qual": True, "theta": 0.05}))]


def run_one(cohort, name, kw):
    """-> (the bytes run_cohort wrote, n_done, the context)"""
    from svjg import genotype
    kw = dict(kw)
    if kw.pop("ploidy_file", False):
        kw["ploidy_file"] = str(cohort / "ploidy.tsv")
    out = cohort / (name + ".vcf")
    n_done = genotype.run_cohort(str(cohort / "cohort.list"), str(cohort / "in.vcf"), str(out), MS, E, **kw)
    return out.read_bytes(), n_done, FixedCtx.made[-1]


@pytest.mark.parametrize("name, kw", RUNS, ids=[r[0] for r in RUNS])
def test_run_cohort_writes_the_pinned_bytes(cohort, capsys, name, kw):
    got, n_done, ctx = run_one(cohort, name, kw)
    with open(os.path.join(GOLDEN, "n_done.json")) as fh:
        want_done = json.load(fh)[name]
    assert n_done == want_done
    assert capsys.readouterr().out == "".join("Genotyped svs (%s): %d\n" % (s, n) for s, n in zip(NAMES, want_done))
    with open(os.path.join(GOLDEN, name + ".vcf"), "rb") as fh:
        assert got == fh.read()
    call = "prior" if kw.get("prior") else "ploidy" if kw.get("ploidy_file") else "plain"
    assert ctx.calls == [(call, len(_ROWS))] + ([("qual", len(_ROWS), 0.05)] if kw.get("qual") else [])


def test_every_branch_of_the_writer_occurs(cohort):
    """what the pinned files are worth: the arrays and the ploidy matrix hold each case the writer tells apart"""
    from svjg import genotype
    rows = genotype.VcfRows(str(cohort / "in.vcf"), SLOT)
    ploidy = genotype.cohort_ploidy_matrix(rows, genotype.load_cohort_ploidy_file(str(cohort / "ploidy.tsv"), NAMES))
    assert sorted(set(ploidy.ravel().tolist())) == [0, 1, 2, 3]
    assert rows.slot[6] == NONE and (rows.slot != NONE).sum() == len(_ROWS) - 1
    assert genotype.cohort_info(_INFO[9], 1, 1) == "NS=1;AN=2;AC=1;AF=0.5"                # the lone `.` that is left is replaced
    row_of = {int(s): v for v, s in enumerate(rows.slot) if s != NONE}
    t = _tables()
    assert [int(ploidy[row_of[AT[k][0]], AT[k][1]]) for k in ("hap", "dip", "tri")] == [1, 2, 3]      # boundary at each ploidy, on a genotyped item
    assert all(t["done"][AT[k]] and t["boundary"][AT[k]] for k in ("hap", "dip", "tri"))
    for k in ("no_gq", "no_call"):                                           # (on items that are genotyped and not of ploidy 0)
        assert ploidy[row_of[AT[k][0]], AT[k][1]] != 0 and t["done"][AT[k]]
    assert t["gq"][AT["no_gq"]] == NO_CALL and not t["no_call"][AT["no_gq"]] and t["no_call"][AT["no_call"]] and not t["done"][AT["not_done"]]
    used = sorted(row_of)
    assert np.isnan(t["af"][3]) and t["steps"][4] >> 31 and np.isnan(t["qual"][2]) and "%.2f" % t["qual"][5] == "-0.00" and t["chroms"][7] == 0 and t["an"][0] == 0
    assert used == list(range(N - 1))
    assert (ploidy[[row_of[s] for s in used]] == 0).any()


@pytest.mark.parametrize("prior", [False, True])
def test_any_chunking_gives_the_same_arrays(cohort, prior):
    from svjg import genotype
    rows = genotype.VcfRows(str(cohort / "in.vcf"), SLOT)
    one = genotype.genotype_cohort_rows(FixedCtx(), rows, S, MS, E, None, prior, step=None)
    ctx = FixedCtx()
    parts = genotype.genotype_cohort_rows(ctx, rows, S, MS, E, None, prior, step=1)
    assert len(ctx.calls) == len(_ROWS) and len(one) == len(parts) and len(one) >= 5
    for a, b in zip(one, parts):
        assert (a is None and b is None) or (a.dtype == b.dtype and np.array_equal(a, b, equal_nan=a.dtype.kind == "f"))
    assert (one[5] is not None) == prior if len(one) > 5 else not prior   # (gq is there with the prior only; a tuple that ends at site has none)


def test_a_lone_dot_info_ends_the_run_before_anything_is_written(cohort):
    """no SVTYPE, so END is looked up and is not there: IndexError from the rows, like the reference (predict-genotype.py:77-87)"""
    from svjg import genotype
    (cohort / "in.vcf").write_text(VCF_TEXT.replace(_INFO[9], "."))
    with pytest.raises(IndexError):
        genotype.run_cohort(str(cohort / "cohort.list"), str(cohort / "in.vcf"), str(cohort / "out.vcf"), MS, E)
    assert not (cohort / "out.vcf").exists()
