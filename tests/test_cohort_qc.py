"""Cohort sample QC (--cohort LIST --cohort-qc PREFIX) on the CPU: the host harness (tests/geno_sim, topic qc: svjg_geno.h's own routines inside a restatement of
both kernels' loops) against the numpy model (tests/cohort_qc_model.py) bit for bit; planted pairs; the kinship, its thresholds and its text; both
writers; the chunked host flow; the script's refusal; run_cohort(qc=...) on the golden cohort with a stand-in context that answers from the models."""
import math
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import cohort_qc_model as M
from tests import standin_capi
from tests.geno_sim import qc as qc_sim
from tests.test_cohort_joint_ins import CohortModelCtx

AMD = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "svjedi-graph_amd")
C = qc_sim.constants()
SIZES = [1, 2, 3, C["TJ"] - 1, C["TJ"], C["TJ"] + 1, 2 * C["TJ"] + 2]
ROWS = [1, 63, 64, 65, 64 * C["stage"] - 1, 64 * C["stage"] + 1]
GT_VALUES = np.array([0, 1, 2, 3, 4, 5, 6, 7, 8, 0xFF], np.uint8)


def random_call(rng, n, S, mode):
    """gt from {0..8, 0xFF}; mode: "none" (no ploidy array), "two" (all 2), "mixed" (0..8)"""
    gt = rng.choice(GT_VALUES, size=(n, S))
    ploidy = None if mode == "none" else np.full((n, S), 2, np.uint8) if mode == "two" else rng.integers(0, 9, (n, S)).astype(np.uint8)
    return gt, ploidy


# ---- the harness against the model ----

def test_constants_are_the_documented_ones():
    assert C["max_samples"] == 2048 and C["TI"] * 2 == C["TJ"] == 64 and C["RI"] * C["waves"] == C["TI"]
    assert C["lds_slots"] * 8 == 3 * C["stage"] * (C["TI"] + C["TJ"]) * 8 <= 65536


@pytest.mark.parametrize("g, P, want", [(0, 2, "eligible called dip"), (1, 2, "eligible called carrier dip het"), (2, 2, "eligible called carrier dip homalt"),
                                        (3, 2, "eligible"), (0xFF, 2, "eligible"), (0, 0, ""), (0xFF, 0, ""), (1, 1, "eligible called carrier"),
                                        (2, 1, "eligible"), (2, 3, "eligible called carrier"), (8, 8, "eligible called carrier"), (0, 8, "eligible called")])
def test_item_classes(g, P, want):
    bits = qc_sim.qc_class(g, P)
    assert {f for q, f in enumerate(M.SAMPLE_FIELDS) if bits >> q & 1} == set(want.split()) and bits < 64


@pytest.mark.parametrize("S", SIZES)
def test_harness_equals_model_bit_for_bit(S):
    rng = np.random.default_rng(4100 + S)
    for n in ROWS:
        for mode in ("none", "two", "mixed"):
            gt, ploidy = random_call(rng, n, S, mode)
            sample, pair = qc_sim.run(gt, ploidy, grid_planes=(n + S) % 3, grid_pairs=(n * S) % 4)
            want_s, want_p = M.qc(gt, ploidy)
            assert sample.dtype == pair.dtype == np.uint32 and pair.shape == (S * (S - 1) // 2, 5)
            assert np.array_equal(sample, want_s) and np.array_equal(pair, want_p), (S, n, mode)


def test_model_is_the_definition_item_by_item():
    """the matrix products against three nested loops over a small call"""
    rng = np.random.default_rng(5)
    gt, ploidy = random_call(rng, 40, 5, "mixed")
    ploidy[:, :2] = 2
    sample, pair = M.qc(gt, ploidy)
    k = 0
    for i in range(5):
        for j in range(i + 1, 5):
            want = [0] * 5
            for r in range(40):
                di, dj = ploidy[r, i] == 2 and gt[r, i] <= 2, ploidy[r, j] == 2 and gt[r, j] <= 2
                if di and dj:
                    a, b = int(gt[r, i]), int(gt[r, j])
                    want[0] += 1; want[1] += a == 1; want[2] += b == 1; want[3] += a == 1 and b == 1; want[4] += {a, b} == {0, 2}
            assert pair[k].tolist() == want
            k += 1
    assert sample[0].tolist() == [40, (gt[:, 0] <= 2).sum()] + [((gt[:, 0] >= 1) & (gt[:, 0] <= 2)).sum(), (gt[:, 0] <= 2).sum(), (gt[:, 0] == 1).sum(), (gt[:, 0] == 2).sum()]


def test_tiles_cover_every_pair_once():
    """tile t -> (ti, tj): in order, none twice, and exactly the tiles that hold a pair i < j < S"""
    for S in [1, 2, 3, 32, 33, 34, 63, 64, 65, 66, 96, 97, 129, 130, 1000, 2047, 2048]:
        got = [qc_sim.tile_at(t, S) for t in range(qc_sim.tiles(S))]
        want = [(ti, tj) for ti in range((S + C["TI"] - 1) // C["TI"]) for tj in range((S + C["TJ"] - 1) // C["TJ"])
                if ti * C["TI"] < min(S, (tj + 1) * C["TJ"]) - 1 and ti * C["TI"] <= S - 2]
        assert got == want, S
    assert qc_sim.tiles(2048) == 1056


@pytest.mark.parametrize("n_rows, S, per_item", [(0, 1, False), (1, 1, True), (65, 3, True), (1000, 130, False), (10_000, 2048, True)])
def test_qc_layout(n_rows, S, per_item):
    L = qc_sim.layout(n_rows, S, per_item)
    n, pairs, words = n_rows * S, S * (S - 1) // 2, (n_rows + 63) // 64
    sample = (20 * pairs + 7) & ~7
    planes = (sample + 24 * S + 8 + n * (2 if per_item else 1) + 7) & ~7
    assert L == {"pair": 0, "sample": sample, "maxn": sample + 24 * S, "in_at": sample + 24 * S + 8, "in_bytes": n * (2 if per_item else 1),
                 "gt": sample + 24 * S + 8, "ploidy": sample + 24 * S + 8 + n if per_item else 0, "planes": planes, "total": planes + 3 * 8 * words * S + 64}
    from svjg import genotype
    step = genotype.cohort_qc_chunk_rows(S, per_item)
    assert qc_sim.layout(step, S, per_item)["total"] <= 1 << 30 < qc_sim.layout(2 * step + 64, S, per_item)["total"] and step < 1 << 32


def test_harness_under_the_sanitizers():
    """the same code as a stand-alone program with its own main under -fsanitize=address,undefined (nothing is loaded into Python)"""
    p = subprocess.run([qc_sim.build_main(), "qc"], capture_output=True, text=True)
    assert p.returncode == 0 and p.stdout.startswith("qc_sim ok") and not p.stderr, (p.stdout, p.stderr)


# ---- planted pairs, kinship, text ----

def _planted():
    """columns: 0 a random diploid sample, 1 its copy, 2 homozygotes only, 3 the complement of 2's homozygotes, 4 without a het"""
    from svjg import genotype
    rng = np.random.default_rng(77)
    gt = np.zeros((500, 5), np.uint8)
    gt[:, 0] = rng.integers(0, 4, 500)
    gt[:, 1] = gt[:, 0]
    gt[:, 2] = rng.choice(np.array([0, 2], np.uint8), 500)
    gt[:, 3] = 2 - gt[:, 2]
    gt[:, 4] = rng.choice(np.array([0, 2, 3], np.uint8), 500)
    sample, pair = qc_sim.run(gt)
    i, j = M.pair_index(5)
    return genotype, sample, {(int(a), int(b)): pair[k].tolist() for k, (a, b) in enumerate(zip(i, j))}


def test_planted_pairs():
    genotype, sample, pair = _planted()
    both, het1, het2, hethet, ibs0 = pair[0, 1]
    assert het1 == het2 == hethet == sample[0, 4] > 0 and ibs0 == 0 and both == sample[0, 3]
    phi = genotype.kinship(het1, het2, hethet, ibs0)
    assert phi == 0.5 and genotype.relation(phi) == "DUP"
    both, het1, het2, hethet, ibs0 = pair[2, 3]
    assert ibs0 == both == 500 and het1 == het2 == hethet == 0 and genotype.kinship(het1, het2, hethet, ibs0) is None
    for other in range(4):
        assert genotype.kinship(*pair[other, 4][1:]) is None                # a sample without hets: no estimate against anyone
    assert genotype.kinship(*pair[0, 2][1:]) is None and pair[0, 2][1] > 0  # het1 > 0, het2 = 0: the minimum decides


def test_relation_on_both_sides_of_each_threshold():
    from svjg import genotype
    names = ["DUP", "1ST", "2ND", "3RD", "UN"]
    N = 10 ** 6                                                              # het1 = het2 = N, hethet = h, ibs0 = 0: phi = h / (2 N)
    for k, e in enumerate((-1.5, -2.5, -3.5, -4.5)):
        bound = 2.0 ** e
        assert genotype.relation(bound) == names[k + 1] and genotype.relation(math.nextafter(bound, 1.0)) == names[k]
        h = int(2 * N * bound)
        above, below = genotype.kinship(N, N, h + 1, 0), genotype.kinship(N, N, h, 0)
        assert below < bound < above and genotype.relation(above) == names[k] and genotype.relation(below) == names[k + 1]
    assert genotype.relation(-0.3) == "UN" and genotype.relation(0.5) == "DUP"
    assert genotype.kinship(7, 5, 3, 1) == 0.5 - (4 + 4 + 2) / 20 and genotype.kinship(0, 5, 0, 1) is None and genotype.kinship(5, 0, 0, 0) is None


def test_kinship_text_and_the_negative_zero_rule():
    from svjg import genotype
    assert genotype.kinship_text(0.5) == "0.5000" and genotype.kinship_text(-0.00004) == "0.0000" and genotype.kinship_text(-0.0) == "0.0000"
    assert genotype.kinship_text(-0.00006) == "-0.0001" and genotype.kinship_text(0.00004) == "0.0000" and genotype.kinship_text(-1.25) == "-1.2500"
    phi = genotype.kinship(100000, 100000, 0, 1)
    assert -0.00005 < phi < 0 and "%.4f" % phi == "-0.0000" and genotype.kinship_text(phi) == "0.0000" and genotype.relation(phi) == "UN"


def test_writers_exact_text(tmp_path):
    from svjg import genotype
    names = ["A", "B b", "C"]
    sample = np.array([[10, 8, 5, 6, 3, 2], [0, 0, 0, 0, 0, 0], [7, 7, 1, 7, 1, 0]])
    pair = np.array([[6, 3, 3, 3, 0], [5, 2, 0, 0, 1], [100000, 100000, 100000, 0, 1]])
    genotype.write_qc_samples(str(tmp_path / "q.samples.tsv"), names, sample)
    genotype.write_qc_pairs(str(tmp_path / "q.pairs.tsv"), names, pair)
    assert (tmp_path / "q.samples.tsv").read_text() == (
        "#SAMPLE\tN_ELIGIBLE\tN_CALLED\tCALL_RATE\tN_CARRIER\tN_DIPLOID\tN_HET\tN_HOMALT\tHET_HOMALT\n"
        "A\t10\t8\t0.8\t5\t6\t3\t2\t1.5\n"
        "B b\t0\t0\t.\t0\t0\t0\t0\t.\n"
        "C\t7\t7\t1\t1\t7\t1\t0\t.\n")
    assert (tmp_path / "q.pairs.tsv").read_text() == (
        "#SAMPLE1\tSAMPLE2\tN_BOTH\tHET1\tHET2\tHETHET\tIBS0\tKINSHIP\tRELATION\n"
        "A\tB b\t6\t3\t3\t3\t0\t0.5000\tDUP\n"
        "A\tC\t5\t2\t0\t0\t1\t.\t.\n"
        "B b\tC\t100000\t100000\t100000\t0\t1\t0.0000\tUN\n")
    genotype.write_qc_samples(str(tmp_path / "one.samples.tsv"), ["only"], sample[2:])
    genotype.write_qc_pairs(str(tmp_path / "one.pairs.tsv"), ["only"], np.zeros((0, 5), np.int64))
    assert (tmp_path / "one.pairs.tsv").read_text() == genotype.QC_PAIRS_HEADER and (tmp_path / "one.samples.tsv").read_text().count("\n") == 2
    assert "%.6g" % (1 / 3) == "0.333333"


# ---- the host flow ----

class _Recorder(qc_sim.SimQc):
    def __init__(self):
        self.calls = []

    def cohort_qc(self, gt, ploidy=None):
        self.calls.append((np.array(gt), None if ploidy is None else np.array(ploidy)))
        return super().cohort_qc(gt, ploidy)


@pytest.mark.parametrize("mode", ["none", "mixed"])
def test_any_chunking_gives_the_same_numbers(mode):
    from svjg import genotype
    rng = np.random.default_rng(12)
    n, S = 200, 7
    gt, ploidy = random_call(rng, n, S, mode)
    done = (rng.random((n, S)) < 0.8).astype(np.uint8)
    masked = np.where(done != 0, gt, 0xFF).astype(np.uint8)
    want = M.qc(masked, ploidy)
    for step in (None, 1, 64, 65, n - 1, n, 10 * n):
        ctx = _Recorder()
        sample, pair = genotype.cohort_qc_rows(ctx, gt, done, ploidy, step)
        assert sample.dtype == pair.dtype == np.int64 and np.array_equal(sample, want[0]) and np.array_equal(pair, want[1]), step
        assert len(ctx.calls) == (1 if step is None else -(-n // step))
        assert np.array_equal(np.concatenate([c[0] for c in ctx.calls]), masked)         # done == 0 goes in as 0xFF
        assert all((c[1] is None) == (ploidy is None) for c in ctx.calls)
    sample, pair = genotype.cohort_qc_rows(_Recorder(), np.zeros((0, 3), np.uint8), np.zeros((0, 3), np.uint8), None)
    assert sample.shape == (3, 6) and pair.shape == (3, 5) and not sample.any() and not pair.any()


def test_script_refuses_cohort_qc_without_cohort(tmp_path):
    (tmp_path / "in.vcf").write_text("##fileformat=VCFv4.2\n")
    (tmp_path / "d.json").write_text("{}")
    p = subprocess.run([sys.executable, os.path.join(AMD, "predict-genotype.py"), "-d", "d.json", "-v", "in.vcf", "-o", "out.vcf", "--cohort-qc", "qc"],
                       capture_output=True, text=True, cwd=tmp_path)
    assert p.returncode != 0 and "usage:" in p.stderr and "--cohort-qc needs --cohort" in p.stderr
    assert sorted(os.listdir(tmp_path)) == ["d.json", "in.vcf"]             # no output file of any kind


def test_script_lets_cohort_qc_through_with_every_cohort_option(tmp_path):
    """the parser and the options check let the combinations through: the run gets as far as the cohort list, which does not exist"""
    (tmp_path / "in.vcf").write_text("##fileformat=VCFv4.2\n")
    for extra in ([], ["--cohort-prior"], ["--cohort-ploidy", "p.txt"], ["--joint-ins"], ["--joint-ins", "--joint-prior"], ["--cohort-qual"]):
        p = subprocess.run([sys.executable, os.path.join(AMD, "predict-genotype.py"), "--cohort", "none.list", "-v", "in.vcf", "-o", "out.vcf",
                            "--cohort-qc", "qc", *extra], capture_output=True, text=True, cwd=tmp_path)
        assert p.returncode != 0 and "usage:" not in p.stderr and "none.list" in p.stderr, (extra, p.stderr)
        assert sorted(os.listdir(tmp_path)) == ["in.vcf"]


class _NoGpu:
    def __init__(self, *a):
        raise AssertionError("a context was made before the options were checked")


def test_nothing_is_written_when_an_option_check_fails(tmp_path, monkeypatch):
    from svjg import capi, genotype
    monkeypatch.setattr(capi, "Context", _NoGpu)
    for extra in ({"joint_ins": True, "prior": True}, {"qc": ""}):
        with pytest.raises(ValueError):
            genotype.run_cohort(str(tmp_path / "none.list"), str(tmp_path / "in.vcf"), str(tmp_path / "out.vcf"), **{"qc": str(tmp_path / "qc"), **extra})
    assert os.listdir(tmp_path) == []


class QcStandinCtx(standin_capi.Context, CohortModelCtx, M.ModelQc):
    """the stand-in context of the CPU tests with the cohort calls answered from the models (tests/test_cohort_joint_ins.py) and cohort_qc from
    tests/cohort_qc_model.py"""
    qc_calls = []

    def __init__(self, device=0):
        standin_capi.Context.__init__(self, device)
        CohortModelCtx.__init__(self, device)

    def cohort_qc(self, gt, ploidy=None):
        QcStandinCtx.qc_calls.append(np.array(gt))
        return M.ModelQc.cohort_qc(self, gt, ploidy)


GT_CODE = {"0/0": 0, "0/1": 1, "1/1": 2, "./.": 0xFF}


def vcf_gt(path):
    """(sample names, gt[n, S]) parsed back out of a diploid multi-sample VCF"""
    names, rows = None, []
    for line in open(path).read().split("\n"):
        if line.startswith("#CHROM"):
            names = line.split("\t")[9:]
        elif line and not line.startswith("#"):
            rows.append([GT_CODE[c.split(":")[0]] for c in line.split("\t")[9:]])
    return names, np.array(rows, np.uint8).reshape(len(rows), len(names))


def model_tsvs(tmp_path, names, gt, ploidy=None):
    """both files' text from the model on gt (and the writers, whose text test_writers_exact_text pins)"""
    from svjg import genotype
    sample, pair = M.qc(gt, ploidy)
    genotype.write_qc_samples(str(tmp_path / "want.samples.tsv"), names, sample)
    genotype.write_qc_pairs(str(tmp_path / "want.pairs.tsv"), names, pair)
    return (tmp_path / "want.samples.tsv").read_text(), (tmp_path / "want.pairs.tsv").read_text()


@pytest.mark.parametrize("joint_ins", [False, True])
@pytest.mark.parametrize("which", ["plain", "edited"])
def test_run_cohort_qc_on_the_golden_cohort(golden, tmp_path, monkeypatch, which, joint_ins):
    from svjg import capi, genotype
    from tests import cohort_model as CM
    monkeypatch.setenv("SVJG_PY_VCF", "1")
    monkeypatch.setattr(capi, "Context", QcStandinCtx)
    co = CM.Cohort(golden, which)
    a, b, prefix = str(tmp_path / "plain.vcf"), str(tmp_path / "qc.vcf"), str(tmp_path / "cohort_qc")
    assert genotype.run_cohort(co.list, co.vcf, a, joint_ins=joint_ins) == genotype.run_cohort(co.list, co.vcf, b, joint_ins=joint_ins, qc=prefix)
    assert open(a, "rb").read() == open(b, "rb").read()
    assert sorted(os.listdir(tmp_path)) == ["cohort_qc.pairs.tsv", "cohort_qc.samples.tsv", "plain.vcf", "qc.vcf"]
    names, gt = vcf_gt(b)
    assert names == co.names and gt.shape == co.gt.shape and len(QcStandinCtx.qc_calls[-1]) == len(gt)
    want = model_tsvs(tmp_path, names, gt)
    assert (open(prefix + ".samples.tsv").read(), open(prefix + ".pairs.tsv").read()) == want
    lines = want[1].split("\n")
    assert len(lines) == 1 + len(names) * (len(names) - 1) // 2 + 1 and lines[1].startswith(names[0] + "\t" + names[1] + "\t")
    assert any(l.split("\t")[7] != "." for l in lines[1:-1])                 # the fixture gives estimates
