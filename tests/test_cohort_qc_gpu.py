"""svjg_cohort_qc on the device against the numpy model (tests/cohort_qc_model.py), all bytes: the shapes at which k_qc_planes and k_qc_pairs take
another path (tests/geno_sim/qc.py: constants), the largest triangle, chunked calls, the argument errors, and predict-genotype.py
--cohort --cohort-qc on the golden cohort.  Needs an MI355X: run with -m gpu."""
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import cohort_model as CM
from tests import cohort_qc_model as M
from tests.geno_sim import qc as qc_sim
from tests.test_cohort_qc import AMD, ROWS, SIZES, model_tsvs, random_call, vcf_gt

pytestmark = pytest.mark.gpu

E_ARG = -3
STEP_SECONDS = 120                      # every run of the script is a process of its own under this limit


@pytest.fixture(scope="module")
def ctx():
    from svjg import capi
    c = capi.Context(0)
    yield c
    c.close()


def _equal(got, want):
    return got[0].dtype == got[1].dtype == np.uint32 and np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]) and got[1].shape == want[1].shape


@pytest.mark.parametrize("S", SIZES)                # (130 = 2 TJ + 2 is the last of them)
def test_device_equals_model_all_bytes(ctx, S):
    rng = np.random.default_rng(8200 + S)
    for n in ROWS:
        for mode in ("none", "two", "mixed"):
            gt, ploidy = random_call(rng, n, S, mode)
            got = ctx.cohort_qc(gt, ploidy)
            assert _equal(got, M.qc(gt, ploidy)), (S, n, mode)
            again = ctx.cohort_qc(gt, ploidy)
            assert got[0].tobytes() == again[0].tobytes() and got[1].tobytes() == again[1].tobytes()


def test_every_tile_of_the_largest_triangle(ctx):
    """2048 samples x 65 rows: all 1056 tiles, more than one trip of the grid (at most four blocks a compute unit), the second word one row long"""
    S = qc_sim.constants()["max_samples"]
    assert 130 in SIZES and qc_sim.tiles(S) == 1056 > 4 * 256             # the grid: at most four blocks on each of the MI355X's 256 compute units
    rng = np.random.default_rng(2048)
    gt = rng.choice(np.array([0, 0, 1, 1, 2, 3], np.uint8), size=(65, S))
    ploidy = np.where(rng.random((65, S)) < 0.9, 2, 1).astype(np.uint8)
    got = ctx.cohort_qc(gt, ploidy)
    assert _equal(got, M.qc(gt, ploidy))
    again = ctx.cohort_qc(gt, ploidy)
    assert got[0].tobytes() == again[0].tobytes() and got[1].tobytes() == again[1].tobytes()


@pytest.mark.parametrize("mode", ["none", "mixed"])
def test_one_call_equals_the_sum_of_its_chunks(ctx, mode):
    from svjg import genotype
    rng = np.random.default_rng(31)
    n, S = 260, 67
    gt, ploidy = random_call(rng, n, S, mode)
    done = np.ones((n, S), np.uint8)
    one = ctx.cohort_qc(gt, ploidy)
    assert _equal(one, M.qc(gt, ploidy))
    for step in (1, 64, 65, n - 1):
        sample, pair = genotype.cohort_qc_rows(ctx, gt, done, ploidy, step)
        assert sample.dtype == pair.dtype == np.int64 and np.array_equal(sample, one[0]) and np.array_equal(pair, one[1]), step


def test_argument_errors_launch_nothing(ctx):
    S = 5
    gt = np.zeros((4, S), np.uint8)
    ctx.cohort_qc(gt)
    ms_before = ctx.kernel_ms()
    sample, pair = np.full((2048, 6), 0xABABABAB, np.uint32), np.full((10, 5), 0xABABABAB, np.uint32)
    g, s, p = gt.ctypes.data, sample.ctypes.data, pair.ctypes.data

    def refused(text, *args):
        rc = ctx.lib.svjg_cohort_qc(ctx.h, *args)
        assert rc == E_ARG and text in ctx.lib.svjg_last_error(ctx.h), (text, rc, ctx.lib.svjg_last_error(ctx.h))
        assert (sample == 0xABABABAB).all() and (pair == 0xABABABAB).all() and ctx.kernel_ms() == ms_before

    refused(b"null", None, None, 4, S, s, p)
    refused(b"null", g, None, 4, S, None, p)
    refused(b"null", g, None, 4, S, s, None)
    refused(b"null", g, None, 4, 2, s, None)
    refused(b"no sample", g, None, 4, 0, s, p)
    refused(b"SVJG_QC_MAX_SAMPLES", g, None, 4, 2049, s, p)
    refused(b"too many items", g, None, (1 << 29) + 1, 2048, s, p)           # 2^40 + 2048 items, below 2^32 rows
    refused(b"too many items", g, None, (1 << 32) - 1, 257, s, p)
    refused(b"too many rows", g, None, 1 << 32, 1, s, p)
    refused(b"too many rows", g, None, (1 << 64) - 1, 1, s, p)
    # the edges that are no errors: no row at all (zeroed outputs), one sample (no pair is written, pair may be null)
    assert ctx.lib.svjg_cohort_qc(ctx.h, g, None, 0, S, s, p) == 0 and not sample[:S].any() and not pair.any() and (sample[S:] == 0xABABABAB).all()
    pair[:] = 0xABABABAB
    one = np.array([[1], [2], [3], [0xFF]], np.uint8)
    assert ctx.lib.svjg_cohort_qc(ctx.h, one.ctypes.data, None, 4, 1, s, None) == 0
    assert sample[0].tolist() == [4, 2, 2, 2, 1, 1] and (pair == 0xABABABAB).all()
    out = ctx.cohort_qc(one)
    assert out[0].tolist() == [[4, 2, 2, 2, 1, 1]] and out[1].shape == (0, 5)
    assert _equal(ctx.cohort_qc(gt), M.qc(gt))                               # the context works afterwards


# ---- the drop-in script ----

def _script(tmp_path, name, *args):
    out = str(tmp_path / (name + ".vcf"))
    p = subprocess.run([sys.executable, os.path.join(AMD, "predict-genotype.py"), *args, "--minsupport", "3", "-o", out], capture_output=True, text=True,
                       timeout=STEP_SECONDS)
    assert p.returncode == 0, p.stderr
    return out


MIXED_PLOIDY = [("S1", "2\t1"), ("S2", "2\t1"), ("S3", "1\t30000\t40000\t0"), ("S4", "1\t3"), ("*", "2\t2")]      # as tests/test_cohort_ploidy_gpu.py


def _ploidy_gt(path, ploidy):
    """gt[n, S] out of a --cohort-ploidy file: the 1s of the GT text, 0xFF for dots"""
    data = [ln.split("\t")[9:] for ln in open(path).read().split("\n") if ln and not ln.startswith("#")]
    gt = np.array([[0xFF if "." in c.split(":")[0] else c.split(":")[0].count("1") for c in row] for row in data], np.uint8)
    assert gt.shape == ploidy.shape
    return gt


@pytest.mark.parametrize("option", ["plain", "prior", "ploidy", "joint"])
def test_script_writes_both_tables_and_the_same_vcf(golden, tmp_path, option):
    from svjg import genotype
    co = CM.Cohort(golden, "plain")
    extra, ploidy = {"plain": [], "prior": ["--cohort-prior"], "joint": ["--joint-ins"]}.get(option), None
    if option == "ploidy":
        f = tmp_path / "mixed.tsv"
        f.write_text("".join("%s\t%s\n" % x for x in MIXED_PLOIDY))
        extra = ["--cohort-ploidy", str(f)]
        ploidy = genotype.cohort_ploidy_matrix(co.rows, genotype.load_cohort_ploidy_file(str(f), co.names))     # the product's loader
        assert set(np.unique(ploidy).tolist()) == {0, 1, 2, 3}
    without = _script(tmp_path, "without", "--cohort", co.list, "-v", co.vcf, *extra)
    prefix = str(tmp_path / "qc")
    with_qc = _script(tmp_path, "with", "--cohort", co.list, "-v", co.vcf, *extra, "--cohort-qc", prefix)
    assert open(without, "rb").read() == open(with_qc, "rb").read()
    if ploidy is None:
        names, gt = vcf_gt(with_qc)
    else:
        names, gt = co.names, _ploidy_gt(with_qc, ploidy)
    assert names == co.names
    want = model_tsvs(tmp_path, names, gt, ploidy)
    assert (open(prefix + ".samples.tsv").read(), open(prefix + ".pairs.tsv").read()) == want
    assert want[0].count("\n") == 5 and want[1].count("\n") == 7


def test_script_finds_a_duplicated_sample(golden, tmp_path):
    co = CM.Cohort(golden, "plain")
    lines = [ln for ln in open(co.list).read().split("\n") if ln and not ln.startswith("#")]
    name, path = lines[0].split("\t")
    path = path if os.path.isabs(path) else os.path.join(co.dir, path)
    listed = tmp_path / "dup.list"
    listed.write_text("".join("%s\t%s\n" % (ln.split("\t")[0], os.path.join(co.dir, ln.split("\t")[1])) for ln in lines) + "%s_again\t%s\n" % (name, path))
    prefix = str(tmp_path / "dup")
    _script(tmp_path, "dup", "--cohort", str(listed), "-v", co.vcf, "--cohort-qc", prefix)
    pairs = [ln.split("\t") for ln in open(prefix + ".pairs.tsv").read().split("\n")[1:] if ln]
    hit = [p for p in pairs if p[0] == name and p[1] == name + "_again"]
    assert len(pairs) == 10 and len(hit) == 1 and hit[0][7:] == ["0.5000", "DUP"] and hit[0][3] == hit[0][4] == hit[0][5] != "0"
