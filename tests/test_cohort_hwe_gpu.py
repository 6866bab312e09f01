"""svjg_cohort_hwe on the device against the integer model (tests/cohort_hwe_model.py): counts bit for bit, HWE and EXCHET within the derived bound
of tests/test_cohort_hwe.py; every segment width and one, two and three items a lane in both phases; the fixtures; the growth of the log10(i!)
table; more rows than one trip of the grid; equal bytes from call to call and from chunk to chunk; the argument errors; and
predict-genotype.py --cohort --cohort-hwe on the golden cohort beside every other cohort option.  The device's bytes are also compared with the host
harness's (tests/geno_sim, topic hwe): the two differ in exp10 and in the table's log10 only, so the last bits of p may differ — the share of rows that do is
printed, and only the model bound binds.  Needs an MI355X: run with -m gpu."""
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import cohort_hwe_model as M
from tests import cohort_model as CM
from tests.geno_sim import hwe as hwe_sim
from tests.test_cohort_hwe import AMD, FAMILIES, check_tags, draw, held, load

pytestmark = pytest.mark.gpu

E_ARG = -3
STEP_SECONDS = 120                      # every run of the script is a process of its own under this limit
SIZES = [1, 2, 3, 31, 32, 33, 63, 64, 65, 130, 257]
ROWS = [1, 65, 1025]


@pytest.fixture(scope="module")
def ctx():
    from svjg import capi
    c = capi.Context(0)
    yield c
    c.close()


def check(ctx, gt, ploidy, what):
    """one call held to the model, twice for equal bytes -> (counts, p)"""
    want_c, want_p, near = M.hwe(gt, ploidy)
    assert not near.any(), what                                               # (no row is skipped)
    counts, p = ctx.cohort_hwe(gt, ploidy)
    assert counts.dtype == np.uint32 and p.dtype == np.float64 and np.array_equal(counts, want_c), what
    ok, worst = held(p, want_p)
    sim = hwe_sim.run(gt, ploidy)
    differ = (p.view(np.uint64) != sim[1].view(np.uint64)).any(axis=1).sum()
    print("%s: largest relative error %.3g; %d of %d rows differ from the harness in their last bits" % (what, worst, differ, len(p)))
    assert ok, (what, worst)
    again = ctx.cohort_hwe(gt, ploidy)
    assert again[0].tobytes() == counts.tobytes() and again[1].tobytes() == p.tobytes(), what
    return counts, p


@pytest.mark.parametrize("S", SIZES)
def test_device_within_the_bound_of_the_model(ctx, S):
    rng = np.random.default_rng(7300 + S)
    for n in ROWS:
        for mode in ("none", "two", "mixed"):
            gt, ploidy = draw(rng, n, S, mode, hi=0.5 if n != 65 else 0.9)
            if mode == "two" and n == 65:
                gt[:8] = 1                                                    # all het: the most terms a row of S can have (three a lane at 257)
            check(ctx, gt, ploidy, (S, n, mode))


@pytest.mark.parametrize("name", FAMILIES)
def test_device_on_the_fixtures(ctx, name):
    z = load(name)
    counts, p = ctx.cohort_hwe(M.masked(z["gt"], z.get("done")), z.get("ploidy"))
    assert np.array_equal(counts, z["counts"])
    ok, worst = held(p, z["p"])
    print("%s: largest relative error %.3g" % (name, worst))
    assert ok, worst


def test_2048_samples(ctx):
    rng = np.random.default_rng(2048)
    gt, ploidy = draw(rng, 65, 2048, "mixed")
    gt[:4], ploidy[:4] = 1, 2                                                 # 1025 terms: 17 a lane
    check(ctx, gt, ploidy, "2048 x 65")


def test_40000_samples_grow_the_table():
    """a fresh context: the first table has 65 536 entries, the call reserves 2 x 40 000 + 1"""
    from svjg import capi
    rng = np.random.default_rng(40000)
    S = 40000
    f = np.array([[0.02], [0.1]])
    gt = ((rng.random((2, S)) < f).astype(np.uint8) + (rng.random((2, S)) < f).astype(np.uint8)).astype(np.uint8)
    c = capi.Context(0)
    try:
        check(c, gt[:, :100].copy(), None, "100 x 2")
        assert c.logfact_entries() == 65536
        check(c, gt, None, "40000 x 2")
        assert c.logfact_entries() >= 2 * S + 1
        grown = c.logfact_entries()
        check(c, gt[:, :100].copy(), None, "100 x 2 again")
        assert c.logfact_entries() == grown                                   # (never a smaller table)
    finally:
        c.close()


def test_more_rows_than_one_trip_of_the_grid(ctx):
    """64 samples: one row a wave; the grid holds at most eight blocks of four waves a compute unit, 8 192 waves on 256 units"""
    assert hwe_sim.constants() == {"max_samples": 65536, "tpb": 256, "blocks_per_cu": 8} and hwe_sim.segment_width(64) == 64
    rng = np.random.default_rng(64)
    gt, ploidy = draw(rng, 2 * 8192 + 77, 64, "mixed")
    check(ctx, gt, ploidy, "64 x 16461")


@pytest.mark.parametrize("mode", ["none", "mixed"])
def test_chunks_give_the_bytes_of_one_call(ctx, mode):
    from svjg import genotype
    rng = np.random.default_rng(31)
    n, S = 130, 67
    gt, ploidy = draw(rng, n, S, mode)
    done = np.ones((n, S), np.uint8)
    one = check(ctx, gt, ploidy, "one call")
    for step in (1, 64, 65, n - 1):
        counts, p = genotype.cohort_hwe_rows(ctx, gt, done, ploidy, step)
        assert counts.tobytes() == one[0].tobytes() and p.tobytes() == one[1].tobytes(), step


def test_argument_errors_launch_nothing(ctx):
    S = 5
    gt = np.zeros((4, S), np.uint8)
    ctx.cohort_hwe(gt)
    ms_before = ctx.kernel_ms()
    entries = ctx.logfact_entries()
    counts, p = np.full((8, 3), 0xABABABAB, np.uint32), np.full((8, 2), -7.0)
    g, c, q = gt.ctypes.data, counts.ctypes.data, p.ctypes.data

    def refused(text, *args):
        rc = ctx.lib.svjg_cohort_hwe(ctx.h, *args)
        assert rc == E_ARG and text in ctx.lib.svjg_last_error(ctx.h), (text, rc, ctx.lib.svjg_last_error(ctx.h))
        assert (counts == 0xABABABAB).all() and (p == -7.0).all() and ctx.kernel_ms() == ms_before and ctx.logfact_entries() == entries

    refused(b"null", None, None, 4, S, c, q)
    refused(b"null", g, None, 4, S, None, q)
    refused(b"null", g, None, 4, S, c, None)
    refused(b"no sample", g, None, 4, 0, c, q)
    refused(b"SVJG_HWE_MAX_SAMPLES", g, None, 4, 65537, c, q)
    refused(b"too many items", g, None, (1 << 24) + 1, 65536, c, q)           # 2^40 + 65 536 items, below 2^32 rows
    refused(b"too many items", g, None, (1 << 32) - 1, 257, c, q)
    refused(b"too many rows", g, None, 1 << 32, 1, c, q)
    refused(b"too many rows", g, None, (1 << 64) - 1, 1, c, q)
    assert ctx.lib.svjg_cohort_hwe(ctx.h, g, None, 0, S, c, q) == 0 and (counts == 0xABABABAB).all() and (p == -7.0).all()   # no row: nothing written
    got = ctx.cohort_hwe(np.zeros((0, S), np.uint8))
    assert got[0].shape == (0, 3) and got[1].shape == (0, 2)
    one = np.array([[1], [2], [3], [0xFF]], np.uint8)
    got = ctx.cohort_hwe(one)
    assert got[0].tolist() == [[0, 1, 0], [0, 0, 1], [0, 0, 0], [0, 0, 0]] and got[1][:2].tolist() == [[1.0, 1.0], [1.0, 1.0]] and np.isnan(got[1][2:]).all()
    check(ctx, gt, None, "afterwards")                                        # the context works afterwards


# ---- the drop-in script ----

def _script(tmp_path, name, *args):
    out = str(tmp_path / (name + ".vcf"))
    p = subprocess.run([sys.executable, os.path.join(AMD, "predict-genotype.py"), *args, "--minsupport", "3", "-o", out], capture_output=True, text=True,
                       timeout=STEP_SECONDS)
    assert p.returncode == 0, p.stderr
    return out


@pytest.mark.parametrize("option", ["alone", "ploidy", "prior", "qual", "joint_prior", "qc"])
def test_script_end_to_end(golden, tmp_path, option):
    from svjg import genotype
    from tests.test_cohort_qc import vcf_gt
    from tests.test_cohort_qc_gpu import MIXED_PLOIDY, _ploidy_gt
    co = CM.Cohort(golden, "plain")
    extra = {"alone": [], "prior": ["--cohort-prior"], "qual": ["--cohort-qual"], "joint_prior": ["--joint-ins", "--joint-prior"],
             "qc": ["--cohort-qc", str(tmp_path / "qc")]}.get(option)
    ploidy = None
    if option == "ploidy":
        f = tmp_path / "mixed.tsv"
        f.write_text("".join("%s\t%s\n" % x for x in MIXED_PLOIDY))
        extra = ["--cohort-ploidy", str(f)]
        ploidy = genotype.cohort_ploidy_matrix(co.rows, genotype.load_cohort_ploidy_file(str(f), co.names))
    out = _script(tmp_path, "with", "--cohort", co.list, "-v", co.vcf, *extra, "--cohort-hwe")
    if ploidy is None:
        names, gt = vcf_gt(out)
    else:
        names, gt = co.names, _ploidy_gt(out, ploidy)
    assert names == co.names
    counts = check_tags(open(out).read(), gt, ploidy)
    assert (counts.sum(axis=1) > 0).any()
