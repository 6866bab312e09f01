"""Genotypes at any ploidy from 1 to 8 on the GPU (svjg_genotype_ploidy, k_genotype_ploidy) against the diploid kernel at ploidy 2 and
against the model of tests/ploidy_model.py, and the drop-in scripts' --ploidy / --ploidy-file.  Needs an MI355X: run with -m gpu."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import ploidy_model as PM

pytestmark = pytest.mark.gpu

NO_CALL = 0xFF
AMD = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "svjedi-graph_amd")


@pytest.fixture(scope="module")
def ctx():
    from svjg import capi
    c = capi.Context(0)
    yield c
    c.close()


def _call(ctx, rows, ms, e, ok=3):
    """rows (type, ref, alt, ploidy), each with a count slot of its own -> genotype_ploidy's five arrays"""
    n = len(rows)
    ctx.alloc_counts(max(n, 1))
    ctx.set_counts(np.zeros((1, 2), np.uint32) if n == 0 else rows[:, 1:3].astype(np.uint32))
    return ctx.genotype_ploidy(rows[:, 0].astype(np.uint8), np.arange(n, dtype=np.uint32), np.full(n, ok, np.uint8), rows[:, 3].astype(np.uint8), ms, e)


def test_ploidy_2_is_the_diploid_kernel(ctx, golden):
    """ploidy 2 on every lik_kat row: bit-equal to svjg_genotype + svjg_genotype_boundary on the same context"""
    z = np.load(f"{golden}/lik/lik_kat.npz")
    cases, errs = z["cases"], z["err"]
    seen = 0
    for ms in np.unique(cases[:, 3]):
        for e in np.unique(errs):
            sel = np.flatnonzero((cases[:, 3] == ms) & (errs == e))
            if not len(sel):
                continue
            c = cases[sel]
            n = len(c)
            t, slot, ok = c[:, 0].astype(np.uint8), np.arange(n, dtype=np.uint32), np.full(n, 3, np.uint8)
            ctx.alloc_counts(n)
            ctx.set_counts(c[:, 1:3].astype(np.uint32))
            gt2, pl2, raw2, done2 = ctx.genotype(t, slot, ok, int(ms), float(e))
            b2 = ctx.boundary_flags(n)
            gt, pl, raw, done, b = ctx.genotype_ploidy(t, slot, ok, np.full(n, 2, np.uint8), int(ms), float(e))
            assert np.array_equal(np.where(gt == NO_CALL, 3, gt), gt2)
            assert np.array_equal(pl[:, :3], pl2) and not pl[:, 3:].any()
            assert np.array_equal(raw, raw2) and np.array_equal(done, done2) and np.array_equal(b, b2)
            assert np.array_equal(ctx.boundary_flags(n), b2)             # the diploid call's own state is as it was
            assert np.array_equal(gt2, c[:, 4]) and done.all()
            seen += n
    assert seen == len(cases) == 34_568


def test_mixed_ploidy_against_the_model(ctx):
    """3 * 256 + 17 rows of the random set in ONE call per (err, min_support): several blocks, a partial last one, the ploidy differs
    from lane to lane; then one row and no row"""
    rows = PM.random_rows(24_000)[:3 * 256 + 17]
    assert set(rows[:, 3]) == set(range(1, 9)) and len(set(rows[:64, 3])) > 4
    for e, ms in PM.SETTINGS:
        want = [PM.genotype(t, a, b, p, ms, e) for t, a, b, p in rows.tolist()]
        gt, pl, raw, done, boundary = _call(ctx, rows, ms, e)
        assert done.all() and np.array_equal(raw, rows[:, 1:3])
        PM.check_against_model(rows, want, lambda r: (e, ms), gt, pl, boundary)
    e, ms = PM.SETTINGS[1]
    one = rows[5:6]
    gt, pl, raw, done, boundary = _call(ctx, one, ms, e)
    PM.check_against_model(one, [PM.genotype(*one[0, :3].tolist(), int(one[0, 3]), ms, e)], lambda r: (e, ms), gt, pl, boundary)
    out = _call(ctx, rows[:0], ms, e)
    assert [len(x) for x in out] == [0] * 5 and out[1].shape == (0, 9)
    # a row of ploidy 0, a row without a slot and a row whose gate bit is off are not genotyped; the others are untouched by them
    mixed = rows[:6].copy()
    mixed[2, 3] = 0
    ctx.alloc_counts(6)
    ctx.set_counts(mixed[:, 1:3].astype(np.uint32))
    slot = np.arange(6, dtype=np.uint32)
    slot[3] = 0xFFFFFFFF
    ok = np.array([3, 3, 3, 3, 2, 3], np.uint8)
    gt, pl, raw, done, boundary = ctx.genotype_ploidy(mixed[:, 0], slot, ok, mixed[:, 3], ms, e)
    assert done.tolist() == [1, 1, 0, 0, 0, 1] and not raw[2:5].any() and not pl[2:5].any() and (gt[2:5] == NO_CALL).all()
    for r in (0, 1, 5):
        w_gt, w_pl = PM.genotype(*mixed[r, :3].tolist(), int(mixed[r, 3]), ms, e)
        assert int(gt[r]) == (NO_CALL if w_gt is None else w_gt) and (boundary[r] or pl[r, :len(w_pl)].tolist() == w_pl)


@pytest.mark.parametrize("P", [1, 4])
def test_first_call_grows_the_table_and_flags_the_row_beyond_it(P):
    """a FRESH context whose first call holds ordinary rows, one with n >= 65 536 (the log10(i!) table grows inside the call) and one
    with n >= 2^24 (beyond the table's cap: flagged, recomputed on the host)"""
    from svjg import capi, genotype
    rows = PM.random_rows(24_000)[:40].copy()
    rows[:, 3] = P
    rows[7] = (2, 40_000, 30_000, P)                   # n = 70 000
    rows[23] = (2, 9_000_000, 8_999_999, P)            # n >= 2^24
    e, ms = 5e-5, 3
    c = capi.Context(0)
    try:
        gt, pl, raw, done, boundary = _call(c, rows, ms, e)
    finally:
        c.close()
    assert done.all() and boundary[23] == 1
    for r, (t, a, b, p) in enumerate(rows.tolist()):
        w_gt, w_pl = PM.genotype(t, a, b, p, ms, e)
        assert int(gt[r]) == (NO_CALL if w_gt is None else w_gt), r
        got = genotype.exact_pl_ploidy(t, a, b, p, e) if boundary[r] else pl[r, :p + 1].tolist()
        assert got == w_pl and not pl[r, p + 1:].any(), (r, rows[r], got, w_pl)


def test_errors(ctx):
    from svjg import capi
    rows = PM.random_rows(24_000)[:8]
    bad = rows.copy()
    bad[3, 3] = 9
    with pytest.raises(capi.SvjgError):
        _call(ctx, bad, 3, 5e-5)
    ctx.alloc_counts(8)
    ctx.set_counts(rows[:, 1:3].astype(np.uint32))
    slot = np.arange(8, dtype=np.uint32)
    slot[5] = 8
    with pytest.raises(capi.SvjgError):
        ctx.genotype_ploidy(rows[:, 0], slot, np.full(8, 3, np.uint8), rows[:, 3], 3, 5e-5)
    fresh = capi.Context(0)
    try:
        with pytest.raises(capi.SvjgError):
            fresh.genotype_ploidy(rows[:, 0], np.arange(8, dtype=np.uint32), np.full(8, 3, np.uint8), rows[:, 3], 3, 5e-5)
        gt, pl, raw, done, boundary = _call(fresh, rows, 3, 5e-5)      # the context works afterwards
        assert done.all()
    finally:
        fresh.close()
    gt, pl, raw, done, boundary = _call(ctx, rows, 3, 5e-5)
    want = [PM.genotype(t, a, b, p, 3, 5e-5) for t, a, b, p in rows.tolist()]
    PM.check_against_model(rows, want, lambda r: (5e-5, 3), gt, pl, boundary)


# ---- the drop-in scripts on golden/testdir ----

def _predict(golden, tmp_path, name, *opts):
    t = f"{golden}/testdir"
    out = str(tmp_path / f"{name}.vcf")
    p = subprocess.run([sys.executable, f"{AMD}/predict-genotype.py", "-d", f"{t}/ref_informative_aln.json", "-v", f"{t}/test.vcf",
                        "--minsupport", "3", "-o", out, *opts], capture_output=True, text=True)
    assert p.returncode == 0, p.stderr
    return open(out).read().split("\n"), p.stdout


@pytest.fixture(scope="module")
def testdir_counts(golden):
    """per data row of golden/testdir/test.vcf: (type code, ref, alt, CHROM, POS) from the informative-alignment JSON"""
    from svjg import genotype
    t = f"{golden}/testdir"
    inf = json.load(open(f"{t}/ref_informative_aln.json"))
    keys = list(inf)
    rows = genotype.VcfRows(f"{t}/test.vcf", {k: i for i, k in enumerate(keys)}, True)
    assert (rows.ok == 3).all() and (rows.slot != 0xFFFFFFFF).all()
    return [(int(rows.sv_type[r]), len(inf[keys[rows.slot[r]]][0]), len(inf[keys[rows.slot[r]]][1]), rows.chrom[r], int(rows.pos[r]))
            for r in range(len(rows.slot))]


def _data(lines):
    return [l.split("\t") for l in lines if l and not l.startswith("#")]


def _check_rows(data, counts, ploidy_of):
    n_done = 0
    for cols, (t, ref, alt, chrom, pos) in zip(data, counts):
        P = ploidy_of(chrom, pos)
        gt, dp, ad, pl = cols[9].split(":")
        if P == 0:
            assert cols[9] == ".:0:0,0:."
            continue
        n_done += 1
        w_gt, w_pl = PM.genotype(t, ref, alt, P, 3, 5e-5)
        assert gt == ("/".join("." * P) if w_gt is None else "/".join("0" * (P - w_gt) + "1" * w_gt)), cols
        assert [int(x) for x in pl.split(",")] == w_pl, cols
    return n_done


def test_scripts_default_and_ploidy_2(golden, tmp_path, testdir_counts):
    t = f"{golden}/testdir"
    base, so = _predict(golden, tmp_path, "default")
    assert "\n".join(base) == open(f"{t}/ref_genotype.vcf").read() and so == "Genotyped svs: 40\n"
    exp = [l for l in open(f"{t}/expected_genotype.vcf").read().split("\n") if l and not l.startswith("#")]
    assert [l for l in base if l and not l.startswith("#")] == exp
    two, so = _predict(golden, tmp_path, "two", "--ploidy", "2")
    assert so == "Genotyped svs: 40\n" and len(two) == len(base)
    diff = [(a, b) for a, b in zip(base, two) if a != b]
    assert len(diff) == 1 and diff[0][0].startswith("##FORMAT=<ID=PL,Number=3,") and diff[0][1] == diff[0][0].replace("Number=3", "Number=G")


def test_scripts_haploid(golden, tmp_path, testdir_counts):
    one, so = _predict(golden, tmp_path, "one", "--ploidy", "1")
    data = _data(one)
    assert len(data) == len(testdir_counts) == 40 and so == "Genotyped svs: 40\n"
    assert {c[9].split(":")[0] for c in data} <= {"0", "1", "."} and {"0", "1"} <= {c[9].split(":")[0] for c in data}
    assert _check_rows(data, testdir_counts, lambda chrom, pos: 1) == 40
    assert sum(l.startswith("##FORMAT=<ID=PL,Number=G,") for l in one) == 1


def test_scripts_ploidy_file(golden, tmp_path, testdir_counts):
    f = tmp_path / "ploidy.txt"
    f.write_text("# hemizygous contig, a region that is absent\n2\t1\n1 30000 40000 0\n")

    def ploidy_of(default):
        return lambda chrom, pos: 1 if chrom == "2" else 0 if chrom == "1" and 30000 <= pos <= 40000 else default
    n_zero = sum(1 for c in testdir_counts if c[3] == "1" and 30000 <= c[4] <= 40000)
    assert n_zero == 6 and sum(1 for c in testdir_counts if c[3] == "2") == 4
    got, so = _predict(golden, tmp_path, "file", "--ploidy-file", str(f))
    assert _check_rows(_data(got), testdir_counts, ploidy_of(2)) == 40 - n_zero and so == "Genotyped svs: 34\n"
    got, so = _predict(golden, tmp_path, "file3", "--ploidy-file", str(f), "--ploidy", "3")
    assert _check_rows(_data(got), testdir_counts, ploidy_of(3)) == 40 - n_zero and so == "Genotyped svs: 34\n"
    f.write_text("2 1\n1 9\n")
    out = str(tmp_path / "never.vcf")
    p = subprocess.run([sys.executable, f"{AMD}/predict-genotype.py", "-d", f"{golden}/testdir/ref_informative_aln.json", "-v", f"{golden}/testdir/test.vcf",
                        "-o", out, "--ploidy-file", str(f)], capture_output=True, text=True)
    assert p.returncode == 1 and "ValueError" in p.stderr and not os.path.exists(out)
