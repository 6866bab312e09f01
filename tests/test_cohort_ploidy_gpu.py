"""Cohort genotyping at per-sample ploidy on the GPU (svjg_genotype_cohort_ploidy, k_genotype_cohort_ploidy): every (row, sample) item against
svjg_genotype_ploidy on that sample's counts alone, the all-2 matrix against svjg_genotype_cohort, the model of tests/ploidy_model.py at S = 1,
the site tags against sums over gt and ploidy, and predict-genotype.py --cohort --cohort-ploidy against the single-sample script and the
reference-made fixtures of tests/golden/cohort/.  Needs an MI355X: run with -m gpu."""
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import cohort_model as CM
from tests import ploidy_model as PM
from tests.test_cohort_gpu import _load_matrix, _random_case

pytestmark = pytest.mark.gpu

NONE = 0xFFFFFFFF
NO_CALL = 0xFF
E_ARG = -3                                         # svjg.h: SVJG_E_ARG
AMD = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "svjedi-graph_amd")


@pytest.fixture(scope="module")
def ctx():
    from svjg import capi
    c = capi.Context(0)
    yield c
    c.close()


def _site_of(gt, ploidy):
    """NS, AN, AC of every row from its items: the called ones, their ploidies, their alt copies"""
    called = gt != NO_CALL
    return np.stack([called.sum(axis=1), np.where(called, ploidy, 0).sum(axis=1, dtype=np.int64),
                     np.where(called, gt, 0).sum(axis=1, dtype=np.int64)], axis=1).astype(np.uint32)


def _single_sample(ctx, t, slot, ok, counts, present, ploidy, ms, e):
    """svjg_genotype_ploidy on ONE sample's counts and ploidies -> gt, pl[n, 9], raw, genotyped, boundary.  The item is genotyped iff ok bit
    0, a slot and the presence byte (and a ploidy of 1 or more, the kernel's own rule): handed over as ok = 3 (the slot proves presence) or 0"""
    has = (slot != NONE) & ((ok & 1) != 0)
    ok_s = np.where(has & (present[np.where(slot != NONE, slot, 0)] != 0), 3, 0).astype(np.uint8)
    ctx.set_counts(counts)
    return ctx.genotype_ploidy(t, slot, ok_s, ploidy, ms, e)


def _check_columns(ctx, n_slots, counts, present, t, slot, ok, ploidy, mp, ms, e, got, samples=None):
    gt, pl, raw, done, boundary, site = got
    assert pl.shape == gt.shape + (mp + 1,) and site.shape == (len(t), 3)
    ctx.alloc_counts(n_slots)
    for s in (range(counts.shape[1]) if samples is None else samples):
        w = _single_sample(ctx, t, slot, ok, counts[:, s], present[:, s], ploidy[:, s], ms, e)
        assert not w[1][:, mp + 1:].any()
        for name, a, b in zip(("gt", "pl", "raw", "genotyped", "boundary"), (gt[:, s], pl[:, s], raw[:, s], done[:, s], boundary[:, s]),
                              (w[0], w[1][:, :mp + 1], w[2], w[3], w[4])):
            assert np.array_equal(a, b), (name, s)
    assert np.array_equal(site, _site_of(gt, ploidy))


def _check_not_genotyped(got):
    gt, pl, raw, done, boundary, _ = got
    off = done == 0
    assert (gt[off] == NO_CALL).all() and not pl[off].any() and not raw[off].any() and not boundary[off].any()


def _mixed_ploidy(R, S, seed):
    """0..8, every value present, mixed within rows"""
    rng = np.random.default_rng(seed)
    p = rng.integers(0, 9, size=(R, S)).astype(np.uint8)
    p.reshape(-1)[rng.permutation(R * S)[:9]] = np.arange(9)
    return p


def _sex_ploidy(R, S, seed):
    """rows in three classes (autosome, X, Y), samples in two sexes: 2 / 2, 2 / 1, 0 / 1"""
    rng = np.random.default_rng(seed)
    cls = rng.integers(0, 3, R)
    cls[:3] = (0, 1, 2)
    male = rng.random(S) < 0.5
    male[0], male[-1] = False, True
    table = np.array([[2, 2], [2, 1], [0, 1]], np.uint8)            # [class][male]
    return table[cls][:, male.astype(np.int64)]


def _with_a_boundary_item(golden, n_slots, counts, present, t, slot, ok, ploidy):
    """a count pair of lik_boundary.npz (a PL within 4e-7 of an integer at e = 5e-5, found by search) in one diploid item"""
    c = np.load(f"{golden}/lik/lik_boundary.npz")["cases"][0]
    r = int(np.flatnonzero((slot != NONE) & ((ok & 1) != 0))[2])
    s = counts.shape[1] - 1
    t[r] = c[0]
    counts[slot[r], s] = c[1:3]
    present[slot[r], s] = 1
    ploidy[r, s] = 2
    return r, s


# ---- S = 1: the ploidy kernel, and the model ----

def test_one_sample_is_the_ploidy_kernel_and_the_model(ctx):
    from tests.test_ploidy import random_set
    rows, want = random_set()
    n = len(rows)
    assert n == 24_000
    gt, pl, flagged = np.zeros(n, np.uint8), np.zeros((n, 9), np.int64), np.zeros(n, np.uint8)
    for k, (e, ms) in enumerate(PM.SETTINGS):
        c = rows[np.arange(k, n, 6)]
        m = len(c)
        t, slot, cnt, p = c[:, 0].astype(np.uint8), np.arange(m, dtype=np.uint32), c[:, 1:3].astype(np.uint32), c[:, 3].astype(np.uint8)
        ctx.alloc_counts(m)
        ctx.set_counts(cnt)
        w = ctx.genotype_ploidy(t, slot, np.full(m, 3, np.uint8), p, ms, e)
        ctx.cohort_alloc(1, m)
        ctx.cohort_set_counts(0, slot, cnt)
        got = ctx.genotype_cohort_ploidy(t, slot, np.full(m, 1, np.uint8), p[:, None], 8, ms, e)
        assert got[1].shape == (m, 1, 9) and got[5].shape == (m, 3) and got[3].all()
        for name, a, b in zip(("gt", "pl", "raw", "genotyped", "boundary"), (x[:, 0] for x in got[:5]), w):
            assert np.array_equal(a, b), (name, e, ms)
        assert np.array_equal(got[5], _site_of(got[0], p[:, None]))
        gt[k::6], pl[k::6], flagged[k::6] = got[0][:, 0], got[1][:, 0], got[4][:, 0]
    PM.check_against_model(rows, want, lambda r: PM.SETTINGS[r % 6], gt, pl, flagged)


# ---- all-2: the diploid cohort kernel ----

def test_all_diploid_is_the_cohort_kernel(ctx):
    S, R = 65, 29
    n_slots, counts, present, t, slot, ok = _random_case(S, R, 2002)
    _load_matrix(ctx, n_slots, counts, present)
    for ms, e in ((3, 5e-5), (0, 1e-2)):
        d = ctx.genotype_cohort(t, slot, ok, ms, e)
        got = ctx.genotype_cohort_ploidy(t, slot, ok, np.full((R, S), 2, np.uint8), 2, ms, e)
        assert got[1].shape == (R, S, 3)
        assert np.array_equal(np.where(got[0] == NO_CALL, 3, got[0]), d[0]) and set(np.unique(got[0]).tolist()) <= {0, 1, 2, NO_CALL}
        for k in (1, 2, 3, 4):
            assert np.array_equal(got[k], d[k]), k
        assert np.array_equal(got[5][:, [0, 2]], d[5]) and np.array_equal(got[5][:, 1], 2 * d[5][:, 0])
        assert got[3].any() and (got[0] != NO_CALL).any()
    # the diploid cohort block's results are untouched: its pinned twin still holds the call's bytes (the next call returns them again, equal)
    again = ctx.genotype_cohort(t, slot, ok, 0, 1e-2)
    assert all(x.tobytes() == y.tobytes() for x, y in zip(d, again))


# ---- every item against the single-sample call ----

@pytest.mark.parametrize("pattern", ["mixed", "sex"])
@pytest.mark.parametrize("S", [2, 3, 63, 64, 65, 130])
def test_every_item_is_the_single_sample_call(ctx, golden, S, pattern):
    """R = ceil(3 * 256 / S) + 17 rows: several blocks, a partial last wave (but at S = 64), rows that straddle waves and blocks"""
    R = -(-3 * 256 // S) + 17
    n_slots, counts, present, t, slot, ok = _random_case(S, R, 3000 + S)
    assert R * S > 3 * 256 and (S == 64 or (R * S) % 64 != 0)
    if pattern == "mixed":
        ploidy, mp = _mixed_ploidy(R, S, 40 + S), 8
        assert set(np.unique(ploidy).tolist()) == set(range(9)) and (ploidy.min(axis=1) != ploidy.max(axis=1)).mean() > 0.8
    else:
        ploidy, mp = _sex_ploidy(R, S, 50 + S), 2
        assert set(np.unique(ploidy).tolist()) == {0, 1, 2}
    _with_a_boundary_item(golden, n_slots, counts, present, t, slot, ok, ploidy)
    _load_matrix(ctx, n_slots, counts, present)
    ms, e = 3, 5e-5
    got = ctx.genotype_cohort_ploidy(t, slot, ok, ploidy, mp, ms, e)
    gt, pl, raw, done, boundary, site = got
    # the case holds items of every kind: genotyped, not genotyped, ploidy 0, a no-call among the genotyped, a flagged one
    assert done.any() and not done.all() and (ploidy == 0).any() and not done[ploidy == 0].any()
    assert (done[ploidy != 0] == 0).any() and ((gt == NO_CALL) & (done != 0)).any() and (gt != NO_CALL).any() and boundary.any()
    _check_not_genotyped(got)
    _check_columns(ctx, n_slots, counts, present, t, slot, ok, ploidy, mp, ms, e, got)
    got2 = ctx.genotype_cohort_ploidy(t, slot, ok, ploidy, mp, 0, 1e-2)
    _check_not_genotyped(got2)
    _check_columns(ctx, n_slots, counts, present, t, slot, ok, ploidy, mp, 0, 1e-2, got2)


def test_more_items_than_one_trip_of_the_grid(ctx):
    """130 samples x 4100 rows = 533 000 items: more than the 1280 blocks of 256 lanes (five on each of 256 compute units) the launch is capped
    at, so every wave walks the grid-stride loop at least twice where the device has that many units or fewer, and the last trip is partial"""
    S, R = 130, 4100
    n_slots, counts, present, t, slot, ok = _random_case(S, R, 78)
    ploidy = _mixed_ploidy(R, S, 79)
    _load_matrix(ctx, n_slots, counts, present)
    got = ctx.genotype_cohort_ploidy(t, slot, ok, ploidy, 8, 3, 5e-5)
    assert np.array_equal(got[5], _site_of(got[0], ploidy)) and got[5][:, 0].max() > 64
    _check_not_genotyped(got)
    _check_columns(ctx, n_slots, counts, present, t, slot, ok, ploidy, 8, 3, 5e-5, got, samples=(0, 1, 64, 65, 129))
    has = ((slot != NONE) & ((ok & 1) != 0))[:, None] & (present[np.where(slot != NONE, slot, 0)] != 0) & (ploidy != 0)
    assert np.array_equal(got[3] != 0, has)
    assert np.array_equal(got[2], np.where(has[:, :, None], counts[np.where(slot != NONE, slot, 0)], 0))


def test_table_growth_does_not_double_the_site_tags():
    """a FRESH context (the log10(i!) table has its first size) and one item of ref = alt = 70 000: the kernel is launched again behind the
    table's growth, over all items; NS / AN / AC are those of ONE pass"""
    from svjg import capi
    S, R = 3, 90
    n_slots, counts, present, t, slot, ok = _random_case(S, R, 9)
    ploidy = _mixed_ploidy(R, S, 10)
    deep_row = int(np.flatnonzero((slot != NONE) & ((ok & 1) != 0))[4])
    t[deep_row] = 2
    present[slot[deep_row], :] = 1
    counts[counts > 60] = 7                                        # (no other deep item: the growth is this item's)
    counts[slot[deep_row], 1] = (70_000, 70_000)
    ploidy[deep_row, 1] = 4
    c = capi.Context(0)
    try:
        _load_matrix(c, n_slots, counts, present)
        got = c.genotype_cohort_ploidy(t, slot, ok, ploidy, 8, 3, 5e-5)
        assert got[3][deep_row, 1] == 1 and got[2][deep_row, 1].tolist() == [70_000, 70_000] and got[0][deep_row, 1] == 2
        assert got[5][:, 0].max() <= S and got[5][:, 1].max() <= 8 * S and np.array_equal(got[5], _site_of(got[0], ploidy))
        _check_columns(c, n_slots, counts, present, t, slot, ok, ploidy, 8, 3, 5e-5, got)
    finally:
        c.close()


def test_the_same_call_twice_gives_equal_bytes(ctx):
    S, R = 65, 40
    n_slots, counts, present, t, slot, ok = _random_case(S, R, 5)
    ploidy = _mixed_ploidy(R, S, 6)
    _load_matrix(ctx, n_slots, counts, present)
    a = ctx.genotype_cohort_ploidy(t, slot, ok, ploidy, 8, 3, 5e-5)
    b = ctx.genotype_cohort_ploidy(t, slot, ok, ploidy, 8, 3, 5e-5)
    assert all(x.tobytes() == y.tobytes() for x, y in zip(a, b))


def test_empty_and_bad_calls(ctx):
    from svjg import capi
    n_slots, counts, present, t, slot, ok = _random_case(3, 20, 3)
    ploidy = _mixed_ploidy(20, 3, 4)
    fresh = capi.Context(0)
    try:
        with pytest.raises(capi.SvjgError) as ei:                  # no matrix
            fresh.genotype_cohort_ploidy(t, slot, ok, ploidy[:, :0], 8, 3, 5e-5)
        assert "no cohort matrix" in str(ei.value)
    finally:
        fresh.close()
    _load_matrix(ctx, n_slots, counts, present)
    out = ctx.genotype_cohort_ploidy(t[:0], slot[:0], ok[:0], ploidy[:0], 2, 3, 5e-5)
    assert [x.shape for x in out] == [(0, 3), (0, 3, 3), (0, 3, 2), (0, 3), (0, 3), (0, 3)]
    for mp in (0, 9, 255):                                         # max_ploidy outside 1..8
        with pytest.raises(capi.SvjgError) as ei:
            ctx.genotype_cohort_ploidy(t, slot, ok, np.minimum(ploidy, 1), mp, 3, 5e-5)
        assert "max_ploidy" in str(ei.value)
    with pytest.raises(capi.SvjgError) as ei:                      # a ploidy byte above max_ploidy
        ctx.genotype_cohort_ploidy(t, slot, ok, ploidy, 7, 3, 5e-5)
    assert "ploidy above max_ploidy" in str(ei.value)
    nine = ploidy.copy()
    nine[19, 2] = 9
    with pytest.raises(capi.SvjgError):
        ctx.genotype_cohort_ploidy(t, slot, ok, nine, 8, 3, 5e-5)
    # a null array, and n_rows x n_samples beyond 2^40: refused before anything is read
    buf = np.zeros(20 * 3 * 9, np.int64)
    ptrs = [t.ctypes.data, slot.ctypes.data, ok.ctypes.data, ploidy.ctypes.data]
    outs = [buf.ctypes.data] * 6
    lib = ctx.lib
    for k in range(4):
        a = list(ptrs)
        a[k] = None
        assert lib.svjg_genotype_cohort_ploidy(ctx.h, *a, 8, 20, 3, 5e-5, *outs) == E_ARG
    for k in range(6):
        o = list(outs)
        o[k] = None
        assert lib.svjg_genotype_cohort_ploidy(ctx.h, *ptrs, 8, 20, 3, 5e-5, *o) == E_ARG
    assert lib.svjg_genotype_cohort_ploidy(ctx.h, *ptrs, 8, (1 << 40) // 3 + 1, 3, 5e-5, *outs) == E_ARG
    assert b"too many items" in lib.svjg_last_error(ctx.h)
    assert lib.svjg_genotype_cohort_ploidy(None, *ptrs, 8, 20, 3, 5e-5, *outs) == E_ARG
    bad = slot.copy()
    bad[7] = n_slots                                               # reported after the pass, as svjg_genotype reports it
    with pytest.raises(capi.SvjgError) as ei:
        ctx.genotype_cohort_ploidy(t, bad, ok, ploidy, 8, 3, 5e-5)
    assert "slot out of range" in str(ei.value)
    got = ctx.genotype_cohort_ploidy(t, slot, ok, ploidy, 8, 3, 5e-5)   # the context works afterwards
    _check_columns(ctx, n_slots, counts, present, t, slot, ok, ploidy, 8, 3, 5e-5, got)


def test_a_matrix_of_2_to_the_28_samples_is_refused():
    """AN must fit 32 bits: 2^28 samples x 1 slot (2.4 GB of matrix, allocated and zeroed, never read) is refused before any launch"""
    from svjg import capi
    c = capi.Context(0)
    try:
        c.cohort_alloc(1 << 28, 1)
        one, slot = np.zeros(1, np.uint8), np.zeros(1, np.uint32)
        buf = np.zeros(16, np.int64)
        rc = c.lib.svjg_genotype_cohort_ploidy(c.h, one.ctypes.data, slot.ctypes.data, one.ctypes.data, one.ctypes.data, 2, 1, 3, 5e-5,
                                               *([buf.ctypes.data] * 6))
        assert rc == E_ARG and b"too many samples" in c.lib.svjg_last_error(c.h)
    finally:
        c.close()


# ---- the drop-in script ----

def _run(tmp_path, name, *args):
    out = str(tmp_path / f"{name}.vcf")
    p = subprocess.run([sys.executable, f"{AMD}/predict-genotype.py", *args, "--minsupport", "3", "-o", out], capture_output=True, text=True)
    return p, out


def _data(path):
    return [ln.split("\t") for ln in open(path).read().split("\n") if ln and not ln.startswith("#")]


@pytest.mark.parametrize("which", ["plain", "edited"])
def test_script_with_an_all_diploid_file(golden, tmp_path, which):
    co = CM.Cohort(golden, which)
    want = str(tmp_path / "want.vcf")
    co.assemble(want)
    chroms = sorted(set(co.rows.chrom))
    f = tmp_path / "two.tsv"
    f.write_text("# everybody is diploid everywhere\n" + "".join("*\t%s\t2\n" % c for c in chroms))
    p, out = _run(tmp_path, which, "--cohort", co.list, "--cohort-ploidy", str(f), "-v", co.vcf)
    assert p.returncode == 0, p.stderr
    text = open(want).read()
    assert text.count("##FORMAT=<ID=PL,Number=3,") == 1
    assert open(out).read() == text.replace("##FORMAT=<ID=PL,Number=3,", "##FORMAT=<ID=PL,Number=G,")
    assert p.stdout == "".join("Genotyped svs (%s): %d\n" % (n, k) for n, k in zip(co.names, co.genotyped))


def test_script_with_a_mixed_file(golden, tmp_path):
    """S1 and S2 haploid on contig 2, S3 at ploidy 0 on 1:30000-40000, S4 triploid on contig 1: column s is what the single-sample script
    writes with the sample's own lines as its --ploidy-file"""
    co = CM.Cohort(golden, "plain")
    lines = [("S1", "2\t1"), ("S2", "2\t1"), ("S3", "1\t30000\t40000\t0"), ("S4", "1\t3"), ("*", "2\t2")]
    f = tmp_path / "mixed.tsv"
    f.write_text("# SAMPLE CHROM [FROM TO] PLOIDY\n" + "".join("%s\t%s\n" % x for x in lines))
    p, out = _run(tmp_path, "mixed", "--cohort", co.list, "--cohort-ploidy", str(f), "-v", co.vcf)
    assert p.returncode == 0, p.stderr
    data = _data(out)
    assert len(data) == 40 and all(len(d) == 9 + 4 and d[8] == "GT:DP:AD:PL" for d in data)
    stdout = ""
    for s, name in enumerate(co.names):
        own = tmp_path / f"{name}.txt"
        own.write_text("".join(rest + "\n" for who, rest in lines if who in ("*", name)))
        q, single = _run(tmp_path, name, "-d", os.path.join(co.dir, co.manifest["plain"][name]["json"]), "--ploidy-file", str(own), "-v", co.vcf)
        assert q.returncode == 0, q.stderr
        assert [d[9 + s] for d in data] == [d[9] for d in _data(single)], name
        stdout += q.stdout.replace("Genotyped svs:", "Genotyped svs (%s):" % name)
    assert p.stdout == stdout
    gt_of = [[d[9 + s].split(":")[0] for d in data] for s in range(4)]
    assert {"0", "1"} & set(gt_of[0]) and {"0", "1"} & set(gt_of[1]) and any(g.count("/") == 2 for g in gt_of[3])   # haploid and triploid calls show
    assert any(d[9 + 2] == ".:0:0,0:." for d in data) and sum(d[9 + 2] == ".:0:0,0:." for d in data) == 6
    for d in data:                                                 # the site tags say what the row's GT columns say
        called = [g.split("/") for g in (c.split(":")[0] for c in d[9:]) if "." not in g]
        ns, an, ac = len(called), sum(len(g) for g in called), sum(g.count("1") for g in called)
        want = ["NS=%d" % ns, "AN=%d" % an, "AC=%d" % ac] + (["AF=%s" % ("%.6g" % (ac / an))] if an else [])
        assert d[7].split(";")[-len(want):] == want, d[:3]
    assert any(d[7].split(";")[-3] != "AN=%d" % (2 * int(d[7].split(";")[-4][3:])) for d in data if "AF=" in d[7])   # AN is not 2 NS everywhere


@pytest.mark.parametrize("kind", ["no_cohort", "bad_file", "unknown_sample"])
def test_script_error_paths(golden, tmp_path, kind):
    co = CM.Cohort(golden, "plain")
    f = tmp_path / "p.tsv"
    f.write_text({"no_cohort": "*\t1\t2\n", "bad_file": "*\t1\t2\nS1\t1\t9\n", "unknown_sample": "*\t1\t2\nS9\t1\t1\n"}[kind])
    if kind == "no_cohort":
        p, out = _run(tmp_path, "never", "-d", os.path.join(co.dir, "s1.json"), "--cohort-ploidy", str(f), "-v", co.vcf)
        assert p.returncode == 2 and "usage:" in p.stderr and "--cohort-ploidy needs --cohort" in p.stderr
    else:
        p, out = _run(tmp_path, "never", "--cohort", co.list, "--cohort-ploidy", str(f), "-v", co.vcf)
        assert p.returncode == 1 and "ValueError" in p.stderr and "%s:2:" % f in p.stderr
    assert not os.path.exists(out)
