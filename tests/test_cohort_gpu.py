"""Cohort genotyping on the GPU (svjg_cohort_*, svjg_genotype_cohort, k_genotype_cohort): every (row, sample) item against the diploid call
on that sample's counts alone, the site tags against sums over gt, and predict-genotype.py --cohort against the file assembled from the
reference's per-sample outputs (tests/golden/cohort/, tests/cohort_model.py).  Needs an MI355X: run with -m gpu."""
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import cohort_model as CM

pytestmark = pytest.mark.gpu

NONE = 0xFFFFFFFF
AMD = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "svjedi-graph_amd")
NOT_GENOTYPED = "./.:0:0,0:.,.,."


@pytest.fixture(scope="module")
def ctx():
    from svjg import capi
    c = capi.Context(0)
    yield c
    c.close()


def _site_of(gt):
    called = gt != 3
    return np.stack([called.sum(axis=1), np.where(called, gt, 0).sum(axis=1)], axis=1).astype(np.uint32)


def _single_sample(ctx, t, slot, ok, counts, present, ms, e):
    """the diploid call on ONE sample's counts (counts[n_slots, 2], present[n_slots]) -> gt, pl, raw, genotyped, boundary.  The item is
    genotyped iff ok bit 0, a slot, and the presence byte: handed to svjg_genotype as ok = 3 (the slot proves presence) or 0"""
    has = (slot != NONE) & ((ok & 1) != 0)
    ok_s = np.where(has & (present[np.where(slot != NONE, slot, 0)] != 0), 3, 0).astype(np.uint8)
    ctx.set_counts(counts)
    gt, pl, raw, done = ctx.genotype(t, slot, ok_s, ms, e)
    return gt, pl, raw, done, ctx.boundary_flags(len(t))


def _random_case(S, R, seed):
    """R rows over R + 5 slots for S samples: counts 0..60 (some deep), about 20 % of the (slot, sample) entries absent, some present with
    0,0, rows without a slot, rows whose gate bit is off, ok bit 1 set on some rows (ignored by the cohort call)"""
    rng = np.random.default_rng(seed)
    n_slots = R + 5
    counts = rng.integers(0, 61, size=(n_slots, S, 2)).astype(np.uint32)
    deep = rng.random((n_slots, S)) < 0.02
    counts[deep] = rng.integers(0, 30_000, size=(int(deep.sum()), 2))
    counts[rng.random((n_slots, S)) < 0.03] = 0
    present = (rng.random((n_slots, S)) >= 0.2).astype(np.uint8)
    t = rng.integers(0, 4, size=R).astype(np.uint8)
    slot = rng.permutation(n_slots)[:R].astype(np.uint32)
    slot[rng.random(R) < 0.05] = NONE
    ok = rng.choice(np.array([1, 3, 0, 2], np.uint8), size=R, p=[0.6, 0.3, 0.05, 0.05])
    # every case holds each kind of row at least once, whatever the draw gave: gate off (0), gate off with bit 1 (2), no slot, plain, bit 1 set
    at = rng.permutation(R)[:5]
    ok[at[0]], ok[at[1]], ok[at[3]], ok[at[4]] = 0, 2, 1, 3
    slot[at[2]] = NONE
    return n_slots, counts, present, t, slot, ok


def _load_matrix(ctx, n_slots, counts, present):
    S = counts.shape[1]
    ctx.cohort_alloc(S, n_slots)
    for s in range(S):
        keys = np.flatnonzero(present[:, s]).astype(np.uint32)
        ctx.cohort_set_counts(s, keys, counts[keys, s])


def _check_against_single_samples(ctx, n_slots, counts, present, t, slot, ok, ms, e, got):
    gt, pl, raw, done, boundary, site = got
    ctx.alloc_counts(n_slots)
    for s in range(counts.shape[1]):
        w = _single_sample(ctx, t, slot, ok, counts[:, s], present[:, s], ms, e)
        for name, a, b in zip(("gt", "pl", "raw", "genotyped", "boundary"), (gt[:, s], pl[:, s], raw[:, s], done[:, s], boundary[:, s]), w):
            assert np.array_equal(a, b), (name, s)
    assert np.array_equal(site, _site_of(gt))


def test_one_sample_is_the_diploid_kernel(ctx, golden):
    """S = 1 on every lik_kat row: equal to svjg_genotype + svjg_genotype_boundary on the same counts, whose own state stays as it was"""
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
            t, slot = c[:, 0].astype(np.uint8), np.arange(n, dtype=np.uint32)
            ctx.alloc_counts(n)
            ctx.set_counts(c[:, 1:3].astype(np.uint32))
            gt2, pl2, raw2, done2 = ctx.genotype(t, slot, np.full(n, 3, np.uint8), int(ms), float(e))
            b2 = ctx.boundary_flags(n)
            ctx.cohort_alloc(1, n)
            ctx.cohort_set_counts(0, slot, c[:, 1:3].astype(np.uint32))
            gt, pl, raw, done, b, site = ctx.genotype_cohort(t, slot, np.full(n, 1, np.uint8), int(ms), float(e))
            assert gt.shape == (n, 1) and pl.shape == (n, 1, 3) and raw.shape == (n, 1, 2) and site.shape == (n, 2)
            assert np.array_equal(gt[:, 0], gt2) and np.array_equal(pl[:, 0], pl2) and np.array_equal(raw[:, 0], raw2)
            assert np.array_equal(done[:, 0], done2) and np.array_equal(b[:, 0], b2)
            assert np.array_equal(site, _site_of(gt))
            assert np.array_equal(ctx.boundary_flags(n), b2)             # the diploid call's own state is as it was
            assert np.array_equal(gt2, c[:, 4]) and done.all()
            seen += n
    assert seen == len(cases) == 34_568


@pytest.mark.parametrize("S", [2, 3, 63, 64, 65, 130])
def test_every_item_is_the_single_sample_call(ctx, S):
    """R = ceil(3 * 256 / S) + 17 rows: several blocks, a partial last wave (but at S = 64, where every row is one whole wave), rows that
    straddle waves and blocks"""
    R = -(-3 * 256 // S) + 17
    n_slots, counts, present, t, slot, ok = _random_case(S, R, 1000 + S)
    assert R * S > 3 * 256 and (S == 64 or (R * S) % 64 != 0) and (slot == NONE).any() and (ok == 0).any() and not present.all()
    _load_matrix(ctx, n_slots, counts, present)
    for ms, e in ((3, 5e-5), (0, 1e-2)):
        got = ctx.genotype_cohort(t, slot, ok, ms, e)
        assert got[3].any() and not got[3].all() and (got[0] != 3).any()
        # an item that is not genotyped: gt 3, zero PLs, raw 0,0
        off = got[3] == 0
        assert (got[0][off] == 3).all() and not got[1][off].any() and not got[2][off].any() and not got[4][off].any()
        _check_against_single_samples(ctx, n_slots, counts, present, t, slot, ok, ms, e, got)


def test_more_items_than_one_trip_of_the_grid(ctx):
    """130 samples x 4100 rows = 533 000 items: more than 2048 blocks of 256 lanes (eight blocks on each of 256 compute units) hold at once,
    so every wave walks the grid-stride loop at least twice where the device has that many units or fewer, and the last trip is partial"""
    S, R = 130, 4100
    n_slots, counts, present, t, slot, ok = _random_case(S, R, 77)
    _load_matrix(ctx, n_slots, counts, present)
    got = ctx.genotype_cohort(t, slot, ok, 3, 5e-5)
    assert np.array_equal(got[5], _site_of(got[0]))
    ctx.alloc_counts(n_slots)
    for s in (0, 1, 64, 65, 129):
        w = _single_sample(ctx, t, slot, ok, counts[:, s], present[:, s], 3, 5e-5)
        assert all(np.array_equal(a[:, s], b) for a, b in zip(got[:5], w)), s
    # every item's raw counts and genotyped byte are what the matrix and the gate say
    has = ((slot != NONE) & ((ok & 1) != 0))[:, None] & (present[np.where(slot != NONE, slot, 0)] != 0)
    assert np.array_equal(got[3] != 0, has)
    assert np.array_equal(got[2], np.where(has[:, :, None], counts[np.where(slot != NONE, slot, 0)], 0))


def test_the_same_call_twice_gives_equal_bytes(ctx):
    S, R = 65, 40
    n_slots, counts, present, t, slot, ok = _random_case(S, R, 5)
    _load_matrix(ctx, n_slots, counts, present)
    a = ctx.genotype_cohort(t, slot, ok, 3, 5e-5)
    b = ctx.genotype_cohort(t, slot, ok, 3, 5e-5)
    assert all(x.tobytes() == y.tobytes() for x, y in zip(a, b))


def test_table_growth_does_not_double_the_site_tags():
    """a FRESH context (the log10(i!) table has its first size) and one sample with a row of ref = alt = 70 000: the kernel is launched again
    behind the table's growth, over all items; NS / AC are those of ONE pass"""
    from svjg import capi
    S, R = 3, 90
    n_slots, counts, present, t, slot, ok = _random_case(S, R, 9)
    deep_row = int(np.flatnonzero((slot != NONE) & ((ok & 1) != 0))[4])
    t[deep_row] = 2
    counts[slot[deep_row], 1] = (70_000, 70_000)
    present[slot[deep_row], :] = 1
    counts[counts > 60] = 7                                        # (no other deep item: the growth is this row's)
    counts[slot[deep_row], 1] = (70_000, 70_000)
    c = capi.Context(0)
    try:
        _load_matrix(c, n_slots, counts, present)
        got = c.genotype_cohort(t, slot, ok, 3, 5e-5)
        assert got[3][deep_row, 1] == 1 and got[2][deep_row, 1].tolist() == [70_000, 70_000] and got[0][deep_row, 1] == 1
        assert got[5][:, 0].max() <= S and np.array_equal(got[5], _site_of(got[0]))
        _check_against_single_samples(c, n_slots, counts, present, t, slot, ok, 3, 5e-5, got)
    finally:
        c.close()


def test_empty_and_bad_calls(ctx):
    from svjg import capi
    n_slots, counts, present, t, slot, ok = _random_case(3, 20, 3)
    fresh = capi.Context(0)
    try:
        with pytest.raises(capi.SvjgError):                        # no matrix
            fresh.genotype_cohort(t, slot, ok, 3, 5e-5)
        with pytest.raises(capi.SvjgError):
            fresh.cohort_set_counts(0, np.zeros(1, np.uint32), np.zeros((1, 2), np.uint32))
        with pytest.raises(capi.SvjgError):
            fresh.cohort_store_counts(0)
        with pytest.raises(capi.SvjgError):
            fresh.cohort_alloc(0, 5)
    finally:
        fresh.close()
    _load_matrix(ctx, n_slots, counts, present)
    out = ctx.genotype_cohort(t[:0], slot[:0], ok[:0], 3, 5e-5)
    assert [x.shape for x in out] == [(0, 3), (0, 3, 3), (0, 3, 2), (0, 3), (0, 3), (0, 2)]
    one = np.zeros((1, 2), np.uint32)
    with pytest.raises(capi.SvjgError):                            # sample out of range
        ctx.cohort_set_counts(3, np.zeros(1, np.uint32), one)
    with pytest.raises(capi.SvjgError):                            # slot out of range
        ctx.cohort_set_counts(0, np.array([n_slots], np.uint32), one)
    with pytest.raises(capi.SvjgError):                            # a slot named twice
        ctx.cohort_set_counts(0, np.array([2, 5, 2], np.uint32), np.zeros((3, 2), np.uint32))
    for s in range(3):                                             # none of them changed the matrix
        c_s, p_s = ctx.cohort_get_counts(s)
        assert np.array_equal(p_s, present[:, s]) and np.array_equal(c_s, np.where(present[:, s, None] != 0, counts[:, s], 0))
    bad = slot.copy()
    bad[7] = n_slots                                               # reported after the pass, as svjg_genotype reports it
    with pytest.raises(capi.SvjgError) as ei:
        ctx.genotype_cohort(t, bad, ok, 3, 5e-5)
    assert "slot out of range" in str(ei.value)
    got = ctx.genotype_cohort(t, slot, ok, 3, 5e-5)                # the context works afterwards
    _check_against_single_samples(ctx, n_slots, counts, present, t, slot, ok, 3, 5e-5, got)
    # cohort_set_counts replaces the sample's column: the slots it does not name become absent
    ctx.cohort_set_counts(1, np.array([4], np.uint32), np.array([[9, 1]], np.uint32))
    c_1, p_1 = ctx.cohort_get_counts(1)
    assert p_1.sum() == 1 and p_1[4] == 1 and c_1[4].tolist() == [9, 1] and c_1.sum() == 10


def test_store_counts_from_the_classify_kernels(ctx, golden):
    """golden/testdir/test.gaf classified on its graph, stored as sample 0 on the device; sample 1 set from the same counts on the host"""
    from svjg import genotype
    from svjg.graph import Graph
    d = f"{golden}/testdir"
    g = Graph.from_files(f"{d}/test_svs_edges.json", f"{d}/test.gfa")
    ctx.load_graph(g)
    ctx.classify(open(f"{d}/test.gaf", "rb").read())
    counts = ctx.counts()
    assert counts.any()
    ctx.cohort_alloc(2, g.n_slots)
    ctx.cohort_store_counts(0)
    ctx.cohort_set_counts(1, np.arange(g.n_slots, dtype=np.uint32), counts)
    c0, p0 = ctx.cohort_get_counts(0)
    c1, p1 = ctx.cohort_get_counts(1)
    assert np.array_equal(c0, counts) and np.array_equal(c1, counts) and np.array_equal(ctx.counts(), counts)
    assert np.array_equal(p0, (counts.sum(axis=1) != 0).astype(np.uint8)) and p1.all()       # presence of a stored zero count is 0
    rows = genotype.VcfRows(f"{d}/test.vcf", g.slot_of)
    gt, pl, raw, done, boundary, site = ctx.genotype_cohort(rows.sv_type, rows.slot, rows.ok, 3, 5e-5)
    nz = counts[np.where(rows.slot != NONE, rows.slot, 0)].sum(axis=1) != 0
    assert nz.sum() == 40
    for a in (gt, pl, raw, done, boundary):
        assert np.array_equal(a[nz, 0], a[nz, 1])
    w = ctx.genotype(rows.sv_type, rows.slot, rows.ok, 3, 5e-5)   # sample 0 is the ordinary call on the count vector
    assert all(np.array_equal(a[:, 0], b) for a, b in zip((gt, pl, raw, done), w))
    from svjg import capi
    ctx.alloc_counts(g.n_slots + 1)                               # a count vector of another length cannot be stored
    with pytest.raises(capi.SvjgError):
        ctx.cohort_store_counts(0)


# ---- the drop-in script ----

def _run(tmp_path, name, *args):
    out = str(tmp_path / f"{name}.vcf")
    p = subprocess.run([sys.executable, f"{AMD}/predict-genotype.py", *args, "--minsupport", "3", "-o", out], capture_output=True, text=True)
    return p, out


def test_script_on_the_plain_cohort(golden, tmp_path):
    co = CM.Cohort(golden, "plain")
    want = str(tmp_path / "want.vcf")
    co.assemble(want)
    p, out = _run(tmp_path, "plain", "--cohort", co.list, "-v", co.vcf)
    assert p.returncode == 0, p.stderr
    assert open(out, "rb").read() == open(want, "rb").read()
    assert p.stdout == "".join("Genotyped svs (%s): %d\n" % (n, k) for n, k in zip(co.names, co.genotyped))
    data = [ln.split("\t") for ln in open(out).read().split("\n") if ln and not ln.startswith("#")]
    exp = [ln.split("\t") for ln in open(f"{golden}/testdir/expected_genotype.vcf").read().split("\n") if ln and not ln.startswith("#")]
    assert [d[9] for d in data] == [e[9] for e in exp]             # sample 1 is the reference JSON at depth 1.0


def test_script_on_the_edited_cohort(golden, tmp_path):
    co = CM.Cohort(golden, "edited")
    want = str(tmp_path / "want.vcf")
    co.assemble(want)
    p, out = _run(tmp_path, "edited", "--cohort", co.list, "-v", co.vcf)
    assert p.returncode == 0, p.stderr
    assert open(out, "rb").read() == open(want, "rb").read()
    assert p.stdout == "".join("Genotyped svs (%s): %d\n" % (n, k) for n, k in zip(co.names, co.genotyped))
    data = [ln.split("\t") for ln in open(out).read().split("\n") if ln and not ln.startswith("#")]
    e = co.manifest["edits"]
    row_of = {co.keys[sl]: r for r, sl in enumerate(co.rows.slot) if sl != NONE}
    assert data[row_of[e["deleted_from_sample_2"]]][9 + 1] == NOT_GENOTYPED                   # an absent key
    assert data[row_of[e["deleted_from_sample_2"]]][9] != NOT_GENOTYPED
    assert data[row_of[e["empty_lists_in_sample_3"]]][9 + 2] == "./.:0:0,0:0,0,0"             # a key with two empty lists: genotyped with 0,0
    only4 = data[row_of[e["only_in_sample_4"]]][9:]
    assert only4[:3] == [NOT_GENOTYPED] * 3 and only4[3] != NOT_GENOTYPED
    for d in data:                                                 # the site tags say what the row's GT columns say
        gts = [c.split(":")[0] for c in d[9:]]
        ns, ac = sum(g != "./." for g in gts), sum(g.count("1") for g in gts if g != "./.")
        want = ["NS=%d" % ns, "AN=%d" % (2 * ns), "AC=%d" % ac] + (["AF=%s" % ("%.6g" % (ac / (2 * ns)))] if ns else [])
        assert d[7].split(";")[-len(want):] == want, d[:3]


@pytest.mark.parametrize("args", [("--cohort", "LIST", "-d", "JSON"), ("--cohort", "LIST", "--ploidy", "2"), ()])
def test_script_error_paths(golden, tmp_path, args):
    co = CM.Cohort(golden, "plain")
    args = [{"LIST": co.list, "JSON": os.path.join(co.dir, "s1.json")}.get(a, a) for a in args]
    p, out = _run(tmp_path, "never", *args, "-v", co.vcf)
    assert p.returncode != 0 and not os.path.exists(out)
    assert "usage:" in p.stderr
