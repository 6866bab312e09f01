"""The four genotype kernels on the device where the ROUNDING of each product c * L decides the answer (tests/golden/lik/lik_products.npz,
tests/products_items.py): deep one-sided rows whose PL turns by one if a product enters its sum unrounded (a fused multiply-add), rows at
err = 0.5 whose GT the roundings alone decide, ties l0 == l2.  k_genotype and k_genotype_cohort against the reference's own answers,
k_genotype_ploidy and k_genotype_sites against the models the CPU stand-ins are held to (tests/test_ploidy.py, tests/test_joint_ins.py), on
the same items.  The CPU stand-ins cannot speak for the device here: g++ on x86-64 never fuses.  Needs an MI355X: run with -m gpu.

On one MI355X (2026-10-19, ROCm 7.2.0; profiles/r12/experiments/geno_row_products.txt has the runs), rows that differ from the reference while
geno_row was compiled with fused multiply-adds: 5 788 GTs and 40 PLs in test_rows_kernel (PL0 of (INV, 0, 3 000 280 009): 129042943140 for
129042943141), the same items in test_cohort_kernel, all 40 rows of the fresh context; with `fp contract(off)` alone 1 236 GTs remained (here and
at ploidy 2, 4, 8), where the reference's rounding of a SUM to 28 digits decides against the one product it never rounds (svjg_geno.h:
dec28_round_dir)."""
import types

import numpy as np
import pytest

from tests import ploidy_model as PM
from tests import products_items as PI
from tests import site_model as SM

pytestmark = pytest.mark.gpu

NONE = 0xFFFFFFFF
NO_CALL = 0xFF
LOGFACT_FIRST = 65536                          # svjg_geno.h: logfact_first()


@pytest.fixture(scope="module")
def ctx():
    from svjg import capi
    c = capi.Context(0)
    yield c
    c.close()


def _genotype(ctx, c, ms, e):
    """rows c (type, ref, alt, ..), each with a count slot of its own -> gt, pl, raw, genotyped, boundary flags"""
    n = len(c)
    ctx.alloc_counts(n)
    ctx.set_counts(c[:, 1:3].astype(np.uint32))
    gt, pl, raw, done = ctx.genotype(c[:, 0].astype(np.uint8), np.arange(n, dtype=np.uint32), np.full(n, 3, np.uint8), ms, e)
    return gt, pl, raw, done, ctx.boundary_flags(n)


def _report(name, what, rows):
    """every figure is printed before anything is asserted (the record of a run that fails)"""
    print("%s: %s: %d rows%s" % (name, what, len(rows), "".join("\n    " + str(r) for r in rows[:40])))


def test_rows_kernel(ctx):
    """svjg_genotype per (min_support, err) group of the fixture: no one-sided row is flagged (its binomial term is log10(1)); GT is the
    reference's on every row (the host never recomputes GT); the PLs are the reference's straight from the kernel on every row that is not
    flagged and after apply_boundary_guard on all; fewer than 1 % of the half and equal rows are flagged (0 of 7 750 lie within 1e-6 of an
    integer by the reference's own values: the guard cannot hide a failure)"""
    from svjg import genotype
    cases, _, src = PI.fixture()
    one_sided = PI.one_sided()
    bad_gt, bad_pl, bad_guarded, flagged_one_sided, n_flag, n_he = [], [], [], [], 0, 0
    for ms, e, sel in PI.groups():
        c = cases[sel]
        gt, pl, raw, done, flags = _genotype(ctx, c, ms, e)
        assert done.all() and np.array_equal(raw, c[:, 1:3])
        flagged_one_sided += c[(flags != 0) & one_sided[sel]].tolist()
        bad_gt += [(src[sel[i]], c[i].tolist(), int(gt[i])) for i in np.flatnonzero(gt != c[:, 4])]
        bad_pl += [(src[sel[i]], c[i].tolist(), pl[i].tolist()) for i in np.flatnonzero((flags == 0) & (pl != c[:, 5:8]).any(axis=1))]
        guarded, _ = genotype.apply_boundary_guard(ctx, types.SimpleNamespace(sv_type=c[:, 0]), pl, raw, done, e)
        bad_guarded += [(src[sel[i]], c[i].tolist(), guarded[i].tolist()) for i in np.flatnonzero((guarded != c[:, 5:8]).any(axis=1))]
        he = np.isin(src[sel], ("half", "equal"))
        n_flag, n_he = n_flag + int((flags[he] != 0).sum()), n_he + int(he.sum())
    _report("k_genotype", "one-sided rows flagged", flagged_one_sided)
    _report("k_genotype", "GT differs from the reference", bad_gt)
    _report("k_genotype", "PLs of an unflagged row differ from the reference", bad_pl)
    _report("k_genotype", "PLs differ after the boundary guard", bad_guarded)
    print("k_genotype: %d of %d half and equal rows flagged" % (n_flag, n_he))
    assert n_he > 7000 and n_flag < 0.01 * n_he
    assert not flagged_one_sided and not bad_gt and not bad_pl and not bad_guarded


def _rotation(c, s):
    """row r of sample s holds the counts (and the reference's answers) of row _rotation(c, s)[r]: the rows of r's own SV type (the halving
    of a count depends on it) rotated by s * (their number // 3)"""
    src_row = np.arange(len(c))
    for t in range(4):
        at = np.flatnonzero(c[:, 0] == t)
        if len(at):
            src_row[at] = np.roll(at, -s * (len(at) // 3))
    return src_row


@pytest.mark.parametrize("S", [1, 3])
def test_cohort_kernel(ctx, S):
    """the same rows through svjg_genotype_cohort, one call per (min_support, err) group: sample s holds the group rotated (_rotation), so
    the S lanes of a row carry different counts and a segment mixes deep and small ones.  Every item against the REFERENCE's answers, NS and
    AC of every row against counts over the reference's GTs"""
    from svjg import genotype
    cases, _, _ = PI.fixture()
    bad_gt, bad_pl, bad_site, flagged_one_sided = [], [], [], []
    mixed = 0
    for ms, e, sel in PI.groups():
        c = cases[sel]
        n = len(c)
        slot = np.arange(n, dtype=np.uint32)
        want = np.stack([c[_rotation(c, s)] for s in range(S)], axis=1)                  # [n, S, 8]
        deep = want[:, :, 1:3].max(axis=2) >= 2**27
        mixed += int((deep.any(axis=1) & ~deep.all(axis=1)).sum())
        ctx.cohort_alloc(S, n)
        for s in range(S):
            ctx.cohort_set_counts(s, slot, want[:, s, 1:3].astype(np.uint32))
        gt, pl, raw, done, boundary, site = ctx.genotype_cohort(c[:, 0].astype(np.uint8), slot, np.full(n, 1, np.uint8), ms, e)
        assert done.all() and np.array_equal(raw, want[:, :, 1:3])
        t = c[:, 0][:, None]
        r1 = np.rint(np.where(t == 0, want[:, :, 1] / 2, want[:, :, 1]))                  # (half to even, like int(round(c, 0)))
        r2 = np.rint(np.where(t == 1, want[:, :, 2] / 2, want[:, :, 2]))
        flagged_one_sided += want[(boundary != 0) & ((r1 == 0) | (r2 == 0))].tolist()     # no binomial term, nothing to flag
        bad_gt += [(int(s), want[r, s].tolist(), int(gt[r, s])) for r, s in zip(*np.nonzero(gt != want[:, :, 4]))]
        for r, s in zip(*np.nonzero((pl != want[:, :, 5:8]).any(axis=2))):
            w = want[r, s].tolist()
            got = genotype.exact_pl(w[0], w[1], w[2], e) if boundary[r, s] else pl[r, s].tolist()
            if got != w[5:8]:
                bad_pl.append((int(s), w, got))
        called = want[:, :, 4] != 3
        ref_site = np.stack([called.sum(axis=1), np.where(called, want[:, :, 4], 0).sum(axis=1)], axis=1)
        bad_site += [(c[r].tolist(), site[r].tolist(), ref_site[r].tolist()) for r in np.flatnonzero((site != ref_site).any(axis=1))]
    _report("k_genotype_cohort S=%d" % S, "items without a binomial term flagged", flagged_one_sided)
    _report("k_genotype_cohort S=%d" % S, "GT differs from the reference", bad_gt)
    _report("k_genotype_cohort S=%d" % S, "PLs differ from the reference", bad_pl)
    _report("k_genotype_cohort S=%d" % S, "NS / AC differ from the reference's", bad_site)
    assert S == 1 or mixed > 50                                                           # rows whose lanes hold deep and small counts
    assert not flagged_one_sided and not bad_gt and not bad_pl and not bad_site


@pytest.mark.parametrize("kind,P", PI.PLOIDY_CASES)
def test_ploidy_kernel(ctx, kind, P):
    """k_genotype_ploidy on the items of tests/test_ploidy.py::test_row_arithmetic_where_the_products_roundings_decide, held to the model
    through the same call; no deep one-sided row is flagged"""
    for ms, e, rows, want in PI.ploidy_items(kind, P):
        n = len(rows)
        ctx.alloc_counts(n)
        ctx.set_counts(rows[:, 1:3].astype(np.uint32))
        gt, pl, raw, done, boundary = ctx.genotype_ploidy(rows[:, 0].astype(np.uint8), np.arange(n, dtype=np.uint32), np.full(n, 3, np.uint8),
                                                          rows[:, 3].astype(np.uint8), ms, e)
        assert done.all() and np.array_equal(raw, rows[:, 1:3])
        n_flagged = PM.check_against_model(rows, want, lambda r: (e, ms), gt, pl, boundary)
        assert kind == "half" or n_flagged == 0


def test_ploidy_2_is_the_reference(ctx):
    """k_genotype_ploidy at ploidy 2 on every row of the fixture: GT and the three PLs are the reference's (a flagged row: after
    exact_pl_ploidy), no one-sided row is flagged"""
    from svjg import genotype
    cases, _, src = PI.fixture()
    one_sided = PI.one_sided()
    bad = []
    for ms, e, sel in PI.groups():
        c = cases[sel]
        n = len(c)
        ctx.alloc_counts(n)
        ctx.set_counts(c[:, 1:3].astype(np.uint32))
        gt, pl, raw, done, boundary = ctx.genotype_ploidy(c[:, 0].astype(np.uint8), np.arange(n, dtype=np.uint32), np.full(n, 3, np.uint8),
                                                          np.full(n, 2, np.uint8), ms, e)
        assert done.all() and not pl[:, 3:].any() and not boundary[one_sided[sel]].any()
        for i in np.flatnonzero(boundary):
            pl[i, :3] = genotype.exact_pl_ploidy(int(c[i, 0]), int(c[i, 1]), int(c[i, 2]), 2, e)
        off = (np.where(gt == NO_CALL, 3, gt) != c[:, 4]) | (pl[:, :3] != c[:, 5:8]).any(axis=1)
        bad += [(src[sel[i]], c[i].tolist(), int(gt[i]), pl[i, :3].tolist()) for i in np.flatnonzero(off)]
    _report("k_genotype_ploidy P=2", "GT or PLs differ from the reference", bad)
    assert not bad


def _site_call(ctx, sites, ms, e):
    """every member a count slot of its own, each holding the site's ref count -> svjg_genotype_sites' four arrays"""
    counts, slots = [], np.full((len(sites), 6), NONE, np.uint32)
    for s, (ref, alts) in enumerate(sites):
        for j, a in enumerate(alts):
            slots[s, j] = len(counts)
            counts.append((ref, a))
    ctx.alloc_counts(len(counts))
    ctx.set_counts(np.array(counts, np.uint32))
    return ctx.genotype_sites(slots, ms, e)


@pytest.mark.parametrize("kind", ["one_sided", "half"])
def test_sites_kernel(ctx, kind):
    """k_genotype_sites on the sites of tests/test_joint_ins.py::test_site_arithmetic_where_the_products_roundings_decide, held to the model
    through the same call; no site with one deep count beside zeros is flagged (T = 0)"""
    for ms, e, sites, want in PI.site_items(kind):
        gt, pl, raw, boundary = _site_call(ctx, sites, ms, e)
        assert all(raw[s, 0] == ref and raw[s, 1:len(alts) + 1].tolist() == alts for s, (ref, alts) in enumerate(sites))
        n_flagged = SM.check_against_model(sites, want, lambda s: (e, ms), gt, pl, boundary)
        assert kind == "half" or n_flagged == 0


def test_deep_one_sided_on_a_fresh_context():
    """the fused rows alone as the FIRST call of a new context (no table yet, every binomial term log10(1)): the reference's GT and PLs, no
    flag, and the log10(i!) table stays at its first size — no one-sided row asks for a larger one"""
    from svjg import capi
    cases, err, src = PI.fixture()
    c = cases[src == "fused"]
    assert len(c) >= 24 and [2, 0, 3000280009] in c[:, 0:3].tolist() and (err[src == "fused"] == PI.E_DEEP).all() and (c[:, 3] == 3).all()
    fresh = capi.Context(0)
    try:
        assert fresh.logfact_entries() == 0
        gt, pl, raw, done, flags = _genotype(fresh, c, 3, PI.E_DEEP)
        entries = fresh.logfact_entries()
    finally:
        fresh.close()
    bad = [(c[i].tolist(), int(gt[i]), pl[i].tolist()) for i in np.flatnonzero((gt != c[:, 4]) | (pl != c[:, 5:8]).any(axis=1))]
    _report("k_genotype, fresh context", "fused rows that differ from the reference", bad)
    assert done.all() and not flags.any() and entries == LOGFACT_FIRST
    assert not bad
