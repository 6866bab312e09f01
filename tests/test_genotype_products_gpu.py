"""The six bit-exact genotype kernels on the device where the ROUNDING of each product c * L decides the answer (tests/golden/lik/lik_products.npz,
tests/golden/lik/site_products.npz, tests/products_items.py): deep one-sided rows whose PL turns by one if a product enters its sum unrounded
(a fused multiply-add), rows at err = 0.5 whose GT the roundings alone decide, ties l0 == l2, and sites found by search on which a PL turns.
k_genotype and k_genotype_cohort against the reference's own answers, k_genotype_ploidy, k_genotype_cohort_ploidy, k_genotype_sites and
k_genotype_cohort_sites against the models the CPU stand-ins are held to (tests/test_ploidy.py, tests/test_joint_ins.py), on the same
items.  The CPU stand-ins cannot speak for the device here: g++ on x86-64 never fuses; what the CPU tests do assert is that every set has
items a fused product would turn, by an exact emulation of the fused instructions in both orders (PI.sensitive_rows, PI.sensitive_sites).
By that emulation 18 of the 1 392 "one_sided" sites change a PL, every "searched" site does, 26 or 27 per K and order; of the 2 077 "half"
sites none was red even on a library built without the pragmas (at e = 0.5 the three site logarithms differ and nothing is near a tie).
k_cohort_prior stays out: it is not bit-exact but held to the 60-digit model within EM_F_BOUND, on deep one-sided items its weights underflow to 0, at the fixture's small counts a fused product moves f by less than that bound, and its PL / raw / genotyped / boundary
arrays are compared array for array with the two first kernels (tests/test_cohort_prior_gpu.py).  Needs an MI355X: run with -m gpu.

On one MI355X (2026-10-19, ROCm 7.2.0; profiles/r12/experiments/geno_row_products.txt has the runs), rows that differ from the reference while
geno_row was compiled with fused multiply-adds: 5 788 GTs and 40 PLs in test_rows_kernel (PL0 of (INV, 0, 3 000 280 009): 129042943140 for
129042943141), the same items in test_cohort_kernel, all 40 rows of the fresh context; with `fp contract(off)` alone 1 236 GTs remained (here and
at ploidy 2, 4, 8), where the reference's rounding of a SUM to 28 digits decides against the one product it never rounds (svjg_geno.h:
dec28_round_dir).  A later run (2026-10-20, ROCm 7.2, profiles/r19/experiments/cohort_products.txt) against a library without the three pragmas of
svjg_geno.h: 26 of these 28 tests red — all but test_sites_kernel[half] and test_ploidy_kernel[half-1], where the emulation predicts no
change either —, every searched site, every cohort site item and 37 / 112 one-sided cohort-ploidy items (S = 1 / 3), the counts the
emulation predicts."""
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


_rotation = PI.rotation                        # row r of sample s holds the rows of r's own SV type rotated


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


@pytest.mark.parametrize("kind", ["one_sided", "half", "searched"])
def test_sites_kernel(ctx, kind):
    """k_genotype_sites on the sites of tests/test_joint_ins.py::test_site_arithmetic_where_the_products_roundings_decide, held to the model
    through the same call; no site with one deep count beside zeros is flagged (T = 0).  "searched": every site has a PL that a fused product
    turns, nothing is flagged, the PLs are compared straight from the kernel"""
    for ms, e, sites, want in PI.site_items(kind):
        gt, pl, raw, boundary = _site_call(ctx, sites, ms, e)
        assert all(raw[s, 0] == ref and raw[s, 1:len(alts) + 1].tolist() == alts for s, (ref, alts) in enumerate(sites))
        red = [(sites[s], pl[s, :len(w_pl)].tolist(), w_pl) for s, (w_call, w_pl) in enumerate(want)
               if not boundary[s] and (pl[s, :len(w_pl)].tolist() != w_pl or tuple(gt[s]) != ((NO_CALL, NO_CALL) if w_call is None else w_call))]
        _report("k_genotype_sites %s err %g" % (kind, e), "unflagged sites whose call or PLs differ from the model, of %d" % len(sites), red)
        n_flagged = SM.check_against_model(sites, want, lambda s: (e, ms), gt, pl, boundary)
        assert kind == "half" or n_flagged == 0


@pytest.mark.parametrize("S", [1, 3])
def test_cohort_sites_kernel(ctx, S):
    """k_genotype_cohort_sites on the searched sites (PI.cohort_site_items, the arrays of
    tests/test_joint_ins.py::test_cohort_site_items_where_the_products_roundings_decide): every (site, sample) item is one searched site of K'
    members on a subset of the site's six candidates, K' and the masks differ from lane to lane, one item in eight has no site call.  GT pair
    and PLs are the model's for the embedded site, members the mask, raw the site's counts, nothing is flagged, NS_j / AC_j are recounted from
    the model's calls (PI.brute_site)"""
    for item in PI.cohort_site_items(S):
        PI.load_cohort(ctx, item.counts, item.present)
        gt, pl, raw, members, boundary, site = ctx.genotype_cohort_sites(item.slots, item.ms, item.e)
        red = [(int(k), int(s), raw[k, s].tolist(), gt[k, s].tolist(), [(int(g), int(pl[k, s, g]), int(item.pl[k, s, g])) for g in np.flatnonzero(pl[k, s] != item.pl[k, s])])
               for k, s in zip(*np.nonzero((pl != item.pl).any(axis=2) | (gt != item.gt).any(axis=2)))]
        _report("k_genotype_cohort_sites S=%d err %g" % (S, item.e), "items whose call or PLs differ from the model, of %d with a site call" % (item.site_of >= 0).sum(), red)
        assert np.array_equal(members, item.members) and np.array_equal(raw, item.raw) and not boundary.any()
        want_site = PI.brute_site(item.gt, item.members)
        bad_site = np.flatnonzero((site != want_site).any(axis=(1, 2)))
        _report("k_genotype_cohort_sites S=%d err %g" % (S, item.e), "sites whose NS_j / AC_j differ from the model's", bad_site.tolist())
        assert want_site[:, :, 0].max() == S and want_site[:, :, 1].any()
        assert not red and len(bad_site) == 0


def _cohort_ploidy_call(ctx, item):
    n, S = item.on.shape
    slot = np.arange(n, dtype=np.uint32)
    ctx.cohort_alloc(S, n)
    for s in range(S):
        ctx.cohort_set_counts(s, slot, np.ascontiguousarray(item.counts[:, s]))
    return ctx.genotype_cohort_ploidy(item.type, slot, np.full(n, 1, np.uint8), item.ploidy, 8, item.ms, item.e)


@pytest.mark.parametrize("S", [1, 3])
@pytest.mark.parametrize("kind", ["one_sided", "half"])
def test_cohort_ploidy_kernel(ctx, kind, S):
    """k_genotype_cohort_ploidy on the fixture's rows (PI.cohort_ploidy_items, the items of
    tests/test_ploidy.py::test_cohort_items_where_the_products_roundings_decide): sample s holds the rows rotated, the ploidy of item (r, s) is
    1 + (r + 3 s) mod 8 so that every ploidy occurs and ploidies mix within a row and a wave, every 11th item has ploidy 0.  Every item
    against the model through PM.check_against_model (no one-sided item flagged, fewer than 1 % of the half ones), the items at ploidy 0 not
    genotyped, NS / AN / AC against counts over the model's GTs"""
    for item in PI.cohort_ploidy_items(kind, S):
        gt, pl, raw, done, boundary, site = _cohort_ploidy_call(ctx, item)
        on, rows = item.on, item.rows
        assert pl.shape == on.shape + (9,) and np.array_equal(done != 0, on) and np.array_equal(raw, np.where(on[:, :, None], item.counts, 0))
        assert (gt[~on] == NO_CALL).all() and not pl[~on].any() and not boundary[~on].any()
        w_gt, w_site = PI.cohort_ploidy_expected(item)
        i_gt, i_pl, i_flag = gt[on], pl[on], boundary[on]
        red = [(rows[r].tolist(), int(i_gt[r]), i_pl[r, :rows[r, 3] + 1].tolist(), item.want[r]) for r in range(len(rows))
               if int(i_gt[r]) != (NO_CALL if item.want[r][0] is None else item.want[r][0]) or (not i_flag[r] and i_pl[r, :rows[r, 3] + 1].tolist() != item.want[r][1])]
        name = "k_genotype_cohort_ploidy %s S=%d min_support %d" % (kind, S, item.ms)
        _report(name, "items whose GT or (unflagged) PLs differ from the model, of %d" % len(rows), red)
        bad_site = np.flatnonzero((site != w_site).any(axis=1))
        _report(name, "rows whose NS / AN / AC differ from the model's", [(int(r), site[r].tolist(), w_site[r].tolist()) for r in bad_site])
        n_flagged = PM.check_against_model(rows, item.want, lambda r: (item.e, item.ms), i_gt, i_pl, i_flag)
        print("%s: %d of %d items flagged" % (name, n_flagged, len(rows)))
        assert n_flagged == 0 if kind == "one_sided" else n_flagged < 0.01 * len(rows)
        assert not red and len(bad_site) == 0


@pytest.mark.parametrize("kind", ["one_sided", "half"])
def test_cohort_ploidy_all_diploid_is_the_reference(ctx, kind):
    """the same calls at S = 1 with every ploidy 2: GT and the three PLs are the REFERENCE's stored answers (a flagged item: after
    exact_pl_ploidy), no one-sided item is flagged"""
    from svjg import genotype
    for item in PI.cohort_ploidy_items(kind, 1, True):
        gt, pl, raw, done, boundary, site = _cohort_ploidy_call(ctx, item)
        gt, pl, boundary, ref = gt[:, 0], pl[:, 0].copy(), boundary[:, 0], item.ref[:, 0]
        assert done.all() and not pl[:, 3:].any() and (kind == "half" or not boundary.any())
        for i in np.flatnonzero(boundary):
            pl[i, :3] = genotype.exact_pl_ploidy(int(item.type[i]), int(item.counts[i, 0, 0]), int(item.counts[i, 0, 1]), 2, item.e)
        off = np.flatnonzero((np.where(gt == NO_CALL, 3, gt) != ref[:, 0]) | (pl[:, :3] != ref[:, 1:4]).any(axis=1))
        _report("k_genotype_cohort_ploidy %s, every ploidy 2, min_support %d" % (kind, item.ms), "items that differ from the reference, of %d" % len(gt),
                [(int(item.type[i]), item.counts[i, 0].tolist(), int(gt[i]), pl[i, :3].tolist(), ref[i].tolist()) for i in off])
        called = ref[:, 0] != 3
        assert np.array_equal(site, np.stack([called, 2 * called, np.where(called, ref[:, 0], 0)], axis=1).astype(np.uint32))
        assert len(off) == 0


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
