"""Cohort calls for insertions that share a position on the GPU (svjg_genotype_cohort_sites, k_genotype_cohort_sites): every (site, sample) item
against svjg_genotype_sites on that sample's present members alone (the same geno_site, in a kernel the parent has), the members and the site
sums against brute force, the table's growth inside a call, repeats and neighbours, the errors, and the drop-in script.  Needs an MI355X: run
with -m gpu."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import products_items as PI
from tests import site_model as SM

pytestmark = pytest.mark.gpu

NO_CALL = 0xFF
NONE = 0xFFFFFFFF
AMD = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "svjedi-graph_amd")
N_SITES = 3 * 64 + 17
E, MS = 5e-5, 3


@pytest.fixture(scope="module")
def ctx():
    from svjg import capi
    c = capi.Context(0)
    yield c
    c.close()


def _cohort(S, n_sites=N_SITES, seed=0, presence=0.75):
    """n_sites candidate sites of 2..6 candidates (K mixed as in SM.random_sites), every candidate a slot of its own -> (slots[n, 6],
    counts[S, n_slots, 2]: 0..60, a tenth of the items up to 20 000, present[S, n_slots])"""
    rng = np.random.default_rng(1000 * S + seed)
    K = [len(a) for _, a in SM.random_sites(n_sites, seed=77 + seed)]
    slots = np.full((n_sites, 6), NONE, np.uint32)
    at = 0
    for k, n in enumerate(K):
        slots[k, :n] = np.arange(at, at + n)
        at += n
    deep = rng.random((S, at, 1)) < 0.1
    counts = np.where(deep, rng.integers(0, 20_001, (S, at, 2)), rng.integers(0, 61, (S, at, 2))).astype(np.uint32)
    return slots, counts, rng.random((S, at)) < presence


_load = PI.load_cohort                          # (shared with tests/test_genotype_products_gpu.py)


def _members(slots, present):
    """[n, S] bytes: bit j = candidate j of site k is present for sample s"""
    ok = slots != NONE
    bits = present[:, np.where(ok, slots, 0)] & ok[None]                     # [S, n, 6]
    return (bits << np.arange(6)).sum(axis=2).astype(np.uint8).T


_brute_site = PI.brute_site                     # site[n, 6, 2] = NS_j, AC_j from the items' calls


def _single_sample(c, slots, counts_s, present_s):
    """svjg_genotype_sites on one sample's present members alone -> (which sites it has, gt, pl, raw, boundary of those)"""
    ok = slots != NONE
    bits = present_s[np.where(ok, slots, 0)] & ok
    has = np.flatnonzero(bits.sum(axis=1) >= 2)
    own = np.full((len(has), 6), NONE, np.uint32)
    for n, k in enumerate(has.tolist()):
        m = slots[k, bits[k]]
        own[n, :len(m)] = m
    c.alloc_counts(len(counts_s))
    c.set_counts(counts_s)
    return (has,) + tuple(c.genotype_sites(own, MS, E))


@pytest.mark.parametrize("S", [1, 2, 3, 63, 64, 65, 130])
def test_every_item_is_the_single_sample_sites_call(ctx, S):
    """3 * 64 + 17 sites: K and K' differ from lane to lane, items with K' < 2 sit inside full waves, sites straddle waves and (from S = 2 on)
    blocks.  gt, pl, raw and boundary bit for bit; members = the presence bits; the site sums = brute force over gt"""
    slots, counts, present = _cohort(S)
    _load(ctx, counts, present)
    gt, pl, raw, members, boundary, site = ctx.genotype_cohort_sites(slots, MS, E)
    print("k_genotype_cohort_sites, %d sites x %d samples: genotype_ms = %.4f" % (N_SITES, S, ctx.kernel_ms()[2]))
    want_members = _members(slots, present)
    assert np.array_equal(members, want_members)
    k_of = np.array([bin(int(m)).count("1") for m in want_members.ravel()]).reshape(want_members.shape)
    none = k_of < 2
    assert none.ravel()[:N_SITES * S // 64 * 64].any() and len(np.unique(k_of)) >= 5       # K' < 2 inside full waves; K' mixed
    assert (gt[none] == NO_CALL).all() and not pl[none].any() and not raw[none].any() and not boundary[none].any()
    for s in range(S):
        has, s_gt, s_pl, s_raw, s_boundary = _single_sample(ctx, slots, counts[s], present[s])
        assert np.array_equal(has, np.flatnonzero(~none[:, s]))
        assert np.array_equal(gt[has, s], s_gt) and np.array_equal(pl[has, s], s_pl) and np.array_equal(raw[has, s], s_raw), s
        assert np.array_equal(boundary[has, s], s_boundary), s
    assert np.array_equal(site, _brute_site(gt, members))
    if S == 1:
        has = np.flatnonzero(~none[:, 0])
        sites = [(int(raw[k, 0, 0]), raw[k, 0, 1:k_of[k, 0] + 1].tolist()) for k in has]
        SM.check_against_model(sites, [SM.genotype(ref, alts, MS, E) for ref, alts in sites], lambda s: (E, MS), gt[has, 0], pl[has, 0], boundary[has, 0])


def test_first_call_grows_the_table_and_the_sums_are_not_doubled():
    """a FRESH context whose first call holds one item with s_K >= 65 536 (the log10(i!) table grows inside the call and the kernel runs over all
    items again: the site words are zeroed in front of EVERY launch, or the sums would be doubled) and one with s_K >= 2^24 (beyond the cap:
    flagged, recomputed on the host)"""
    from svjg import capi, genotype
    S = 3
    slots, counts, present = _cohort(S, 40, seed=5, presence=0.9)
    deep = next(k for k in range(40) if slots[k, 2] != NONE)                 # a site of three candidates or more
    huge = 23 if deep != 23 else 24
    present[:, slots[deep, :3]] = True
    present[:, slots[huge, :2]] = True
    counts[1, slots[deep, :3]] = [(40_000, 60_000), (3, 30_000), (0, 7)]     # s_K = 85 000 and more
    counts[2, slots[huge, :2]] = [(9_000_000, 8_999_999), (12, 7_000_001)]   # s_K >= 2^24
    c = capi.Context(0)
    try:
        _load(c, counts, present)
        gt, pl, raw, members, boundary, site = c.genotype_cohort_sites(slots, MS, E)
        again = c.genotype_cohort_sites(slots, MS, E)
    finally:
        c.close()
    assert np.array_equal(members, _members(slots, present))
    assert boundary[huge, 2] == 1 and raw[deep, 1, 0] == 40_000 and raw[huge, 2, 0] == 9_000_000
    assert site.any() and np.array_equal(site, _brute_site(gt, members))
    assert all(np.array_equal(a, b) for a, b in zip((gt, pl, raw, members, boundary, site), again))
    for k, s in np.ndindex(40, S):
        K = bin(int(members[k, s])).count("1")
        if K < 2:
            assert gt[k, s, 0] == NO_CALL and not pl[k, s].any()
            continue
        ref, alts = int(raw[k, s, 0]), raw[k, s, 1:K + 1].tolist()
        w_call, w_pl = SM.genotype(ref, alts, MS, E)
        assert (int(gt[k, s, 0]), int(gt[k, s, 1])) == ((NO_CALL, NO_CALL) if w_call is None else w_call), (k, s)
        got = genotype.exact_pl_site(ref, alts, E) if boundary[k, s] else pl[k, s, :len(w_pl)].tolist()
        assert got == w_pl and not pl[k, s, len(w_pl):].any(), (k, s, ref, alts)


def test_repeat_and_neighbours(ctx):
    """two calls return equal bytes; a plain cohort call's outputs and an ordinary call's views are unchanged by a sites call in between"""
    from tests import ploidy_model as PM
    S = 65
    slots, counts, present = _cohort(S, 100, seed=9)
    _load(ctx, counts, present)
    n_slots = present.shape[1]
    rows = PM.random_rows(24_000)[:n_slots]
    ctx.alloc_counts(n_slots)
    ctx.set_counts(rows[:, 1:3].astype(np.uint32))
    types, all_slots, ok = np.ones(n_slots, np.uint8), np.arange(n_slots, dtype=np.uint32), np.ones(n_slots, np.uint8)
    views = ctx.genotype(rows[:, 0].astype(np.uint8), all_slots, np.full(n_slots, 3, np.uint8), 3, 5e-5, reuse_outputs=True)
    kept, flags = [np.array(v) for v in views], ctx.boundary_flags(n_slots)
    before = ctx.genotype_cohort(types, all_slots, ok, MS, E)
    a = ctx.genotype_cohort_sites(slots, MS, E)
    b = ctx.genotype_cohort_sites(slots, MS, E)
    assert all(np.array_equal(x, y) and x.tobytes() == y.tobytes() for x, y in zip(a, b))
    assert all(np.array_equal(v, k) for v, k in zip(views, kept)) and np.array_equal(ctx.boundary_flags(n_slots), flags)
    assert np.array_equal(ctx.counts(), rows[:, 1:3].astype(np.uint32))
    after = ctx.genotype_cohort(types, all_slots, ok, MS, E)
    assert all(np.array_equal(x, y) for x, y in zip(before, after))
    assert np.array_equal(a[5], _brute_site(a[0], a[3]))


def test_errors(ctx):
    from svjg import capi
    S = 3
    slots, counts, present = _cohort(S, 8, seed=3)
    n_slots = present.shape[1]
    fresh = capi.Context(0)
    try:
        with pytest.raises(capi.SvjgError):                                  # no matrix
            fresh.genotype_cohort_sites(slots, MS, E)
        _load(fresh, counts, present)
        assert np.array_equal(fresh.genotype_cohort_sites(slots, MS, E)[3], _members(slots, present))      # the context works afterwards
    finally:
        fresh.close()
    _load(ctx, counts, present)
    good = ctx.genotype_cohort_sites(slots, MS, E)

    def bad(change):
        s = slots.copy()
        change(s)
        with pytest.raises(capi.SvjgError):
            ctx.genotype_cohort_sites(s, MS, E)

    def one_member(s): s[3, 1:] = NONE
    def no_member(s): s[3, :] = NONE
    def hole(s): s[2, 0], s[2, 1] = NONE, s[2, 0]
    def hole_inside(s): s[1, :4] = (s[1, 0], NONE, s[1, 1], NONE)
    def out_of_range(s): s[5, 1] = n_slots
    def twice(s): s[4, 1] = s[4, 0]
    for change in (one_member, no_member, hole, hole_inside, out_of_range, twice):
        bad(change)
    out = [np.zeros((8, S, 2), np.uint8), np.zeros((8, S, 28), np.int64), np.zeros((8, S, 7), np.uint32), np.zeros((8, S), np.uint8), np.zeros((8, S), np.uint8),
           np.zeros((8, 6, 2), np.uint32)]
    for null in range(7):                                                    # a null array: the slots, then each output
        args = [slots.ctypes.data] + [x.ctypes.data for x in out]
        args[null] = None
        with pytest.raises(capi.SvjgError):
            ctx._chk(ctx.lib.svjg_genotype_cohort_sites(ctx.h, args[0], 8, MS, E, *args[1:]))
    assert ctx.lib.svjg_genotype_cohort_sites(ctx.h, None, 0, MS, E, *[None] * 6) == 0        # no site: nothing to do
    empty = ctx.genotype_cohort_sites(np.zeros((0, 6), np.uint32), MS, E)
    assert [x.shape for x in empty] == [(0, S, 2), (0, S, 28), (0, S, 7), (0, S), (0, S), (0, 6, 2)]
    again = ctx.genotype_cohort_sites(slots, MS, E)                          # the context works afterwards
    assert all(np.array_equal(x, y) for x, y in zip(good, again))


def test_script_columns_are_the_single_sample_joint_runs(tmp_path):
    """predict-genotype.py --cohort LIST --joint-ins on four samples: column s is what --joint-ins writes for sample s alone, but for `:.:.`"""
    from svjg import genotype
    from tests.test_cohort_joint_ins import VCF_TEXT, _sample_counts, _data
    vcf = tmp_path / "in.vcf"
    vcf.write_text(VCF_TEXT)
    samples = _sample_counts()
    for name, counts in samples:
        (tmp_path / (name + ".json")).write_text(json.dumps({k: [["r%d\n" % i for i in range(a)], ["a%d\n" % i for i in range(b)]] for k, (a, b) in counts.items()}, indent=4))
    (tmp_path / "cohort.list").write_text("".join("%s\t%s.json\n" % (name, name) for name, _ in samples))
    out = tmp_path / "cohort.vcf"
    p = subprocess.run([sys.executable, f"{AMD}/predict-genotype.py", "--cohort", str(tmp_path / "cohort.list"), "--joint-ins", "-v", str(vcf),
                        "--minsupport", str(MS), "-o", str(out)], capture_output=True, text=True)
    assert p.returncode == 0, (p.stdout, p.stderr)
    assert len([l for l in p.stderr.split("\n") if l.startswith("--joint-ins:")]) == 1 and "chr4:900" in p.stderr
    data = _data(out.read_text().split("\n"))
    n_site = n_dots = 0
    for s, (name, _) in enumerate(samples):
        alone = tmp_path / (name + ".vcf")
        genotype.run(str(tmp_path / (name + ".json")), str(vcf), str(alone), MS, E, joint_ins=True)
        for r, (got, want) in enumerate(zip(data, _data(alone.read_text().split("\n")))):
            assert got[:7] == want[:7]
            if got[8] == want[8]:
                assert got[9 + s] == want[9], (r, s)
                n_site += got[8].endswith(":SGT:SAL")
            else:
                assert got[8] == "GT:DP:AD:PL:SGT:SAL" and want[8] == "GT:DP:AD:PL" and got[9 + s] == want[9] + ":.:.", (r, s)
                n_dots += 1
    assert n_site == 17 and n_dots == 3
    for d in data:                                                           # the site tags say what the row's GT columns say
        gts = [c.split(":")[0] for c in d[9:]]
        ns, ac = sum(g != "./." for g in gts), sum(g.count("1") for g in gts if g != "./.")
        want = ["NS=%d" % ns, "AN=%d" % (2 * ns), "AC=%d" % ac] + (["AF=%s" % ("%.6g" % (ac / (2 * ns)))] if ns else [])
        assert d[7].split(";")[-len(want):] == want, d[:3]
