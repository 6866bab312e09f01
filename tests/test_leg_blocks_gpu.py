"""The eleven step-by-step calls share one host leg (svjg_capi.hip: genotype_leg; the three cohort calls one more, cohort_call, the three site
calls another, sites_call, the two statistics over a run's calls a fourth, calls_leg) and keep a block each (svjg_ctx::leg[]).  The eight genotype
calls (CALLS) run on ONE context in any of four orders: every call returns the bytes it returns on a context of its own, whichever calls ran in
between, and a view of the diploid call's pinned block outlives the other seven.  The three statistics (STATS: svjg_cohort_qc, svjg_cohort_hwe,
svjg_cohort_qual) run between the eight, one statistic a test: nothing of the eleven disturbs another.  Needs an MI355X: run with -m gpu."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

NONE = 0xFFFFFFFF
R, S, N_SLOTS = 65, 3, 90              # two waves of rows with a ragged end; three samples; the sites' members lie behind the rows' slots
MS, ERR = 3, 5e-5
CALLS = ("rows", "ploidy", "sites", "cohort", "cohort_ploidy", "cohort_prior", "cohort_sites", "cohort_sites_prior")
STATS = ("cohort_qc", "cohort_hwe", "cohort_qual")


def _case():
    rng = np.random.default_rng(2610)
    c = {}
    c["counts"] = rng.integers(0, 61, size=(N_SLOTS, 2)).astype(np.uint32)        # the count vector: no row beyond the first table
    c["t"] = rng.integers(0, 4, size=R).astype(np.uint8)
    c["slot"] = rng.permutation(R).astype(np.uint32)
    c["slot"][7] = NONE
    c["ok"] = np.full(R, 3, np.uint8)
    c["ok"][11] = 0
    c["ploidy"] = np.resize(np.array([1, 2, 3, 8], np.uint8), R)
    c["item_ploidy"] = np.resize(np.array([1, 2, 3, 8], np.uint8), R * S).reshape(R, S)       # cycled over the items
    sites = np.full((5, 6), NONE, np.uint32)
    at = R
    for i, K in enumerate((2, 3, 6, 2, 3)):
        sites[i, :K] = np.arange(at, at + K)
        at += K
    assert at <= N_SLOTS
    c["sites"] = sites
    # the matrix: its own counts, a fifth of the entries absent, and ONE item with ref + alt = 80 000 > 65 536 (sv_type 2: nothing is halved):
    # only the three cohort-matrix calls meet it, so the table grows inside the first of their legs, whichever legs ran in front of it
    cm = rng.integers(0, 61, size=(N_SLOTS, S, 2)).astype(np.uint32)
    present = (rng.random((N_SLOTS, S)) >= 0.2).astype(np.uint8)
    deep = 20
    assert c["slot"][deep] != NONE and c["ok"][deep] & 1
    c["t"][deep] = 2
    cm[c["slot"][deep], 1] = (40_000, 40_000)
    present[c["slot"][deep], 1] = 1
    c["cm"], c["present"], c["deep"] = cm, present, deep
    return c


def _load(ctx, c):
    ctx.alloc_counts(N_SLOTS)
    ctx.set_counts(c["counts"])
    ctx.cohort_alloc(S, N_SLOTS)
    for s in range(S):
        keys = np.flatnonzero(c["present"][:, s]).astype(np.uint32)
        ctx.cohort_set_counts(s, keys, c["cm"][keys, s])


def _call(ctx, c, which, view=False):
    """-> the call's arrays (rows: with the boundary flags behind them); view: the diploid call's arrays as views of the pinned block"""
    if which == "rows":
        out = ctx.genotype(c["t"], c["slot"], c["ok"], MS, ERR, reuse_outputs=view)
        return (*out, ctx.boundary_flags(R))
    if which == "ploidy":
        return ctx.genotype_ploidy(c["t"], c["slot"], c["ok"], c["ploidy"], MS, ERR)
    if which == "sites":
        return ctx.genotype_sites(c["sites"], MS, ERR)
    if which == "cohort_sites":
        return ctx.genotype_cohort_sites(c["sites"], MS, ERR)              # (the same five sites, as candidates in the matrix)
    if which == "cohort_sites_prior":
        return ctx.genotype_cohort_sites_prior(c["sites"], MS, ERR)        # (its first six arrays are the call's without the prior)
    if which == "cohort_ploidy":
        return ctx.genotype_cohort_ploidy(c["t"], c["slot"], c["ok"], c["item_ploidy"], 8, MS, ERR)
    if which == "cohort_prior":
        return ctx.genotype_cohort_prior(c["t"], c["slot"], c["ok"], None, 2, MS, ERR)
    return ctx.genotype_cohort(c["t"], c["slot"], c["ok"], MS, ERR)


def _bytes(arrays):
    return [np.array(a).tobytes() for a in arrays]


@pytest.fixture(scope="module")
def case():
    return _case()


@pytest.fixture(scope="module")
def alone(case):
    """every call on a fresh context of its own with the same counts -> {call: bytes of its arrays}"""
    from svjg import capi
    want = {}
    for which in CALLS:
        ctx = capi.Context(0)
        try:
            _load(ctx, case)
            assert ctx.logfact_entries() == 0
            want[which] = _bytes(_call(ctx, case, which))
            assert (ctx.logfact_entries() > 65536) == (which in ("cohort", "cohort_ploidy", "cohort_prior"))   # the deep item is a ROW's, in the matrix alone
        finally:
            ctx.close()
    gt, pl, raw, done, boundary, site = (np.frombuffer(b, dt) for b, dt in zip(want["cohort"], (np.uint8, np.int64, np.uint32, np.uint8, np.uint8, np.uint32)))
    item = case["deep"] * S + 1
    assert done[item] == 1 and raw[2 * item: 2 * item + 2].tolist() == [40_000, 40_000] and pl[3 * item: 3 * item + 3].any()
    assert any(want["rows"][0]) and any(want["ploidy"][1]) and any(want["sites"][1]) and any(want["cohort_ploidy"][1]) and any(want["cohort_prior"][1])
    assert any(want["cohort_sites"][1]) and any(want["cohort_sites"][5])      # PLs and site words
    assert all(any(want["cohort_sites_prior"][i]) for i in (1, 6, 8))         # PLs, posterior calls, frequencies
    return want


@pytest.mark.parametrize("order", [("rows", "ploidy", "sites", "cohort", "cohort_sites", "cohort_ploidy", "cohort_prior", "rows"),
                                   ("rows", "cohort_sites", "cohort_prior", "cohort", "sites", "cohort_ploidy", "ploidy", "rows"),
                                   ("rows", "cohort_sites", "cohort_sites_prior", "cohort_prior", "sites", "cohort_sites_prior", "cohort", "ploidy", "rows"),
                                   ("rows", "cohort_sites_prior", "cohort", "cohort_sites", "cohort_sites_prior", "cohort_ploidy", "cohort_prior",
                                    "cohort_sites_prior", "rows")])
def test_every_call_in_a_block_of_its_own(case, alone, order):
    from svjg import capi
    ctx = capi.Context(0)
    try:
        _load(ctx, case)
        view = _call(ctx, case, order[0], view=True)[:4]             # gt, pl, raw, genotyped: pointers into the pinned block
        assert _bytes(view) == alone["rows"][:4] and ctx.logfact_entries() == 65536
        for which in order[1:-1]:
            got = _bytes(_call(ctx, case, which))
            assert got == alone[which], which
            assert which != "cohort_sites_prior" or got[:6] == alone["cohort_sites"]
            assert _bytes(view) == alone["rows"][:4], f"the view after {which}"
            assert ctx.boundary_flags(R).tobytes() == alone["rows"][4], f"the boundary bytes after {which}"
        assert ctx.logfact_entries() > 65536                         # the table grew inside a leg that was not the first
        assert _bytes(_call(ctx, case, order[-1])) == alone["rows"]
    finally:
        ctx.close()


def _statistic(case, stat):
    """-> (the arguments of Context method `stat`, first(ctx) -> its arrays, held to the statistic's expected answer).  cohort_qc and cohort_hwe: 130
    rows x 70 samples at mixed ploidy, against tests/cohort_qc_model.py and by tests/test_cohort_hwe_gpu.py's check.  cohort_qual: the case's own rows
    and samples, the smallest shape with two waves of rows, a ragged end and every ploidy class; a quality on at least one row."""
    if stat == "cohort_qual":
        args = (case["t"], case["slot"], case["ok"], case["item_ploidy"], 8, ERR)

        def first(ctx):
            out = ctx.cohort_qual(*args)
            assert np.isfinite(out[0]).any()
            return out
    elif stat == "cohort_qc":
        from tests import cohort_qc_model
        from tests.test_cohort_qc import random_call
        from tests.test_cohort_qc_gpu import _equal
        args = random_call(np.random.default_rng(9), 130, 70, "mixed")

        def first(ctx):
            out = ctx.cohort_qc(*args)
            assert _equal(out, cohort_qc_model.qc(*args))
            return out
    else:
        from tests.test_cohort_hwe import draw
        from tests.test_cohort_hwe_gpu import check
        args = draw(np.random.default_rng(9), 130, 70, "mixed")

        def first(ctx):
            return check(ctx, *args, "alone")
    return args, first


@pytest.mark.parametrize("stat", STATS)
def test_a_statistic_in_a_block_of_its_own(case, alone, stat):
    """a statistic's call between a call and a reading of that call's outputs changes nothing of them: the diploid call's pinned views and boundary
    bytes survive it, every other call returns what it returns on a context of its own with the statistic's calls in between, and the statistic's
    own bytes stay what they are on a fresh context"""
    from svjg import capi
    args, first = _statistic(case, stat)

    def again(ctx):
        return _bytes(getattr(ctx, stat)(*args))

    def rows_intact(ctx, view):
        return _bytes(view) == alone["rows"][:4] and ctx.boundary_flags(R).tobytes() == alone["rows"][4]
    ctx = capi.Context(0)
    try:
        _load(ctx, case)
        want = _bytes(first(ctx))
    finally:
        ctx.close()
    ctx = capi.Context(0)
    try:
        _load(ctx, case)
        assert _bytes(first(ctx)) == want and ctx.logfact_entries() > 0      # (before any other call: the first table is the call's leg's)
        view = _call(ctx, case, "rows", view=True)[:4]
        assert _bytes(view) == alone["rows"][:4]
        assert again(ctx) == want and rows_intact(ctx, view)
        for which in CALLS[1:]:
            got = _bytes(_call(ctx, case, which))
            assert again(ctx) == want, which
            assert got == alone[which], which
            assert rows_intact(ctx, view), which
        if stat == "cohort_hwe":                                             # the two that stage through calls_leg, one behind the other
            qc = _bytes(ctx.cohort_qc(*args))
            assert again(ctx) == want and _bytes(ctx.cohort_qc(*args)) == qc
    finally:
        ctx.close()
