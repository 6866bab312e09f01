"""The device's log10(i!) table (k_logfact_local, k_logfact_bsum, k_logfact_add; read back through svjg_logfact_read) held entry by entry to
the bounds of tests/logfact_model.py — the terms of the guard's budget in svjg_geno.h — at the three sizes where the kernels differ: the first
table (64 blocks), a table grown inside a genotype call, and the cap (2^24 entries, 16 384 blocks: the only size at which the accumulated
error reaches what the budget bounds).  Needs an MI355X: run with -m gpu."""
import numpy as np
import pytest

from tests import logfact_model as LM

pytestmark = pytest.mark.gpu

CAP = LM.LOGFACT_CAP


def _genotype_one(ctx, sv_type, ref, alt):
    ctx.alloc_counts(1)
    ctx.set_counts(np.array([[ref, alt]], np.uint32))
    return ctx.genotype(np.array([sv_type], np.uint8), np.zeros(1, np.uint32), np.full(1, 3, np.uint8), 3, 5e-5)


def _check_all(t, name):
    LM.check_shape(t)
    LM.check_absolute(t, name)
    LM.check_increments(t, name)


@pytest.fixture(scope="module")
def sizes():
    """(first table, the table a row of n = 140 000 grows it to) from svjg_geno.h through tests/hostsim"""
    from tests.hostsim import sim
    _, first, cap, grow_to = sim.geno_constants()
    built, _ = sim.logfact_sizes()
    assert cap == CAP
    return first, built(grow_to(140_000))


@pytest.fixture(scope="module")
def cap_table():
    """the device's table at the cap, read back once (256 MB) and left unchanged"""
    from svjg import capi
    c = capi.Context(0)
    try:
        c.logfact_reserve(CAP)
        assert c.logfact_entries() == CAP
        t = c.logfact_table()
    finally:
        c.close()
    assert t.shape == (CAP, 2)
    t.flags.writeable = False
    return t


def test_first_table_and_growth_through_a_genotype_call(sizes):
    """a fresh context: the first genotype call builds 65 536 entries; a row with ref = alt = 70 000 grows the table inside its call; the old
    entries come out bit for bit (a block's local scan and the sequential scan of block sums do not depend on how many blocks follow); a
    second fresh context that reserves the same size holds the same bytes"""
    from svjg import capi
    first, grown = sizes
    c = capi.Context(0)
    try:
        assert c.logfact_entries() == 0
        _genotype_one(c, 3, 5, 5)
        assert c.logfact_entries() == first == 65536
        t1 = c.logfact_table()
        _, _, raw, done = _genotype_one(c, 2, 70_000, 70_000)
        assert done[0] == 1 and raw.tolist() == [[70_000, 70_000]]
        assert c.logfact_entries() == grown
        t2 = c.logfact_table()
    finally:
        c.close()
    assert t1.shape == (first, 2) and t2.shape == (grown, 2)
    _check_all(t1, "device, first table")
    _check_all(t2, "device, grown table")
    assert t2[:first].tobytes() == t1.tobytes()
    c = capi.Context(0)
    try:
        c.logfact_reserve(grown)
        assert c.logfact_entries() == grown
        t3 = c.logfact_table()
    finally:
        c.close()
    assert t3.tobytes() == t2.tobytes()


def test_cap_shape_and_absolute_value(cap_table):
    LM.check_shape(cap_table)
    LM.check_absolute(cap_table, "device at the cap")


def test_cap_every_increment(cap_table):
    """all 2^24 - 2 increments against log10(i): the budget's "each within one ulp" of the DEVICE's log10, measured"""
    LM.check_longdouble_log10(CAP)
    LM.check_increments(cap_table, "device at the cap")


def test_cap_binomial_term(golden, cap_table):
    """what geno_row takes from the table, on every (n, k) of the golden/lik files and the ten extra pairs, against the reference's double"""
    pairs = LM.all_pairs(golden)
    assert len(pairs) == 8846
    LM.check_pairs(cap_table, pairs, "device at the cap")


def test_cap_against_the_host_libm_table(cap_table):
    """the CPU stand-ins build the table with the host's log10 in another association: both lie inside the budget, so no entry differs by more
    than twice the per-entry bound.  This is what lets tests/hostsim and tests/geno_sim speak for the device."""
    from tests.hostsim import sim
    host = sim.logfact_table(CAP)
    differ, worst, at = LM.compare_tables(cap_table, host, "device against the host-libm table")
    assert worst <= 2 * LM.ABS_BOUND, (worst, at)
    assert cap_table[:4].tobytes() == host[:4].tobytes()            # 0, 0, log10(2), log10(6): nothing to disagree about yet


def test_calls(cap_table):
    """svjg_logfact_reserve / svjg_logfact_read: sizes, slices, errors"""
    from svjg import capi
    c = capi.Context(0)
    try:
        assert c.logfact_entries() == 0 and c.logfact_table().shape == (0, 2)
        with pytest.raises(capi.SvjgError) as ei:
            c.logfact_table(0, 1)
        assert "svjg_logfact_read" in str(ei.value)
        c.logfact_reserve(0)
        assert c.logfact_entries() == 0
        c.logfact_reserve(3000)
        assert c.logfact_entries() == 3072
        full = c.logfact_table()
        assert full.shape == (3072, 2) and full.tobytes() == cap_table[:3072].tobytes()
        for n in (0, 1, 1024, 3072):                                 # at or below the current size: nothing changes
            c.logfact_reserve(n)
            assert c.logfact_entries() == 3072 and c.logfact_table().tobytes() == full.tobytes()
        for first, n in ((0, 1), (1023, 2), (1, 3071), (3071, 1), (3072, 0), (2000, None)):
            got = c.logfact_table(first, n)
            assert got.tobytes() == full[first:(None if n is None else first + n)].tobytes(), (first, n)
        for first, n in ((3072, 1), (0, 3073), (3073, 0), (2**32 - 2, 1)):
            with pytest.raises(capi.SvjgError):
                c.logfact_table(first, n)
        assert c.logfact_table().tobytes() == full.tobytes()         # the context works afterwards
        _genotype_one(c, 3, 5, 5)                                    # the first genotype call finds a table: it keeps it
        assert c.logfact_entries() == 3072
    finally:
        c.close()


def test_genotypes_do_not_depend_on_the_table_size(golden):
    """all 320 rows of lik_boundary.npz (PLs next to an integer: where a changed table entry shows first) before and after a reserve to the cap"""
    from svjg import capi
    z = np.load(f"{golden}/lik/lik_boundary.npz")
    cases, errs = z["cases"], z["err"]
    assert len(cases) == 320

    def run(c):
        out = []
        for ms in np.unique(cases[:, 3]):
            for e in np.unique(errs):
                sel = np.flatnonzero((cases[:, 3] == ms) & (errs == e))
                if not len(sel):
                    continue
                n = len(sel)
                c.alloc_counts(n)
                c.set_counts(cases[sel, 1:3].astype(np.uint32))
                res = c.genotype(cases[sel, 0].astype(np.uint8), np.arange(n, dtype=np.uint32), np.full(n, 3, np.uint8), int(ms), float(e))
                out.append(b"".join(np.ascontiguousarray(x).tobytes() for x in res) + c.boundary_flags(n).tobytes())
                assert np.array_equal(res[0], cases[sel, 4]) and res[3].all()
        return out
    c = capi.Context(0)
    try:
        before = run(c)
        small = c.logfact_entries()
        c.logfact_reserve(CAP)
        assert small < CAP and c.logfact_entries() == CAP
        after = run(c)
    finally:
        c.close()
    assert sum(len(x) for x in before) == 320 * (1 + 24 + 8 + 1 + 1)
    assert before == after
