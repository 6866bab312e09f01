"""The cohort call with an allele-frequency prior on the GPU (svjg_genotype_cohort_prior, k_cohort_prior) against the 60-digit model of
tests/cohort_prior_model.py, whose answers for the cases of tests/cohort_prior_cases.py are stored under tests/golden/cohort_prior/: about
1 500 rows x S for S on both sides of every segment width, once with every item diploid (ploidy NULL) and once with ploidies 0..8 mixed
within rows, min_support 0 and 3, planted rows, one case of deep counts; 200 or 300 rows x S at the shapes that only the kernel's body knows
(segment widths 2 and 16, two and three staged items on every lane, recomputed items behind three staged ones: S up to 320), and calls of more
rows than one trip of the grid holds.  Needs an MI355X: run with -m gpu.

What may be left out of a comparison is decided by the model alone, before any device ran (tests/golden/make_cohort_prior.py): rows whose
deciding EM step lies within 1e-6 of EM_TOL (left out of everything), items whose -10 log10(rest) lies within 1e-6 of an integer or whose two
largest posteriors lie within 1e-9 of each other (left out of GT / GQ); at most 1 % of the rows and of the items of a case, asserted here."""
import functools
import os
import subprocess
import sys
import types

import numpy as np
import pytest

from tests import cohort_model as CM
from tests import cohort_prior_cases as CC
from tests import cohort_prior_model as M
from tests.geno_sim import prior as sim
from tests.test_cohort_gpu import _load_matrix

pytestmark = pytest.mark.gpu

NO_CALL = 0xFF
E_ARG = -3                                         # svjg.h: SVJG_E_ARG
FLAG = 1 << 31
AMD = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "svjedi-graph_amd")
NAMES = ("gt", "pl", "raw", "genotyped", "boundary", "site", "gq", "af", "em_steps")


@pytest.fixture(scope="module")
def ctx():
    from svjg import capi
    c = capi.Context(0)
    yield c
    c.close()


def _prior(ctx, c, ms):
    return ctx.genotype_cohort_prior(c["t"], c["slot"], c["ok"], c["ploidy"], c["max_ploidy"], ms, CC.ERR)


def _independent(ctx, c, ms):
    """the call without the prior on the same inputs, gt as alt copies or 0xFF"""
    if c["ploidy"] is None:
        got = ctx.genotype_cohort(c["t"], c["slot"], c["ok"], ms, CC.ERR)
        return (np.where(got[0] == 3, NO_CALL, got[0]).astype(np.uint8),) + got[1:]
    return ctx.genotype_cohort_ploidy(c["t"], c["slot"], c["ok"], c["ploidy"], c["max_ploidy"], ms, CC.ERR)


def _check_against_model(c, got, want, ms):
    """-> the largest |f_device - f_model|, absolute and relative, over the rows that are compared"""
    gt, pl, raw, done, boundary, site, gq, af, steps = got
    keep = ~want["row_out"]
    left = want["item_out"] | want["row_out"][:, None]
    assert want["row_out"].mean() <= CC.CAP and left.mean() <= CC.CAP
    has = ~np.isnan(want["f_hi"])
    assert np.array_equal(np.isnan(af), ~has)
    assert np.array_equal((steps & ~np.uint32(FLAG))[keep], want["steps"][keep]) and np.array_equal(((steps & FLAG) != 0)[keep], want["flag"][keep])
    assert not steps[~has].any()
    on = keep & has
    diff = np.abs((af[on] - want["f_hi"][on]) - want["f_lo"][on])
    rel = diff / np.maximum(np.abs(want["f_hi"][on]), 1e-300)
    big = want["f_hi"][on] > 1e-6
    worst = (float(diff.max()) if on.any() else 0.0, float(rel[big].max()) if big.any() else 0.0)
    print("%s min_support %d: max |f - f_model| = %.3e absolute, %.3e relative (f > 1e-6), over %d rows; steps mean %.2f max %d; left out %d rows, %d items"
          % (c["name"], ms, worst[0], worst[1], int(on.sum()), float(want["steps"][has].mean()) if has.any() else 0.0, int(want["steps"].max()),
             int(want["row_out"].sum()), int(left.sum())))
    assert worst[0] <= sim.constants()[3]
    w_gt, w_gq = CC.with_support(want["gt"], want["gq"], c["t"], raw, ms)
    assert np.array_equal(gt[~left], w_gt[~left]) and np.array_equal(gq[~left], w_gq[~left])
    assert np.array_equal(gq == NO_CALL, gt == NO_CALL)
    assert np.array_equal(site, M.site_of(gt, c["ploidy"]))
    return worst


@pytest.mark.parametrize("name", [c[0] for c in CC.CASES])
def test_case_against_the_model(ctx, name):
    c = CC.inputs(name)
    want = CC.load_golden(name, c)
    _load_matrix(ctx, c["n_slots"], c["counts"], c["present"])
    done, raw = CC.gate(c)
    for ms in (3, 0):
        got = _prior(ctx, c, ms)
        assert got[1].shape == got[0].shape + (c["max_ploidy"] + 1,) and got[5].shape == (len(c["t"]), 3)
        assert np.array_equal(got[3], done) and np.array_equal(got[2], raw)
        _check_against_model(c, got, want, ms)
        # PL, raw, genotyped and boundary are the call's without the prior, array for array
        alone = _independent(ctx, c, ms)
        for k in (1, 2, 3, 4):
            assert np.array_equal(got[k], alone[k]), NAMES[k]
        # the same call again: equal bytes in every output (NaN included)
        again = _prior(ctx, c, ms)
        assert all(x.tobytes() == y.tobytes() for x, y in zip(got, again))
    # the planted rows
    gt, af, site = got[0], got[7], got[5]
    p, P = c["planted"], (np.full(done.shape, 2) if c["ploidy"] is None else c["ploidy"].astype(np.int64))
    part = done != 0
    for row, copies in ((p["hom_ref"], 0 * P), (p["hom_alt"], P)):
        assert np.array_equal(gt[row][part[row]], copies[row][part[row]].astype(np.uint8))
    if part[p["hom_ref"]].any():
        assert af[p["hom_ref"]] < 1e-3 and af[p["hom_alt"]] > 1 - 1e-3
    for row in (p["absent"], p["zero_reads"]):
        assert np.isnan(af[row]) and got[8][row] == 0 and (gt[row] == NO_CALL).all() and (got[6][row] == NO_CALL).all() and not site[row].any()
    assert not done[p["absent"]].any() and (c["ploidy"] is not None or done[p["zero_reads"]].all())
    carrier = c["S"] // 2
    if part[p["one_carrier"], carrier] and P[p["one_carrier"], carrier] == 2 and c["S"] > 1:
        others = part[p["one_carrier"]].copy()
        others[carrier] = False
        assert gt[p["one_carrier"], carrier] not in (0, NO_CALL) and not gt[p["one_carrier"]][others].any()


def test_the_prior_changes_calls(ctx):
    """a kernel that ignored f would pass nothing here: at least 20 items whose posterior GT is another one than the call without the prior (both
    from the device, the posterior one equal to the model's)"""
    n = 0
    for name in ("null_31", "mixed_31", "null_5"):
        c = CC.inputs(name)
        want = CC.load_golden(name, c)
        _load_matrix(ctx, c["n_slots"], c["counts"], c["present"])
        got, alone = _prior(ctx, c, 0), _independent(ctx, c, 0)
        left = want["item_out"] | want["row_out"][:, None]
        moved = (got[0] != alone[0]) & (got[0] != NO_CALL) & (alone[0] != NO_CALL) & ~left
        assert np.array_equal(got[0][moved], want["gt"][moved])
        n += int(moved.sum())
    print("the prior changes %d calls" % n)
    assert n >= 20


def test_one_sample_rows(ctx):
    """S = 1: a segment of one lane, 64 rows a wave; every row's f comes from its one sample (x / P at the fixed point), or there is none"""
    c = CC.inputs("null_1")
    _load_matrix(ctx, c["n_slots"], c["counts"], c["present"])
    gt, _, raw, done, _, site, gq, af, steps = _prior(ctx, c, 0)
    part = (done[:, 0] != 0) & (raw[:, 0].sum(axis=1) > 0)
    assert part.any() and not part.all() and np.array_equal(~np.isnan(af), part) and (steps[part] >= 1).all()
    assert ((af[part] >= 0) & (af[part] <= 1)).all()
    called = gt[:, 0] != NO_CALL
    assert np.array_equal(site, np.stack([called, 2 * called, np.where(called, gt[:, 0], 0)], axis=1).astype(np.uint32))


@pytest.mark.parametrize("name", ["null_65", "null_130", "mixed_130", "null_192", "mixed_193", "null_256", "mixed_257", "mixed_320", "deep_257"])
def test_further_items_staged_in_lds_or_recomputed(ctx, monkeypatch, name):
    """S > 64: a lane's items beyond its first are recomputed at every step or kept in LDS (SVJG_PRIOR_STAGE, tools/cohort_prior_timing.py
    measures the two): the same bytes either way.  Two staged items on every lane (192), the third on one lane and on all (193, 256), one and 64
    recomputed items behind three staged ones (257, 320), weights that underflow to 0 in both arms (deep_257)"""
    c = CC.inputs(name)
    _load_matrix(ctx, c["n_slots"], c["counts"], c["present"])
    got = {}
    for how in ("recompute", "lds"):
        monkeypatch.setenv("SVJG_PRIOR_STAGE", how)
        got[how] = _prior(ctx, c, 3)
    monkeypatch.delenv("SVJG_PRIOR_STAGE")
    assert all(x.tobytes() == y.tobytes() for x, y in zip(got["recompute"], got["lds"]))
    assert all(x.tobytes() == y.tobytes() for x, y in zip(got["lds"], _prior(ctx, c, 3)))


def test_chunks_equal_one_call(ctx):
    from svjg import genotype
    for name in ("null_33", "mixed_5", "null_9", "mixed_257"):            # (at 9 samples a wave holds 4 rows: chunks of 97 end inside a wave)
        c = CC.inputs(name)
        _load_matrix(ctx, c["n_slots"], c["counts"], c["present"])
        rows = types.SimpleNamespace(sv_type=c["t"], slot=c["slot"], ok=c["ok"])
        one = genotype.genotype_cohort_rows(ctx, rows, c["S"], 3, CC.ERR, c["ploidy"], True)
        parts = genotype.genotype_cohort_rows(ctx, rows, c["S"], 3, CC.ERR, c["ploidy"], True, step=97)
        assert len(one) == 8 and all(x.tobytes() == y.tobytes() and x.shape == y.shape for x, y in zip(one, parts))


def _equal_bytes_in_every_copy(got, one, K):
    """got[K * R, ...] holds K times the bytes of one[R, ...] (NaN included)"""
    u = "u%d" % one.dtype.itemsize
    return got.shape == (K * one.shape[0],) + one.shape[1:] and np.array_equal(got.view(u).reshape(K, -1), np.broadcast_to(one.view(u).reshape(1, -1), (K, one.size)))


@functools.lru_cache(maxsize=None)
def _compute_units():
    """the device's compute units as the library's launch cap counts them, else 256.  Asked of torch in a child process, once: torch brings a HIP
    runtime of its own, and a second runtime in this process is what tests/test_context_teardown_gpu.py would then measure the free memory with"""
    p = subprocess.run([sys.executable, "-c", "import torch; print(torch.cuda.get_device_properties(0).multi_processor_count)"], capture_output=True, text=True)
    last = p.stdout.split()[-1:] if p.returncode == 0 else []
    return int(last[0]) if last and last[0].isdigit() and int(last[0]) > 0 else 256


@pytest.mark.parametrize("name", ["mixed_33", "null_3", "mixed_257"])
def test_more_rows_than_one_trip_of_the_grid(ctx, name):
    """The launch is capped at 8 blocks of 4 waves a compute unit: a case's rows, repeated until the call has more waves than that plus a partial
    last trip (row i of copy k has the type, slot, ok and ploidy of row i), so that waves take the grid-stride loop a second time and set up
    `it`, `sum_p` and `row` again.  Every output of every copy has the bytes of the one-trip call on the case itself, which
    test_case_against_the_model holds to the model.  One row a wave (mixed_33), 16 rows a wave (null_3), staged and recomputed items on the
    second trip (mixed_257).  (A trip's rows are no multiple of a case's rows on 256 or 304 units: a wave's second row is another one than its first.)"""
    cus = _compute_units()
    c = CC.inputs(name)
    R, per_wave = len(c["t"]), 64 // sim.width(c["S"])
    trip = 32 * cus                                                # waves
    K = -(-(trip + trip // 8) * per_wave // R)
    waves = -(-K * R // per_wave)
    assert waves > 32 * cus and waves % trip != 0
    _load_matrix(ctx, c["n_slots"], c["counts"], c["present"])
    one = _prior(ctx, c, 3)
    assert R <= trip * per_wave and np.array_equal(one[5], M.site_of(one[0], c["ploidy"]))
    many = dict(c, t=np.tile(c["t"], K), slot=np.tile(c["slot"], K), ok=np.tile(c["ok"], K), ploidy=None if c["ploidy"] is None else np.tile(c["ploidy"], (K, 1)))
    got = _prior(ctx, many, 3)
    for k in range(9):
        assert _equal_bytes_in_every_copy(got[k], one[k], K), NAMES[k]
    assert np.array_equal(got[5], M.site_of(got[0], many["ploidy"]))


def test_empty_and_bad_calls(ctx):
    from svjg import capi
    c = CC.inputs("mixed_3")
    t, slot, ok, ploidy = c["t"][:20], c["slot"][:20], c["ok"][:20], c["ploidy"][:20]
    fresh = capi.Context(0)
    try:
        with pytest.raises(capi.SvjgError) as ei:                  # no matrix
            fresh.genotype_cohort_prior(t, slot, ok, None, 2, 3, 5e-5)
        assert "no cohort matrix" in str(ei.value)
    finally:
        fresh.close()
    _load_matrix(ctx, c["n_slots"], c["counts"], c["present"])
    out = ctx.genotype_cohort_prior(t[:0], slot[:0], ok[:0], None, 2, 3, 5e-5)
    assert [x.shape for x in out] == [(0, 3), (0, 3, 3), (0, 3, 2), (0, 3), (0, 3), (0, 3), (0, 3), (0,), (0,)]
    for mp in (0, 9, 255):
        with pytest.raises(capi.SvjgError) as ei:
            ctx.genotype_cohort_prior(t, slot, ok, np.minimum(ploidy, 1), mp, 3, 5e-5)
        assert "max_ploidy" in str(ei.value)
    for mp in (1, 3, 8):                                           # without a ploidy array the call is diploid
        with pytest.raises(capi.SvjgError) as ei:
            ctx.genotype_cohort_prior(t, slot, ok, None, mp, 3, 5e-5)
        assert "max_ploidy must be 2" in str(ei.value)
    with pytest.raises(capi.SvjgError) as ei:
        ctx.genotype_cohort_prior(t, slot, ok, ploidy, int(ploidy.max()) - 1, 3, 5e-5)
    assert "ploidy above max_ploidy" in str(ei.value)
    buf = np.zeros(20 * 3 * 9, np.int64)
    ptrs = [t.ctypes.data, slot.ctypes.data, ok.ctypes.data, ploidy.ctypes.data]
    outs = [buf.ctypes.data] * 9
    lib = ctx.lib
    for k in range(3):
        a = list(ptrs)
        a[k] = None
        assert lib.svjg_genotype_cohort_prior(ctx.h, *a, 8, 20, 3, 5e-5, *outs) == E_ARG
    for k in range(9):
        o = list(outs)
        o[k] = None
        assert lib.svjg_genotype_cohort_prior(ctx.h, *ptrs, 8, 20, 3, 5e-5, *o) == E_ARG
    assert lib.svjg_genotype_cohort_prior(ctx.h, *ptrs, 8, (1 << 40) // 3 + 1, 3, 5e-5, *outs) == E_ARG
    assert b"too many items" in lib.svjg_last_error(ctx.h)
    assert lib.svjg_genotype_cohort_prior(None, *ptrs, 8, 20, 3, 5e-5, *outs) == E_ARG
    bad = slot.copy()
    bad[7] = c["n_slots"]                                          # reported after the pass, as svjg_genotype reports it
    with pytest.raises(capi.SvjgError) as ei:
        ctx.genotype_cohort_prior(t, bad, ok, ploidy, 8, 3, 5e-5)
    assert "slot out of range" in str(ei.value)
    got = ctx.genotype_cohort_prior(t, slot, ok, ploidy, 8, 3, 5e-5)    # the context works afterwards
    assert np.array_equal(got[5], M.site_of(got[0], ploidy))


def test_table_growth_runs_both_kernels_again():
    """a FRESH context (the log10(i!) table has its first size) and one item of ref = alt = 70 000: both kernels run again behind the table's
    growth; the outputs are those of a context whose table was large from the start"""
    from svjg import capi
    c = CC.inputs("null_4")
    r = c["planted"]["one_carrier"]
    c["counts"][c["slot"][r], 1] = (70_000, 70_000)
    out = []
    for reserve in (False, True):
        x = capi.Context(0)
        try:
            if reserve:
                x.logfact_reserve(200_000)
            _load_matrix(x, c["n_slots"], c["counts"], c["present"])
            out.append(_prior(x, c, 3))
        finally:
            x.close()
    assert out[0][2][r, 1].tolist() == [70_000, 70_000] and out[0][0][r, 1] == 1
    assert all(a.tobytes() == b.tobytes() for a, b in zip(*out))
    assert np.array_equal(out[0][5], M.site_of(out[0][0], None))


# ---- the drop-in script ----

def _run(tmp_path, name, *args):
    out = str(tmp_path / f"{name}.vcf")
    p = subprocess.run([sys.executable, f"{AMD}/predict-genotype.py", *args, "--minsupport", "3", "-o", out], capture_output=True, text=True)
    return p, out


def _data(path):
    return [ln.split("\t") for ln in open(path).read().split("\n") if ln and not ln.startswith("#")]


@pytest.mark.parametrize("which", ["plain", "edited"])
def test_script(golden, tmp_path, which):
    """--cohort LIST --cohort-prior (and, on the edited list, an all-diploid --cohort-ploidy file): the file written from the model's arrays and
    the reference-made PLs by the same writer; DP / AD / PL as the run without --cohort-prior"""
    from svjg import genotype
    co = CM.Cohort(golden, which)
    extra, ploidy = [], None
    if which == "edited":
        f = tmp_path / "two.tsv"
        f.write_text("".join("*\t%s\t2\n" % c for c in sorted(set(co.rows.chrom))))
        extra, ploidy = ["--cohort-ploidy", str(f)], np.full(co.done.shape, 2, np.uint8)
    m = M.run(co.rows.sv_type, co.raw, co.done, ploidy, 5e-5, 3)
    assert (np.abs(m["ratio"] - 1) > 1e-3)[~np.isnan(m["ratio"])].all()
    part = ~np.isnan(m["gap"])
    assert (m["gq_margin"][part] > 1e-3).all() and (m["gap"][part] > 1e-6).all()    # nothing of these fixtures sits near a decision
    want = str(tmp_path / "want.vcf")
    steps = m["steps"] | np.where(m["flag"], np.uint32(FLAG), np.uint32(0))
    genotype.write_vcf_cohort(want, co.rows, co.names, genotype.CohortCalls(m["gt"], co.pl, co.raw, co.done, M.site_of(m["gt"], ploidy), m["gq"], m["f_hi"], steps), ploidy)
    p, out = _run(tmp_path, which, "--cohort", co.list, "--cohort-prior", *extra, "-v", co.vcf)
    assert p.returncode == 0, p.stderr
    assert open(out).read() == open(want).read()
    assert p.stdout == "".join("Genotyped svs (%s): %d\n" % (n, k) for n, k in zip(co.names, co.genotyped))
    q, plain = _run(tmp_path, which + "_plain", "--cohort", co.list, *extra, "-v", co.vcf)
    assert q.returncode == 0, q.stderr
    a, b = _data(out), _data(plain)
    assert len(a) == len(b) and all(x[8] == "GT:DP:AD:PL:GQ" and y[8] == "GT:DP:AD:PL" for x, y in zip(a, b))
    assert [[col.split(":")[1:4] for col in x[9:]] for x in a] == [[col.split(":")[1:4] for col in y[9:]] for y in b]
    assert any("EMAF=" in x[7] for x in a) and any(col.split(":")[4] != "." for x in a for col in x[9:])
