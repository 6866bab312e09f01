"""The cohort site quality on the GPU (svjg_cohort_qual, k_cohort_qual) against the 60-digit model of tests/cohort_qual_model.py, whose answers
for the cases of tests/cohort_qual_cases.py are stored under tests/golden/cohort_qual/: 300 rows x S diploid samples with M + 1 on both sides of
64 and 128, 300 rows x S at ploidies 0..8 mixed within rows, deep counts, 20 rows x 600 shallow samples, 2 rows x 2 048 samples (M = the call's
limit); the shapes that max_ploidy and the ploidy array decide (the chrX / chrY pattern under max_ploidy 2, haploid under max_ploidy 1, ploidies
0..P under max_ploidy P = 3..7, 128 samples at 0..8, the shallow regime at mixed ploidy, haploid and at 512 samples of ploidy 8, the steepest
shrink per step), one array under every max_ploidy; chunked calls, calls of more rows than one trip of the grid, the rows that only the cohort
decides, the argument errors, the script.
Needs an MI355X: run with -m gpu.

What may be left out of a comparison is decided by the model alone, before any device ran (tests/golden/make_cohort_qual.py): mlac on rows whose
two largest phi_k y_k lie within a relative 1e-9 of each other, the script's text on rows whose 100 SVQ lies within 1e-6 of a half-integer; at most
1 % of a case's rows, asserted here."""
import os
import subprocess
import sys
import types

import numpy as np
import pytest

from tests import cohort_model as CM
from tests import cohort_prior_model as PM
from tests import cohort_qual_cases as QC
from tests import cohort_qual_model as M
from tests.geno_sim import qual as sim
from tests.test_cohort_gpu import _load_matrix
from tests.test_cohort_prior_gpu import _compute_units, _equal_bytes_in_every_copy

pytestmark = pytest.mark.gpu

E_ARG = -3                                         # svjg.h: SVJG_E_ARG
NONE = 0xFFFFFFFF
AMD = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "svjedi-graph_amd")
NAMES = ("qual", "mlac", "chroms")


@pytest.fixture(scope="module")
def ctx():
    from svjg import capi
    c = capi.Context(0)
    yield c
    c.close()


def _qual(ctx, c, theta=QC.THETA):
    return ctx.cohort_qual(c["t"], c["slot"], c["ok"], c["ploidy"], c["max_ploidy"], QC.ERR, theta)


def _check_against_model(name, want, got, rows=None):
    """chroms equal, the NaN pattern equal, mlac equal outside the margin, |qual - model| <= QUAL_ABS + QUAL_REL model -> the largest difference
    among the rows with model < 1, the largest relative one among the others"""
    q, ml, ch = got
    sel = np.ones(len(q), bool) if rows is None else rows
    assert want["mlac_out"].mean() <= QC.CAP and want["text_out"].mean() <= QC.CAP
    assert q.dtype == np.float64 and ml.dtype == np.uint32 and ch.dtype == np.uint32
    assert np.array_equal(ch[sel], want["chroms"][sel])
    has = ~np.isnan(want["qual"])
    assert np.array_equal(np.isnan(q[sel]), ~has[sel]) and not ml[sel & ~has].any()
    on = sel & ~want["mlac_out"]
    assert np.array_equal(ml[on], want["mlac"][on])
    at = sel & has
    d, m = np.abs((q[at] - want["qual"][at]) - want["qual_lo"][at]), want["qual"][at]
    worst = (float(d[m < 1].max()) if (m < 1).any() else 0.0, float((d[m >= 1] / m[m >= 1]).max()) if (m >= 1).any() else 0.0)
    print("%s: max |qual - model| = %.3e absolute (model < 1), %.3e relative (model >= 1), over %d rows; left out: mlac %d"
          % (name, worst[0], worst[1], int(at.sum()), int(want["mlac_out"].sum())))
    k = sim.constants()
    assert (d <= k["abs"] + k["rel"] * m).all()
    assert not np.signbit(q[at]).any()
    return worst


@pytest.mark.parametrize("name", [c[0] for c in QC.CASES])
def test_case_against_the_model(ctx, name):
    c = QC.inputs(name)
    want = QC.load_golden(name, c)
    _load_matrix(ctx, c["n_slots"], c["counts"], c["present"])
    got = _qual(ctx, c)
    assert all(x.shape == (len(c["t"]),) for x in got)
    _check_against_model(name, want, got)
    again = _qual(ctx, c)                                          # the same call again: equal bytes in every output (NaN included)
    assert all(x.tobytes() == y.tobytes() for x, y in zip(got, again))
    done, raw = QC.gate(c)
    QC.check_planted(c, done, raw, *got)
    if name == "het_2048":
        assert (got[2] == sim.constants()["max_chroms"]).all() and np.array_equal(got[1], got[2] // 2)
    if name == "shallow_600":
        assert (got[1][:10] == 0).all() and (got[0][:10] < 0.1).all()
    if name == "shallow_poly_512":                                 # the call's limit at max_ploidy 8: the request beyond 64 KiB of LDS, with every entry in use
        assert (got[2] == 4096).all() and c["S"] * c["max_ploidy"] == sim.constants()["max_chroms"]
    if name == "steep_64":                                         # row 1 is row 0 in reverse sample order: the model does not know the order
        k = sim.constants()
        assert got[1][0] == got[1][1] == 256 and abs(got[0][0] - got[0][1]) <= k["abs"] + k["rel"] * want["qual"][0]


@pytest.mark.parametrize("name", ["sex_65", "hap_65", "mixed_m3_20", "mixed_m5_20", "shallow_sex_300"])
def test_one_array_under_every_max_ploidy(ctx, name):
    """tests/test_cohort_qual.py's test of the same name, on the device: one ploidy array called at every max_ploidy from the array's largest value
    to 8.  max_ploidy sizes the two rows in LDS, the harmonic table and the launch, and sets the rescaling's cadence; every call is within the
    bound of the model, and has the bytes of the call at the case's own max_ploidy (a rescaling multiplies by an exact power of two, so when it
    happens changes no bit until something underflows; the host harness has equal bytes on every one of these cases)"""
    from tests.test_cohort_qual import UNDER, max_ploidies_of
    assert name in UNDER                                           # equal bytes are asserted there
    c = QC.inputs(name)
    want = QC.load_golden(name, c)
    _load_matrix(ctx, c["n_slots"], c["counts"], c["present"])
    own = _qual(ctx, c)
    _check_against_model(name, want, own)
    wider = max_ploidies_of(c)[1:]
    assert wider[-1] == 8 and len(wider) == 8 - c["max_ploidy"]
    for mp in wider:
        got = _qual(ctx, dict(c, max_ploidy=mp))
        _check_against_model("%s at max_ploidy %d" % (name, mp), want, got)
        assert all(x.tobytes() == y.tobytes() for x, y in zip(own, got)), (name, mp)


def test_chunks_equal_one_call(ctx):
    from svjg import genotype
    for name in ("null_33", "mixed_9", "null_65", "sex_65", "hap_129", "mixed_m3_20"):
        c = QC.inputs(name)
        _load_matrix(ctx, c["n_slots"], c["counts"], c["present"])
        rows = types.SimpleNamespace(sv_type=c["t"], slot=c["slot"], ok=c["ok"])
        seen = []                                                   # the max_ploidy of every call: the array's largest value (2, 1 and 3 for the last three)
        spy = types.SimpleNamespace(cohort_qual=lambda t, slot, ok, ploidy, mp, *rest: seen.append(mp) or ctx.cohort_qual(t, slot, ok, ploidy, mp, *rest))
        one = genotype.cohort_qual_rows(spy, rows, c["S"], c["ploidy"], QC.ERR)
        parts = genotype.cohort_qual_rows(spy, rows, c["S"], c["ploidy"], QC.ERR, step=97)
        assert len(seen) == 1 + -(-len(c["t"]) // 97) and set(seen) == {c["max_ploidy"]}
        assert len(one) == 3 and all(x.tobytes() == y.tobytes() and x.shape == y.shape for x, y in zip(one, parts))
        assert all(x.tobytes() == y.tobytes() for x, y in zip(one, _qual(ctx, c)))


@pytest.mark.parametrize("name", ["null_33", "mixed_9", "shallow_600", "sex_65", "hap_129", "mixed_m3_20"])
def test_more_rows_than_one_trip_of_the_grid(ctx, name):
    """The launch is capped at what a compute unit holds of one-wave blocks (16 by registers, fewer where the rows' LDS decides): a case's rows,
    repeated until the call has more rows than that plus a partial last trip, so that blocks take the grid-stride loop a second time and set up y,
    M, E and D_0 again.  Every output of every copy has the bytes of the one-trip call on the case itself, which test_case_against_the_model holds
    to the model."""
    cus = _compute_units()
    c = QC.inputs(name)
    R = len(c["t"])
    per_cu = min(16, 163840 // (16 * (c["S"] * c["max_ploidy"] + 1) + 720))
    trip = cus * per_cu
    K = -(-(trip + trip // 8) // R)
    assert K * R > trip and R <= trip
    _load_matrix(ctx, c["n_slots"], c["counts"], c["present"])
    one = _qual(ctx, c)
    many = dict(c, t=np.tile(c["t"], K), slot=np.tile(c["slot"], K), ok=np.tile(c["ok"], K), ploidy=None if c["ploidy"] is None else np.tile(c["ploidy"], (K, 1)))
    got = _qual(ctx, many)
    for k in range(3):
        assert _equal_bytes_in_every_copy(got[k], one[k], K), NAMES[k]


def test_the_cohort_decides(ctx):
    """a kernel that looked at calls instead of likelihoods passes nothing here: at least 10 rows where every sample is a no-call at min_support 3
    (NS = AC = 0 from svjg_genotype_cohort) and yet SVQ > 30, equal to the model"""
    n = 0
    for name in ["null_%d" % S for S in QC.NULL_SIZES]:
        c = QC.inputs(name)
        want = QC.load_golden(name, c)
        _load_matrix(ctx, c["n_slots"], c["counts"], c["present"])
        gt, _, _, _, _, site = ctx.genotype_cohort(c["t"], c["slot"], c["ok"], 3, QC.ERR)
        got = _qual(ctx, c)
        silent = (gt == 3).all(axis=1) & ~site.any(axis=1) & (got[0] > 30)
        assert all(silent[c["planted"][w]] for w in QC.WHISPER) or c["S"] == 1
        if silent.any():
            _check_against_model(name + " (no sample is called)", want, got, silent)
            assert (want["qual"][silent] > 30).all() and (got[1][silent] > 0).all()
        n += int(silent.sum())
    print("%d rows without a single call and SVQ > 30" % n)
    assert n >= 10


def test_theta_is_the_prior(ctx):
    """a larger theta leaves chroms alone and raises the quality of a row with alt reads (its prior odds of k > 0 grow)"""
    c = QC.inputs("null_31")
    _load_matrix(ctx, c["n_slots"], c["counts"], c["present"])
    a, b = _qual(ctx, c, 1e-3), _qual(ctx, c, 0.05)
    has = ~np.isnan(a[0])
    assert np.array_equal(a[2], b[2]) and (b[0][has] >= a[0][has]).all() and (b[0][has] > a[0][has]).any()
    done, raw = QC.gate(c)
    rows = [c["planted"]["whisper_0"], c["planted"]["hom_ref"]]
    m = M.run(c["t"], raw, done, None, QC.ERR, 0.05, rows=rows)
    k = sim.constants()
    for r in rows:
        assert abs((b[0][r] - m["qual"][r]) - m["qual_lo"][r]) <= k["abs"] + k["rel"] * m["qual"][r] and b[1][r] == m["mlac"][r]


def test_empty_and_bad_calls(ctx):
    from svjg import capi
    c = QC.inputs("mixed_3")
    t, slot, ok, ploidy = c["t"][:20], c["slot"][:20], c["ok"][:20], c["ploidy"][:20]
    fresh = capi.Context(0)
    try:
        with pytest.raises(capi.SvjgError) as ei:                  # no matrix
            fresh.cohort_qual(t, slot, ok, None, 2, 5e-5)
        assert "no cohort matrix" in str(ei.value)
    finally:
        fresh.close()
    _load_matrix(ctx, c["n_slots"], c["counts"], c["present"])
    out = ctx.cohort_qual(t[:0], slot[:0], ok[:0], None, 2, 5e-5)
    assert [x.shape for x in out] == [(0,), (0,), (0,)]
    for mp in (0, 9, 255):
        with pytest.raises(capi.SvjgError) as ei:
            ctx.cohort_qual(t, slot, ok, np.minimum(ploidy, 1), mp, 5e-5)
        assert "max_ploidy" in str(ei.value)
    for mp in (1, 3, 8):                                           # without a ploidy array the call is diploid
        with pytest.raises(capi.SvjgError) as ei:
            ctx.cohort_qual(t, slot, ok, None, mp, 5e-5)
        assert "max_ploidy must be 2" in str(ei.value)
    with pytest.raises(capi.SvjgError) as ei:
        ctx.cohort_qual(t, slot, ok, ploidy, int(ploidy.max()) - 1, 5e-5)
    assert "ploidy above max_ploidy" in str(ei.value)
    for theta in (0.0, -1e-3, 0.0500001, 1.0, float("nan"), float("inf")):
        with pytest.raises(capi.SvjgError) as ei:
            ctx.cohort_qual(t, slot, ok, ploidy, 8, 5e-5, theta)
        assert "theta is not in (0, 0.05]" in str(ei.value)
    ctx.cohort_qual(t, slot, ok, ploidy, 8, 5e-5, 0.05)            # the range's end is inside
    buf = np.zeros(64, np.float64)
    ptrs = [t.ctypes.data, slot.ctypes.data, ok.ctypes.data, ploidy.ctypes.data]
    outs = [buf.ctypes.data] * 3
    lib = ctx.lib
    for k in range(3):
        a = list(ptrs)
        a[k] = None
        assert lib.svjg_cohort_qual(ctx.h, *a, 8, 20, 5e-5, 1e-3, *outs) == E_ARG and b"a null array" in lib.svjg_last_error(ctx.h)
    for k in range(3):
        o = list(outs)
        o[k] = None
        assert lib.svjg_cohort_qual(ctx.h, *ptrs, 8, 20, 5e-5, 1e-3, *o) == E_ARG and b"a null array" in lib.svjg_last_error(ctx.h)
    assert lib.svjg_cohort_qual(ctx.h, *ptrs, 8, (1 << 40) // 3 + 1, 5e-5, 1e-3, *outs) == E_ARG
    assert b"too many items" in lib.svjg_last_error(ctx.h)
    assert lib.svjg_cohort_qual(None, *ptrs, 8, 20, 5e-5, 1e-3, *outs) == E_ARG
    bad = slot.copy()
    bad[7] = c["n_slots"]                                          # reported after the pass, as svjg_genotype reports it
    with pytest.raises(capi.SvjgError) as ei:
        ctx.cohort_qual(t, bad, ok, ploidy, 8, 5e-5)
    assert "slot out of range" in str(ei.value)
    # the context works afterwards
    want = QC.load_golden("mixed_3", c)
    got = _qual(ctx, c)
    _check_against_model("mixed_3 behind the bad calls", want, got)


def test_too_many_chromosomes_are_refused_before_launch(ctx):
    """2 049 diploid samples: M_max = 4 098 > SVJG_QUAL_MAX_CHROMS; 513 samples at max_ploidy 8 likewise; the message names the limit"""
    from svjg import capi
    t, slot, ok = np.zeros(3, np.uint8), np.array([0, 1, NONE], np.uint32), np.ones(3, np.uint8)
    for S, ploidy, mp in ((2049, None, 2), (513, np.ones((3, 513), np.uint8), 8)):
        ctx.cohort_alloc(S, 4)
        ctx.cohort_set_counts(0, np.array([0, 1], np.uint32), np.array([[3, 9], [8, 0]], np.uint32))
        with pytest.raises(capi.SvjgError) as ei:
            ctx.cohort_qual(t, slot, ok, ploidy, mp, 5e-5)
        assert "SVJG_QUAL_MAX_CHROMS = 4096" in str(ei.value)
    # one sample fewer at max_ploidy 8 is a call: 512 x 8 = 4 096; only sample 0 has reads, at ploidy 1
    ctx.cohort_alloc(512, 4)
    ctx.cohort_set_counts(0, np.array([0, 1], np.uint32), np.array([[3, 9], [8, 0]], np.uint32))
    q, ml, ch = ctx.cohort_qual(t, slot, ok, np.ones((3, 512), np.uint8), 8, 5e-5)
    assert ch.tolist() == [1, 1, 0] and ml.tolist() == [1, 0, 0] and q[0] > 30 and q[1] < 1 and np.isnan(q[2])


# ---- the drop-in script ----

def _run(tmp_path, name, *args):
    out = str(tmp_path / f"{name}.vcf")
    p = subprocess.run([sys.executable, f"{AMD}/predict-genotype.py", *args, "--minsupport", "3", "-o", out], capture_output=True, text=True)
    return p, out


def _lines(path):
    return open(path).read().split("\n")


def _presence(co):
    """done[n, S], raw[n, S, 2] as the gate leaves them for the fixtures: a row with ok & 1 and a slot, a sample that has the row's key"""
    n, S = len(co.rows.slot), len(co.names)
    done, raw = np.zeros((n, S), np.uint8), np.zeros((n, S, 2), np.uint32)
    for r in range(n):
        if (int(co.rows.ok[r]) & 1) and int(co.rows.slot[r]) != NONE:
            key = co.keys[int(co.rows.slot[r])]
            for s in range(S):
                if key in co.jsons[s]:
                    done[r, s] = 1
                    raw[r, s] = [len(co.jsons[s][key][0]), len(co.jsons[s][key][1])]
    return done, raw


def _without_quality(line):
    f = line.split("\t")
    if len(f) > 7 and not line.startswith("#"):
        f[7] = ";".join(x for x in f[7].split(";") if x.split("=", 1)[0] not in ("SVQ", "MLAC", "MLAF"))
    return "\t".join(f)


PLOIDY_LINES = [("S1", "2\t1"), ("S2", "2\t1"), ("S3", "1\t30000\t40000\t0"), ("S4", "1\t3"), ("*", "2\t2")]   # tests/test_cohort_ploidy_gpu.py's mixed file


def _ploidy_of_lines(co):
    """the ploidy matrix that PLOIDY_LINES say, by hand: a sample's own lines and the `*` lines in file order, the first that matches the row's
    CHROM (and POS, for a region line) wins, 2 without one"""
    out = np.full((len(co.rows.chrom), len(co.names)), 2, np.uint8)
    for s, name in enumerate(co.names):
        for r, (chrom, pos) in enumerate(zip(co.rows.chrom, co.rows.pos)):
            for who, rest in PLOIDY_LINES:
                f = rest.split("\t")
                if who in (name, "*") and f[0] == chrom and (len(f) == 2 or int(f[1]) <= int(pos) <= int(f[2])):
                    out[r, s] = int(f[-1])
                    break
    return out


def _quality_tags(line):
    return [x for x in line.split("\t")[7].split(";") if x.split("=", 1)[0] in ("SVQ", "MLAC", "MLAF")]


def _script_with_a_ploidy_file(co, tmp_path):
    """--cohort LIST --cohort-ploidy FILE --cohort-qual: the three tags of every row are what the writer prints from the model's answer on the
    file's ploidy matrix (S1 and S2 haploid on contig 2, S3 at ploidy 0 on 1:30000-40000, S4 triploid on contig 1); every other byte is the run
    without --cohort-qual; --cohort-theta changes the three tags only"""
    from svjg import genotype
    ploidy = _ploidy_of_lines(co)
    assert sorted(np.unique(ploidy).tolist()) == [0, 1, 2, 3] and (ploidy[:, 2] == 0).sum() == 6 and ploidy.max() == 3
    done, raw = _presence(co)
    done = done & (ploidy != 0)
    raw = np.where(done[:, :, None] != 0, raw, 0).astype(np.uint32)
    f = tmp_path / "mixed.tsv"
    f.write_text("# SAMPLE CHROM [FROM TO] PLOIDY\n" + "".join("%s\t%s\n" % x for x in PLOIDY_LINES))
    base = ["--cohort", co.list, "--cohort-ploidy", str(f)]
    lines = {}
    for tag, theta in (("qual", 1e-3), ("theta", 0.05)):
        m = M.run(co.rows.sv_type, raw, done, ploidy, 5e-5, theta)
        has = ~np.isnan(m["qual"])
        band = has & (m["half"] < QC.HALF_BAND)                      # the model alone decides what is left out
        assert has.sum() >= 5 and band.mean() <= QC.CAP
        assert (m["chroms"][has] != 2 * ((done != 0) & (raw.sum(axis=2) > 0)).sum(axis=1)[has]).any()        # the ploidies are in the answer
        p, out = _run(tmp_path, tag, *base, "--cohort-qual", *(["--cohort-theta", "0.05"] if tag == "theta" else []), "-v", co.vcf)
        assert p.returncode == 0, p.stderr
        a = lines[tag] = _lines(out)
        data = [ln for ln in a if ln and not ln.startswith("#")]
        assert len(data) == len(has)
        for v, ln in enumerate(data):
            want = _quality_tags("\t" * 7 + genotype.cohort_info(".", 0, 0, qual=(m["qual"][v], m["mlac"][v], m["chroms"][v])))
            got = _quality_tags(ln)
            if band[v]:
                want, got = ([x for x in tags if not x.startswith("SVQ=")] for tags in (want, got))
            info = ln.split("\t")[7].split(";")
            assert got == want and info[len(info) - len(got):] == got, (tag, v, got, want)
        assert sum("SVQ=" in ln for ln in data) == int(has.sum()) and sum("MLAC=" in ln for ln in data) == int((m["chroms"] > 0).sum())
    q, plain = _run(tmp_path, "plain", *base, "-v", co.vcf)
    assert q.returncode == 0, q.stderr
    for tag in lines:
        assert [_without_quality(x) for x in lines[tag] if not x.startswith("##INFO=<ID=SVQ") and not x.startswith("##INFO=<ID=MLA")] == _lines(plain)
        assert genotype.COHORT_QUAL_INFO_LINES in "\n".join(lines[tag])
    assert lines["qual"] != lines["theta"] and p.stdout == q.stdout


@pytest.mark.parametrize("prior", [False, True, "ploidy"])
def test_script(golden, tmp_path, prior):
    """--cohort LIST --cohort-qual, alone, with --cohort-prior and with --cohort-ploidy FILE: the file the writer makes from the model's arrays;
    every sample column and every other INFO tag as in the run without the flag; and that run is byte for byte what it was before the flag
    existed (with the ploidy file: _script_with_a_ploidy_file)"""
    from svjg import genotype
    co = CM.Cohort(golden, "plain")
    if prior == "ploidy":
        return _script_with_a_ploidy_file(co, tmp_path)
    done, raw = _presence(co)
    m = M.run(co.rows.sv_type, raw, done, None, 5e-5, 1e-3)
    has = ~np.isnan(m["qual"])
    assert has.sum() >= 5 and (m["gap"][has] > 1e-6).all()
    band = has & (m["half"] < QC.HALF_BAND)
    assert band.mean() <= QC.CAP
    qual = (m["qual"], m["mlac"], m["chroms"])
    want = str(tmp_path / "want.vcf")
    extra = []
    if prior:
        pm = PM.run(co.rows.sv_type, co.raw, co.done, None, 5e-5, 3)
        steps = pm["steps"] | np.where(pm["flag"], np.uint32(1 << 31), np.uint32(0))
        genotype.write_vcf_cohort(want, co.rows, co.names, genotype.CohortCalls(pm["gt"], co.pl, co.raw, co.done, PM.site_of(pm["gt"], None), pm["gq"], pm["f_hi"], steps), qual=qual)
        extra = ["--cohort-prior"]
    else:
        genotype.write_vcf_cohort(want, co.rows, co.names, genotype.CohortCalls(co.gt, co.pl, co.raw, co.done, co.site), qual=qual)
    p, out = _run(tmp_path, "qual", "--cohort", co.list, "--cohort-qual", *extra, "-v", co.vcf)
    assert p.returncode == 0, p.stderr
    a, b = _lines(out), _lines(want)
    data = [i for i, ln in enumerate(b) if ln and not ln.startswith("#")]
    assert len(a) == len(b) and len(data) == len(has)
    for v, i in enumerate(data):
        if band[v]:                                                 # the text of a value next to a rounding boundary is the model's to leave out
            a[i], b[i] = (";".join(x for x in ln.split(";") if not x.startswith("SVQ=")) for ln in (a[i], b[i]))
    assert a == b
    assert p.stdout == "".join("Genotyped svs (%s): %d\n" % (n, k) for n, k in zip(co.names, co.genotyped))
    assert sum("SVQ=" in ln for ln in a) == int(has.sum()) and any("MLAC=" in ln for ln in a)
    # --cohort-theta reaches the library
    t, out_t = _run(tmp_path, "theta", "--cohort", co.list, "--cohort-qual", "--cohort-theta", "0.05", *extra, "-v", co.vcf)
    assert t.returncode == 0 and _lines(out_t) != a and [_without_quality(x) for x in _lines(out_t)] == [_without_quality(x) for x in a]
    # without the flag: every other byte, and the file the parent wrote
    q, plain = _run(tmp_path, "plain", "--cohort", co.list, *extra, "-v", co.vcf)
    assert q.returncode == 0, q.stderr
    c = _lines(plain)
    assert [_without_quality(x) for x in a if not x.startswith("##INFO=<ID=SVQ") and not x.startswith("##INFO=<ID=MLA")] == c
    before = str(tmp_path / "before.vcf")
    if prior:
        genotype.write_vcf_cohort(before, co.rows, co.names, genotype.CohortCalls(pm["gt"], co.pl, co.raw, co.done, PM.site_of(pm["gt"], None), pm["gq"], pm["f_hi"], steps))
    else:
        co.assemble(before)
    assert c == _lines(before)
