"""The cohort call with an allele-frequency prior without a GPU: the per-item routines of svjg_geno.h and a sequential row EM compiled with g++
(tests/geno_sim) against the 60-digit model (tests/cohort_prior_model.py), the stored answers of the model
(tests/golden/cohort_prior/) against the model itself on a sample of rows, the block's layout, the writer's text over tests/golden/cohort/, the
driver's joining of chunks, and the script's argument errors."""
import os
import subprocess
import sys
import types

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests import cohort_model as CM                  # noqa: E402
from tests import cohort_prior_cases as CC            # noqa: E402
from tests import cohort_prior_model as M             # noqa: E402
from tests.geno_sim import prior as sim              # noqa: E402

AMD = os.path.join(ROOT, "svjedi-graph_amd")
NO_CALL = 0xFF
FLAG = 1 << 31
# the host harness against the model: the harness's exp10 is glibc's pow (below one ulp), its sums run over at most 320 terms
SIM_F_BOUND = 2e-14


# ---- the per-item routines and the row EM, compiled with g++, against the model ----

def test_constants_are_the_models():
    tol, max_it, flag, bound = sim.constants()
    assert tol == float(M.EM_TOL) and max_it == M.EM_MAX_IT and flag == FLAG and 0 < bound <= 1e-12


@pytest.mark.parametrize("S, W", [(1, 1), (2, 2), (3, 4), (4, 4), (5, 8), (7, 8), (8, 8), (9, 16), (15, 16), (16, 16), (17, 32), (31, 32), (32, 32), (33, 64), (63, 64), (64, 64), (65, 64),
                                  (128, 64), (129, 64), (130, 64), (192, 64), (193, 64), (256, 64), (257, 64), (320, 64), (1 << 27, 64)])
def test_segment_width(S, W):
    assert sim.width(S) == W and 64 % W == 0


def test_segment_grid():
    """svjg_geno.h: segment_grid on 256 units, worked by hand: W = width(S), 64 / W rows a wave, ceil(n_rows / that) waves, ceil(waves * 64 / tpb)
    blocks, at most 256 * per_cu"""
    for (n_rows, S, tpb, per_cu), blocks in {(1, 1, 256, 8): 1,                       # one wave of 64 rows, one block
                                             (1000, 5, 256, 8): 32,                   # W 8: 125 waves, 31.25 blocks
                                             (1000, 5, 128, 2): 63,                   # 125 waves, 62.5 blocks of two waves
                                             (65, 33, 256, 8): 17,                    # W 64: 65 waves, 16.25 blocks
                                             (100000, 64, 256, 8): 2048,              # 25 000 blocks: the cap
                                             (10000, 2048, 256, 8): 2048}.items():    # 2 500 blocks: the cap
        assert sim.segment_grid(n_rows, S, tpb, 256, per_cu) == blocks, (n_rows, S, tpb, per_cu)


def test_item_weights_against_the_model():
    from decimal import localcontext
    rng = np.random.default_rng(3)
    with localcontext() as ctx:
        ctx.prec = M.PREC
        for k in range(600):
            t, P = int(rng.integers(0, 4)), int(rng.integers(1, 9))
            ref, alt = (int(x) for x in (rng.integers(0, 61, 2) if k % 3 else rng.integers(0, 5, 2)))
            if k % 50 == 0:
                ref = int(rng.integers(1000, 5001))               # deep: the far weights underflow to 0 in doubles
            p, w, gmax = sim.item(t, ref, alt, P, CC.ERR)
            c1, c2 = M.norm_counts(t, ref, alt)
            if c1 + c2 == 0:
                assert p == 0 and not w.any()
                continue
            want, want_gmax = M.weights(c1, c2, P, CC.ERR)
            assert p == P and gmax == want_gmax and not w[P + 1:].any()
            for g in range(P + 1):
                exact = float(want[g] * M._COMB[P][g])
                assert abs(w[g] - exact) <= 4e-16 * exact + 1e-320, (t, ref, alt, P, g)
    assert sim.item(0, 7, 7, 0, CC.ERR)[0] == 0 and sim.item(0, 7, 7, 9, CC.ERR)[0] == 0


def _against_golden(name, rows, wave=False):
    """the harness on `rows` of a case (None: all) against the stored answers, a step's sum sample after sample or (wave) in the kernel's order;
    -> the largest |f - f_model|"""
    c = CC.inputs(name)
    want = CC.load_golden(name, c)
    done, raw = CC.gate(c)
    rows = np.arange(len(c["t"])) if rows is None else np.asarray(rows)
    ploidy = None if c["ploidy"] is None else c["ploidy"][rows]
    worst = 0.0
    for ms in (0, 3):
        f, steps, gt, gq, site = sim.rows(c["t"][rows], raw[rows], done[rows], ploidy, CC.ERR, ms, wave=wave)
        keep = ~want["row_out"][rows]
        left = (want["item_out"] | want["row_out"][:, None])[rows]
        has = ~np.isnan(want["f_hi"][rows])
        assert np.array_equal(np.isnan(f), ~has)
        assert np.array_equal((steps & ~np.uint32(FLAG))[keep], want["steps"][rows][keep]) and np.array_equal(((steps & FLAG) != 0)[keep], want["flag"][rows][keep])
        on = keep & has
        if on.any():
            worst = max(worst, float(np.abs((f[on] - want["f_hi"][rows][on]) - want["f_lo"][rows][on]).max()))
        w_gt, w_gq = CC.with_support(want["gt"][rows], want["gq"][rows], c["t"][rows], raw[rows], ms)
        assert np.array_equal(gt[~left], w_gt[~left]) and np.array_equal(gq[~left], w_gq[~left]), name
        assert np.array_equal(site, M.site_of(gt, ploidy))
    return worst, c, want


@pytest.mark.parametrize("name", ["null_5", "mixed_1", "mixed_5", "sex_4", "deep_33", "mixed_33"] + list(CC.SHAPE_CASES))
def test_every_row_of_a_case_through_the_harness(name):
    """sample after sample and in the kernel's order (lanes, strides, butterfly): steps, flag, GT, GQ and site as stored, f within SIM_F_BOUND"""
    for wave in (False, True):
        worst, c, want = _against_golden(name, None, wave)
        print("%s, %s: max |f - f_model| = %.3e" % (name, "the kernel's order" if wave else "sample after sample", worst))
        assert worst <= SIM_F_BOUND
    assert want["row_out"].mean() <= CC.CAP and (want["item_out"] | want["row_out"][:, None]).mean() <= CC.CAP


@pytest.mark.parametrize("name", [c[0] for c in CC.CASES])
def test_kernel_order_f_within_the_device_bound(name):
    """every row of every case with the sums in the kernel's order: f within EM_F_BOUND of the model, the bound the device is held to (the kernel
    differs from this arithmetic in exp10 and log10 only), and everything else as stored"""
    worst = _against_golden(name, None, wave=True)[0]
    print("%s: max |f - f_model| = %.3e in the kernel's order" % (name, worst))
    assert worst <= sim.constants()[3]


@pytest.mark.parametrize("name", [c[0] for c in CC.CASES])
def test_stored_answers_are_the_models(name):
    """a sample of rows of every case, the planted ones among them: the 60-digit model again, against what is stored; the harness on the same rows"""
    c = CC.inputs(name)
    want = CC.load_golden(name, c)
    done, raw = CC.gate(c)
    rows = sorted(set(range(7, len(c["t"]), 211)) | set(c["planted"].values()))
    m = M.run(c["t"], raw, done, c["ploidy"], CC.ERR, 0, rows=rows)
    for k in ("f_hi", "steps", "flag", "gt", "gq"):
        assert np.array_equal(m[k][rows], want[k][rows], equal_nan=(k == "f_hi")), k
    assert np.allclose(m["f_lo"][rows], want["f_lo"][rows], rtol=1e-6, atol=1e-37)    # (stored as float32)
    part = ~np.isnan(m["gap"][rows])
    assert np.array_equal(want["item_out"][rows], part & ((m["gq_margin"][rows] < CC.GQ_MARGIN) | (m["gap"][rows] < CC.TOP_GAP)))
    assert np.array_equal(want["row_out"][rows], ~np.isnan(m["ratio"][rows]) & (np.abs(m["ratio"][rows] - 1) <= CC.RATIO_BAND))
    assert want["row_out"].mean() <= CC.CAP and (want["item_out"] | want["row_out"][:, None]).mean() <= CC.CAP
    p = c["planted"]
    assert np.isnan(want["f_hi"][p["absent"]]) and np.isnan(want["f_hi"][p["zero_reads"]]) and want["steps"][p["absent"]] == 0
    if done[p["hom_ref"]].any():
        assert want["f_hi"][p["hom_ref"]] < 1e-3 and want["f_hi"][p["hom_alt"]] > 1 - 1e-3
    assert _against_golden(name, rows)[0] <= SIM_F_BOUND


def test_the_cases_hold_what_the_issue_asks_for():
    total, capped = 0, 0
    for name, S, R, pattern, _ in CC.CASES:
        z = np.load(CC.golden_path(name))
        total += int(z["prior_differs"])
        capped += int(z["flag"].sum())
        assert z["gt"].shape == (R, S)
    assert total >= 20 and capped >= 1                            # the prior decides calls, and the step cap is reached somewhere
    assert {c[1] for c in CC.CASES} == set(CC.SIZES) | set(CC.SHAPE_SIZES) and {c[3] for c in CC.CASES} == {None, "mixed", "sex", "deep"}
    # every segment width, full and not; no, one, two and three further items of a lane, and recomputed ones behind three staged ones
    assert {sim.width(S) for S in CC.SIZES + CC.SHAPE_SIZES} == {1, 2, 4, 8, 16, 32, 64} and {4, 8, 16, 32, 64} <= set(CC.SIZES + CC.SHAPE_SIZES)
    assert {min((S + 63) // 64 - 1, 4) for S in CC.SIZES + CC.SHAPE_SIZES} == {0, 1, 2, 3, 4} and {192, 256, 257, 320} <= set(CC.SHAPE_SIZES)
    deep = CC.inputs("deep_33")
    assert deep["counts"].max() >= 4900 and (sim.item(2, 5000, 3, 2, CC.ERR)[1][:3] == [1.0, 0.0, 0.0]).all()


def test_harness_under_the_sanitizers():
    """the stand-alone program (its own main) built with -fsanitize=address,undefined"""
    p = subprocess.run([sim.build_main(), "prior"], capture_output=True, text=True)
    assert p.returncode == 0 and p.stdout.startswith("cohort_prior_sim ok:"), p.stdout + p.stderr
    assert "runtime error" not in p.stderr and "AddressSanitizer" not in p.stderr


# ---- the block ----

@pytest.mark.parametrize("per_item", [False, True])
@pytest.mark.parametrize("max_ploidy", [1, 2, 8])
@pytest.mark.parametrize("S", [1, 3, 64, 65])
@pytest.mark.parametrize("n_rows", [1, 7, 1000])
def test_cohort_prior_layout(n_rows, S, max_ploidy, per_item):
    L = sim.layout(n_rows, S, max_ploidy, per_item)
    n, npl, words = n_rows * S, max_ploidy + 1, 16 if per_item else 8
    assert (L["pl"], L["raw"], L["gt"], L["flags"], L["boundary"], L["gq"]) == (0, 8 * npl * n, 8 * npl * n + 8 * n, 8 * npl * n + 9 * n, 8 * npl * n + 10 * n, 8 * npl * n + 11 * n)
    af = (8 * npl * n + 12 * n + 7) & ~7
    assert (L["af"], L["psite"], L["steps"], L["site"], L["maxn"]) == (af, af + 8 * n_rows, af + 20 * n_rows, af + 24 * n_rows, af + (24 + words) * n_rows)
    at = 0
    for name, size, align in [("pl", 8 * npl * n, 8), ("raw", 8 * n, 4), ("gt", n, 1), ("flags", n, 1), ("boundary", n, 1), ("gq", n, 1), ("af", 8 * n_rows, 8),
                              ("psite", 12 * n_rows, 4), ("steps", 4 * n_rows, 4), ("site", words * n_rows, 8), ("maxn", 8, 8), ("logtab", 2 * 45 * 8, 8),
                              ("slot", 4 * n_rows, 4), ("type", n_rows, 1), ("ok", n_rows, 1)] + ([("ploidy", n, 1)] if per_item else []):
        assert L[name] >= at, f"{name} overlaps the field in front of it"
        assert L[name] % align == 0, f"{name} at {L[name]} is not {align}-byte aligned"
        at = L[name] + size
    assert at <= L["total"], "the last field ends behind the block"
    # the first kernel's site words and the max_n pair: ONE memset; the inputs: ONE contiguous region right behind the pair
    assert L["in_at"] == L["maxn"] + 8 == L["logtab"] and L["slot"] == L["logtab"] + 720 and L["type"] == L["slot"] + 4 * n_rows
    assert L["ok"] == L["type"] + n_rows and L["ploidy"] == L["ok"] + n_rows and L["in_bytes"] == 720 + 6 * n_rows + (n if per_item else 0)
    assert L["total"] == L["in_at"] + L["in_bytes"] + 64
    assert L["total"] <= (8 * npl + 13) * n + 46 * n_rows + 808  # the 8 (max_ploidy + 1) + 13 an item the Python side budgets, 46 a row


# ---- the driver ----

def test_driver_joins_what_a_call_returns_behind_site():
    from svjg import genotype
    n, S = 10, 3
    rows = types.SimpleNamespace(sv_type=np.zeros(n, np.uint8), slot=np.arange(n, dtype=np.uint32), ok=np.ones(n, np.uint8))
    seen = []

    def call(lo, hi, ms, e):
        k = min(hi, n) - lo
        seen.append((lo, hi, ms, e))
        z = np.zeros((k, S), np.uint8)
        return (z + 1, np.zeros((k, S, 3), np.int64), np.zeros((k, S, 2), np.uint32), z, z, np.full((k, 3), lo, np.uint32),
                z + 7, np.arange(lo, lo + k, dtype=np.float64), np.full(k, lo, np.uint32))
    out = genotype._cohort_rows(call, rows, 4, None, -1, 5e-5)
    assert [x[:2] for x in seen] == [(0, 4), (4, 8), (8, 12)] and seen[0][2:] == (0, 5e-5)
    assert len(out) == 8 and out[0].shape == (n, S) and out[4][:, 0].tolist() == [0] * 4 + [4] * 4 + [8] * 2
    assert (out[5] == 7).all() and out[6].tolist() == list(range(n)) and out[7].tolist() == [0] * 4 + [4] * 4 + [8] * 2
    five = genotype._cohort_rows(lambda lo, hi, ms, e: call(lo, hi, ms, e)[:6], rows, 4, None, 3, 5e-5)
    assert five.site.shape == (n, 3) and five.gq is None and five.af is None and five.em_steps is None      # the calls without a prior: nothing behind site
    assert all(np.array_equal(x, y) for x, y in zip(five[:5], out[:5]))
    assert genotype.cohort_chunk_rows(64, 2, True) * (64 * 37 + 46) <= 1 << 30 < (genotype.cohort_chunk_rows(64, 2, True) + 1) * (64 * 37 + 46)
    assert genotype.cohort_chunk_rows(10**9, 8, True) == 1


# ---- the writer ----

@pytest.mark.parametrize("info, em, want", [
    (".", (0.25, False), "NS=3;AN=6;AC=2;AF=0.333333;EMAF=0.25"),
    ("SVTYPE=DEL;EMAF=0.9;END=5;EMNC", (0.123456789, True), "SVTYPE=DEL;END=5;NS=3;AN=6;AC=2;AF=0.333333;EMAF=0.123457;EMNC"),
    ("EMNC;SVTYPE=DEL;EMNCX=1", (float("nan"), False), "SVTYPE=DEL;EMNCX=1;NS=3;AN=6;AC=2;AF=0.333333"),
    ("EMAF=1", (1e-12, False), "NS=3;AN=6;AC=2;AF=0.333333;EMAF=1e-12"),
])
def test_info_with_the_em_fields(info, em, want):
    from svjg import genotype
    assert genotype.cohort_info(info, 3, 2, 6, em=em) == want
    assert "EMAF=0.9" in genotype.cohort_info("SVTYPE=DEL;EMAF=0.9", 3, 2)      # without the prior an input's EMAF stays, as before


def test_sample_column_with_gq():
    from svjg import genotype
    assert genotype.sample_column(0, 2, 1, [10, 0, 20], 3, 3, 1) == "0/1:4.5:1.5,3:10,0,20"
    assert genotype.sample_column(0, 2, 1, [10, 0, 20], 3, 3, 1, 42) == "0/1:4.5:1.5,3:10,0,20:42"
    assert genotype.sample_column(0, 2, NO_CALL, [10, 0, 20], 3, 3, 1, NO_CALL) == "./.:4.5:1.5,3:10,0,20:."
    assert genotype.sample_column(0, 3, NO_CALL, [0] * 4, 0, 0, 0, NO_CALL) == "././.:0:0,0:.,.,.,.:."
    assert genotype.sample_column(0, 0, NO_CALL, [0], 0, 0, 0, NO_CALL) == ".:0:0,0:.:."


@pytest.mark.parametrize("which", ["plain", "edited"])
def test_writer_over_the_reference_made_fixtures(golden, tmp_path, which):
    """the model over tests/golden/cohort/ -> the file: the header lines, GQ and `.`, EMAF / EMNC, and DP / AD / PL equal to the reference's per-sample files"""
    from svjg import genotype
    co = CM.Cohort(golden, which)
    ploidy = None if which == "plain" else np.full(co.done.shape, 2, np.uint8)
    m = M.run(co.rows.sv_type, co.raw, co.done, ploidy, 5e-5, 3)
    steps = m["steps"].copy()
    has = np.flatnonzero(~np.isnan(m["f_hi"]))
    assert len(has) >= 3
    steps[has[1]] |= FLAG                                          # (no row of these fixtures reaches the cap: one is marked by hand)
    out = str(tmp_path / "out.vcf")
    n_done = genotype.write_vcf_cohort(out, co.rows, co.names, genotype.CohortCalls(m["gt"], co.pl, co.raw, co.done, M.site_of(m["gt"], ploidy), m["gq"], m["f_hi"], steps), ploidy)
    assert n_done == co.genotyped
    lines = open(out).read().split("\n")
    head = [ln for ln in lines if ln.startswith("##")]
    k = next(i for i, ln in enumerate(head) if ln.startswith("##INFO=<ID=NS,"))
    assert [ln.split(",")[0] for ln in head[k:k + 6]] == ["##INFO=<ID=NS", "##INFO=<ID=AN", "##INFO=<ID=AC", "##INFO=<ID=AF", "##INFO=<ID=EMAF", "##INFO=<ID=EMNC"]
    assert [ln.split(",")[0] for ln in head[k + 6:k + 11]] == ["##FORMAT=<ID=GT", "##FORMAT=<ID=DP", "##FORMAT=<ID=AD", "##FORMAT=<ID=PL", "##FORMAT=<ID=GQ"]
    assert head[k + 9].startswith("##FORMAT=<ID=PL,Number=%s," % ("3" if which == "plain" else "G")) and head[k + 10].startswith("##FORMAT=<ID=GQ,Number=1,Type=Integer,")
    assert lines[len(head)] == "#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\t" + "\t".join(co.names)
    data = [ln.split("\t") for ln in lines if ln and not ln.startswith("#")]
    assert len(data) == len(co.rows.slot) and all(d[8] == "GT:DP:AD:PL:GQ" and len(d) == 9 + len(co.names) for d in data)
    gt_text = {0: "0/0", 1: "0/1", 2: "1/1", NO_CALL: "./."}
    for r, d in enumerate(data):
        for s in range(len(co.names)):
            got, ref = d[9 + s].split(":"), co.ref_data[s][r][9].split(":")
            assert got[1:4] == ref[1:4]                            # DP, AD, PL: the reference's own text for this sample
            assert got[0] == gt_text[int(m["gt"][r, s])] and got[4] == ("." if m["gt"][r, s] == NO_CALL else str(int(m["gq"][r, s])))
        info = d[7].split(";")
        ns, an, ac = M.site_of(m["gt"], ploidy)[r]
        tail = ["NS=%d" % ns, "AN=%d" % an, "AC=%d" % ac] + (["AF=%s" % ("%.6g" % (ac / an))] if an else [])
        if not np.isnan(m["f_hi"][r]):
            tail.append("EMAF=%s" % ("%.6g" % m["f_hi"][r]))
        if r == has[1]:
            tail.append("EMNC")
        assert info[-len(tail):] == tail and sum(f.startswith(("NS=", "AN=", "AC=", "AF=", "EMAF=", "EMNC")) for f in info) == len(tail)
    assert any(m["gt"][r, s] != NO_CALL for r in range(len(data)) for s in range(len(co.names))) and (m["gt"] == NO_CALL).any()


def test_writer_drops_the_inputs_tags(tmp_path):
    from svjg import genotype
    f = tmp_path / "in.vcf"
    f.write_text("##fileformat=VCFv4.2\n#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\n"
                 "chr1\t100\td1\tN\t<DEL>\t.\tPASS\tSVTYPE=DEL;EMAF=0.5;END=400;AC=9;EMNC\n")
    rows = genotype.VcfRows(str(f), {})
    one = np.ones((1, 1), np.uint8)
    out = tmp_path / "out.vcf"
    genotype.write_vcf_cohort(str(out), rows, ["s"], genotype.CohortCalls(one, np.array([[[10, 0, 20]]], np.int64), np.array([[[4, 4]]], np.uint32), one, np.array([[1, 2, 1]], np.uint32),
                                                                           one * 33, np.array([0.5]), np.array([3], np.uint32)))
    assert out.read_text().split("\n")[-2] == "chr1\t100\td1\tN\t<DEL>\t.\tPASS\tSVTYPE=DEL;END=400;NS=1;AN=2;AC=1;AF=0.5;EMAF=0.5\tGT:DP:AD:PL:GQ\t0/1:6.0:2.0,4:10,0,20:33"


# ---- the script ----

def test_cohort_prior_needs_cohort(golden, tmp_path):
    co = CM.Cohort(golden, "plain")
    out = str(tmp_path / "never.vcf")
    p = subprocess.run([sys.executable, f"{AMD}/predict-genotype.py", "-d", os.path.join(co.dir, "s1.json"), "--cohort-prior", "-v", co.vcf, "-o", out],
                       capture_output=True, text=True)
    assert p.returncode == 2 and "usage:" in p.stderr and "--cohort-prior needs --cohort" in p.stderr and not os.path.exists(out)
    p = subprocess.run([sys.executable, f"{AMD}/predict-genotype.py", "--cohort", co.list, "--cohort-prior", "--ploidy", "3", "-v", co.vcf, "-o", out],
                       capture_output=True, text=True)
    assert p.returncode == 2 and "--cohort is diploid" in p.stderr and not os.path.exists(out)
    p = subprocess.run([sys.executable, f"{AMD}/predict-genotype.py", "--help"], capture_output=True, text=True)
    assert p.returncode == 0 and "--cohort-prior" in p.stdout
