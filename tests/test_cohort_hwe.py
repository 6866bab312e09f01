"""Cohort site test for Hardy-Weinberg equilibrium (--cohort LIST --cohort-hwe) on the CPU: the integer model's self-checks
(tests/cohort_hwe_model.py); the fixtures under tests/golden/cohort_hwe; the host harness (tests/geno_sim, topic hwe: svjg_geno.h's own routines inside a
restatement of k_cohort_hwe's loops) against the model within the derived bound; layout, chunking, INFO text and writer; run_cohort(hwe=True) with
stand-in contexts that answer cohort_hwe from the harness."""
import math
import os
import subprocess
import sys
from fractions import Fraction

import numpy as np
import pytest

from tests import cohort_hwe_model as M
from tests.geno_sim import hwe as hwe_sim

AMD = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "svjedi-graph_amd")
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "cohort_hwe")
FAMILIES = ("hwe", "excess", "deficit", "mono", "ties", "mixed", "deep")
# The bound of the issue: two orders under the tie rule's 1e-7, so that rounding cannot flip a tie decision; the expected error is 1e-13..1e-12
# (the table's entries, the rounding of a difference of some hundreds to a double, exp10).  Below P_FLOOR the device's terms underflow against the
# mode: a value of at most P_TINY, possibly 0.
REL, P_FLOOR, P_TINY = 1e-9, 1e-280, 1e-279
GT_VALUES = np.array([0, 0, 0, 1, 1, 2, 2, 3, 5, 8, 0xFF], np.uint8)


def held(p, want):
    """-> (every value within the bound, the largest relative error among the values the bound is relative for)"""
    p, want = np.asarray(p, np.float64).ravel(), np.asarray(want, np.float64).ravel()
    nan = np.isnan(want)
    big = ~nan & (want >= P_FLOOR)
    small = ~nan & ~big
    rel = np.abs(p[big] - want[big]) / want[big]
    ok = np.isnan(p[nan]).all() and (rel <= REL).all() and ((p[small] >= 0) & (p[small] <= P_TINY)).all()
    return bool(ok), float(rel.max()) if rel.size else 0.0


def draw(rng, n, S, mode, lo=0.01, hi=0.5):
    """calls in Hardy-Weinberg proportions at a frequency per row in [lo, hi]; mode: "none" (no ploidy array), "two" (all 2), "mixed" (ploidy 0..8,
    calls of every code)"""
    f = rng.uniform(lo, hi, (n, 1))
    gt = ((rng.random((n, S)) < f).astype(np.uint8) + (rng.random((n, S)) < f).astype(np.uint8)).astype(np.uint8)
    if mode == "mixed":
        other = rng.choice(GT_VALUES, size=(n, S))
        gt = np.where(rng.random((n, S)) < 0.2, other, gt).astype(np.uint8)
        return gt, rng.choice(np.array([2, 2, 2, 2, 2, 0, 1, 3, 4, 5, 6, 7, 8], np.uint8), size=(n, S))
    return gt, None if mode == "none" else np.full((n, S), 2, np.uint8)


def load(name):
    z = np.load(os.path.join(GOLDEN, name + ".npz"))
    return {k: z[k] for k in z.files}


# ---- the model ----

def test_weights_sum_to_the_binomial_and_are_symmetric():
    rng = np.random.default_rng(1)
    for _ in range(200):
        a, h, b = (int(x) for x in rng.integers(0, 40, 3))
        m, w = M.weights(a, h, b)                                            # (asserts sum w = C(2 n, m) itself)
        assert m == min(2 * a + h, 2 * b + h) and sum(w.values()) == math.comb(2 * (a + h + b), m)
        assert M.weights(b, h, a) == (m, w) and M.row(a, h, b) == M.row(b, h, a)
        n = a + h + b
        for hh, x in w.items():                                              # the closed form of every weight
            assert x == 2 ** hh * math.factorial(n) // (math.factorial((m - hh) // 2) * math.factorial(hh) * math.factorial(n - hh - (m - hh) // 2))


def test_known_answers_by_hand():
    assert M.row(0, 2, 0)[0] == 1.0 and M.row(1, 0, 1)[0] == 1 / 3            # weights {0: 2, 2: 4} of 6
    assert M.row(0, 2, 0)[1] == 4 / 6 and M.row(1, 0, 1)[1] == 1.0
    assert M.row(5, 0, 0)[:2] == (1.0, 1.0) and M.row(0, 0, 9)[:2] == (1.0, 1.0)        # m = 0
    assert all(math.isnan(x) for x in M.row(0, 0, 0)[:2])                    # n = 0
    assert M.fis(1, 0, 1) == 1.0 and M.fis(0, 2, 0) == -1.0 and M.fis(3, 0, 0) is None and M.fis(1, 2, 1) == 0.0
    # n = 4, m = 4: w(0) = 4! / (2! 2!) = 6, w(2) = 4 * 4! / 2! = 48, w(4) = 16, together C(8, 4) = 70
    assert M.weights(1, 2, 1) == (4, {0: 6, 2: 48, 4: 16})
    assert M.row(1, 2, 1)[:2] == (1.0, 64 / 70) and M.row(2, 0, 2)[:2] == (6 / 70, 1.0) and M.row(0, 4, 0)[:2] == (22 / 70, 16 / 70)


def test_an_exact_tie_is_selected_from_both_sides():
    ties = M.exact_ties(20)
    assert (6, 4, 2, 4) in ties and (9, 5, 3, 5) in ties
    n, m, h1, h2 = 6, 4, 2, 4
    _, w = M.weights(n - h1 - (m - h1) // 2, h1, (m - h1) // 2)
    assert w[h1] == w[h2] and Fraction(M.row(3, 2, 1)[0]) == Fraction(M.row(2, 4, 0)[0])
    total = sum(w.values())
    assert M.row(3, 2, 1)[0] == sum(x for x in w.values() if x <= w[h1]) / total == 1.0 and w[0] < w[2]
    assert not M.row(3, 2, 1)[2]                                             # a tie is far from the edge of the rule: ratio 1 against 1 + 1e-7


def test_near_is_the_definition_in_rationals():
    """near: some w(h) / w(n_het) within 1e-8 of 1 + 1e-7"""
    for counts in [(1, 0, 1), (3, 2, 1), (10, 5, 2), (20, 20, 20), (300, 200, 100)]:
        _, w = M.weights(*counts)
        w0 = w[counts[1]]
        want = any(abs(Fraction(x, w0) - (1 + Fraction(1, M.TIE))) <= Fraction(1, M.NEAR) for x in w.values())
        assert M.row(*counts)[2] == want


# ---- the fixtures ----

@pytest.mark.parametrize("name", FAMILIES)
def test_fixture_holds_what_the_model_gives_and_no_row_near_the_edge(name):
    z = load(name)
    assert os.path.getsize(os.path.join(GOLDEN, name + ".npz")) < 64 << 10
    counts, p, near = M.hwe(M.masked(z["gt"], z.get("done")), z.get("ploidy"))
    assert np.array_equal(counts, z["counts"]) and z["counts"].dtype == np.uint32
    assert p.tobytes() == z["p"].tobytes() and not near.any()                 # no row may be skipped: none is near


def test_fixture_families_are_what_they_say():
    z = {k: load(k) for k in FAMILIES}
    assert (z["excess"]["counts"][:, [0, 2]] == 0).all() and (z["excess"]["counts"][:, 1] > 0).all()
    assert (z["deficit"]["counts"][:, 1] == 0).all() and (z["deficit"]["p"][:, 1] == 1.0).all()
    mono = z["mono"]["counts"]
    assert ((mono > 0).sum(axis=1) <= 1).all() and np.isnan(z["mono"]["p"][mono.sum(axis=1) == 0]).all() and (z["mono"]["p"][mono.sum(axis=1) > 0] == 1.0).all()
    assert z["deep"]["gt"].shape[1] == 2048 and (z["deep"]["p"][:, 0] < 1e-300).sum() >= 2 and (z["deep"]["p"][:, 0] > 1e-3).any()
    assert set(np.unique(z["mixed"]["ploidy"]).tolist()) == set(range(9)) and {3, 0xFF} <= set(np.unique(z["mixed"]["gt"]).tolist()) and (z["mixed"]["done"] == 0).any()
    f = (2 * z["hwe"]["counts"][:, 2] + z["hwe"]["counts"][:, 1]) / (2 * z["hwe"]["counts"].sum(axis=1))
    assert f.min() < 0.05 and f.max() > 0.4
    for a, h, b in z["ties"]["counts"].tolist():                              # every row has a partner h2 with the same weight
        _, w = M.weights(a, h, b)
        assert sum(1 for x in w.values() if x == w[h]) >= 2


# ---- the harness against the model ----

@pytest.mark.parametrize("name", FAMILIES)
def test_harness_on_the_fixtures(name):
    z = load(name)
    for grid in (0, 1):
        counts, p = hwe_sim.run(M.masked(z["gt"], z.get("done")), z.get("ploidy"), grid=grid)
        assert np.array_equal(counts, z["counts"]) and counts.dtype == np.uint32
        ok, worst = held(p, z["p"])
        print("%s: largest relative error %.3g" % (name, worst))
        assert ok, worst


# every segment width (1, 2, 4, .., 64); one, two and three items a lane in phase 1 (S <= 64, 65..128, 129..192) and in phase 2 (m / 2 + 1 terms over
# 64 lanes: more than 64 terms from S = 130 at frequency 1/2, more than 128 from S = 257)
SHAPES = [1, 2, 3, 5, 9, 17, 31, 32, 33, 63, 64, 65, 128, 129, 130, 192, 193, 257, 300]


def test_shapes_take_every_path():
    assert sorted({hwe_sim.segment_width(S) for S in SHAPES}) == [1, 2, 4, 8, 16, 32, 64]
    assert {-(-S // 64) for S in SHAPES if S >= 64} >= {1, 2, 3}
    terms = [hwe_sim.row(0, S, 0)["terms"] for S in SHAPES]                   # all het: m = n = S
    assert {-(-t // 64) for t in terms} >= {1, 2, 3}
    assert hwe_sim.row(0, 300, 0) == {"n": 300, "m": 300, "par": 0, "het": 300, "h0": 150, "terms": 151}
    assert hwe_sim.row(3, 0, 0)["terms"] == 0 and hwe_sim.row(0, 0, 0)["terms"] == 0 and hwe_sim.row(10, 1, 0) == {"n": 11, "m": 1, "par": 1, "het": 1, "h0": 1, "terms": 1}


@pytest.mark.parametrize("S", SHAPES)
def test_harness_within_the_bound_of_the_model(S):
    rng = np.random.default_rng(2300 + S)
    for n in (1, 65, 130):
        for mode in ("none", "two", "mixed"):
            gt, ploidy = draw(rng, n, S, mode, hi=0.5 if n != 65 else 0.9)
            if mode == "two" and n == 130:
                gt[:8] = 1                                                    # all het: the most terms a row of S can have
            want_c, want_p, near = M.hwe(gt, ploidy)
            assert not near.any()                                             # (no row is skipped)
            counts, p = hwe_sim.run(gt, ploidy, grid=(n + S) % 2)             # a grid of one block (4 waves) against 65 or 130 rows: strides
            assert np.array_equal(counts, want_c), (S, n, mode)
            ok, worst = held(p, want_p)
            assert ok, (S, n, mode, worst)


def test_a_row_does_not_depend_on_its_neighbours_or_the_grid():
    rng = np.random.default_rng(5)
    gt, ploidy = draw(rng, 70, 20, "mixed")
    one = hwe_sim.run(gt, ploidy)
    for grid in (1, 2, 3):
        got = hwe_sim.run(gt, ploidy, grid=grid)
        assert got[0].tobytes() == one[0].tobytes() and got[1].tobytes() == one[1].tobytes()
    for r in (0, 1, 33, 69):
        alone = hwe_sim.run(gt[r:r + 1], ploidy[r:r + 1])
        assert alone[0].tobytes() == one[0][r:r + 1].tobytes() and alone[1].tobytes() == one[1][r:r + 1].tobytes()


def test_harness_under_the_sanitizers():
    """the same code as a stand-alone program with its own main under -fsanitize=address,undefined (nothing is loaded into Python)"""
    p = subprocess.run([hwe_sim.build_main(), "hwe"], capture_output=True, text=True)
    assert p.returncode == 0 and p.stdout.startswith("hwe_sim ok") and not p.stderr, (p.stdout, p.stderr)


# ---- layout, chunks ----

@pytest.mark.parametrize("n_rows, S, per_item", [(0, 1, False), (1, 1, True), (65, 3, True), (1000, 130, False), (10_000, 2048, True), (3, 65536, False)])
def test_hwe_layout(n_rows, S, per_item):
    L = hwe_sim.layout(n_rows, S, per_item)
    n, maxn = n_rows * S, (28 * n_rows + 7) & ~7
    assert L == {"p": 0, "counts": 16 * n_rows, "maxn": maxn, "in_at": maxn + 8, "in_bytes": n * (2 if per_item else 1), "gt": maxn + 8,
                 "ploidy": maxn + 8 + n if per_item else 0, "total": maxn + 8 + n * (2 if per_item else 1) + 64}
    from svjg import genotype
    step = genotype.cohort_hwe_chunk_rows(S, per_item)
    assert hwe_sim.layout(step, S, per_item)["total"] <= 1 << 30 < hwe_sim.layout(2 * step + 64, S, per_item)["total"] and step < 1 << 32


def test_constants():
    from svjg import capi
    assert hwe_sim.constants() == {"max_samples": 65536, "tpb": 256, "blocks_per_cu": 8} and capi.HWE_MAX_SAMPLES == 65536
    assert "svjg_cohort_hwe" in capi.EXPORTS


class _Recorder(hwe_sim.SimHwe):
    def __init__(self):
        self.calls = []

    def cohort_hwe(self, gt, ploidy=None):
        self.calls.append((np.array(gt), None if ploidy is None else np.array(ploidy)))
        return super().cohort_hwe(gt, ploidy)


@pytest.mark.parametrize("mode", ["none", "mixed"])
def test_any_chunking_gives_the_same_bytes(mode):
    from svjg import genotype
    rng = np.random.default_rng(12)
    n, S = 200, 7
    gt, ploidy = draw(rng, n, S, mode)
    done = (rng.random((n, S)) < 0.8).astype(np.uint8)
    masked = M.masked(gt, done)
    want = hwe_sim.run(masked, ploidy)
    assert np.array_equal(want[0], M.hwe(masked, ploidy)[0])
    for step in (None, 1, 64, 65, n - 1, n, 10 * n):
        ctx = _Recorder()
        counts, p = genotype.cohort_hwe_rows(ctx, gt, done, ploidy, step)
        assert counts.dtype == np.uint32 and p.dtype == np.float64 and counts.tobytes() == want[0].tobytes() and p.tobytes() == want[1].tobytes(), step
        assert len(ctx.calls) == (1 if step is None else -(-n // step))
        assert np.array_equal(np.concatenate([c[0] for c in ctx.calls]), masked)         # done == 0 goes in as 0xFF
        assert all((c[1] is None) == (ploidy is None) for c in ctx.calls)
    counts, p = genotype.cohort_hwe_rows(_Recorder(), np.zeros((0, 3), np.uint8), np.zeros((0, 3), np.uint8), None)
    assert counts.shape == (0, 3) and p.shape == (0, 2)


# ---- INFO text and the writer ----

def test_cohort_info_tags_order_and_dropped_fields():
    from svjg import genotype
    info = "SVTYPE=DEL;DGC=9,9,9;END=600;HWE=0.5;NS=9;EXCHET=1;FIS=-1;SVQ=3;XHWE=1;MLAC=2"
    got = genotype.cohort_info(info, 3, 2, None, (0.25, True), (12.345, 2, 6), ((1, 2, 1), 1.0, 0.5))
    assert got == "SVTYPE=DEL;END=600;XHWE=1;NS=3;AN=6;AC=2;AF=0.333333;EMAF=0.25;EMNC;SVQ=12.35;MLAC=2;MLAF=0.333333;DGC=1,2,1;HWE=1;EXCHET=0.5;FIS=0"
    assert genotype.cohort_info(info, 3, 2) == "SVTYPE=DEL;DGC=9,9,9;END=600;HWE=0.5;EXCHET=1;FIS=-1;SVQ=3;XHWE=1;MLAC=2;NS=3;AN=6;AC=2;AF=0.333333"   # without the option: kept
    assert genotype.cohort_info("HWE=1", 0, 0, 0, hwe=((0, 0, 0), math.nan, math.nan)) == "NS=0;AN=0;AC=0;DGC=0,0,0"          # n = 0: DGC alone
    assert genotype.cohort_info(".", 1, 0, hwe=((4, 0, 0), 1.0, 1.0)) == "NS=1;AN=2;AC=0;AF=0;DGC=4,0,0;HWE=1;EXCHET=1"       # m = 0: no FIS
    assert genotype.cohort_info(".", 1, 0, hwe=((1, 0, 1), 1 / 3, 1.0)).endswith("DGC=1,0,1;HWE=0.333333;EXCHET=1;FIS=1")
    assert genotype.cohort_info(".", 1, 0, hwe=((0, 2, 0), 1.0, 2 / 3)).endswith("DGC=0,2,0;HWE=1;EXCHET=0.666667;FIS=-1")
    assert genotype.cohort_info(".", 1, 0, hwe=((1000, 3, 1000), 1e-300, 1.0)).endswith("HWE=1e-300;EXCHET=1;FIS=0.997004")         # 1 - 6 / 2003
    assert genotype.cohort_info(".", 1, 0, hwe=((7, 0, 7), 0.0, 1.0)).endswith("HWE=0;EXCHET=1;FIS=1")


def test_fis_and_the_negative_zero_rule():
    from svjg import genotype
    assert genotype.hwe_fis(1, 2, 1) == 0.0 and genotype.hwe_fis(5, 0, 0) is None and genotype.hwe_fis(0, 0, 0) is None and genotype.hwe_fis(0, 0, 3) is None
    for counts in [(1, 0, 1), (0, 2, 0), (10, 5, 2), (1000, 3, 1000)]:
        assert genotype.hwe_fis(*counts) == M.fis(*counts)
    assert "%.6g" % -0.0 == "-0" and "%.6g" % -1e-9 == "-1e-09"               # the only text the rule is about: a FIS that is -0.0 itself
    assert genotype.cohort_info(".", 1, 0, hwe=((1, 2, 1), 1.0, 0.8)).endswith("FIS=0")


HEADER_IDS = ("DGC", "HWE", "EXCHET", "FIS")


def strip_hwe(text):
    """a VCF's text without the four INFO header lines and the four tags (they are the last of INFO)"""
    out = []
    for line in text.split("\n"):
        if line.startswith(tuple("##INFO=<ID=%s," % k for k in HEADER_IDS)):
            continue
        if line and not line.startswith("#"):
            f = line.split("\t")
            keep = [x for x in f[7].split(";") if x.split("=", 1)[0] not in HEADER_IDS]
            f[7] = ";".join(keep)
            line = "\t".join(f)
        out.append(line)
    return "\n".join(out)


def info_tags(text):
    """per data line: {key: value} of INFO, and the order of the keys"""
    rows = []
    for line in text.split("\n"):
        if line and not line.startswith("#"):
            fields = line.split("\t")[7].split(";")
            rows.append(([x.split("=", 1)[0] for x in fields], dict(x.split("=", 1) for x in fields if "=" in x)))
    return rows


def check_tags(text, gt, ploidy=None):
    """the four header lines follow the other cohort INFO lines; per row DGC = the model's counts on gt, HWE / EXCHET within 1e-5 of the model's, FIS
    the writer's text of the integers; the tags are the last of INFO, in order, and absent where they must be"""
    from svjg import genotype
    lines = text.split("\n")
    head = [l for l in lines if l.startswith("##INFO=<ID=")]
    ours = [i for i, l in enumerate(head) if l.startswith(tuple("##INFO=<ID=%s," % k for k in HEADER_IDS))]
    assert [head[i].split(",")[0][11:] for i in ours] == list(HEADER_IDS) and all("called diploid samples only" in head[i] for i in ours)
    assert ours == list(range(ours[0], ours[0] + 4)) and head[ours[0] - 1].startswith(("##INFO=<ID=AF,", "##INFO=<ID=EMNC,", "##INFO=<ID=MLAF,"))
    assert "Number=3,Type=Integer" in head[ours[0]] and all("Number=1,Type=Float" in head[i] for i in ours[1:])
    counts, p, _ = M.hwe(gt, ploidy)
    rows = info_tags(text)
    assert len(rows) == len(counts)
    for (order, tags), c, q in zip(rows, counts.tolist(), p.tolist()):
        assert tags["DGC"] == "%d,%d,%d" % tuple(c)
        want = ["DGC"] + (["HWE", "EXCHET"] if sum(c) else []) + (["FIS"] if M.fis(*c) is not None else [])
        assert order[-len(want):] == want and not set(HEADER_IDS) & set(order[:-len(want)])
        if sum(c):
            assert abs(float(tags["HWE"]) - q[0]) <= 1e-5 * q[0] and abs(float(tags["EXCHET"]) - q[1]) <= 1e-5 * q[1]
        if M.fis(*c) is not None:
            want_fis = "%.6g" % M.fis(*c)
            assert tags["FIS"] == ("0" if want_fis == "-0" else want_fis)
    return counts


# ---- run_cohort with stand-in contexts: the golden cohort (plain, --joint-ins, --joint-prior), and fixed arrays for the other options ----

def _golden_ctx(joint_prior):
    from tests import standin_capi
    from tests.test_cohort_joint_ins import CohortModelCtx
    base = CohortModelCtx
    if joint_prior:
        from tests.test_cohort_site_prior import SitePriorModelCtx
        base = SitePriorModelCtx

    class HweStandinCtx(standin_capi.Context, base, hwe_sim.SimHwe):
        hwe_calls = []

        def __init__(self, device=0):
            standin_capi.Context.__init__(self, device)
            base.__init__(self, device)

        def cohort_hwe(self, gt, ploidy=None):
            HweStandinCtx.hwe_calls.append(np.array(gt))
            return hwe_sim.SimHwe.cohort_hwe(self, gt, ploidy)
    return HweStandinCtx


@pytest.mark.parametrize("option", ["plain", "joint_ins", "joint_prior"])
@pytest.mark.parametrize("which", ["plain", "edited"])
def test_run_cohort_hwe_on_the_golden_cohort(golden, tmp_path, monkeypatch, which, option):
    from svjg import capi, genotype
    from tests import cohort_model as CM
    from tests.test_cohort_qc import vcf_gt
    monkeypatch.setenv("SVJG_PY_VCF", "1")
    ctx = _golden_ctx(option == "joint_prior")
    monkeypatch.setattr(capi, "Context", ctx)
    co = CM.Cohort(golden, which)
    kw = {"plain": {}, "joint_ins": {"joint_ins": True}, "joint_prior": {"joint_ins": True, "joint_prior": True}}[option]
    a, b = str(tmp_path / "without.vcf"), str(tmp_path / "with.vcf")
    assert genotype.run_cohort(co.list, co.vcf, a, **kw) == genotype.run_cohort(co.list, co.vcf, b, hwe=True, **kw)
    without, with_hwe = open(a).read(), open(b).read()
    assert strip_hwe(with_hwe) == without and with_hwe != without
    names, gt = vcf_gt(b)
    assert names == co.names and len(ctx.hwe_calls[-1]) == len(gt)
    counts = check_tags(with_hwe, gt)
    assert (counts.sum(axis=1) > 0).any() and sorted(os.listdir(tmp_path)) == ["with.vcf", "without.vcf"]


def _fixed_ctx():
    from tests.test_cohort_run_pinned import FixedCtx

    class FixedHweCtx(FixedCtx, hwe_sim.SimHwe):
        def cohort_hwe(self, gt, ploidy=None):
            self.calls.append(("hwe", len(gt)))
            self.hwe_in = (np.array(gt), None if ploidy is None else np.array(ploidy))
            return hwe_sim.SimHwe.cohort_hwe(self, gt, ploidy)
    return FixedHweCtx


@pytest.mark.parametrize("name", ["plain", "ploidy", "prior", "prior_ploidy", "plain_qual", "prior_ploidy_qual"])
def test_run_cohort_hwe_beside_every_other_option(tmp_path, monkeypatch, capsys, name):
    """the pinned run of tests/test_cohort_run_pinned.py with hwe=True: but for the four tags and header lines the bytes are the pinned file's; the
    tags are the model's on the calls the run handed to cohort_hwe, and those are the printed ones (done == 0 as 0xFF)"""
    from svjg import capi
    from tests import test_cohort_run_pinned as P
    cohort = P.make_inputs(tmp_path, monkeypatch)
    ctx_class = _fixed_ctx()
    monkeypatch.setattr(capi, "Context", ctx_class)
    kw = dict(P.RUNS)[name]
    got, _, ctx = P.run_one(cohort, name, dict(kw, hwe=True))
    with open(os.path.join(P.GOLDEN, name + ".vcf"), "rb") as fh:
        pinned = fh.read().decode()
    assert strip_hwe(got.decode()) == pinned
    assert ctx.calls[-1] == ("hwe", len(P._ROWS))
    gt, ploidy = ctx.hwe_in
    assert (ploidy is not None) == bool(kw.get("ploidy_file"))
    check_tags(got.decode(), gt, ploidy)
    # the calls handed in are the printed ones: a dot in the GT text is a no-call, the 1s of a called item its alt copies
    data = [ln.split("\t")[9:] for ln in got.decode().split("\n") if ln and not ln.startswith("#")]
    text_gt = np.array([[0xFF if "." in c.split(":")[0] else c.split(":")[0].count("1") for c in row] for row in data], np.uint8)
    P2 = np.full(gt.shape, 2) if ploidy is None else ploidy
    called = (gt <= P2) & (P2 >= 1)
    assert np.array_equal(np.where(called, gt, 0xFF), text_gt)


# ---- the script ----

def test_script_refuses_cohort_hwe_without_cohort(tmp_path):
    (tmp_path / "in.vcf").write_text("##fileformat=VCFv4.2\n")
    (tmp_path / "d.json").write_text("{}")
    p = subprocess.run([sys.executable, os.path.join(AMD, "predict-genotype.py"), "-d", "d.json", "-v", "in.vcf", "-o", "out.vcf", "--cohort-hwe"],
                       capture_output=True, text=True, cwd=tmp_path)
    assert p.returncode != 0 and "usage:" in p.stderr and "--cohort-hwe needs --cohort" in p.stderr
    assert sorted(os.listdir(tmp_path)) == ["d.json", "in.vcf"]


def test_script_lets_cohort_hwe_through_with_every_cohort_option(tmp_path):
    """the parser and the options check let the combinations through: the run gets as far as the cohort list, which does not exist"""
    (tmp_path / "in.vcf").write_text("##fileformat=VCFv4.2\n")
    for extra in ([], ["--cohort-prior"], ["--cohort-ploidy", "p.txt"], ["--joint-ins"], ["--joint-ins", "--joint-prior"], ["--cohort-qual"], ["--cohort-qc", "qc"]):
        p = subprocess.run([sys.executable, os.path.join(AMD, "predict-genotype.py"), "--cohort", "none.list", "-v", "in.vcf", "-o", "out.vcf",
                            "--cohort-hwe", *extra], capture_output=True, text=True, cwd=tmp_path)
        assert p.returncode != 0 and "usage:" not in p.stderr and "none.list" in p.stderr, (extra, p.stderr)
        assert sorted(os.listdir(tmp_path)) == ["in.vcf"]


def test_check_cohort_options_gains_the_parameter_and_no_rule():
    from svjg import genotype
    for kw in ({}, {"prior": True}, {"ploidy_file": "x"}, {"joint_ins": True}, {"joint_ins": True, "joint_prior": True}, {"qual": True}, {"qc": "q"}):
        genotype.check_cohort_options(**kw, hwe=True)
    for kw in ({"joint_ins": True, "prior": True}, {"joint_prior": True}, {"qc": ""}):
        for hwe in (False, True):
            with pytest.raises(ValueError):
                genotype.check_cohort_options(**kw, hwe=hwe)
