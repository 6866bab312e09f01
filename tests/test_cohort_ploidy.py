"""Cohort genotyping at per-sample ploidy without a GPU: the --cohort-ploidy file, the ploidy matrix, the INFO rewrite with AN, the writer's
text, and the integer pieces of the device leg compiled with g++ (tests/geno_sim: cohort_layout per item, cohort_ploidy_sums under
cohort_segment's masks)."""
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests.geno_sim import cohort as sim             # noqa: E402

NAMES = ["A", "B b", "C"]
VCF = ("##fileformat=VCFv4.2\n"
       "##FORMAT=<ID=GT,Number=1,Type=String,Description=\"old\">\n"
       "#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\tOLD\n"
       "chr1\t100\td1\tN\t<DEL>\t.\tPASS\tSVTYPE=DEL;END=400;AC=9\n"
       "chr1\t5000\td2\tN\t<DEL>\t.\tPASS\tSVTYPE=DEL;END=5400\n"
       "chrX\t100\td3\tN\t<DEL>\t.\tPASS\tSVTYPE=DEL;END=400\n"
       "chrX\t2000\td4\tN\t<DEL>\t.\tPASS\tSVTYPE=DEL;END=2400\n"
       "chrY\t7\td5\tN\t<DEL>\t.\tPASS\tSVTYPE=DEL;END=407\n"
       "chrM\tabc\td6\tN\tNACGT\t.\tPASS\tSVTYPE=INS\n")           # (a POS that is no plain decimal matches whole-contig lines only)


def _rows(tmp_path):
    from svjg import genotype
    f = tmp_path / "in.vcf"
    f.write_text(VCF)
    return genotype.VcfRows(str(f), {})


# ---- the --cohort-ploidy file ----

def test_file_good_lines_star_and_first_match(tmp_path):
    from svjg import genotype
    f = tmp_path / "p.tsv"
    f.write_text("# sex chromosomes\n\nA\tchrX\t1\r\n*\tchrY\t0\nB b\tchrX\t1000\t3000\t3\nA\tchrX\t2\n*\tchrX\t2\n   \nC\tchrY\t1\nA\tchrY\t1\n")
    per = genotype.load_cohort_ploidy_file(str(f), NAMES)
    assert per == [[("chrX", None, None, 1), ("chrY", None, None, 0), ("chrX", None, None, 2), ("chrX", None, None, 2), ("chrY", None, None, 1)],
                   [("chrY", None, None, 0), ("chrX", 1000, 3000, 3), ("chrX", None, None, 2)],
                   [("chrY", None, None, 0), ("chrX", None, None, 2), ("chrY", None, None, 1)]]
    m = genotype.cohort_ploidy_matrix(_rows(tmp_path), per)
    # rows: chr1:100, chr1:5000, chrX:100, chrX:2000, chrY:7, chrM:abc — the first match wins (A's second chrX line and C's chrY line never do)
    assert m.dtype == np.uint8 and m.tolist() == [[2, 2, 2], [2, 2, 2], [1, 2, 2], [1, 3, 2], [0, 0, 0], [2, 2, 2]]


@pytest.mark.parametrize("text, line", [
    ("A\tchrX\t1\nA chrX 1\n", 2),                     # blanks do not separate
    ("A\tchrX\n", 1),                                  # too few fields
    ("A\tchrX\t1\t2\n", 1),                            # four fields
    ("A\tchrX\t1\t2\t3\t4\n", 1),                      # six
    ("A\tchrX\t9\n", 1),                               # ploidy above 8
    ("A\tchrX\t-1\n", 1),
    ("A\tchrX\t+1\n", 1),
    ("A\tchrX\t1.0\n", 1),
    ("A\tchrX\t\n", 1),                                # an empty field
    ("A\t\t1\n", 1),
    ("\tchrX\t1\n", 1),                                # an empty sample
    ("A\tchr X\t1\n", 1),                              # a blank inside a field behind SAMPLE
    ("A\tchrX\t 1\n", 1),
    ("# ok\nA\tchrX\t0\t5\t1\n", 2),                   # FROM below 1
    ("A\tchrX\t9\t5\t1\n", 1),                         # TO below FROM
    ("A\tchrX\t1\tx\t1\n", 1),
    ("*\tchrX\t1\n\nD\tchrX\t1\n", 3),                 # a sample that is not in the list
    ("b\tchrX\t1\n", 1),                               # (names are compared whole and exactly)
    ("B\tchrX\t1\n", 1),
])
def test_file_bad_lines_name_file_and_line(tmp_path, text, line):
    from svjg import genotype
    f = tmp_path / "bad.tsv"
    f.write_text(text)
    with pytest.raises(ValueError) as ei:
        genotype.load_cohort_ploidy_file(str(f), NAMES)
    assert "%s:%d:" % (f, line) in str(ei.value)


def test_matrix_is_rows_ploidy_on_the_samples_own_lines(tmp_path):
    """the definition: sample s's column = rows_ploidy over the lines whose first field is its name or `*`, that field removed, in file order —
    here through a --ploidy-file written per sample and read by load_ploidy_file"""
    from svjg import genotype
    rng = np.random.default_rng(11)
    rows = _rows(tmp_path)
    chroms = ["chr1", "chrX", "chrY", "chrM", "chr9"]
    for trial in range(20):
        lines = []
        for _ in range(int(rng.integers(0, 12))):
            who = ["*"] + NAMES
            name = who[int(rng.integers(0, 4))]
            c = chroms[int(rng.integers(0, 5))]
            if rng.random() < 0.5:
                lines.append((name, [c, str(int(rng.integers(0, 9)))]))
            else:
                lo = int(rng.integers(1, 4000))
                lines.append((name, [c, str(lo), str(lo + int(rng.integers(0, 4000))), str(int(rng.integers(0, 9)))]))
        f = tmp_path / ("m%d.tsv" % trial)
        f.write_text("".join("\t".join([n] + rest) + "\n" for n, rest in lines))
        m = genotype.cohort_ploidy_matrix(rows, genotype.load_cohort_ploidy_file(str(f), NAMES))
        assert m.shape == (6, 3)
        for s, name in enumerate(NAMES):
            own = tmp_path / ("m%d_%d.txt" % (trial, s))
            own.write_text("".join(" ".join(rest) + "\n" for n, rest in lines if n in ("*", name)))
            assert np.array_equal(m[:, s], genotype.rows_ploidy(rows, None, genotype.load_ploidy_file(str(own)))), (trial, name)
    empty = tmp_path / "none.tsv"
    empty.write_text("# nothing\n")
    assert (genotype.cohort_ploidy_matrix(rows, genotype.load_cohort_ploidy_file(str(empty), NAMES)) == 2).all()


def test_ploidy_file_parser_is_unchanged(tmp_path):
    from svjg import genotype
    f = tmp_path / "p.txt"
    f.write_text("# c\nchrX 1\nchr1\t10\t20\t0\n")
    assert genotype.load_ploidy_file(str(f)) == [("chrX", None, None, 1), ("chr1", 10, 20, 0)]
    f.write_text("chrX 1\nchrX 1 2\n")
    with pytest.raises(ValueError) as ei:
        genotype.load_ploidy_file(str(f))
    assert str(ei.value) == "%s:2: expected `CHROM PLOIDY` or `CHROM FROM TO PLOIDY`: 'chrX 1 2'" % f
    f.write_text("chrX 9\n")
    with pytest.raises(ValueError) as ei:
        genotype.load_ploidy_file(str(f))
    assert str(ei.value) == "%s:1: ploidy 9 is not in 0..8" % f


# ---- INFO ----

@pytest.mark.parametrize("info, ns, ac, an, want", [
    (".", 3, 2, None, "NS=3;AN=6;AC=2;AF=0.333333"),                                             # without an: 2 NS, as before
    ("SVTYPE=DEL;END=5", 4, 8, None, "SVTYPE=DEL;END=5;NS=4;AN=8;AC=8;AF=1"),
    (".", 3, 2, 5, "NS=3;AN=5;AC=2;AF=0.4"),
    ("AN=1;SVTYPE=DEL;AF=0.1;END=5", 3, 4, 6, "SVTYPE=DEL;END=5;NS=3;AN=6;AC=4;AF=0.666667"),
    ("SVTYPE=DEL", 2, 0, 2, "SVTYPE=DEL;NS=2;AN=2;AC=0;AF=0"),                                   # two haploid samples
    ("SVTYPE=DEL", 0, 0, 0, "SVTYPE=DEL;NS=0;AN=0;AC=0"),                                        # AN = 0: no AF
    ("SVTYPE=INS", 64, 200, 512, "SVTYPE=INS;NS=64;AN=512;AC=200;AF=0.390625"),
])
def test_info_with_and_without_an(info, ns, ac, an, want):
    from svjg import genotype
    assert (genotype.cohort_info(info, ns, ac) if an is None else genotype.cohort_info(info, ns, ac, an)) == want
    if an is not None:
        assert genotype.cohort_info(info, ns, ac, an=an) == want


def test_chunk_rows_keep_a_call_under_one_gib():
    from svjg import genotype
    for mp in (1, 2, 8):
        item = 8 * (mp + 1) + 12
        for S in (1, 2, 64, 3000, 10**7, 10**9):
            n = genotype.cohort_chunk_rows(S, mp)
            assert n >= 1 and (n * S * item <= 1 << 30 or n == 1) and (n + 1) * S * item > 1 << 30


# ---- the writer ----

def test_writer_text_of_a_mixed_row(tmp_path):
    """one row over six samples: ploidy 0, a haploid call, a diploid call, a triploid no-call, a diploid item that is not genotyped, a triploid call"""
    from svjg import genotype
    f = tmp_path / "one.vcf"
    f.write_text("\n".join(VCF.split("\n")[:4]) + "\n")
    rows = genotype.VcfRows(str(f), {})
    names = ["s0", "s 1", "s2", "s3", "s4", "s5"]
    ploidy = np.array([[0, 1, 2, 3, 2, 3]], np.uint8)
    done = np.array([[0, 1, 1, 1, 0, 1]], np.uint8)
    gt = np.array([[0xFF, 1, 1, 0xFF, 0xFF, 2]], np.uint8)
    raw = np.array([[[0, 0], [4, 6], [3, 3], [0, 0], [0, 0], [2, 9]]], np.uint32)
    pl = np.zeros((1, 6, 4), np.int64)
    pl[0, 1, :2] = (50, 0)
    pl[0, 2, :3] = (10, 0, 20)
    pl[0, 5] = (90, 30, 0, 40)
    site = np.array([[3, 6, 4]], np.uint32)                       # NS, AN = 1 + 2 + 3, AC = 1 + 1 + 2
    out = tmp_path / "out.vcf"
    assert genotype.write_vcf_cohort(str(out), rows, names, genotype.CohortCalls(gt, pl, raw, done, site), ploidy) == [0, 1, 1, 1, 0, 1]
    lines = out.read_text().split("\n")
    assert lines[-1] == "" and lines[0] == "##fileformat=VCFv4.2"
    assert [ln.split(",")[0] for ln in lines[1:5]] == ["##INFO=<ID=NS", "##INFO=<ID=AN", "##INFO=<ID=AC", "##INFO=<ID=AF"]
    assert [ln.split(",")[0] for ln in lines[5:9]] == ["##FORMAT=<ID=GT", "##FORMAT=<ID=DP", "##FORMAT=<ID=AD", "##FORMAT=<ID=PL"]
    assert lines[8].startswith("##FORMAT=<ID=PL,Number=G,Type=Integer,") and "Number=3" not in out.read_text()
    assert lines[9] == "#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\t" + "\t".join(names)
    assert lines[10] == ("chr1\t100\td1\tN\t<DEL>\t.\tPASS\tSVTYPE=DEL;END=400;NS=3;AN=6;AC=4;AF=0.666667\tGT:DP:AD:PL\t"
                         ".:0:0,0:.\t1:8.0:2.0,6:50,0\t0/1:4.5:1.5,3:10,0,20\t././.:0:0,0:0,0,0,0\t./.:0:0,0:.,.,.\t0/1/1:10.0:1.0,9:90,30,0,40")
    assert len(lines) == 12


# ---- the device leg's integers ----

@pytest.mark.parametrize("max_ploidy", [1, 2, 8])
@pytest.mark.parametrize("S", [1, 3, 64, 65])
@pytest.mark.parametrize("n_rows", [1, 7, 1000])
def test_cohort_ploidy_layout(n_rows, S, max_ploidy):
    L = sim.layout(n_rows, S, max_ploidy, True, False)
    n, npl = n_rows * S, max_ploidy + 1
    assert (L["pl"], L["raw"], L["gt"], L["flags"], L["boundary"]) == (0, 8 * npl * n, 8 * npl * n + 8 * n, 8 * npl * n + 9 * n, 8 * npl * n + 10 * n)
    at = 0
    for name, size, align in [("pl", 8 * npl * n, 8), ("raw", 8 * n, 4), ("gt", n, 1), ("flags", n, 1), ("boundary", n, 1), ("site", 16 * n_rows, 8),
                              ("maxn", 8, 8), ("logtab", 2 * 45 * 8, 8), ("slot", 4 * n_rows, 4), ("type", n_rows, 1), ("ok", n_rows, 1), ("ploidy", n, 1)]:
        assert L[name] >= at, f"{name} overlaps the field in front of it"
        assert L[name] % align == 0, f"{name} at {L[name]} is not {align}-byte aligned"
        at = L[name] + size
    assert at <= L["total"], "the last field ends behind the block"
    assert L["site"] - (L["boundary"] + n) < 8                   # nothing but the alignment in between
    assert L["maxn"] == L["site"] + 16 * n_rows                   # ONE memset zeroes the site words and the max_n pair
    # the inputs are ONE contiguous region right behind the pair: the logarithms, the three row arrays, the ploidy bytes
    assert L["in_at"] == L["maxn"] + 8 == L["logtab"] and L["slot"] == L["logtab"] + 720 and L["type"] == L["slot"] + 4 * n_rows
    assert L["ok"] == L["type"] + n_rows and L["ploidy"] == L["ok"] + n_rows and L["in_bytes"] == 720 + 6 * n_rows + n
    assert L["total"] == L["in_at"] + L["in_bytes"] + 64
    assert L["total"] <= (8 * npl + 12) * n + 22 * n_rows + 808  # the 8 (max_ploidy + 1) + 12 an item the Python side budgets, 22 a row


@pytest.mark.parametrize("S", [1, 2, 3, 31, 63, 64, 65, 130])
def test_site_sums_from_ballots_against_brute_force(S):
    rng = np.random.default_rng(500 + S)
    full = 3 * 64 * S
    for n_items in (full, full - S, (full // S // 2) * S + S):     # (whole rows; the last wave is partial unless 64 divides n_items)
        ploidy = rng.integers(0, 9, n_items).astype(np.uint8)
        gt = rng.integers(0, 9, n_items).astype(np.uint8)
        gt[rng.random(n_items) < 0.25] = 0xFF
        called = gt != 0xFF
        R = n_items // S
        tot = np.zeros((R, 3), np.int64)
        words = np.zeros(R, np.uint64)
        adds = np.zeros(R, np.int64)
        for w0 in range(0, n_items, 64):
            leader, ns, an, ac, word = sim.sums(w0, S, n_items, gt, ploidy)
            mask, seg_leader = sim.wave(w0, S, n_items)              # cohort_segment's own masks
            assert np.array_equal(leader, seg_leader)
            for lane in np.flatnonzero(leader):
                at = w0 + np.array([l for l in range(64) if (int(mask[lane]) >> l) & 1])
                assert at.max() < n_items and len(set((at // S).tolist())) == 1
                c = called[at]
                want = (int(c.sum()), int(ploidy[at][c].sum()), int(gt[at][c].sum()))
                assert (int(ns[lane]), int(an[lane]), int(ac[lane])) == want, (S, n_items, w0, lane)
                assert int(word[lane]) == want[0] | (want[2] << 32)
                r = (w0 + lane) // S
                tot[r] += want
                words[r] += word[lane]
                adds[r] += 1
            off = leader == 0
            assert not ns[off].any() and not an[off].any() and not ac[off].any() and not word[off].any()
        g2, p2, c2 = gt.reshape(R, S).astype(np.int64), ploidy.reshape(R, S).astype(np.int64), called.reshape(R, S)
        want = np.stack([c2.sum(axis=1), np.where(c2, p2, 0).sum(axis=1), np.where(c2, g2, 0).sum(axis=1)], axis=1)
        assert np.array_equal(tot, want)
        assert np.array_equal(words, (want[:, 0] | (want[:, 2] << 32)).astype(np.uint64))
        assert adds.min() >= 1 and adds.max() <= (S + 62) // 64 + 1  # a row of S items lies in at most that many waves


def test_harness_under_the_sanitizers():
    """the stand-alone program (its own main) built with -fsanitize=address,undefined: every wave again, and the layouts"""
    p = subprocess.run([sim.build_main(), "cohort"], capture_output=True, text=True)
    assert p.returncode == 0 and p.stdout.startswith("cohort_sim ok:"), p.stdout + p.stderr
    assert "runtime error" not in p.stderr and "AddressSanitizer" not in p.stderr
