"""Cohort genotyping without a GPU: the cohort list, the union of the samples' keys, the INFO rewrite, the multi-sample writer fed with the
reference's per-sample columns (tests/golden/cohort/, tests/cohort_model.py), and the two integer pieces of the device leg compiled with
g++ (tests/geno_sim: cohort_layout, cohort_segment)."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests import cohort_model as CM      # noqa: E402
from tests.geno_sim import cohort as sim  # noqa: E402


# ---- the cohort list ----

def test_list_good_lines_and_relative_paths(tmp_path):
    from svjg import genotype
    sub = tmp_path / "lists"
    sub.mkdir()
    f = sub / "c.list"
    f.write_text("# a comment\n\nA\ta.json\nB b\t../x/b.json\r\nC\t/abs/c.json\n#D\td.json\n")
    assert genotype.load_cohort_list(str(f)) == [("A", str(sub / "a.json")), ("B b", os.path.join(str(sub), "../x/b.json")), ("C", "/abs/c.json")]


@pytest.mark.parametrize("text, line", [("A\ta.json\nB\n", 2), ("A\ta.json\tmore\n", 1), ("\ta.json\n", 1), ("A\t\n", 1),
                                        ("A a.json\n", 1), ("A\ta.json\n# c\nA\tb.json\n", 3)])
def test_list_bad_lines_name_file_and_line(tmp_path, text, line):
    from svjg import genotype
    f = tmp_path / "bad.list"
    f.write_text(text)
    with pytest.raises(ValueError) as ei:
        genotype.load_cohort_list(str(f))
    assert "%s:%d:" % (f, line) in str(ei.value)


def test_list_without_a_sample(tmp_path):
    from svjg import genotype
    f = tmp_path / "empty.list"
    f.write_text("# nobody\n\n")
    with pytest.raises(ValueError) as ei:
        genotype.load_cohort_list(str(f))
    assert str(f) in str(ei.value)


# ---- the union of the samples' keys ----

def test_union_first_seen_order_and_last_wins():
    from svjg import genotype
    a = (["k1", "k2", "k1"], np.array([[1, 2], [3, 4], [5, 6]], np.uint32))          # k1 twice: the last one wins
    b = (["k3", "k2"], np.array([[7, 8], [0, 0]], np.uint32))
    c = ([], np.zeros((0, 2), np.uint32))
    keys, per = genotype.cohort_union([a, b, c])
    assert keys == ["k1", "k2", "k3"]
    got = [dict(zip(s.tolist(), map(tuple, cnt.tolist()))) for s, cnt in per]
    assert got == [{0: (5, 6), 1: (3, 4)}, {2: (7, 8), 1: (0, 0)}, {}]
    assert all(s.dtype == np.uint32 and cnt.dtype == np.uint32 and len(set(s.tolist())) == len(s) for s, cnt in per)


# ---- INFO ----

@pytest.mark.parametrize("info, ns, ac, want", [
    (".", 3, 2, "NS=3;AN=6;AC=2;AF=0.333333"),
    ("SVTYPE=DEL;END=5", 4, 8, "SVTYPE=DEL;END=5;NS=4;AN=8;AC=8;AF=1"),
    ("AC=9;SVTYPE=DEL;END=5", 1, 1, "SVTYPE=DEL;END=5;NS=1;AN=2;AC=1;AF=0.5"),                   # an existing tag first,
    ("SVTYPE=DEL;AF=0.1;END=5", 2, 0, "SVTYPE=DEL;END=5;NS=2;AN=4;AC=0;AF=0"),                   # in the middle,
    ("SVTYPE=DEL;END=5;NS=7", 2, 1, "SVTYPE=DEL;END=5;NS=2;AN=4;AC=1;AF=0.25"),                  # last,
    ("NS=1;AN=2;AC=1;AF=0.5", 0, 0, "NS=0;AN=0;AC=0"),                                           # all of them, and AN = 0: no AF
    ("SVTYPE=DEL;ANN=x;MAC=3;NSAMP=2;AFR=1", 0, 0, "SVTYPE=DEL;ANN=x;MAC=3;NSAMP=2;AFR=1;NS=0;AN=0;AC=0"),   # whole fields, exact key
    ("SVTYPE=INS", 64, 1, "SVTYPE=INS;NS=64;AN=128;AC=1;AF=0.0078125"),
    ("SVTYPE=INS", 3000, 1, "SVTYPE=INS;NS=3000;AN=6000;AC=1;AF=0.000166667"),
])
def test_info_rewrite(info, ns, ac, want):
    from svjg import genotype
    assert genotype.cohort_info(info, ns, ac) == want


def test_chunk_rows_keep_a_call_under_one_gib():
    from svjg import genotype
    for S in (1, 2, 64, 3000, 10**7, 10**9):
        n = genotype.cohort_chunk_rows(S)
        assert n >= 1 and (n * S * 37 <= 1 << 30 or n == 1) and (n + 1) * S * 37 > 1 << 30


# ---- the writer, fed with the reference's per-sample columns ----

@pytest.mark.parametrize("which", ["plain", "edited"])
def test_writer_against_the_reference_columns(golden, tmp_path, which):
    co = CM.Cohort(golden, which)
    assert co.names == (["S1", "S2", "S3", "S4"] if which == "plain" else ["E1", "E2", "E3", "E4"])
    out = str(tmp_path / "merged.vcf")
    assert co.assemble(out) == co.genotyped                       # the reference's `Genotyped svs` numbers
    lines = open(out).read().split("\n")
    assert lines[-1] == ""
    head = [ln for ln in lines if ln.startswith("#")]
    ref_head = [ln for ln in co.ref_lines[0] if ln.startswith("#")]
    # the reference's header with the four INFO lines in front of the FORMAT lines and the sample names in the column line
    at = next(i for i, ln in enumerate(head) if ln.startswith("##FORMAT"))
    assert [ln.split(",")[0] for ln in head[at - 4:at]] == ["##INFO=<ID=NS", "##INFO=<ID=AN", "##INFO=<ID=AC", "##INFO=<ID=AF"]
    assert head[:at - 4] + head[at:-1] == ref_head[:-1]
    assert ref_head[-1].endswith("\tFORMAT\tSAMPLE") and head[-1] == ref_head[-1][:-len("SAMPLE")] + "\t".join(co.names)
    data = [ln.split("\t") for ln in lines if ln and not ln.startswith("#")]
    inp = [ln.split("\t") for ln in open(co.vcf).read().split("\n") if ln and not ln.startswith("#")]
    assert len(data) == len(inp) == 40
    for r, (got, src) in enumerate(zip(data, inp)):
        assert got[:7] == src[:7] and got[8] == "GT:DP:AD:PL" and len(got) == 9 + len(co.names)
        gts = []
        for s in range(len(co.names)):
            assert got[9 + s] == co.ref_data[s][r][9], (r, s)     # column s IS the reference's SAMPLE column for sample s
            assert co.ref_data[s][r][:8] == src[:8]
            gts.append(co.ref_data[s][r][9].split(":")[0])
        ns = sum(g != "./." for g in gts)
        ac = sum(g.count("1") for g in gts if g != "./.")
        fields = got[7].split(";")
        kept = [f for f in src[7].split(";") if f.split("=")[0] not in ("NS", "AN", "AC", "AF")]
        tags = ["NS=%d" % ns, "AN=%d" % (2 * ns), "AC=%d" % ac] + (["AF=%s" % ("%.6g" % (ac / (2 * ns)))] if ns else [])
        assert fields == kept + tags, r
    if which == "plain":                                          # sample 1 is the testdir's JSON at full depth
        exp = [ln.split("\t") for ln in open(f"{golden}/testdir/expected_genotype.vcf").read().split("\n") if ln and not ln.startswith("#")]
        assert [d[9] for d in data] == [e[9] for e in exp]
    else:
        e = co.manifest["edits"]
        row_of = {co.keys[sl]: r for r, sl in enumerate(co.rows.slot) if sl != 0xFFFFFFFF}
        assert data[row_of[e["deleted_from_sample_2"]]][9 + 1] == "./.:0:0,0:.,.,."
        assert data[row_of[e["empty_lists_in_sample_3"]]][9 + 2] == "./.:0:0,0:0,0,0"             # genotyped, with no alignment
        only4 = data[row_of[e["only_in_sample_4"]]][9:]
        assert only4[:3] == ["./.:0:0,0:.,.,."] * 3 and only4[3] != "./.:0:0,0:.,.,."
        tagged = next(d for d in data if d[2] == e["vcf_row_with_site_tags"]["id"])
        assert tagged[7].count("AC=") == 1 and tagged[7].count("AF=") == 1 and "AC=7" not in tagged[7].split(";")


# ---- the device leg's integers ----

@pytest.mark.parametrize("n_rows, S", [(0, 1), (1, 1), (1, 65), (257, 3), (1000, 130)])
def test_cohort_layout(n_rows, S):
    full = sim.layout(n_rows, S, 2, False, False)                 # the one layout at max_ploidy 2, neither switch
    assert not any(full[k] for k in ("gq", "af", "psite", "steps", "logtab")) and full["slot"] == full["in_at"] and full["ploidy"] == full["ok"] + n_rows
    L = {k: full[k] for k in ("pl", "raw", "gt", "flags", "boundary", "site", "maxn", "slot", "type", "ok", "in_bytes", "total")}
    n = n_rows * S
    site = (35 * n + 7) & ~7
    maxn = site + 8 * n_rows
    assert L == {"pl": 0, "raw": 24 * n, "gt": 32 * n, "flags": 33 * n, "boundary": 34 * n, "site": site, "maxn": maxn,
                 "slot": maxn + 8, "type": maxn + 8 + 4 * n_rows, "ok": maxn + 8 + 5 * n_rows, "in_bytes": 6 * n_rows, "total": maxn + 8 + 6 * n_rows + 64}
    at = 0
    for name, off, size, align in [("pl", L["pl"], 24 * n, 8), ("raw", L["raw"], 8 * n, 4), ("gt", L["gt"], n, 1), ("flags", L["flags"], n, 1),
                                   ("boundary", L["boundary"], n, 1), ("site", L["site"], 8 * n_rows, 8), ("maxn", L["maxn"], 8, 8),
                                   ("slot", L["slot"], 4 * n_rows, 4), ("type", L["type"], n_rows, 1), ("ok", L["ok"], n_rows, 1)]:
        assert off >= at, f"{name} overlaps the field in front of it"
        assert off % align == 0, f"{name} at {off} is not {align}-byte aligned"
        at = off + size
    assert at <= L["total"], "the last field ends behind the block"
    assert L["maxn"] == L["site"] + 8 * n_rows                    # ONE memset zeroes the site words and the max_n pair
    assert L["total"] <= 35 * n + 14 * n_rows + 80                # 35 bytes an item, 14 a row: the 37 an item the Python side budgets, from S = 7 on


@pytest.mark.parametrize("S", [1, 2, 3, 31, 63, 64, 65, 130])
def test_segment_mask_is_the_set_of_lanes_with_the_same_row(S):
    full = 3 * 64 * S
    lanes = np.arange(64, dtype=np.uint64)
    for n_items in (full, full - S, (full // S // 2) * S + S):     # (whole rows; the last wave is partial unless 64 divides n_items)
        for w0 in range(0, n_items, 64):
            mask, leader = sim.wave(w0, S, n_items)
            items = np.uint64(w0) + lanes
            inside = items < np.uint64(n_items)
            row = items // np.uint64(S)
            same = (row[:, None] == row[None, :]) & inside[:, None] & inside[None, :]            # brute force: [lane, other lane]
            want = (same.astype(np.uint64) << lanes[None, :]).sum(axis=1, dtype=np.uint64)
            assert np.array_equal(mask, want), (S, n_items, w0)
            assert not mask[~inside].any() and not leader[~inside].any()                         # beyond the last item: no segment
            first = np.array([np.flatnonzero(same[l])[0] if inside[l] else 64 for l in range(64)])
            assert np.array_equal(leader != 0, first == np.arange(64)), (S, n_items, w0)
            # exactly one leader per (wave, row) segment
            assert int(leader.sum()) == len(np.unique(row[inside]))



@pytest.mark.parametrize("S", [1, 2, 3, 31, 63, 64, 65, 130])
def test_diploid_site_sums_from_the_leaders_against_brute_force(S):
    """k_genotype_cohort's three ballots (called, het, hom; gt 3 = no call) under cohort_segment's masks: NS and AC of every row, summed over its
    segments' leaders, are the brute-force counts, and the word a leader adds is NS | AC << 32"""
    rng = np.random.default_rng(700 + S)
    full = 3 * 64 * S
    for n_items in (full, full - S, (full // S // 2) * S + S):     # (the segment test's waves)
        gt = rng.integers(0, 4, n_items).astype(np.uint8)          # 0, 1, 2, no call
        R = n_items // S
        tot, words = np.zeros((R, 2), np.int64), np.zeros(R, np.uint64)
        for w0 in range(0, n_items, 64):
            leader, ns, an, ac, word = sim.sums(w0, S, n_items, gt)
            assert np.array_equal(leader, sim.wave(w0, S, n_items)[1]) and np.array_equal(an, 2 * ns)
            assert np.array_equal(word, ns.astype(np.uint64) | (ac.astype(np.uint64) << np.uint64(32)))
            off = leader == 0
            assert not ns[off].any() and not ac[off].any() and not word[off].any()
            r = (w0 + np.flatnonzero(leader)) // S
            np.add.at(tot, r, np.stack([ns[leader != 0], ac[leader != 0]], axis=1))
            np.add.at(words, r, word[leader != 0])
        g2 = gt.reshape(R, S).astype(np.int64)
        want = np.stack([(g2 != 3).sum(axis=1), np.where(g2 != 3, g2, 0).sum(axis=1)], axis=1)
        assert np.array_equal(tot, want), (S, n_items)
        assert np.array_equal(words, (want[:, 0] | (want[:, 1] << 32)).astype(np.uint64))
