"""Genotypes at any ploidy from 1 to 8, on the CPU: the model of tests/ploidy_model.py against the reference's own answers at ploidy 2;
the kernel's per-row arithmetic (svjg_geno.h: geno_row_ploidy, compiled with g++ by tests/geno_sim) against the model, with the
boundary guard held to its budget; the host recomputation exact_pl_ploidy; the ploidy file; the writer's text."""
import functools

import numpy as np
import pytest

from tests import ploidy_model as PM
from tests import products_items as PI

NO_CALL = 0xFF
N_RANDOM = 24_000                             # 4 000 rows under each of the six (err, min_support) settings
TABLE_N = (1 << 21) + 1024                    # log10(i!) entries: beyond any n = r1 + r2 of the random set (<= 2 * 10^6)

@functools.lru_cache(maxsize=None)
def random_set():
    """rows int64[n, 4] = (type, ref, alt, ploidy); per row the model's (gt, pls) under PM.SETTINGS[r % 6]"""
    rows = PM.random_rows(N_RANDOM)
    want = []
    for r, (t, a, b, p) in enumerate(rows.tolist()):
        e, ms = PM.SETTINGS[r % 6]
        want.append(PM.genotype(t, a, b, p, ms, e))
    return rows, want


@functools.lru_cache(maxsize=None)
def host_table():
    from tests.geno_sim import ploidy as sim
    return sim.logfact_table(TABLE_N)


@functools.lru_cache(maxsize=None)
def harness_on_random_set():
    from tests.geno_sim import ploidy as sim
    rows, _ = random_set()
    n = len(rows)
    gt, pl, near, st = np.zeros(n, np.uint8), np.zeros((n, 9), np.int64), np.zeros(n, np.uint8), np.zeros(n, np.uint8)
    for k, (e, ms) in enumerate(PM.SETTINGS):
        sel = np.arange(k, n, 6)
        gt[sel], pl[sel], near[sel], st[sel] = sim.genotype_rows(rows[sel, 0], rows[sel, 1:3], rows[sel, 3], ms, e, host_table())
    return gt, pl, near, st


def test_model_at_ploidy_2_is_the_reference(golden):
    """all 34 568 rows of lik_kat.npz (the reference's own answers): GT and the three PLs"""
    z = np.load(f"{golden}/lik/lik_kat.npz")
    cases, errs = z["cases"], z["err"]
    assert len(cases) == 34_568
    bad = []
    for c, e in zip(cases.tolist(), errs.tolist()):
        gt, pl = PM.genotype(c[0], c[1], c[2], 2, c[3], e)
        if (3 if gt is None else gt) != c[4] or pl != c[5:8]:
            bad.append((c, gt, pl))
    assert not bad, bad[:5]


def test_row_arithmetic_against_the_model():
    rows, want = random_set()
    assert len(rows) >= 20_000 and set(rows[:, 3]) == set(range(1, 9)) and set(rows[:, 0]) == {0, 1, 2, 3}
    deep = (rows[:, 1:3] > 60).any(axis=1).mean()
    assert 0.08 < deep < 0.12 and rows[:, 1:3].max() > 900_000
    gt, pl, near, st = harness_on_random_set()
    assert not st.any()                                                  # the table holds every row
    n_flagged = PM.check_against_model(rows, want, lambda r: PM.SETTINGS[r % 6], gt, pl, near)
    print("flagged rows:", n_flagged, "of", len(rows))


def test_log_table_is_the_models():
    from tests.geno_sim import ploidy as sim
    for e in (5e-5, 1e-2, 0.3, 0.5, 0.999):
        lr, la = sim.log_table(e)
        for P in range(1, 9):
            for g in range(P + 1):
                w = PM.log_pair(P, g, e)
                assert (lr[P * (P + 1) // 2 + g], la[P * (P + 1) // 2 + g]) == w[:2], (e, P, g)


def test_ploidy_2_equals_the_diploid_routine(golden):
    """geno_row_ploidy at P = 2 against geno_row on the lik_kat rows: gt, three PLs, near — and, geno_row being that routine at the literal
    ploidy 2, both against the fixture's own columns (the reference's answers): GT on every row, the PLs on every row that is not flagged"""
    from tests.geno_sim import ploidy as sim
    z = np.load(f"{golden}/lik/lik_kat.npz")
    cases, errs = z["cases"], z["err"]
    tab = host_table()
    assert int(cases[:, 1:3].sum(axis=1).max()) < len(tab)
    seen = 0
    for e in np.unique(errs):
        for ms in np.unique(cases[:, 3]):
            sel = np.flatnonzero((errs == e) & (cases[:, 3] == ms))
            if not len(sel):
                continue
            c = cases[sel]
            g2, p2, n2, s2 = sim.genotype_rows_diploid(c[:, 0], c[:, 1:3], int(ms), float(e), tab)
            g, p, n, s = sim.genotype_rows(c[:, 0], c[:, 1:3], np.full(len(c), 2), int(ms), float(e), tab)
            assert np.array_equal(np.where(g == NO_CALL, 3, g), g2) and np.array_equal(p[:, :3], p2) and not p[:, 3:].any()
            assert np.array_equal(n, n2) and np.array_equal(s, s2)
            for gt_, pl_, near_ in ((g2, p2, n2), (np.where(g == NO_CALL, 3, g), p[:, :3], n)):
                assert np.array_equal(gt_, c[:, 4]), c[gt_ != c[:, 4]][:5]
                bad = np.flatnonzero((near_ == 0) & (pl_ != c[:, 5:8]).any(axis=1))
                assert len(bad) == 0, (c[bad[:5]], pl_[bad[:5]])
            seen += len(sel)
    assert seen == len(cases)


@pytest.mark.parametrize("kind,P", PI.PLOIDY_CASES)
def test_row_arithmetic_where_the_products_roundings_decide(kind, P):
    """geno_row_ploidy on the rows of lik_products.npz (tests/products_items.py): deep one-sided rows at P = 1, 2, 3, 5, 6, 7, 8 — their binomial
    term is log10(1), so none may be flagged and every PL is the routine's own — and the rows at err = 0.5, where all P + 1 likelihoods
    coincide mathematically and the roundings of the products (and of the reference's 28-digit sums) decide GT, at P = 1, 2, 4, 6, 8"""
    from tests.geno_sim import ploidy as sim
    seen = 0
    for ms, e, rows, want in PI.ploidy_items(kind, P):
        gt, pl, near, st = sim.genotype_rows(rows[:, 0], rows[:, 1:3], rows[:, 3], ms, e, host_table())
        assert not st.any()
        n_flagged = PM.check_against_model(rows, want, lambda r: (e, ms), gt, pl, near)
        assert kind == "half" or n_flagged == 0
        seen += len(rows)
    assert seen == int((PI.one_sided() if kind == "one_sided" else PI.fixture()[2] == "half").sum())


@pytest.mark.parametrize("S", [1, 3])
@pytest.mark.parametrize("kind", ["one_sided", "half"])
def test_cohort_items_where_the_products_roundings_decide(kind, S):
    """geno_row_ploidy on the items of the cohort calls at per-sample ploidy that tests/test_genotype_products_gpu.py hands to
    k_genotype_cohort_ploidy (PI.cohort_ploidy_items: the fixture's rows rotated from sample to sample, ploidy 1 + (r + 3 s) mod 8, every
    11th item off), and, by an exact emulation of a fused product in either order, that the set could fail on the device: under either order at
    least 5 one-sided items at EVERY ploidy 1..8 change a PL or the GT at S = 3, and at least 4 at S = 1 (the ploidy formula and "every 11th
    item off" leave 219 items there, 37 of them sensitive: 4 at ploidies 1, 3 and 6, 5 at the others — 5 at every ploidy cannot be reached by
    one sample); half items at every even ploidy change their GT (at an odd ploidy all P + 1 likelihoods are one value: a tie stays a tie)"""
    from tests.geno_sim import ploidy as sim
    for item in PI.cohort_ploidy_items(kind, S):
        rows = item.rows
        assert len(item.type) * S < 8000 and set(rows[:, 3].tolist()) == set(range(1, 9)) and 0.08 < 1 - item.on.mean() < 0.1
        assert S == 1 or (item.ploidy.min(axis=1) != item.ploidy.max(axis=1)).all()          # ploidies mix within every row
        gt, pl, near, st = sim.genotype_rows(rows[:, 0], rows[:, 1:3], rows[:, 3], item.ms, item.e, host_table())
        assert not st.any()
        n_flagged = PM.check_against_model(rows, item.want, lambda r: (item.e, item.ms), gt, pl, near)
        assert n_flagged == 0 if kind == "one_sided" else n_flagged < 0.01 * len(rows)
        w_gt, w_site = PI.cohort_ploidy_expected(item)
        assert (w_gt[~item.on] == NO_CALL).all() and (w_site[:, 0] <= S).all() and w_site[:, 0].any()
        if kind == "one_sided":
            orders = PI.sensitive_rows(rows, item.want, item.ms, item.e)
            per_p = {P: {o: sum(1 for r, x in enumerate(orders) if rows[r, 3] == P and o in x) for o in PI.ORDERS} for P in range(1, 9)}
            either = {P: sum(1 for r, x in enumerate(orders) if rows[r, 3] == P and x) for P in range(1, 9)}
            print("one_sided, S = %d: sensitive items per ploidy (first, second, either):" % S, [(P, *per_p[P].values(), either[P]) for P in range(1, 9)])
            assert min(min(v.values()) for v in per_p.values()) >= (4 if S == 1 else 5)    # (under either order)
        else:
            orders = PI.sensitive_rows(rows, item.want, item.ms, item.e, gt_only=True)
            per_p = {P: {o: sum(1 for r, x in enumerate(orders) if rows[r, 3] == P and o in x) for o in PI.ORDERS} for P in range(1, 9)}
            print("half, S = %d, min_support %d: items whose GT a fused product changes, per ploidy (first, second):" % (S, item.ms),
                  [(P, *per_p[P].values()) for P in range(1, 9)], "of", len(rows))
            assert all(min(per_p[P].values()) >= 20 for P in (2, 4, 6, 8)) and not any(max(per_p[P].values()) for P in (1, 3, 5, 7))


def test_ties_are_no_calls():
    from tests.geno_sim import ploidy as sim
    tab = host_table()[:4096]
    # INV (type 2): counts are not normalised.  P = 1: ref == alt ties lik_0 and lik_1.  P = 3: 10 / 10 ties g = 1 and g = 2.
    for P, ref, alt in ((1, 7, 7), (3, 10, 10)):
        gt, pl, _, _ = sim.genotype_rows([2], [[ref, alt]], [P], 3, 5e-5, tab)
        assert gt[0] == NO_CALL, (P, gt)
        assert PM.genotype(2, ref, alt, P, 3, 5e-5)[0] is None
    gt, _, _, _ = sim.genotype_rows([2, 2], [[10, 9], [9, 10]], [3, 3], 3, 5e-5, tab)      # next to the tie: a call on either side
    assert gt.tolist() == [1, 2]
    gt, _, _, _ = sim.genotype_rows([2, 2], [[1, 0], [0, 40]], [1, 8], 3, 5e-5, tab)       # below min_support; a clear call
    assert gt.tolist() == [NO_CALL, 8]


def test_harness_under_the_sanitizers():
    """the stand-alone program (its own main) built with -fsanitize=address,undefined: 200 000 seeded rows through geno_row_ploidy and geno_row"""
    import subprocess
    from tests.geno_sim import ploidy as sim
    p = subprocess.run([sim.build_main(), "ploidy"], capture_output=True, text=True)
    assert p.returncode == 0 and p.stdout.startswith("ploidy_sim ok:") and not p.stderr, (p.stdout, p.stderr)


def test_exact_pl_ploidy_is_the_model(golden):
    from svjg import genotype
    rows, want = random_set()
    for r, (t, a, b, p) in enumerate(rows.tolist()):
        assert genotype.exact_pl_ploidy(t, a, b, p, PM.SETTINGS[r % 6][0]) == want[r][1], rows[r]
    z = np.load(f"{golden}/lik/lik_kat.npz")
    for c, e in list(zip(z["cases"].tolist(), z["err"].tolist()))[::7]:
        assert genotype.exact_pl_ploidy(c[0], c[1], c[2], 2, e) == genotype.exact_pl(c[0], c[1], c[2], e), c
    with pytest.raises(ValueError):
        genotype.exact_pl_ploidy(2, 5, 5, 9, 5e-5)


VCF_TEXT = (
    "##fileformat=VCFv4.2\n"
    '##FORMAT=<ID=GT,Number=1,Type=String,Description="old">\n'
    "#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\tSAMPLE\n"
    "chrX\t1000\t.\tN\t<DEL>\t.\tPASS\tSVTYPE=DEL;END=1100\n"
    "chrX\t5000\t.\tN\t<DEL>\t.\tPASS\tSVTYPE=DEL;END=5100\n"
    "chrX\t9000\t.\tN\t<INV>\t.\tPASS\tSVTYPE=INV;END=9100\n"
    "chrM\t10\t.\tN\t<DEL>\t.\tPASS\tSVTYPE=DEL;END=200\n"
    "chr1\t7\t.\tN\t<DEL>\t.\tPASS\tSVTYPE=DEL;END=90\n"
    "chr2\tx7\t.\tN\t" + "ACGT" * 15 + "\t.\tPASS\tSVTYPE=INS\n"            # (an INS row's POS is never read as a number)
)


def _rows(tmp_path):
    from svjg import genotype
    p = tmp_path / "in.vcf"
    p.write_text(VCF_TEXT)
    return genotype.VcfRows(str(p), {})


def test_ploidy_file(tmp_path):
    from svjg import genotype
    f = tmp_path / "ploidy.txt"
    f.write_text("# contig or region, ploidy\n"
                 "\n"
                 "chrX 4000 6000 0\n"                    # a region line ahead of the whole-chromosome line
                 "chrX\t900\t1000\t3\n"
                 "chrX 1000 1000 4\n"                    # matches the first row too: the line above wins
                 "chrX 1\n"
                 "chrX 8\n"                              # never reached
                 "chrM   1\n"
                 "chr2 1 100 5\n")                       # a region line cannot match a POS that is no plain decimal
    regions = genotype.load_ploidy_file(str(f))
    assert regions == [("chrX", 4000, 6000, 0), ("chrX", 900, 1000, 3), ("chrX", 1000, 1000, 4), ("chrX", None, None, 1), ("chrX", None, None, 8),
                       ("chrM", None, None, 1), ("chr2", 1, 100, 5)]
    rows = _rows(tmp_path)
    assert rows.chrom == ["chrX", "chrX", "chrX", "chrM", "chr1", "chr2"] and rows.pos == ["1000", "5000", "9000", "10", "7", "x7"]
    assert genotype.rows_ploidy(rows, None, regions).tolist() == [3, 0, 1, 1, 2, 2]        # unmatched: 2
    assert genotype.rows_ploidy(rows, 6, regions).tolist() == [3, 0, 1, 1, 6, 6]           # unmatched: --ploidy
    assert genotype.rows_ploidy(rows, 4).tolist() == [4] * 6
    for bad in ("chrX\n", "chrX 1 2\n", "chrX 1 2 3 4\n", "chrX two\n", "chrX 10 5 2\n", "chrX 0 5 2\n", "chrX -1\n", "chrX 1.0\n", "chrX 1 x 2\n"):
        f.write_text("chr1 2\n" + bad)
        with pytest.raises(ValueError):
            genotype.load_ploidy_file(str(f))
    f.write_text("chrX 9\n")
    with pytest.raises(ValueError):
        genotype.load_ploidy_file(str(f))
    for bad in (0, 9):
        with pytest.raises(ValueError):
            genotype.rows_ploidy(rows, bad)


class _NoGpu:
    """genotype_with_counts must have read the ploidy file before it asks the device for anything"""
    def genotype_ploidy(self, *a):
        raise AssertionError("the kernel was asked before the ploidy file was read")


def test_bad_ploidy_file_raises_before_any_output(tmp_path):
    from svjg import genotype
    _rows(tmp_path)
    f = tmp_path / "ploidy.txt"
    f.write_text("chrX 9\n")
    out = tmp_path / "out.vcf"
    with pytest.raises(ValueError):
        genotype.genotype_with_counts(_NoGpu(), str(tmp_path / "in.vcf"), {}, str(out), ploidy_file=str(f))
    assert not out.exists()


def test_writer_text(tmp_path):
    from svjg import genotype
    rows = _rows(tmp_path)
    ploidy = np.array([1, 3, 8, 0, 2, 3], np.uint8)
    gt = np.array([1, 2, 0, NO_CALL, NO_CALL, NO_CALL], np.uint8)
    pl = np.zeros((6, 9), np.int64)
    pl[0, :2] = [120, 0]
    pl[1, :4] = [300, 20, 0, 40]
    pl[2] = [0, 11, 22, 33, 44, 55, 66, 77, 88]
    pl[5, :4] = [5, 5, 5, 5]
    raw = np.array([[0, 12], [4, 8], [9, 0], [0, 0], [0, 0], [2, 2]], np.uint32)
    done = np.array([1, 1, 1, 0, 0, 1], np.uint8)
    out = tmp_path / "out.vcf"
    assert genotype.write_vcf_ploidy(str(out), rows, ploidy, gt, pl, raw, done) == 4
    lines = out.read_text().split("\n")
    data = [l.split("\t")[8:] for l in lines if l and not l.startswith("#")]
    assert data == [["GT:DP:AD:PL", "1:12:0,12:120,0"],                               # haploid
                    ["GT:DP:AD:PL", "0/1/1:10.0:2.0,8:300,20,0,40"],                  # P = 3, DEL: the ref count is halved as ever
                    ["GT:DP:AD:PL", "0/0/0/0/0/0/0/0:9:9,0:0,11,22,33,44,55,66,77,88"],
                    ["GT:DP:AD:PL", ".:0:0,0:."],                                     # ploidy 0
                    ["GT:DP:AD:PL", "./.:0:0,0:.,.,."],                               # not genotyped, P = 2
                    ["GT:DP:AD:PL", "././.:3.0:2,1.0:5,5,5,5"]]                       # genotyped, no call, P = 3 (INS: the alt count halved)
    assert genotype.gt_text_ploidy(1, 0) == "0" and genotype.gt_text_ploidy(1, NO_CALL) == "." and genotype.gt_text_ploidy(8, 8) == "/".join("1" * 8)
    assert genotype.gt_text_ploidy(4, 1) == "0/0/0/1"
    done[:] = 0
    ploidy[:] = [1, 3, 8, 0, 2, 3]
    genotype.write_vcf_ploidy(str(out), rows, ploidy, gt, pl, raw, done)
    tails = [l.split("\t")[9] for l in out.read_text().split("\n") if l and not l.startswith("#")]
    assert tails[:3] == [".:0:0,0:.,.", "././.:0:0,0:.,.,.,.", "/".join("." * 8) + ":0:0,0:" + ",".join("." * 9)]


def test_header_says_number_g(tmp_path):
    from svjg import genotype
    rows = _rows(tmp_path)
    n = len(rows.chrom)
    z = np.zeros(n, np.uint8)
    a, b = tmp_path / "a.vcf", tmp_path / "b.vcf"
    genotype.write_vcf(str(a), rows, np.full(n, 3, np.uint8), np.zeros((n, 3), np.int64), np.zeros((n, 2), np.uint32), z)
    genotype.write_vcf_ploidy(str(b), rows, np.full(n, 2, np.uint8), z, np.zeros((n, 9), np.int64), np.zeros((n, 2), np.uint32), z)
    la, lb = a.read_text().split("\n"), b.read_text().split("\n")
    diff = [(x, y) for x, y in zip(la, lb) if x != y]
    assert len(la) == len(lb) and len(diff) == 1
    assert diff[0][0].startswith("##FORMAT=<ID=PL,Number=3,") and diff[0][1] == diff[0][0].replace("Number=3", "Number=G")
    assert sum(l.startswith("##FORMAT=<ID=GT") for l in lb) == 1                      # the input's own FORMAT line is dropped as ever
