"""Insertions that share a position, genotyped together, on the GPU (svjg_genotype_sites, k_genotype_sites) against the model of
tests/site_model.py, and the drop-in script's --joint-ins.  Needs an MI355X: run with -m gpu."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import ploidy_model as PM
from tests import site_model as SM

pytestmark = pytest.mark.gpu

NO_CALL = 0xFF
NONE = 0xFFFFFFFF
AMD = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "svjedi-graph_amd")


@pytest.fixture(scope="module")
def ctx():
    from svjg import capi
    c = capi.Context(0)
    yield c
    c.close()


def _layout(sites):
    """every member a count slot of its own: member s % K of site s holds the site's ref count, the others half of it (the kernel takes the
    maximum) -> (counts[n_slots, 2], slots[n, 6])"""
    counts, slots = [], np.full((len(sites), 6), NONE, np.uint32)
    for s, (ref, alts) in enumerate(sites):
        for j, a in enumerate(alts):
            slots[s, j] = len(counts)
            counts.append((ref if j == s % len(alts) else ref // 2, a))
    return np.array(counts, np.uint32).reshape(-1, 2), slots


def _call(ctx, sites, ms, e):
    counts, slots = _layout(sites)
    ctx.alloc_counts(max(len(counts), 1))
    ctx.set_counts(counts if len(counts) else np.zeros((1, 2), np.uint32))
    return ctx.genotype_sites(slots, ms, e)


def _raw(sites):
    raw = np.zeros((len(sites), 7), np.uint32)
    for s, (ref, alts) in enumerate(sites):
        raw[s, 0], raw[s, 1:len(alts) + 1] = ref, alts
    return raw


def test_mixed_sites_against_the_model(ctx):
    """3 * 256 + 17 sites of the random set in ONE call per (err, min_support): several blocks, a partial last one, K differs from lane to lane;
    then one site and no site"""
    sites = SM.random_sites(6_000)[:3 * 256 + 17]
    assert {len(a) for _, a in sites} == {2, 3, 4, 5, 6} and len({len(a) for _, a in sites[:64]}) == 5
    for e, ms in PM.SETTINGS:
        want = [SM.genotype(ref, alts, ms, e) for ref, alts in sites]
        gt, pl, raw, boundary = _call(ctx, sites, ms, e)
        print("k_genotype_sites, %d sites, err %g, min_support %d: genotype_ms = %.4f" % (len(sites), e, ms, ctx.kernel_ms()[2]))
        assert np.array_equal(raw, _raw(sites))
        SM.check_against_model(sites, want, lambda s: (e, ms), gt, pl, boundary)
    e, ms = PM.SETTINGS[1]
    one = sites[5:6]
    gt, pl, raw, boundary = _call(ctx, one, ms, e)
    SM.check_against_model(one, [SM.genotype(*one[0], ms, e)], lambda s: (e, ms), gt, pl, boundary)
    out = _call(ctx, [], ms, e)
    assert [len(x) for x in out] == [0] * 4 and out[0].shape == (0, 2) and out[1].shape == (0, 28) and out[2].shape == (0, 7)


def test_first_call_grows_the_table_and_flags_the_site_beyond_it():
    """a FRESH context whose first call holds ordinary sites, one with s_K >= 65 536 (the log10(i!) table grows inside the call) and one with
    s_K >= 2^24 (beyond the table's cap: flagged, recomputed on the host)"""
    from svjg import capi, genotype
    sites = SM.random_sites(6_000)[:40]
    sites[7] = (40_000, [60_000, 30_000, 7])               # s_K = 85 004
    sites[23] = (9_000_000, [8_999_999, 12, 7_000_001])    # s_K >= 2^24
    e, ms = 5e-5, 3
    c = capi.Context(0)
    try:
        gt, pl, raw, boundary = _call(c, sites, ms, e)
    finally:
        c.close()
    assert boundary[23] == 1 and np.array_equal(raw, _raw(sites))
    for s, (ref, alts) in enumerate(sites):
        w_call, w_pl = SM.genotype(ref, alts, ms, e)
        assert (int(gt[s, 0]), int(gt[s, 1])) == ((NO_CALL, NO_CALL) if w_call is None else w_call), s
        got = genotype.exact_pl_site(ref, alts, e) if boundary[s] else pl[s, :len(w_pl)].tolist()
        assert got == w_pl and not pl[s, len(w_pl):].any(), (s, sites[s], got, w_pl)


def test_errors(ctx):
    from svjg import capi
    sites = SM.random_sites(6_000)[:8]
    counts, slots = _layout(sites)
    n_slots = len(counts)
    # an ordinary call first: its views and boundary bytes must survive everything below
    rows = PM.random_rows(24_000)[:n_slots]
    ctx.alloc_counts(n_slots)
    ctx.set_counts(rows[:, 1:3].astype(np.uint32))
    views = ctx.genotype(rows[:, 0].astype(np.uint8), np.arange(n_slots, dtype=np.uint32), np.full(n_slots, 3, np.uint8), 3, 5e-5, reuse_outputs=True)
    kept = [np.array(v) for v in views]
    flags = ctx.boundary_flags(n_slots)

    def bad(change):
        s = slots.copy()
        change(s)
        with pytest.raises(capi.SvjgError):
            ctx.genotype_sites(s, 3, 5e-5)

    def one_member(s): s[3, 1:] = NONE
    def no_member(s): s[3, :] = NONE
    def hole(s): s[2, 0], s[2, 1] = NONE, s[2, 0]
    def hole_inside(s): s[1, :4] = (s[1, 0], NONE, s[1, 1], NONE)
    def out_of_range(s): s[5, 1] = n_slots
    def twice(s): s[4, 1] = s[4, 0]
    for change in (one_member, no_member, hole, hole_inside, out_of_range, twice):
        bad(change)
    out = [np.zeros((8, 2), np.uint8), np.zeros((8, 28), np.int64), np.zeros((8, 7), np.uint32), np.zeros(8, np.uint8)]
    for null in range(5):                                  # a null array: the slots, then each output
        args = [slots.ctypes.data] + [x.ctypes.data for x in out]
        args[null] = None
        with pytest.raises(capi.SvjgError):
            ctx._chk(ctx.lib.svjg_genotype_sites(ctx.h, args[0], 8, 3, 5e-5, *args[1:]))
    fresh = capi.Context(0)
    try:
        with pytest.raises(capi.SvjgError):                # no counts yet
            fresh.genotype_sites(slots, 3, 5e-5)
        gt, pl, raw, boundary = _call(fresh, sites, 3, 5e-5)   # the context works afterwards
        assert np.array_equal(raw, _raw(sites))
    finally:
        fresh.close()
    # this context too, on the counts of the ordinary call above (the sites call reads them by slot)
    gt, pl, raw, boundary = ctx.genotype_sites(slots, 3, 5e-5)
    mine = []
    for s, (_, alts) in enumerate(sites):
        m = slots[s, :len(alts)]
        mine.append((int(rows[m, 1].max()), rows[m, 2].tolist()))
    assert np.array_equal(raw, _raw(mine))
    SM.check_against_model(mine, [SM.genotype(ref, alts, 3, 5e-5) for ref, alts in mine], lambda s: (5e-5, 3), gt, pl, boundary)
    assert all(np.array_equal(v, k) for v, k in zip(views, kept)) and np.array_equal(ctx.boundary_flags(n_slots), flags)


# ---- the drop-in script and the fused route on a small VCF of its own ----

INS60, INS70, INS10 = "ACGTAC" * 10, "ACGTACG" * 10, "ACGTACGTAC"
ROWS = [                                         # (CHROM, POS, ALT, INFO, key, ref alignments, alt alignments)
    ("chr1", "100", INS60, "SVTYPE=INS", "chr1:INS-100-1", 0, 40),
    ("chr1", "100", INS70, "SVTYPE=INS", "chr1:INS-100-2", 0, 20),
    ("chr1", "300", "<DEL>", "SVTYPE=DEL;END=420", "chr1:DEL-300-420", 12, 10),
    ("chr1", "100", INS60 + "T", "SVTYPE=INS", "chr1:INS-100-3", 1, 0),
    ("chr2", "100", INS60, "SVTYPE=INS", "chr2:INS-100-4", 9, 17),           # the same POS on another contig: alone there
    ("chr1", "100", INS10, "SVTYPE=INS", "chr1:INS-100-5", 5, 5),            # shorter than 50 bp
]
SITE = [0, 1, 3]
E, MS = 5e-5, 3


@pytest.fixture()
def files(tmp_path):
    vcf, js = tmp_path / "in.vcf", tmp_path / "in_informative_aln.json"
    vcf.write_text("##fileformat=VCFv4.2\n#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\tSAMPLE\n" +
                   "".join("%s\t%s\t.\tN\t%s\t.\tPASS\t%s\n" % r[:4] for r in ROWS))
    js.write_text(json.dumps({r[4]: [["ref%d\n" % k for k in range(r[5])], ["alt%d\n" % k for k in range(r[6])]] for r in ROWS}, indent=4))
    return str(vcf), str(js)


def _expected_tails(joint):
    from svjg import genotype
    call, pls = SM.genotype(max(ROWS[m][5] for m in SITE), [ROWS[m][6] for m in SITE], MS, E)
    assert call == (1, 2)
    tails = []
    for r, (_, _, alt, info, _, ref, a) in enumerate(ROWS):
        if info == "SVTYPE=INS" and len(alt) < 50:
            tails.append(["GT:DP:AD:PL", "./.:0:0,0:.,.,."])
            continue
        t = genotype.TYPE_CODE[info.split(";")[0][7:]]
        dp, ad = genotype._fmt_counts(t, ref, a)
        if joint and r in SITE:
            i = SITE.index(r) + 1
            g, p = SM.project(3, i, call, pls)
            tails.append(["GT:DP:AD:PL:SGT:SAL", "%s:%s:%s:%d,%d,%d:1/2:%d" % (genotype.GT_TEXT[g], dp, ad, *p, i)])
        else:
            g, p = PM.genotype(t, ref, a, 2, MS, E)
            tails.append(["GT:DP:AD:PL", "%s:%s:%s:%d,%d,%d" % (genotype.GT_TEXT[3 if g is None else g], dp, ad, *p)])
    return tails


def _tails(path):
    return [l.split("\t")[8:] for l in open(path).read().split("\n") if l and not l.startswith("#")]


def test_script_with_and_without_joint_ins(files, tmp_path):
    vcf, js = files
    outs = {}
    for name, opts in (("plain", []), ("joint", ["--joint-ins"])):
        out = str(tmp_path / (name + ".vcf"))
        p = subprocess.run([sys.executable, f"{AMD}/predict-genotype.py", "-d", js, "-v", vcf, "--minsupport", str(MS), "-o", out, *opts],
                           capture_output=True, text=True)
        assert p.returncode == 0 and p.stdout == "Genotyped svs: 5\n", (p.stdout, p.stderr)
        outs[name] = out
    plain, joint = _tails(outs["plain"]), _tails(outs["joint"])
    assert plain == _expected_tails(False)
    assert [t[1].split(":")[0] for t in plain[:2]] == ["1/1", "1/1"]         # four alt copies in a diploid
    assert joint == _expected_tails(True)
    assert [t[1].split(":")[0] for t in joint[:2]] == ["0/1", "0/1"] and [plain[k] == joint[k] for k in range(6)] == [False, False, True, False, True, True]
    head = [l for l in open(outs["joint"]).read().split("\n") if l.startswith("##FORMAT")]
    assert [l.split(",")[0] for l in head] == ["##FORMAT=<ID=" + x for x in ("GT", "DP", "AD", "PL", "SGT", "SAL")]


def test_fused_route(files, tmp_path):
    """genotype_with_counts(ctx, ..., joint_ins=True) with the counts set on a context: what svjedi-graph.py --fused --joint-ins calls"""
    from svjg import capi, genotype
    vcf, _ = files
    c = capi.Context(0)
    try:
        c.alloc_counts(len(ROWS))
        c.set_counts(np.array([r[5:7] for r in ROWS], np.uint32))
        slot_of = {r[4]: k for k, r in enumerate(ROWS)}
        out = str(tmp_path / "fused.vcf")
        assert genotype.genotype_with_counts(c, vcf, slot_of, out, MS, E, joint_ins=True) == 5
        assert _tails(out) == _expected_tails(True)
        plain = str(tmp_path / "fused_plain.vcf")
        assert genotype.genotype_with_counts(c, vcf, slot_of, plain, MS, E) == 5
        assert _tails(plain) == _expected_tails(False)
    finally:
        c.close()
