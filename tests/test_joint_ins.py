"""Insertions that share a position, genotyped together (--joint-ins), on the CPU: the model of tests/site_model.py against the reference's
own answers at K = 1; the kernel's per-site arithmetic (svjg_geno.h: geno_site, compiled with g++ by tests/geno_sim) against the model, with
the boundary guard held to its budget; the host recomputation exact_pl_site; how rows are grouped into sites; the projection and the writer's
text; the refusal together with --ploidy."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import ploidy_model as PM
from tests import site_model as SM

NO_CALL = 0xFF
NONE = 0xFFFFFFFF
N_RANDOM = 6_000                              # 1 000 sites under each of the six (err, min_support) settings
TABLE_N = 1 << 17                             # log10(i!) entries: beyond any s_K of the random set (<= 7 * 10 000)
AMD = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "svjedi-graph_amd")


@functools.lru_cache(maxsize=None)
def random_set():
    """sites [(ref, alts)]; per site the model's (call, pls) under PM.SETTINGS[s % 6]"""
    sites = SM.random_sites(N_RANDOM)
    return sites, [SM.genotype(ref, alts, PM.SETTINGS[s % 6][1], PM.SETTINGS[s % 6][0]) for s, (ref, alts) in enumerate(sites)]


@functools.lru_cache(maxsize=None)
def host_table():
    from tests.geno_sim import site as sim
    return sim.logfact_table(TABLE_N)


def test_model_at_k_1_is_the_reference(golden):
    """every INS row of lik_kat.npz (the reference's own answers): GT and the three PLs"""
    z = np.load(f"{golden}/lik/lik_kat.npz")
    seen, bad = 0, []
    for c, e in zip(z["cases"].tolist(), z["err"].tolist()):
        if c[0] != 1:
            continue
        seen += 1
        call, pl = SM.genotype(c[1], [c[2]], c[3], e)
        if (3 if call is None else call[0] + call[1]) != c[4] or pl != c[5:8]:
            bad.append((c, call, pl))
    assert seen > 5_000 and not bad, (seen, bad[:5])


def test_site_arithmetic_against_the_model():
    from tests.geno_sim import site as sim
    sites, want = random_set()
    assert len(sites) >= 6_000 and {len(a) for _, a in sites} == {2, 3, 4, 5, 6}
    deep = np.mean([max([ref] + alts) > 60 for ref, alts in sites])
    assert 0.07 < deep < 0.13 and max(max(alts) for _, alts in sites) > 19_000
    n = len(sites)
    gt, pl, near, st = np.zeros((n, 2), np.uint8), np.zeros((n, 28), np.int64), np.zeros(n, np.uint8), np.zeros(n, np.uint8)
    for k, (e, ms) in enumerate(PM.SETTINGS):
        sel = np.arange(k, n, 6)
        gt[sel], pl[sel], near[sel], st[sel], s_k = sim.genotype_sites([sites[s] for s in sel], ms, e, host_table())
        assert s_k.tolist() == [sum(SM.counts(*sites[s])[1]) for s in sel]
    assert not st.any()                                                  # the table holds every site
    n_flagged = SM.check_against_model(sites, want, lambda s: PM.SETTINGS[s % 6], gt, pl, near)
    print("flagged sites:", n_flagged, "of", n)


@pytest.mark.parametrize("kind", ["one_sided", "half", "searched"])
def test_site_arithmetic_where_the_products_roundings_decide(kind):
    """geno_site on the sites formed from lik_products.npz (tests/products_items.py): one deep count beside zeros at K = 2 and 6 — the chain
    term T is 0, so none may be flagged and every PL is the routine's own — and K = 2 sites at err = 0.5 over the half pairs; and on the
    sites of site_products.npz, found by search (T = 0, none flagged)"""
    from tests import products_items as PI
    from tests.geno_sim import site as sim
    for ms, e, sites, want in PI.site_items(kind):
        assert len(sites) > (25 if kind == "searched" else 500)
        gt, pl, near, st, s_k = sim.genotype_sites(sites, ms, e, host_table())
        assert not st.any() and s_k.tolist() == [sum(SM.counts(*s)[1]) for s in sites]
        n_flagged = SM.check_against_model(sites, want, lambda s: (e, ms), gt, pl, near)
        assert kind == "half" or n_flagged == 0


def test_searched_sites_are_the_models_and_a_fused_product_turns_them():
    """site_products.npz: the stored answers are the model's, recomputed here; every site has one deep count in [2^27, 2^32) beside zeros or
    one raw 1; and, by an exact emulation of a fused multiply-add in either order the compiler may choose (tests/lik_model.py: FUSED_ORDERS),
    for every K in 2..6 and either order at least 20 sites have a PL that the contraction turns — what gives the device tests on this set
    their teeth (tests/test_genotype_products_gpu.py), asserted where no device is needed; all three err values and the product c * L_ok
    (the homozygous PL of the deep allele) take part"""
    from tests import products_items as PI
    z = PI.searched()
    n_by, at, l_ok_turns = {}, 0, 0
    for ms, e, sites, want in PI.site_items("searched"):
        sel = np.flatnonzero(z["err"] == e)
        assert ms == 3 and e in (5e-5, 0.01, 0.3) and len(sel) == len(sites)
        orders = PI.sensitive_sites(sites, want, e)
        for i, (ref, alts), (call, pls), o in zip(sel.tolist(), sites, want, orders):
            K = len(alts)
            v = sorted([ref] + alts)
            assert 2**27 <= v[-1] < 2**32 and v[-2] <= 1 and not any(v[:-2]) and (ref == v[-1] or ref == 0) and not any(SM.chain(ref, alts))
            assert z["K"][i] == K and not z["alt"][i, K:].any() and z["pl"][i, :len(pls)].tolist() == pls and not z["pl"][i, len(pls):].any()
            assert tuple(z["call"][i]) == ((NO_CALL, NO_CALL) if call is None else call)
            assert o and z["orders"][i] == sum(1 << PI.ORDERS.index(x) for x in o)
            for x in o:
                n_by[(K, x)] = n_by.get((K, x), 0) + 1
            d = ([ref] + alts).index(v[-1])
            hom = d * (d + 1) // 2 + d
            l_ok_turns += "first" in o and SM.fused_pls(ref, alts, e, "first")[hom] != pls[hom]
        at += len(sites)
    print("searched sites: %d; sensitive per (K, order):" % at, sorted(n_by.items()), "; c * L_ok turns on", l_ok_turns)
    assert at == len(z["K"]) and sorted(n_by) == [(K, o) for K in range(2, 7) for o in PI.ORDERS] and min(n_by.values()) >= 20
    assert l_ok_turns >= 20


@pytest.mark.parametrize("S", [1, 3])
def test_cohort_site_items_where_the_products_roundings_decide(S):
    """site_item (svjg_geno.h, through tests/geno_sim) over the cohort sites calls that tests/test_genotype_products_gpu.py hands to
    k_genotype_cohort_sites (PI.cohort_site_items): every (site, sample) item is one searched site embedded on a subset of six candidates —
    gt, PLs, raw, members as expected from the model, nothing flagged, no table needed; the set mixes K' within a site, has masks with holes
    and items without a site call inside full waves"""
    from tests import products_items as PI
    from tests.geno_sim import site as sim
    for item in PI.cohort_site_items(S):
        n = len(item.slots)
        assert n == PI.N_COHORT_SITES
        k_of = np.array([bin(int(m)).count("1") for m in item.members.ravel()]).reshape(n, S)
        none = item.site_of < 0
        assert np.array_equal(none, k_of < 2) and 0.1 < none.mean() < 0.15 and none.ravel()[:n * S // 64 * 64].any()
        assert {2, 3, 4, 6} <= set(k_of[~none].tolist()) and (5 in k_of or item.e == 5e-5) and {0, 1} <= set(k_of[none].tolist())      # (at err 5e-5 and K = 5 L_x is -5: no site)
        assert S == 1 or (k_of.min(axis=1) != k_of.max(axis=1)).mean() > 0.8                   # K' differs within a site
        assert 0b100101 in item.members and sum(1 for m in item.members.ravel().tolist() if m & (m + 1)) > n * S // 2       # masks with holes
        gt, pl, raw, boundary, members, st, _, bad = sim.site_items(item.counts.transpose(1, 0, 2), item.present.T, item.slots, item.ms, item.e, host_table()[:16])
        assert not bad.any() and not st.any() and not boundary.any()
        assert np.array_equal(members, item.members) and np.array_equal(gt, item.gt) and np.array_equal(pl, item.pl) and np.array_equal(raw, item.raw)
        assert (item.gt[none] == NO_CALL).all() and not item.pl[none].any() and not item.raw[none].any()


def test_flagged_sites_of_a_large_set():
    """the random set flags about one site in 6 000: the harness alone runs 240 000 more, and the few dozen it flags are held to the model — one
    value within 2 x SITE_PL_GUARD of an integer, the call equal, exact_pl_site equal"""
    from svjg import genotype
    from tests.geno_sim import site as sim
    sites = SM.random_sites(240_000, seed=7)
    e, ms = 5e-5, 3
    gt, pl, near, st, _ = sim.genotype_sites(sites, ms, e, host_table())
    assert not st.any()
    flagged = np.flatnonzero(near)
    assert 10 <= len(flagged) <= 120                                     # 28 values x 5e-6 x 240 000 ~ 34, fewer for small K
    for s in flagged.tolist():
        ref, alts = sites[s]
        fr, nonzero = SM.pl_fractions(ref, alts, e)
        call, want = SM.genotype(ref, alts, ms, e)
        assert nonzero and min(fr) < 2 * SM.SITE_PL_GUARD, (sites[s], fr)
        assert (int(gt[s, 0]), int(gt[s, 1])) == ((NO_CALL, NO_CALL) if call is None else call)
        assert genotype.exact_pl_site(ref, alts, e) == want
        off = [k for k, (x, y) in enumerate(zip(pl[s].tolist(), want)) if x != y]
        assert all(fr[k] < 2 * SM.SITE_PL_GUARD for k in off), (sites[s], off)       # a value may differ only where it sits at an integer


def test_log_table_is_the_models():
    from tests.geno_sim import site as sim
    for e in (5e-5, 1e-2, 0.3, 0.5, 0.999):
        tab = sim.log_table(e)
        for K in range(2, 7):
            assert (tab[0], tab[K], tab[8 + K]) == SM.logs(K, e), (e, K)


def test_table_too_short_and_beyond_the_cap():
    from tests.geno_sim import site as sim
    tab = host_table()[:4096]
    sites = [(10, [20, 20]), (3000, [4000, 0]), (0, [0, 9000]), (0, [9000, 2]), (1 << 24, [0, 2, 0]), (0, [1 << 25, 0, 0, 0, 0, 0])]
    gt, pl, near, st, s_k = sim.genotype_sites(sites, 3, 5e-5, tab)
    #            fits   s_K = 5000: grow   one non-zero count: T = 0, no table   s_K = 4501   at the cap: host   a lone count needs no table
    assert st.tolist() == [0, 1, 0, 1, 2, 0] and near.tolist() == [0, 0, 0, 0, 1, 0]
    assert s_k.tolist() == [30, 5000, 4500, 4501, (1 << 24) + 1, 1 << 24]


def test_known_answers():
    from svjg import genotype
    from tests.geno_sim import site as sim
    tab = host_table()[:4096]
    e, ms = 5e-5, 3
    sites = [(0, [40, 20]), (10, [20, 20]), (0, [40, 0, 0]), (0, [2, 2])]
    gt, pl, near, st, _ = sim.genotype_sites(sites, ms, e, tab)
    assert gt.tolist() == [[1, 2], [NO_CALL, NO_CALL], [1, 1], [NO_CALL, NO_CALL]] and not st.any()
    for s, (ref, alts) in enumerate(sites):
        call, want = SM.genotype(ref, alts, ms, e)
        assert (tuple(gt[s]) if call else call) == call and (near[s] or pl[s, :len(want)].tolist() == want)
        assert genotype.exact_pl_site(ref, alts, e) == want
    # the defect the option removes: each row alone is 1/1, four alt copies in a diploid; together the site is 1/2 and each row 0/1
    assert PM.genotype(1, 0, 40, 2, ms, e)[0] == 2 and PM.genotype(1, 0, 20, 2, ms, e)[0] == 2
    call, pls = SM.genotype(0, [40, 20], ms, e)
    assert call == (1, 2)
    for i in (1, 2):
        g, p = SM.project(2, i, call, pls)
        assert g == 1 and genotype.GT_TEXT[g] == "0/1" and p[1] == min(p)
        assert genotype.project_site(2, i, gt[0], pl[0, :6]) == (g, p)
    # ref 10, alts (20, 20): c = 10, 10, 10 and the three heterozygotes tie
    call, pls = SM.genotype(10, [20, 20], ms, e)
    assert call is None and pls[1] == pls[3] == pls[4] == min(pls)
    # below min_support: a no-call with its PLs present
    call, pls = SM.genotype(0, [2, 2], ms, e)
    assert call is None and len(pls) == 6 and pl[3, :6].tolist() == pls and any(pls)
    assert SM.genotype(0, [2, 2], 2, e)[0] == (1, 2)
    assert genotype.project_site(2, 1, (NO_CALL, NO_CALL), pls) == (3, SM.project(2, 1, None, pls)[1])
    with pytest.raises(ValueError):
        genotype.exact_pl_site(0, [4], e)
    with pytest.raises(ValueError):
        genotype.exact_pl_site(0, [4] * 7, e)


def test_exact_pl_site_is_the_model():
    from svjg import genotype
    sites, want = random_set()
    for s, (ref, alts) in enumerate(sites):
        assert genotype.exact_pl_site(ref, alts, PM.SETTINGS[s % 6][0]) == want[s][1], sites[s]
    deep = (9_000_000, [8_999_999, 12, 7_000_001])                       # s_K beyond 2^24: the product's Stirling path against mpmath's
    assert genotype.exact_pl_site(*deep, 5e-5) == SM.genotype(*deep, 3, 5e-5)[1]


# ---- grouping, projection, writer: the host logic with a stand-in context that answers from the models ----

INS60, INS70, INS10 = "ACGTAC" * 10, "ACGTACG" * 10, "ACGTACGTAC"
_ROWS = [                                        # (CHROM, POS, ALT, INFO, key in the edge table or None, (ref, alt))
    ("chr1", "100", INS60, "SVTYPE=INS", "chr1:INS-100-1", (0, 40)),          # site X, allele 1
    ("chr1", "500", "<DEL>", "SVTYPE=DEL;END=600", "chr1:DEL-500-600", (12, 10)),
    ("chr1", "100", INS70, "SVTYPE=INS", "chr1:INS-100-2", (0, 20)),          # site X, allele 2: not adjacent to allele 1
    ("chr2", "100", INS60, "SVTYPE=INS", "chr2:INS-100-3", (9, 18)),          # the same POS on another contig: site Y
    ("chr2", "100", INS70, "SVTYPE=INS", "chr2:INS-100-4", (10, 0)),
    ("chr1", "100", INS10, "SVTYPE=INS", "chr1:INS-100-5", (5, 5)),           # shorter than 50 bp: never genotyped, never a member
    ("chr1", "100", INS60, "SVTYPE=INS", None, (0, 0)),                       # no key: never genotyped, never a member
    ("chr1", "100", INS60 + "A", "SVTYPE=INS", "chr1:INS-100-7", (3, 0)),     # site X, allele 3
    ("chr3", "700", INS60, "SVTYPE=INS", "chr3:INS-700-1", (0, 30)),          # a position left with ONE member: the independent call
    ("chr3", "700", INS10, "SVTYPE=INS", "chr3:INS-700-2", (4, 4)),
] + [("chr4", "900", INS60 + "C" * k, "SVTYPE=INS", "chr4:INS-900-%d" % (k + 1), (2, 6 + 2 * k)) for k in range(7)]   # seven: the fallback
VCF_TEXT = ("##fileformat=VCFv4.2\n"
            '##FORMAT=<ID=GT,Number=1,Type=String,Description="old">\n'
            "#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\tSAMPLE\n" +
            "".join("%s\t%s\t.\tN\t%s\t.\tPASS\t%s\n" % r[:4] for r in _ROWS))
KEYS = [r[4] for r in _ROWS if r[4]]
COUNTS = np.array([r[5] for r in _ROWS if r[4]], np.uint32)
E, MS = 5e-5, 3


class ModelCtx:
    """stands in for capi.Context: answers genotype() from tests/ploidy_model at ploidy 2 and genotype_sites() from tests/site_model"""
    def __init__(self, counts):
        self.counts, self.site_calls = counts, []

    def _gate(self, slot, ok):
        return bool(ok & 1) and slot != NONE and ((ok & 2) or self.counts[slot].any())

    def genotype(self, sv_type, slot, ok, min_support, err, reuse_outputs=False):
        n = len(sv_type)
        gt, pl, raw, done = np.full(n, 3, np.uint8), np.zeros((n, 3), np.int64), np.zeros((n, 2), np.uint32), np.zeros(n, np.uint8)
        for r in range(n):
            if self._gate(int(slot[r]), int(ok[r])):
                raw[r] = self.counts[slot[r]]
                g, pl[r] = PM.genotype(int(sv_type[r]), int(raw[r, 0]), int(raw[r, 1]), 2, min_support, err)
                gt[r], done[r] = 3 if g is None else g, 1
        return gt, pl, raw, done

    def boundary_flags(self, n):
        return np.zeros(n, np.uint8)

    def genotype_sites(self, slots, min_support, err):
        self.site_calls.append(np.array(slots))
        n = len(slots)
        gt, pl, raw = np.full((n, 2), NO_CALL, np.uint8), np.zeros((n, 28), np.int64), np.zeros((n, 7), np.uint32)
        for s in range(n):
            m = [int(x) for x in slots[s] if x != NONE]
            raw[s, 0], raw[s, 1:len(m) + 1] = self.counts[m, 0].max(), self.counts[m, 1]
            call, pls = SM.genotype(int(raw[s, 0]), raw[s, 1:len(m) + 1].tolist(), min_support, err)
            pl[s, :len(pls)] = pls
            if call:
                gt[s] = call
        return gt, pl, raw, np.zeros(n, np.uint8)


@pytest.fixture()
def joint_run(tmp_path, capsys, monkeypatch):
    """(plain output lines, --joint-ins output lines, the stand-in context, stderr of the joint run, both returned counts)"""
    from svjg import genotype
    monkeypatch.setenv("SVJG_PY_VCF", "1")
    vcf = tmp_path / "in.vcf"
    vcf.write_text(VCF_TEXT)
    slot_of = {k: i for i, k in enumerate(KEYS)}
    n_plain = genotype.genotype_with_counts(ModelCtx(COUNTS), str(vcf), slot_of, str(tmp_path / "plain.vcf"), MS, E)
    capsys.readouterr()
    ctx = ModelCtx(COUNTS)
    n_joint = genotype.genotype_with_counts(ctx, str(vcf), slot_of, str(tmp_path / "joint.vcf"), MS, E, joint_ins=True)
    return ((tmp_path / "plain.vcf").read_text().split("\n"), (tmp_path / "joint.vcf").read_text().split("\n"), ctx, capsys.readouterr().err,
            (n_plain, n_joint))


def test_grouping(joint_run):
    _, _, ctx, err, _ = joint_run
    assert len(ctx.site_calls) == 1                                      # ONE call for all sites
    slot = {k: i for i, k in enumerate(KEYS)}
    x = [slot["chr1:INS-100-1"], slot["chr1:INS-100-2"], slot["chr1:INS-100-7"], NONE, NONE, NONE]      # file order, not adjacent; rows 5 and 6 excluded
    y = [slot["chr2:INS-100-3"], slot["chr2:INS-100-4"], NONE, NONE, NONE, NONE]                        # the same POS, another contig
    assert ctx.site_calls[0].tolist() == [x, y]                          # chr3:700 has one member, chr4:900 seven: neither is a site
    lines = [l for l in err.split("\n") if l]
    assert len(lines) == 1 and "chr4:900" in lines[0] and "7" in lines[0]


def test_form_sites_takes_up_to_six(tmp_path):
    from svjg import genotype
    vcf = tmp_path / "in.vcf"
    vcf.write_text(VCF_TEXT)
    rows = genotype.VcfRows(str(vcf), {k: i for i, k in enumerate(KEYS)})
    done = np.ones(len(_ROWS), np.uint8)
    done[[5, 6, 9, 16]] = 0                                              # chr4:900 left with six genotyped rows
    sites, skipped = genotype.form_sites(rows, done)
    assert sites == [[0, 2, 7], [3, 4], [10, 11, 12, 13, 14, 15]] and skipped == []
    done[16] = 1
    sites, skipped = genotype.form_sites(rows, done)
    assert sites == [[0, 2, 7], [3, 4]] and skipped == [("chr4", "900", 7)]


def test_output_against_the_models(joint_run):
    """every data row of the --joint-ins output: members carry the site call's projection, everything else the independent call"""
    from svjg import genotype
    plain, joint, _, _, counts = joint_run
    assert counts == (14, 14)                                            # `Genotyped svs:` is unchanged
    data = [l.split("\t") for l in joint if l and not l.startswith("#")]
    assert len(data) == len(_ROWS)
    site_of = {0: ([0, 2, 7], 1), 2: ([0, 2, 7], 2), 7: ([0, 2, 7], 3), 3: ([3, 4], 1), 4: ([3, 4], 2)}
    for r, cols in enumerate(data):
        chrom, pos, alt, info, key, (ref, a) = _ROWS[r]
        assert cols[:8] == [chrom, pos, ".", "N", alt, ".", "PASS", info]
        if key is None or (info == "SVTYPE=INS" and len(alt) < 50):
            assert cols[8:] == ["GT:DP:AD:PL", "./.:0:0,0:.,.,."]
            continue
        t = genotype.TYPE_CODE[info.split(";")[0][7:]]
        dp, ad = genotype._fmt_counts(t, ref, a)
        if r in site_of:
            members, i = site_of[r]
            call, pls = SM.genotype(max(_ROWS[m][5][0] for m in members), [_ROWS[m][5][1] for m in members], MS, E)
            g, p = SM.project(len(members), i, call, pls)
            sgt = "./." if call is None else "%d/%d" % call
            assert cols[8:] == ["GT:DP:AD:PL:SGT:SAL", "%s:%s:%s:%d,%d,%d:%s:%d" % ("./." if g is None else genotype.GT_TEXT[g], dp, ad, *p, sgt, i)], cols
        else:
            g, p = PM.genotype(t, ref, a, 2, MS, E)
            assert cols[8:] == ["GT:DP:AD:PL", "%s:%s:%s:%d,%d,%d" % (genotype.GT_TEXT[3 if g is None else g], dp, ad, *p)], cols
    assert data[0][9].split(":")[0] == "0/1" and data[0][9].endswith(":1/2:1") and data[2][9].split(":")[0] == "0/1" and data[2][9].endswith(":1/2:2")
    assert data[7][9].split(":")[0] == "0/0" and data[7][9].endswith(":1/2:3")
    assert [l.split("\t")[9].split(":")[0] for l in plain if l and not l.startswith("#")][:3:2] == ["1/1", "1/1"]      # what the plain run says there


def test_only_members_and_the_header_differ(joint_run):
    plain, joint, _, _, _ = joint_run
    at = next(k for k, l in enumerate(plain) if l.startswith("##FORMAT=<ID=PL,"))
    assert joint[:at + 1] == plain[:at + 1] and joint[at + 3:] != plain[at + 1:]
    assert joint[at + 1].startswith("##FORMAT=<ID=SGT,Number=1,Type=String,Description=") and joint[at + 1].endswith('">')
    assert joint[at + 2].startswith("##FORMAT=<ID=SAL,Number=1,Type=Integer,Description=") and joint[at + 2].endswith('">')
    rest_p, rest_j = plain[at + 1:], joint[at + 3:]
    assert len(rest_p) == len(rest_j) and rest_p[0] == rest_j[0] and rest_p[0].startswith("#CHROM")
    differ = [k - 1 for k, (a, b) in enumerate(zip(rest_p, rest_j)) if a != b]
    assert differ == [0, 2, 3, 4, 7]                                     # the five member rows, by data row
    assert sum(l.startswith("##FORMAT=<ID=GT") for l in joint) == 1      # the input's own FORMAT line is dropped as ever


def test_writer_text(tmp_path):
    from svjg import genotype
    vcf = tmp_path / "in.vcf"
    vcf.write_text(VCF_TEXT)
    rows = genotype.VcfRows(str(vcf), {})
    n = len(_ROWS)
    gt, pl, raw, done = np.full(n, 3, np.uint8), np.zeros((n, 3), np.int64), np.zeros((n, 2), np.uint32), np.zeros(n, np.uint8)
    done[[0, 1, 2, 3]] = 1
    raw[0], raw[1], raw[2], raw[3] = (0, 41), (12, 10), (0, 20), (7, 7)
    gt[1], pl[1] = 1, (90, 0, 70)
    gt[3], pl[3] = 1, (5, 0, 6)
    member = {0: (1, [301, 0, 299], "1/2", 1), 2: (3, [4, 5, 6], "./.", 2)}
    out = tmp_path / "out.vcf"
    assert genotype.write_vcf_joint(str(out), rows, gt, pl, raw, done, member) == 4
    data = [l.split("\t")[8:] for l in out.read_text().split("\n") if l and not l.startswith("#")]
    assert data[:5] == [["GT:DP:AD:PL:SGT:SAL", "0/1:20.5:0,20.5:301,0,299:1/2:1"],           # DP / AD: the row's own, the alt count halved as ever
                        ["GT:DP:AD:PL", "0/1:16.0:6.0,10:90,0,70"],
                        ["GT:DP:AD:PL:SGT:SAL", "./.:10.0:0,10.0:4,5,6:./.:2"],                   # a no-call site prints its PLs beside ./.
                        ["GT:DP:AD:PL", "0/1:10.5:7,3.5:5,0,6"],                                  # genotyped INS outside any site: as ever
                        ["GT:DP:AD:PL", "./.:0:0,0:.,.,."]]
    assert genotype.project_site(2, 1, (1, 2), [60, 50, 40, 30, 0, 20]) == (1, [20, 0, 40])
    assert genotype.project_site(2, 2, (1, 2), [60, 50, 40, 30, 0, 20]) == (1, [40, 0, 20])
    assert genotype.project_site(3, 3, (0, 0), list(range(10))) == (0, [0, 6, 9])
    assert genotype.project_site(2, 2, (2, 2), [9, 8, 7, 6, 5, 0]) == (2, [7, 5, 0])
    assert genotype.site_genotypes(2) == [(0, 0), (0, 1), (1, 1), (0, 2), (1, 2), (2, 2)]


class _NoGpu:
    """genotype_with_counts must refuse the combination before it asks the device for anything"""
    def __getattr__(self, name):
        raise AssertionError("the context was asked for %s before the options were checked" % name)


@pytest.mark.parametrize("extra", [{"ploidy": 2}, {"ploidy_file": "ploidy.txt"}])
def test_joint_ins_with_ploidy_is_refused_before_any_output(tmp_path, extra):
    from svjg import genotype
    (tmp_path / "in.vcf").write_text(VCF_TEXT)
    out = tmp_path / "out.vcf"
    with pytest.raises(ValueError) as ei:
        genotype.genotype_with_counts(_NoGpu(), str(tmp_path / "in.vcf"), {}, str(out), joint_ins=True, **extra)
    assert "--joint-ins" in str(ei.value) and "--ploidy" in str(ei.value) and not out.exists()
    with pytest.raises(ValueError):
        genotype.run(str(tmp_path / "none.json"), str(tmp_path / "in.vcf"), str(out), joint_ins=True, **extra)
    assert not out.exists()


@pytest.mark.parametrize("script, args", [("predict-genotype.py", ["-d", "none.json", "-v", "in.vcf", "-o", "out.vcf"]),
                                          ("svjedi-graph.py", ["-v", "in.vcf", "-r", "ref.fa", "-q", "reads.fq", "-p", "out"])])
def test_scripts_refuse_joint_ins_with_ploidy(tmp_path, script, args):
    (tmp_path / "in.vcf").write_text(VCF_TEXT)
    for extra in (["--ploidy", "2"], ["--ploidy-file", "ploidy.txt"]):
        p = subprocess.run([sys.executable, os.path.join(AMD, script), *args, "--joint-ins", *extra], capture_output=True, text=True, cwd=tmp_path)
        assert p.returncode != 0 and "--joint-ins" in p.stderr and "--ploidy" in p.stderr
        assert sorted(os.listdir(tmp_path)) == ["in.vcf"]               # no output file of any kind
