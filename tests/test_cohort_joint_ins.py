"""Cohort calls for insertions that share a position (--cohort LIST --joint-ins), on the CPU: the plain pieces of the device leg compiled with
g++ (tests/geno_sim: the member compaction, the site sums under cohort_segment's masks, the layout, and geno_site behind the compaction
against tests/site_model.py on the present members); the host flow with a stand-in context that answers from the models — grouping, the ONE
sites call, every column against the single-sample --joint-ins run of that sample, the site tags, the header; the golden cohort; the refusals."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import ploidy_model as PM
from tests import site_model as SM
from tests.geno_sim import site as sim
from tests.test_joint_ins import _ROWS, KEYS, COUNTS, VCF_TEXT, ModelCtx

NO_CALL = 0xFF
NONE = 0xFFFFFFFF
AMD = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "svjedi-graph_amd")
SIZES = [1, 2, 3, 31, 63, 64, 65, 130]
E, MS = 5e-5, 3


# ---- the harness: integer pieces ----

def test_compaction_of_every_presence_pattern():
    rng = np.random.default_rng(11)
    for bits in range(64):
        for _ in range(4):
            cref, calt = rng.integers(0, 1000, 6), rng.integers(1, 1000, 6)
            at = [j for j in range(6) if bits >> j & 1]
            K, ref, alt = sim.compact(bits, cref, calt)
            assert K == len(at) and ref == (max(cref[at]) if at else 0) and alt == calt[at].tolist() + [0] * (6 - len(at)), (bits, cref, calt)


def _random_items(rng, n_items, S):
    """members and calls as the kernel may leave them: 2..6 candidates a site, each present with probability 0.7; K' >= 2: a call in 7 of 8"""
    cand = 2 + (np.arange(n_items) // S) % 5
    bits = (rng.random((n_items, 6)) < 0.7) & (np.arange(6)[None, :] < cand[:, None])
    members = (bits << np.arange(6)).sum(axis=1).astype(np.uint8)
    K = bits.sum(axis=1)
    gt = np.full((n_items, 2), NO_CALL, np.uint8)
    for i in np.flatnonzero((K >= 2) & (rng.random(n_items) < 0.875)).tolist():
        a = int(rng.integers(0, K[i] + 1))
        gt[i] = a, int(rng.integers(a, K[i] + 1))
    return bits, members, gt


def _brute_sums(bits, gt, S):
    """[n_sites, 6, 2] = NS_j, AC_j: over the items with a call where j is a member, the copies of j's allele"""
    sal = np.cumsum(bits, axis=1) * bits
    called = (gt[:, 0] != NO_CALL)[:, None] & bits
    copies = (gt[:, 0, None] == sal).astype(np.int64) + (gt[:, 1, None] == sal)
    n_sites = len(bits) // S
    return np.stack([called.reshape(n_sites, S, 6).sum(axis=1), np.where(called, copies, 0).reshape(n_sites, S, 6).sum(axis=1)], axis=2)


@pytest.mark.parametrize("S", SIZES)
def test_site_sums_from_the_leaders_against_brute_force(S):
    """every wave of the first 3 * 64 * S items: the 18 ballots under cohort_segment's masks, summed over the leaders, are the brute-force sets;
    the word a leader adds is NS_j | AC_j << 32; a lane that is no leader adds nothing"""
    rng = np.random.default_rng(900 + S)
    full = 3 * 64 * S
    for n_items in (full, full - S, (full // S // 2) * S + S):
        bits, members, gt = _random_items(rng, n_items, S)
        n_sites = n_items // S
        tot, words = np.zeros((n_sites, 6, 2), np.int64), np.zeros((n_sites, 6), np.uint64)
        for w0 in range(0, n_items, 64):
            leader, ns, ac, word = sim.sums(w0, S, n_items, members, gt)
            item = w0 + np.arange(64)
            first = (item < n_items) & ((np.arange(64) == 0) | ((item - 1) // S != item // S))
            assert np.array_equal(leader != 0, first), (S, n_items, w0)
            assert np.array_equal(word, ns.astype(np.uint64) | (ac.astype(np.uint64) << np.uint64(32)))
            assert not ns[leader == 0].any() and not ac[leader == 0].any()
            k = item[leader != 0] // S
            np.add.at(tot, k, np.stack([ns[leader != 0], ac[leader != 0]], axis=2))
            np.add.at(words, k, word[leader != 0])
        want = _brute_sums(bits, gt, S)
        assert np.array_equal(tot, want), (S, n_items)
        assert np.array_equal(words, (want[..., 0] | (want[..., 1] << 32)).astype(np.uint64))


def test_harness_under_the_sanitizers():
    """the same pieces as a stand-alone program with its own main under -fsanitize=address,undefined (nothing is loaded into Python)"""
    p = subprocess.run([sim.build_main(), "site"], capture_output=True, text=True)
    assert p.returncode == 0 and p.stdout.startswith("site_sim ok") and not p.stderr, (p.stdout, p.stderr)


@pytest.mark.parametrize("n_sites, S", [(0, 1), (1, 1), (1, 65), (257, 3), (1000, 130)])
def test_cohort_sites_layout(n_sites, S):
    L = sim.layout(n_sites, S)
    n = n_sites * S
    site = (256 * n + 7) & ~7
    assert L == {"pl": 0, "raw": 224 * n, "gt": 252 * n, "members": 254 * n, "boundary": 255 * n, "site": site, "maxn": site + 48 * n_sites,
                 "in_at": site + 48 * n_sites + 8, "logs": site + 48 * n_sites + 8, "slots": site + 48 * n_sites + 8 + 128, "in_bytes": 128 + 24 * n_sites,
                 "total": site + 48 * n_sites + 8 + 128 + 24 * n_sites + 64}
    assert L["maxn"] == L["site"] + 48 * n_sites and L["site"] % 8 == 0      # ONE memset zeroes the site words and the max_n pair
    from svjg import genotype
    assert L["total"] <= genotype.COHORT_SITES_ITEM_BYTES * n + genotype.COHORT_SITES_SITE_BYTES * n_sites + 208      # what the Python side budgets


def test_chunk_keeps_a_call_under_one_gib():
    from svjg import genotype
    for S in (1, 2, 64, 3000, 10**7):
        n = genotype.cohort_sites_chunk(S)
        assert n >= 1 and (n * (256 * S + 72) <= 1 << 30 or n == 1) and (n + 1) * (256 * S + 72) > 1 << 30


# ---- the harness: arithmetic behind the compaction ----

def test_item_arithmetic_against_the_model_on_the_present_members():
    """random sites of SM.random_sites spread over the six candidate places, candidates dropped at random: K' = 0..6.  An item with K' >= 2 is
    tests/site_model.py on its present members (check_against_model); K' < 2: no call, zeros"""
    from tests.geno_sim import site as site_sim
    rng = np.random.default_rng(5)
    sites = SM.random_sites(2_400, seed=99)
    n = len(sites)
    bits, cref, calt = np.zeros(n, np.uint8), rng.integers(0, 20_000, (n, 6)).astype(np.uint32), rng.integers(0, 20_000, (n, 6)).astype(np.uint32)
    present = []
    for i, (ref, alts) in enumerate(sites):
        at = np.sort(rng.choice(6, len(alts), replace=False))
        calt[i, at] = alts
        cref[i, at] = rng.integers(0, ref + 1, len(alts))
        cref[i, at[rng.integers(len(at))]] = ref
        keep = at[rng.random(len(at)) >= (0.35 if i % 3 == 0 else 0.0)]      # a third of the items lose members
        if i % 40 == 0:
            keep = keep[:i // 40 % 2]                                        # K' = 0 and K' = 1
        bits[i] = sum(1 << int(j) for j in keep)
        present.append((int(cref[i, keep].max()) if len(keep) else 0, calt[i, keep].tolist()))
    assert {len(a) for _, a in present} == set(range(7))
    tab = site_sim.logfact_table(1 << 17)
    e, ms = 5e-5, 3
    gt, pl, raw, near, st, s_k = sim.items(bits, cref, calt, ms, e, tab)
    assert not st.any()
    sel = [i for i, (_, a) in enumerate(present) if len(a) >= 2]
    rest = [i for i, (_, a) in enumerate(present) if len(a) < 2]
    assert len(sel) > 2_000 and len(rest) >= 60
    assert (gt[rest] == NO_CALL).all() and not pl[rest].any() and not raw[rest].any() and not near[rest].any()
    for i in sel:
        ref, alts = present[i]
        assert raw[i].tolist() == [ref] + alts + [0] * (6 - len(alts)) and s_k[i] == sum(SM.counts(ref, alts)[1])
    want = [SM.genotype(*present[i], ms, e) for i in sel]
    SM.check_against_model([present[i] for i in sel], want, lambda s: (e, ms), gt[sel], pl[sel], near[sel])


# ---- the host flow with a stand-in context that answers from the models ----

class CohortModelCtx:
    """stands in for capi.Context in a cohort run: a count matrix with presence bytes, genotype_cohort() answered from tests/ploidy_model at
    ploidy 2 and genotype_cohort_sites() from tests/site_model on the candidates present for each sample"""
    made = []

    def __init__(self, device=0):
        self.cohort_calls, self.site_calls = 0, []
        CohortModelCtx.made.append(self)

    def cohort_alloc(self, n_samples, n_slots):
        self.counts, self.present = np.zeros((n_samples, n_slots, 2), np.uint32), np.zeros((n_samples, n_slots), bool)

    def cohort_set_counts(self, sample, slots, counts):
        self.counts[sample], self.present[sample] = 0, False
        self.counts[sample, slots], self.present[sample, slots] = counts, True

    def genotype_cohort(self, sv_type, slot, ok, min_support, err):
        self.cohort_calls += 1
        n, S = len(sv_type), len(self.counts)
        gt, pl, raw = np.full((n, S), 3, np.uint8), np.zeros((n, S, 3), np.int64), np.zeros((n, S, 2), np.uint32)
        done, site = np.zeros((n, S), np.uint8), np.zeros((n, 2), np.int64)
        for r in range(n):
            for s in range(S):
                if (ok[r] & 1) and slot[r] != NONE and self.present[s, slot[r]]:
                    raw[r, s] = self.counts[s, slot[r]]
                    g, pl[r, s] = PM.genotype(int(sv_type[r]), int(raw[r, s, 0]), int(raw[r, s, 1]), 2, min_support, err)
                    done[r, s] = 1
                    if g is not None:
                        gt[r, s] = g
                        site[r] += (1, g)
        return gt, pl, raw, done, np.zeros((n, S), np.uint8), site.astype(np.uint32)

    def genotype_cohort_sites(self, slots, min_support, err):
        self.site_calls.append(np.array(slots))
        n, S = len(slots), len(self.counts)
        gt, pl, raw = np.full((n, S, 2), NO_CALL, np.uint8), np.zeros((n, S, 28), np.int64), np.zeros((n, S, 7), np.uint32)
        members, site = np.zeros((n, S), np.uint8), np.zeros((n, 6, 2), np.int64)
        for k in range(n):
            for s in range(S):
                at = [j for j in range(6) if slots[k, j] != NONE and self.present[s, slots[k, j]]]
                members[k, s] = sum(1 << j for j in at)
                if len(at) < 2:
                    continue
                m = [int(slots[k, j]) for j in at]
                raw[k, s, 0], raw[k, s, 1:len(m) + 1] = self.counts[s, m, 0].max(), self.counts[s, m, 1]
                call, pls = SM.genotype(int(raw[k, s, 0]), raw[k, s, 1:len(m) + 1].tolist(), min_support, err)
                pl[k, s, :len(pls)] = pls
                if call:
                    gt[k, s] = call
                    for i, j in enumerate(at, 1):
                        site[k, j] += (1, (call[0] == i) + (call[1] == i))
        return gt, pl, raw, members, np.zeros((n, S), np.uint8), site.astype(np.uint32)

    def close(self):
        pass


def _sample_counts():
    """four samples over the keys of tests/test_joint_ins.py: {key: (ref, alt)} each"""
    full = {k: tuple(int(x) for x in c) for k, c in zip(KEYS, COUNTS)}
    s2 = {k: (c[0] + 1, c[1] * 2) for k, c in full.items() if k != "chr1:INS-100-2"}       # lacks a member's key: site X has two members here
    s3 = dict(full, **{"chr1:INS-100-1": (0, 0), "chr2:INS-100-4": (0, 31)})               # a key with two empty lists: present, a member
    s4 = {k: (c[1], c[0] + 3) for k, c in full.items() if k != "chr2:INS-100-4"}           # a single member present at site Y: no site there
    return [("S1", full), ("S2", s2), ("S3", s3), ("S4", s4)]


@pytest.fixture()
def cohort_run(tmp_path, capsys, monkeypatch):
    """(plain --cohort lines, --cohort --joint-ins lines, the joint run's context, its stderr, the four single-sample --joint-ins outputs' lines)"""
    from svjg import capi, genotype
    monkeypatch.setenv("SVJG_PY_VCF", "1")
    monkeypatch.setattr(capi, "Context", CohortModelCtx)
    vcf = tmp_path / "in.vcf"
    vcf.write_text(VCF_TEXT)
    samples = _sample_counts()
    for name, counts in samples:
        (tmp_path / (name + ".json")).write_text(json.dumps({k: [["r"] * a, ["a"] * b] for k, (a, b) in counts.items()}))
    (tmp_path / "cohort.list").write_text("".join("%s\t%s.json\n" % (name, name) for name, _ in samples))
    genotype.run_cohort(str(tmp_path / "cohort.list"), str(vcf), str(tmp_path / "plain.vcf"), MS, E)
    capsys.readouterr()
    genotype.run_cohort(str(tmp_path / "cohort.list"), str(vcf), str(tmp_path / "joint.vcf"), MS, E, joint_ins=True)
    ctx, err = CohortModelCtx.made[-1], capsys.readouterr().err
    single = []
    for name, counts in samples:
        keys = list(counts)
        out = tmp_path / (name + ".joint.vcf")
        genotype.genotype_with_counts(ModelCtx(np.array([counts[k] for k in keys], np.uint32)), str(vcf), {k: i for i, k in enumerate(keys)}, str(out),
                                      MS, E, slot_is_presence=True, joint_ins=True)
        single.append(out.read_text().split("\n"))
    return (tmp_path / "plain.vcf").read_text().split("\n"), (tmp_path / "joint.vcf").read_text().split("\n"), ctx, err, single


def _data(lines):
    return [l.split("\t") for l in lines if l and not l.startswith("#")]


def test_grouping_and_one_sites_call(cohort_run):
    _, _, ctx, err, _ = cohort_run
    assert ctx.cohort_calls == 1 and len(ctx.site_calls) == 1               # the plain cohort call, then ONE call for all sites
    slot = {}
    for _, counts in _sample_counts():                                      # cohort_union: first-seen order
        for k in counts:
            slot.setdefault(k, len(slot))
    x = [slot["chr1:INS-100-1"], slot["chr1:INS-100-2"], slot["chr1:INS-100-7"], NONE, NONE, NONE]      # file order, not adjacent; the short row and the one without a key excluded
    y = [slot["chr2:INS-100-3"], slot["chr2:INS-100-4"], NONE, NONE, NONE, NONE]                        # the same POS on another contig
    assert ctx.site_calls[0].tolist() == [x, y]                             # chr3:700 has one candidate, chr4:900 seven: neither is a site
    lines = [l for l in err.split("\n") if l]
    assert len(lines) == 1 and "chr4:900" in lines[0] and "7" in lines[0]


def test_every_column_is_the_single_sample_joint_run(cohort_run):
    _, joint, _, _, single = cohort_run
    data = _data(joint)
    assert len(data) == len(_ROWS)
    seen = {"site": 0, "dots": 0, "plain": 0}
    for s, lines in enumerate(single):
        alone = _data(lines)
        for r, (got, want) in enumerate(zip(data, alone)):
            assert got[:7] == want[:7]
            if got[8] == want[8]:
                assert got[9 + s] == want[9], (r, s)
                seen["site" if got[8].endswith(":SGT:SAL") else "plain"] += 1
            else:                                                           # the one allowed difference: the row is a member for another sample only
                assert got[8] == "GT:DP:AD:PL:SGT:SAL" and want[8] == "GT:DP:AD:PL" and got[9 + s] == want[9] + ":.:.", (r, s)
                seen["dots"] += 1
    # site X: S1, S3, S4 three members, S2 two of them; site Y: S1, S2, S3; the other items of the rows of X (one) and Y (S4's two): `:.:.`
    assert seen["site"] == 3 + 2 + 3 + 3 + 2 * 3 and seen["dots"] == 1 + 2 and seen["plain"] == 4 * (len(_ROWS) - 5)
    row = {r[4]: k for k, r in enumerate(_ROWS) if r[4]}
    assert data[row["chr1:INS-100-2"]][9 + 1] == "./.:0:0,0:.,.,.:.:."      # S2 lacks the key: not genotyped, no site
    assert data[row["chr1:INS-100-7"]][9 + 1].endswith(":2")               # ... and the third candidate is S2's allele 2
    assert data[row["chr1:INS-100-1"]][9 + 2].split(":")[1:3] == ["0", "0,0"] and data[row["chr1:INS-100-1"]][9 + 2].endswith(":1")   # S3: empty lists, still allele 1
    y3 = data[row["chr2:INS-100-3"]][9 + 3]
    assert y3.endswith(":.:.") and y3.split(":")[0] != "./."                # S4: one member present: its independent call


def test_site_tags_are_the_sums_over_the_printed_gts(cohort_run):
    _, joint, _, _, _ = cohort_run
    members = 0
    for d in _data(joint):
        gts = [c.split(":")[0] for c in d[9:]]
        ns, ac = sum(g != "./." for g in gts), sum(g.count("1") for g in gts if g != "./.")
        want = ["NS=%d" % ns, "AN=%d" % (2 * ns), "AC=%d" % ac] + (["AF=%s" % ("%.6g" % (ac / (2 * ns)))] if ns else [])
        assert d[7].split(";")[-len(want):] == want, d[:3]
        members += d[8].endswith(":SGT:SAL")
    assert members == 5


def test_only_member_rows_and_the_header_differ(cohort_run):
    plain, joint, _, _, _ = cohort_run
    at = next(k for k, l in enumerate(plain) if l.startswith("##FORMAT=<ID=PL,"))
    assert joint[:at + 1] == plain[:at + 1]
    assert joint[at + 1].startswith("##FORMAT=<ID=SGT,Number=1,Type=String,Description=") and joint[at + 2].startswith("##FORMAT=<ID=SAL,Number=1,Type=Integer,Description=")
    rest_p, rest_j = plain[at + 1:], joint[at + 3:]
    assert len(rest_p) == len(rest_j) and rest_p[0] == rest_j[0] and rest_p[0].endswith("\tFORMAT\tS1\tS2\tS3\tS4")
    assert [k - 1 for k, (a, b) in enumerate(zip(rest_p, rest_j)) if a != b] == [0, 2, 3, 4, 7]      # the five member rows, by data row
    assert sum(l.startswith("##INFO=<ID=NS,") for l in joint) == 1 and sum(l.startswith("##FORMAT=<ID=GT") for l in joint) == 1


def test_projection_is_project_site():
    """project_cohort_sites on random items against project_site item by item"""
    from svjg import genotype
    rng = np.random.default_rng(3)
    bits, members, gt = _random_items(rng, 600, 4)
    pl = rng.integers(0, 5000, (150, 4, 28))
    covered, g, pl3, sal = genotype.project_cohort_sites(gt.reshape(150, 4, 2), pl, members.reshape(150, 4))
    bits = bits.reshape(150, 4, 6)
    for k, s in np.ndindex(150, 4):
        at = np.flatnonzero(bits[k, s])
        K = len(at)
        assert covered[k, s].tolist() == (bits[k, s] & (K >= 2)).tolist()
        for i, j in enumerate(at, 1):
            assert sal[k, s, j] == i
            if K >= 2:
                assert (int(g[k, s, j]), pl3[k, s, j].tolist()) == genotype.project_site(K, i, gt.reshape(150, 4, 2)[k, s], pl[k, s, :(K + 1) * (K + 2) // 2])


# ---- the golden cohort ----

@pytest.mark.parametrize("which", ["plain", "edited"])
def test_golden_cohort_rows_outside_any_site_are_byte_equal(golden, tmp_path, monkeypatch, which):
    from svjg import capi, genotype
    from tests import cohort_model as CM
    monkeypatch.setenv("SVJG_PY_VCF", "1")
    monkeypatch.setattr(capi, "Context", CohortModelCtx)
    co = CM.Cohort(golden, which)
    a, b = str(tmp_path / "plain.vcf"), str(tmp_path / "joint.vcf")
    assert genotype.run_cohort(co.list, co.vcf, a) == genotype.run_cohort(co.list, co.vcf, b, joint_ins=True)
    plain, joint = open(a).read().split("\n"), open(b).read().split("\n")
    joint = [l for l in joint if not l.startswith(("##FORMAT=<ID=SGT,", "##FORMAT=<ID=SAL,"))]
    assert len(plain) == len(joint)
    sites = CohortModelCtx.made[-1].site_calls
    n_member = 0
    for p, j in zip(plain, joint):
        if "\tGT:DP:AD:PL:SGT:SAL\t" in j:
            n_member += 1
        else:
            assert p == j
    if not sites:                                                            # the fixture has no shared position: the data rows are byte-equal
        assert n_member == 0 and plain == joint


# ---- the refusals ----

class _NoGpu:
    def __init__(self, *a):
        raise AssertionError("a context was made before the options were checked")


@pytest.mark.parametrize("extra", [{"ploidy_file": "ploidy.txt"}, {"prior": True}, {"ploidy_file": "ploidy.txt", "prior": True}])
def test_joint_ins_with_cohort_ploidy_or_prior_is_refused_before_anything(tmp_path, monkeypatch, extra):
    from svjg import capi, genotype
    monkeypatch.setattr(capi, "Context", _NoGpu)
    out = tmp_path / "out.vcf"
    with pytest.raises(ValueError) as ei:                                    # (neither the list nor the ploidy file exists: nothing is read either)
        genotype.run_cohort(str(tmp_path / "none.list"), str(tmp_path / "in.vcf"), str(out), joint_ins=True, **extra)
    assert "--joint-ins" in str(ei.value) and "--cohort-ploidy" in str(ei.value) and "--cohort-prior" in str(ei.value) and not out.exists()


@pytest.mark.parametrize("extra", [["--cohort-ploidy", "ploidy.txt"], ["--cohort-prior"]])
def test_script_refuses_joint_ins_with_cohort_ploidy_or_prior(tmp_path, extra):
    (tmp_path / "in.vcf").write_text(VCF_TEXT)
    (tmp_path / "cohort.list").write_text("S1\ts1.json\n")
    p = subprocess.run([sys.executable, os.path.join(AMD, "predict-genotype.py"), "--cohort", "cohort.list", "-v", "in.vcf", "-o", "out.vcf", "--joint-ins", *extra],
                       capture_output=True, text=True, cwd=tmp_path)
    assert p.returncode != 0 and "usage:" in p.stderr and "--joint-ins" in p.stderr and extra[0] in p.stderr
    assert sorted(os.listdir(tmp_path)) == ["cohort.list", "in.vcf"]       # no output file of any kind


def test_script_accepts_cohort_with_joint_ins(tmp_path):
    """the parser lets the combination through: the run gets as far as the cohort list, which does not exist"""
    (tmp_path / "in.vcf").write_text(VCF_TEXT)
    p = subprocess.run([sys.executable, os.path.join(AMD, "predict-genotype.py"), "--cohort", "none.list", "-v", "in.vcf", "-o", "out.vcf", "--joint-ins"],
                       capture_output=True, text=True, cwd=tmp_path)
    assert p.returncode != 0 and "usage:" not in p.stderr and "none.list" in p.stderr and not (tmp_path / "out.vcf").exists()
