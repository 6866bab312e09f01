"""Joint insertion calls in a cohort under an allele-frequency prior (--cohort LIST --joint-ins --joint-prior), on the CPU: the 60-digit model
(tests/site_prior_model.py) against a brute-force EM; the routines of svjg_geno.h behind k_cohort_sites_prior, compiled with g++
(tests/geno_sim, topic site_prior), against the model's stored answers in sequential order and in the kernel's order of the sums; the weights' expansion to
candidate order; site_lik behind the factoring; the layout; the harness under the sanitizers; the option's refusals; the writer on a hand-made
cohort against the model's calls; the run without the option against the parent's bytes."""
import json
import os
import subprocess
import sys
from decimal import Decimal, localcontext
from fractions import Fraction

import mpmath
import numpy as np
import pytest

from tests import cohort_site_prior_cases as CS
from tests import site_model as SM
from tests import site_prior_model as M
from tests.geno_sim import site_prior as H
from tests.geno_sim import site as geno_site_sim
from tests.test_cohort_joint_ins import CohortModelCtx, _sample_counts, _NoGpu
from tests.test_joint_ins import _ROWS, VCF_TEXT

AMD = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "svjedi-graph_amd")
NO_CALL, NONE = 0xFF, 0xFFFFFFFF
E, MS = 5e-5, 3
EM_TOL, EM_MAX_IT, EM_FLAG, P_BOUND = H.constants()
CASE_NAMES = [c[0] for c in CS.CASES]


def _case(name):
    c = CS.inputs(name)
    members, raw = CS.first_kernel(c)
    return c, members, raw


# ---- the model against brute force ----

def _brute(raw, members, C, err):
    """EM written naively with mpmath at 60 digits over ALL genotypes (A, B) on 0..C of every sample, a genotype naming an absent candidate
    weighing 0: l from exact Fractions, the prior as the multinomial term, copies by counting -> (p or None, steps, not converged)"""
    mpmath.mp.dps = 60
    S = len(members)
    items = []
    for s in range(S):
        cand = [j + 1 for j in range(6) if members[s] >> j & 1]
        if len(cand) < 2:
            continue
        c = [mpmath.mpf(0)] * (C + 1)
        c[0] = mpmath.mpf(int(raw[s, 0]))
        for t, j in enumerate(cand):
            c[j] = mpmath.mpf(int(raw[s, 1 + t])) / 2
        N = sum(c)
        if N == 0:
            continue
        l_ok, l_x, l_he = M.site_logs(err, len(cand))
        ls = {}
        for b in range(C + 1):
            for a in range(b + 1):
                if all(x == 0 or x in cand for x in (a, b)):
                    own = float(c[a]) if a == b else float(c[a]) + float(c[b])
                    ls[a, b] = Fraction(own * (l_ok if a == b else l_he)) + Fraction((float(N) - own) * l_x)
        top = max(ls.values())
        items.append({g: mpmath.power(10, mpmath.mpf(float(l - top))) for g, l in ls.items()})
    if not items:
        return None, 0, False
    p = [mpmath.mpf(1) / (C + 1)] * (C + 1)
    for step in range(1, EM_MAX_IT + 1):
        x = [mpmath.mpf(0)] * (C + 1)
        for w in items:
            post = {g: (1 if g[0] == g[1] else 2) * p[g[0]] * p[g[1]] * v for g, v in w.items()}
            z = sum(post.values())
            for j in range(C + 1):
                x[j] += sum(g.count(j) * v for g, v in post.items()) / z
        pn = [v / (2 * len(items)) for v in x]
        far = max(abs(a - b) for a, b in zip(pn, p))
        p = pn
        if far <= mpmath.mpf("1e-9"):
            return p, step, False
    return p, EM_MAX_IT, True


def test_model_is_the_brute_force_em():
    rng = np.random.default_rng(5)
    seen = 0
    for _ in range(60):
        S, C = int(rng.integers(1, 4)), int(rng.integers(2, 4))
        members = np.array([sum(1 << j for j in range(C) if rng.random() < 0.8) for _ in range(S)], np.uint8)
        raw = np.zeros((S, 7), np.uint32)
        for s in range(S):
            K = bin(members[s]).count("1")
            if K >= 2:
                raw[s, :K + 1] = rng.integers(0, 12, K + 1)
        res = M.run(raw[None], members[None], [C], E, 0)
        p, steps, flag = _brute(raw, members, C, E)
        assert (res["p"][0] is None) == (p is None) and res["steps"][0] == steps and res["flag"][0] == flag
        if p is not None:
            seen += 1
            assert all(abs(mpmath.mpf(str(a)) - b) < mpmath.mpf("1e-50") for a, b in zip(res["p"][0], p))
            assert all(a == 0 for a in res["p"][0][C + 1:])
    assert seen >= 40


# ---- the harness against the stored answers ----

_MEASURED = {}


@pytest.mark.parametrize("name", CASE_NAMES)
def test_harness_is_the_model(name):
    """sequential order and the kernel's order (lanes, strides, butterfly): steps, the not-converged bit and the NaN pattern on every site, sgt and
    sgq on every item the model decides, psite = the sums of the harness's own calls, p within SITE_EM_P_BOUND; at most 1 % undecided"""
    c, members, raw = _case(name)
    gold = CS.load_golden(name, c)
    assert gold["item_out"].mean() <= M.CAP and not gold["site_out"].any()
    for k in np.random.default_rng(1).permutation(len(members))[:3].tolist():         # a sample of sites through the model again: the stored answer is the model's
        again = M.run(raw, members, c["C"], CS.ERR, 0, sites=[k])
        assert again["steps"][k] == gold["steps"][k] and np.array_equal(again["sgt"][k], gold["sgt"][k]) and np.array_equal(again["sgq"][k], gold["sgq"][k])
        assert np.array_equal(again["p_hi"][k], gold["p_hi"][k], equal_nan=True)
    est = ~np.isnan(gold["p_hi"][:, 0])
    for ms in (0, 3):
        want_gt, want_gq = CS.with_support(gold["sgt"], gold["sgq"], raw, ms)
        for wave in (0, 1):
            got = H.sites(raw, members, c["slots"], CS.ERR, ms, wave)
            assert np.array_equal(got["steps"] & ~np.uint32(EM_FLAG), gold["steps"]) and np.array_equal((got["steps"] & EM_FLAG) != 0, gold["flag"])
            assert np.array_equal(np.isnan(got["p"]), np.isnan(gold["p_hi"])) and np.array_equal(np.isnan(got["p"]).all(axis=1), ~est)
            ok = ~gold["item_out"]
            assert np.array_equal(got["sgt"][ok], want_gt[ok]) and np.array_equal(got["sgq"][ok], want_gq[ok])
            assert np.array_equal(got["psite"], M.psite_of(got["sgt"], members))
            if est.any():
                d = np.abs((got["p"][est] - gold["p_hi"][est]) - gold["p_lo"][est])
                big = gold["p_hi"][est] > 1e-6
                if wave and ms == 0:
                    _MEASURED[name] = (d.max(), (d[big] / gold["p_hi"][est][big]).max() if big.any() else 0.0)
                    print("%s: max |p - model| %.3e absolute, %.3e relative among p > 1e-6" % ((name,) + _MEASURED[name]))
                assert d.max() <= P_BOUND, (name, wave, d.max())


def test_measured_p_error_report():
    """prints the maximum over the cases run before it in this process (what svjg_geno.h quotes beside SITE_EM_P_BOUND)"""
    if _MEASURED:
        a = max(_MEASURED, key=lambda n: _MEASURED[n][0])
        r = max(_MEASURED, key=lambda n: _MEASURED[n][1])
        print("max absolute %.3e (%s), max relative %.3e (%s), %d cases" % (_MEASURED[a][0], a, _MEASURED[r][1], r, len(_MEASURED)))
        assert P_BOUND >= _MEASURED[a][0]


# ---- the weights in candidate order ----

@pytest.mark.parametrize("C", [2, 3, 4, 5, 6])
def test_weights_expand_to_candidate_order_for_every_presence_pattern(C):
    """all 64 presence patterns (the bits beyond C are dropped by the site's slots, so they are tried too: a candidate beyond C is never present)
    against the model's weights placed by brute force; a strided store touches nothing between the slots"""
    rng = np.random.default_rng(40 + C)
    with localcontext() as ctx:
        ctx.prec = M.PREC
        ctx.Emin, ctx.Emax = -10 ** 12, 10 ** 12
        for bits in range(64):
            bits &= (1 << C) - 1
            K = bin(bits).count("1")
            for deep in (0, 1):
                raw = np.zeros(7, np.uint32)
                if K >= 2:
                    raw[:K + 1] = rng.integers(0, 40000 if deep else 30, K + 1)
                w, top, N, part = H.item(raw, bits, E, stride=1 + 2 * deep)
                got = M.weights(raw, bits, E)
                assert part == (got is not None)
                want = np.zeros(28)
                if got is not None:
                    n_model, pairs, ws, top_model = got
                    assert N == n_model
                    for (a, b), v in zip(pairs, ws):
                        want[b * (b + 1) // 2 + a] = float(v)
                    a, b = pairs[top_model]
                    assert top == b * (b + 1) // 2 + a and w[top] == 1.0
                    named = {b * (b + 1) // 2 + a for a, b in pairs}
                    assert all(w[i] == 0.0 for i in range(28) if i not in named)
                assert np.allclose(w, want, rtol=1e-12, atol=1e-300), (bits, raw)


# ---- site_lik behind the factoring ----

def test_site_lik_is_the_exact_sum_and_geno_site_has_not_moved():
    """site_lik returns the exact sum of the two rounded products (hi + lo as Fractions), for every genotype of random sites; geno_site, which now
    calls it, still gives the calls and PLs of tests/site_model.py on the same sites"""
    rng = np.random.default_rng(77)
    sites = []
    for _ in range(200):
        K = int(rng.integers(2, 7))
        ref, alt = int(rng.integers(0, 200)), rng.integers(0, 200, K).tolist()
        sites.append((ref, alt))
        hi, lo = H.lik(K, ref, alt, E)
        l_ok, l_x, l_he = M.site_logs(E, K)
        c = [float(ref)] + [a / 2 for a in alt]
        N = sum(c)
        for b in range(K + 1):
            for a in range(b + 1):
                own = c[a] if a == b else c[a] + c[b]
                rest = N - c[a] if a == b else N - c[a] - c[b]
                at = b * (b + 1) // 2 + a
                assert Fraction(hi[at]) + Fraction(lo[at]) == Fraction(own * (l_ok if a == b else l_he)) + Fraction(rest * l_x)
    tab = geno_site_sim.logfact_table(4096)
    gt, pl, near, st, _ = geno_site_sim.genotype_sites(sites, MS, E, tab)
    assert not st.any()
    SM.check_against_model(sites, [SM.genotype(ref, alt, MS, E) for ref, alt in sites], lambda s: (E, MS), gt, pl, near)


# ---- the layout ----

@pytest.mark.parametrize("n, S", [(0, 1), (1, 1), (1, 65), (257, 3), (1000, 130)])
def test_layout_with_the_prior_switch(n, S):
    old = geno_site_sim.layout(n, S, True)
    plain = H.layout(n, S, True, False)
    for k, v in old.items():                                                   # the cohort call's offsets are what they were, field by field
        assert plain[k] == v, k
    assert all(plain[k] == 0 for k in ("sgt", "sgq", "af", "psite", "steps"))
    single = H.layout(n, 1, False, False)
    assert single == H.layout(n, 1, False, True)                               # the switch means nothing without the cohort
    for k, v in geno_site_sim.layout(n, 1, False).items():
        assert single[k] == v, k
    L = H.layout(n, S, True, True)
    items = n * S
    assert [L[k] for k in ("pl", "raw", "gt", "members", "boundary")] == [plain[k] for k in ("pl", "raw", "gt", "members", "boundary")]
    assert L["sgt"] == L["boundary"] + items and L["sgq"] == L["sgt"] + 2 * items
    assert L["af"] == (L["sgq"] + items + 7) // 8 * 8 and L["psite"] == L["af"] + 56 * n and L["steps"] == L["psite"] + 48 * n
    assert L["site"] == (L["steps"] + 4 * n + 7) // 8 * 8 and L["maxn"] == L["site"] + 48 * n and L["in_at"] == L["maxn"] + 8
    assert L["logs"] == L["in_at"] and L["slots"] == L["logs"] + 128 and L["in_bytes"] == 128 + 24 * n and L["total"] == L["in_at"] + L["in_bytes"] + 64
    from svjg import genotype
    assert L["maxn"] <= genotype.COHORT_SITES_PRIOR_ITEM_BYTES * items + genotype.COHORT_SITES_PRIOR_SITE_BYTES * n + 16
    step = genotype.cohort_sites_chunk(S, True)
    assert H.layout(step, S, True, True)["total"] <= 1 << 30 and step <= genotype.cohort_sites_chunk(S)


def test_harness_under_the_sanitizers():
    """the seeded checks as a stand-alone program with its own main under -fsanitize=address,undefined, every array at exactly its size"""
    p = subprocess.run([H.build_main(), "site_prior"], capture_output=True, text=True)
    assert p.returncode == 0 and p.stdout.startswith("site_prior_sim ok") and not p.stderr, (p.stdout, p.stderr)


# ---- the C prototype ----

def test_prototype_is_exported():
    from svjg import capi
    import ctypes
    assert "svjg_genotype_cohort_sites_prior" in capi.EXPORTS
    restype, args = capi._SIGS["svjg_genotype_cohort_sites_prior"]
    assert restype is ctypes.c_int and len(args) == 16 and args[:5] == capi._SIGS["svjg_genotype_cohort_sites"][1][:5]
    header = open(os.path.join(os.path.dirname(AMD), "include", "svjg.h")).read()
    assert "int svjg_genotype_cohort_sites_prior(svjg_ctx *ctx, const uint32_t *slots" in header


# ---- the refusals ----

def _script(tmp_path, *extra):
    (tmp_path / "in.vcf").write_text(VCF_TEXT)
    return subprocess.run([sys.executable, os.path.join(AMD, "predict-genotype.py"), "-v", "in.vcf", "-o", "out.vcf", *extra], capture_output=True, text=True, cwd=tmp_path)


@pytest.mark.parametrize("extra, word", [(["-d", "x.json", "--joint-ins", "--joint-prior"], "--cohort"), (["--cohort", "none.list", "--joint-prior"], "--joint-ins"),
                                         (["-d", "x.json", "--joint-prior"], "--cohort")])
def test_script_refuses_joint_prior_without_cohort_or_joint_ins(tmp_path, extra, word):
    p = _script(tmp_path, *extra)
    assert p.returncode != 0 and "usage:" in p.stderr and "--joint-prior needs" in p.stderr and word in p.stderr
    assert sorted(os.listdir(tmp_path)) == ["in.vcf"]


@pytest.mark.parametrize("extra", [["--cohort-prior"], ["--cohort-ploidy", "p.txt"], ["--cohort-qual"]])
def test_script_keeps_every_refusal_of_joint_ins(tmp_path, extra):
    p = _script(tmp_path, "--cohort", "none.list", "--joint-ins", "--joint-prior", *extra)
    assert p.returncode != 0 and "usage:" in p.stderr and "--joint-ins" in p.stderr and extra[0] in p.stderr
    assert sorted(os.listdir(tmp_path)) == ["in.vcf"]


def test_script_accepts_the_option_as_far_as_the_missing_list(tmp_path):
    p = _script(tmp_path, "--cohort", "none.list", "--joint-ins", "--joint-prior")
    assert p.returncode != 0 and "usage:" not in p.stderr and "none.list" in p.stderr
    assert sorted(os.listdir(tmp_path)) == ["in.vcf"]


@pytest.mark.parametrize("extra, word", [({}, "--joint-ins"), ({"prior": True}, "--joint-ins"), ({"joint_ins": True, "prior": True}, "--cohort-prior"),
                                         ({"joint_ins": True, "ploidy_file": "p.txt"}, "--cohort-ploidy"), ({"joint_ins": True, "qual": True}, "--cohort-qual")])
def test_run_cohort_refuses_before_anything(tmp_path, monkeypatch, extra, word):
    from svjg import capi, genotype
    monkeypatch.setattr(capi, "Context", _NoGpu)
    out = tmp_path / "out.vcf"
    with pytest.raises(ValueError) as ei:                                      # (nothing exists: nothing is read either)
        genotype.run_cohort(str(tmp_path / "none.list"), str(tmp_path / "in.vcf"), str(out), joint_prior=True, **extra)
    assert word in str(ei.value) and not out.exists()


# ---- the writer on a hand-made cohort, against the model's calls ----

class SitePriorModelCtx(CohortModelCtx):
    """CohortModelCtx whose genotype_cohort_sites_prior answers from the 60-digit model on what genotype_cohort_sites (the site model) leaves"""
    not_converged = ()                                                         # sites reported with bit 31, for the writer's EMNC

    def genotype_cohort_sites_prior(self, slots, min_support, err):
        gt, pl, raw, members, boundary, site = self.genotype_cohort_sites(slots, min_support, err)
        C = (np.asarray(slots) != NONE).sum(axis=1)
        res = M.run(raw, members, C, err, min_support)
        self.model = dict(res, members=members, raw=raw, slots=np.array(slots))
        steps = res["steps"] | np.where(res["flag"], 1 << 31, 0).astype(np.uint32)
        for k in self.not_converged:
            steps[k] |= np.uint32(1 << 31)
        return gt, pl, raw, members, boundary, site, res["sgt"], res["sgq"], res["p_hi"], steps, M.psite_of(res["sgt"], members)


def _write_cohort(tmp_path, samples):
    (tmp_path / "in.vcf").write_text(VCF_TEXT)
    for name, counts in samples:
        (tmp_path / (name + ".json")).write_text(json.dumps({k: [["r"] * a, ["a"] * b] for k, (a, b) in counts.items()}))
    (tmp_path / "cohort.list").write_text("".join("%s\t%s.json\n" % (name, name) for name, _ in samples))


def _samples():
    """the four samples of tests/test_cohort_joint_ins.py with one count moved: there S3 has as many reads on candidate 1 of the second site as on
    the reference, beside two samples that are 0/1 — p_0 = p_1 at every step and S3's 0/2 and 1/2 tie to all 60 digits, which the model's margin
    leaves undecided.  Four more reads on candidate 1 decide it, so that the device's file can be held to the model's"""
    samples = _sample_counts()
    ref, alt = samples[2][1]["chr2:INS-100-3"]
    samples[2][1]["chr2:INS-100-3"] = (ref, alt + 4)
    return samples


def _data(text):
    return [l.split("\t") for l in text.split("\n") if l and not l.startswith("#")]


@pytest.fixture()
def handmade(tmp_path, capsys, monkeypatch):
    """(--cohort --joint-ins text, --cohort --joint-ins --joint-prior text, the prior run's context, the plain --cohort text)"""
    from svjg import capi, genotype
    monkeypatch.setenv("SVJG_PY_VCF", "1")
    monkeypatch.setattr(capi, "Context", SitePriorModelCtx)
    monkeypatch.setattr(SitePriorModelCtx, "not_converged", (1,))
    _write_cohort(tmp_path, _samples())
    args = (str(tmp_path / "cohort.list"), str(tmp_path / "in.vcf"))
    genotype.run_cohort(*args, str(tmp_path / "plain.vcf"), MS, E)
    genotype.run_cohort(*args, str(tmp_path / "joint.vcf"), MS, E, joint_ins=True)
    genotype.run_cohort(*args, str(tmp_path / "prior.vcf"), MS, E, joint_ins=True, joint_prior=True)
    capsys.readouterr()
    return (tmp_path / "joint.vcf").read_text(), (tmp_path / "prior.vcf").read_text(), SitePriorModelCtx.made[-1], (tmp_path / "plain.vcf").read_text()


def test_run_without_the_option_is_the_parents_bytes(tmp_path, capsys, monkeypatch):
    from svjg import capi, genotype
    monkeypatch.setenv("SVJG_PY_VCF", "1")
    monkeypatch.setattr(capi, "Context", CohortModelCtx)
    _write_cohort(tmp_path, _sample_counts())
    genotype.run_cohort(str(tmp_path / "cohort.list"), str(tmp_path / "in.vcf"), str(tmp_path / "joint.vcf"), MS, E, joint_ins=True)
    capsys.readouterr()
    with open(os.path.join(CS.GOLDEN, "handmade_joint_ins.vcf")) as fh:        # written by the parent commit's code on the same cohort
        assert (tmp_path / "joint.vcf").read_text() == fh.read()


def test_writer_against_the_models_calls(handmade):
    joint, prior, ctx, plain = handmade
    m = ctx.model
    took_part = ~np.isnan(m["gap"])
    assert (m["gap"][took_part] >= M.TOP_GAP).all() and (m["gq_margin"][took_part] >= M.GQ_MARGIN).all() and not (np.abs(m["ratio"] - 1) < M.RATIO_BAND).any()   # the model decides every item: tests/test_cohort_site_prior_gpu.py holds the device's file to it
    dj, dp, dplain = _data(joint), _data(prior), _data(plain)
    hj, hp = [l for l in joint.split("\n") if l.startswith("#")], [l for l in prior.split("\n") if l.startswith("#")]
    added = [l for l in hp if l not in hj]
    assert [l.split(",")[0] for l in added] == ["##INFO=<ID=EMAF", "##INFO=<ID=EMNC", "##FORMAT=<ID=SGQ"]
    assert hp.index(added[2]) == hp.index(next(l for l in hp if l.startswith("##FORMAT=<ID=SAL"))) + 1 and [l for l in hp if l not in added] == hj
    # which data row is candidate j of site k: the slots of the call name the keys' slots, in the union's first-seen order
    slot = {}
    for _, counts in _samples():
        for key in counts:
            slot.setdefault(key, len(slot))
    key_of = {v: k for k, v in slot.items()}
    row_of = {r[4]: i for i, r in enumerate(_ROWS) if r[4]}                     # tests/test_joint_ins.py: the key of a data row
    member_rows, seen = set(), {"site": 0, "dots": 0, "nocall": 0}
    for k in range(len(m["slots"])):
        for j in range(6):
            if m["slots"][k, j] == NONE:
                continue
            key = key_of[int(m["slots"][k, j])]
            r = row_of[key]
            covered = [(m["members"][k, s] >> j & 1) and bin(m["members"][k, s]).count("1") >= 2 for s in range(4)]
            if not any(covered):
                continue
            member_rows.add(r)
            assert dp[r][8] == "GT:DP:AD:PL:SGT:SAL:SGQ" and dj[r][8] == "GT:DP:AD:PL:SGT:SAL"
            ns = ac = 0
            for s in range(4):
                fp, fj = dp[r][9 + s].split(":"), dj[r][9 + s].split(":")
                assert fp[1:4] == fj[1:4]                                       # DP, AD, PL byte for byte
                if not covered[s]:
                    assert dp[r][9 + s] == dplain[r][9 + s] + ":.:.:."
                    seen["dots"] += 1
                    g = fp[0]
                else:
                    a, b = (int(x) for x in m["sgt"][k, s])
                    al = 1 + bin(m["members"][k, s] & ((1 << j) - 1)).count("1")
                    assert fp[5] == str(al) == fj[5]
                    if a == NO_CALL:
                        assert fp[0] == "./." and fp[4] == "./." and fp[6] == "."
                        seen["nocall"] += 1
                    else:
                        copies = (a == al) + (b == al)
                        assert fp[0] == ("0/0", "0/1", "1/1")[copies] and fp[4] == "%d/%d" % (a, b) and fp[6] == str(int(m["sgq"][k, s]))
                        seen["site"] += 1
                    g = fp[0]
                if g != "./.":
                    ns, ac = ns + 1, ac + g.count("1")
            info = dp[r][7].split(";")
            want = ["NS=%d" % ns, "AN=%d" % (2 * ns), "AC=%d" % ac] + (["AF=%s" % ("%.6g" % (ac / (2 * ns)))] if ns else [])
            want += ["EMAF=%s" % ("%.6g" % float(m["p_hi"][k, 1 + j]))] + (["EMNC"] if k == 1 else [])
            assert info[-len(want):] == want, (r, info)
    assert seen["site"] >= 10 and seen["dots"] == 3 and len(member_rows) == 5
    for r in range(len(dp)):                                                    # every non-member row is byte for byte the plain --cohort row
        if r not in member_rows:
            assert dp[r] == dplain[r]


def test_emaf_is_left_out_where_no_item_took_part(tmp_path, capsys, monkeypatch):
    """every sample's lists are empty: the sites exist (the keys are present), no item has a read — no estimate, no EMAF, calls all ./."""
    from svjg import capi, genotype
    monkeypatch.setenv("SVJG_PY_VCF", "1")
    monkeypatch.setattr(capi, "Context", SitePriorModelCtx)
    _write_cohort(tmp_path, [(name, {k: (0, 0) for k in counts}) for name, counts in _sample_counts()])
    genotype.run_cohort(str(tmp_path / "cohort.list"), str(tmp_path / "in.vcf"), str(tmp_path / "prior.vcf"), MS, E, joint_ins=True, joint_prior=True)
    capsys.readouterr()
    rows = [d for d in _data((tmp_path / "prior.vcf").read_text()) if d[8].endswith(":SGQ")]
    assert len(rows) == 5 and all("EMAF" not in d[7] and "EMNC" not in d[7] and d[7].endswith("NS=0;AN=0;AC=0") for d in rows)
    assert all(c.startswith("./.") and c.endswith(":./.:%s:." % c.split(":")[5]) for d in rows for c in d[9:] if not c.endswith(":.:.:."))


def test_golden_cohort_with_the_option(golden, tmp_path, monkeypatch):
    """tests/golden/cohort/edited (shared-position insertions): only member rows and the three header lines differ from the run without the option"""
    from svjg import capi, genotype
    from tests import cohort_model as CM
    monkeypatch.setenv("SVJG_PY_VCF", "1")
    monkeypatch.setattr(capi, "Context", SitePriorModelCtx)
    co = CM.Cohort(golden, "edited")
    a, b = str(tmp_path / "joint.vcf"), str(tmp_path / "prior.vcf")
    assert genotype.run_cohort(co.list, co.vcf, a, joint_ins=True) == genotype.run_cohort(co.list, co.vcf, b, joint_ins=True, joint_prior=True)
    joint, prior = open(a).read().split("\n"), open(b).read().split("\n")
    prior = [l for l in prior if not l.startswith(("##INFO=<ID=EMAF,", "##INFO=<ID=EMNC,", "##FORMAT=<ID=SGQ,"))]
    assert len(joint) == len(prior)
    n_member = 0
    for j, p in zip(joint, prior):
        if "\tGT:DP:AD:PL:SGT:SAL\t" in j:
            assert "\tGT:DP:AD:PL:SGT:SAL:SGQ\t" in p
            n_member += 1
            for cj, cp in zip(j.split("\t")[9:], p.split("\t")[9:]):
                assert cj.split(":")[1:4] == cp.split(":")[1:4] and cj.split(":")[5] == cp.split(":")[5]
        else:
            assert j == p
    assert n_member > 0 and len(SitePriorModelCtx.made[-1].site_calls) == 1
