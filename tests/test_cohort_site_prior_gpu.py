"""Joint insertion calls in a cohort under an allele-frequency prior on the GPU (svjg_genotype_cohort_sites_prior, k_cohort_sites_prior) against the
60-digit model's stored answers (tests/site_prior_model.py, tests/golden/cohort_site_prior/): every segment width, one to three items a lane, a
site count that is no multiple of a wave's sites, more sites than one trip of the grid, the table's growth inside the call, chunks, repeats, and
the drop-in script.  Needs an MI355X: run with -m gpu."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import cohort_site_prior_cases as CS
from tests import products_items as PI
from tests import site_prior_model as M
from tests.geno_sim import site_prior as H

pytestmark = pytest.mark.gpu

AMD = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "svjedi-graph_amd")
EM_TOL, EM_MAX_IT, EM_FLAG, P_BOUND = H.constants()
NAMES = ("gt", "pl", "raw", "members", "boundary", "site", "sgt", "sgq", "af", "em_steps", "psite")
MS = 3
_MEASURED = {}


@pytest.fixture(scope="module")
def ctx():
    from svjg import capi
    c = capi.Context(0)
    yield c
    c.close()


def _load(ctx, c):
    PI.load_cohort(ctx, np.ascontiguousarray(c["counts"].transpose(1, 0, 2)).astype(np.uint32), np.ascontiguousarray(c["present"].T) != 0)


def _same(a, b):
    return all(x.shape == y.shape and x.tobytes() == y.tobytes() for x, y in zip(a, b))


@pytest.mark.parametrize("name", [c[0] for c in CS.CASES])
def test_case_against_the_model(ctx, name):
    """the first kernel's six outputs bit for bit those of svjg_genotype_cohort_sites; steps, the not-converged bit and the NaN pattern on every
    site; sgt and sgq on every item the model decides (at most 1 % are not); psite = the sums of the kernel's own sgt; p within SITE_EM_P_BOUND;
    a second call returns the same bytes"""
    c = CS.inputs(name)
    members, raw = CS.first_kernel(c)
    gold = CS.load_golden(name, c)
    assert gold["item_out"].mean() <= M.CAP and not gold["site_out"].any()
    _load(ctx, c)
    plain = ctx.genotype_cohort_sites(c["slots"], MS, CS.ERR)
    got = ctx.genotype_cohort_sites_prior(c["slots"], MS, CS.ERR)
    assert len(got) == 11 and _same(got[:6], plain), "the first kernel's outputs moved"
    assert np.array_equal(got[3], members) and np.array_equal(got[2], raw)
    assert _same(ctx.genotype_cohort_sites_prior(c["slots"], MS, CS.ERR), got), "two calls differ"
    sgt, sgq, af, steps, psite = got[6:]
    est = ~np.isnan(gold["p_hi"][:, 0])
    assert np.array_equal(steps & ~np.uint32(EM_FLAG), gold["steps"]) and np.array_equal((steps & EM_FLAG) != 0, gold["flag"])
    assert np.array_equal(np.isnan(af), np.isnan(gold["p_hi"])) and np.array_equal(np.isnan(af).all(axis=1), ~est)
    want_gt, want_gq = CS.with_support(gold["sgt"], gold["sgq"], raw, MS)
    ok = ~gold["item_out"]
    assert np.array_equal(sgt[ok], want_gt[ok]) and np.array_equal(sgq[ok], want_gq[ok])
    assert np.array_equal(psite, PI.brute_site(sgt, got[3]))
    if est.any():
        d = np.abs((af[est] - gold["p_hi"][est]) - gold["p_lo"][est])
        big = gold["p_hi"][est] > 1e-6
        _MEASURED[name] = (d.max(), (d[big] / gold["p_hi"][est][big]).max() if big.any() else 0.0)
        print("%s: max |p - model| %.3e absolute, %.3e relative among p > 1e-6; genotype_ms %.4f" % ((name,) + _MEASURED[name] + (ctx.kernel_ms()[2],)))
        assert d.max() <= P_BOUND, (name, d.max())
        assert (af[est][:, 0] >= 0).all() and (af[est] <= 1).all() and all((af[k, c["C"][k] + 1:] == 0).all() for k in np.flatnonzero(est))


def test_measured_p_error_report():
    """prints the maximum over the cases run before it in this process (what svjg_geno.h quotes beside SITE_EM_P_BOUND)"""
    if _MEASURED:
        a = max(_MEASURED, key=lambda n: _MEASURED[n][0])
        r = max(_MEASURED, key=lambda n: _MEASURED[n][1])
        print("max absolute %.3e (%s), max relative %.3e (%s), %d cases" % (_MEASURED[a][0], a, _MEASURED[r][1], r, len(_MEASURED)))


def test_first_call_of_a_fresh_context_grows_the_table(ctx):
    """deep_65 holds sites whose s_K lies beyond the first table: on a fresh context both kernels run, the table grows, both run again — what the
    second kernel wrote is rewritten, not added to: the bytes of a second call, and of the warm context"""
    from svjg import capi
    c = CS.inputs("deep_65")
    fresh = capi.Context(0)
    try:
        _load(fresh, c)
        assert fresh.logfact_entries() == 0
        first = fresh.genotype_cohort_sites_prior(c["slots"], MS, CS.ERR)
        assert fresh.logfact_entries() > 65536
        second = fresh.genotype_cohort_sites_prior(c["slots"], MS, CS.ERR)
    finally:
        fresh.close()
    _load(ctx, c)
    assert _same(first, second) and _same(first, ctx.genotype_cohort_sites_prior(c["slots"], MS, CS.ERR))


def test_chunks_equal_one_call(ctx):
    """through svjg.genotype's chunking argument the calls are the same; here the capi's: chunks of 37 sites end inside a wave at every width"""
    for name in ("mixed_3", "mixed_9", "mixed_130"):
        c = CS.inputs(name)
        _load(ctx, c)
        one = ctx.genotype_cohort_sites_prior(c["slots"], MS, CS.ERR)
        parts = [ctx.genotype_cohort_sites_prior(c["slots"][at:at + 37], MS, CS.ERR) for at in range(0, len(c["slots"]), 37)]
        assert _same(one, [np.concatenate([p[k] for p in parts]) for k in range(11)])


@functools.lru_cache(maxsize=None)
def _compute_units():
    """the device's compute units as the library's launch cap counts them, else 256 (asked of torch in a child process: tests/test_cohort_prior_gpu.py says why)"""
    p = subprocess.run([sys.executable, "-c", "import torch; print(torch.cuda.get_device_properties(0).multi_processor_count)"], capture_output=True, text=True)
    last = p.stdout.split()[-1:] if p.returncode == 0 else []
    return int(last[0]) if last and last[0].isdigit() and int(last[0]) > 0 else 256


def _equal_bytes_in_every_copy(got, one, K):
    u = "u%d" % one.dtype.itemsize
    return got.shape == (K * one.shape[0],) + one.shape[1:] and np.array_equal(got.view(u).reshape(K, -1), np.broadcast_to(one.view(u).reshape(1, -1), (K, one.size)))


@pytest.mark.parametrize("name", ["mixed_64", "mixed_3", "mixed_130"])
def test_more_sites_than_one_trip_of_the_grid(ctx, name):
    """The launch is capped at two blocks of two waves a compute unit: a case's sites, repeated until the call has more waves than that plus a
    partial last trip, so that waves take the grid-stride loop a second time and set up the item, n and the site's state again.  Every output of
    every copy has the bytes of the one-trip call on the case itself, which test_case_against_the_model holds to the model."""
    cus = _compute_units()
    c = CS.inputs(name)
    n, per_wave = len(c["slots"]), 64 // H.width(c["S"])
    trip = 4 * cus                                                 # waves
    K = -(-(trip + trip // 8) * per_wave // n)
    waves = -(-K * n // per_wave)
    assert waves > trip and waves % trip != 0 and n <= trip * per_wave
    _load(ctx, c)
    one = ctx.genotype_cohort_sites_prior(c["slots"], MS, CS.ERR)
    got = ctx.genotype_cohort_sites_prior(np.tile(c["slots"], (K, 1)), MS, CS.ERR)
    for k in range(11):
        assert _equal_bytes_in_every_copy(got[k], one[k], K), NAMES[k]


def test_empty_and_bad_calls(ctx):
    from svjg import capi
    c = CS.inputs("mixed_3")
    fresh = capi.Context(0)
    try:
        with pytest.raises(capi.SvjgError) as ei:                  # no matrix
            fresh.genotype_cohort_sites_prior(c["slots"][:5], MS, CS.ERR)
        assert "no cohort matrix" in str(ei.value)
    finally:
        fresh.close()
    _load(ctx, c)
    out = ctx.genotype_cohort_sites_prior(c["slots"][:0], MS, CS.ERR)
    assert [x.shape for x in out] == [(0, 3, 2), (0, 3, 28), (0, 3, 7), (0, 3), (0, 3), (0, 6, 2), (0, 3, 2), (0, 3), (0, 7), (0,), (0, 6, 2)]
    bad = c["slots"][:5].copy()
    bad[2, 1] = bad[2, 0]
    with pytest.raises(capi.SvjgError) as ei:
        ctx.genotype_cohort_sites_prior(bad, MS, CS.ERR)
    assert "twice" in str(ei.value)


def test_script_writes_the_cpu_writers_file(tmp_path, monkeypatch, capsys):
    """predict-genotype.py --cohort LIST --joint-ins --joint-prior on the hand-made cohort of tests/test_cohort_site_prior.py: the device's file
    is the one the writer makes from the model's answers (the model decides every item of that cohort: the CPU test asserts it)"""
    from svjg import capi, genotype
    from tests.test_cohort_site_prior import SitePriorModelCtx, _samples, _write_cohort
    _write_cohort(tmp_path, _samples())
    p = subprocess.run([sys.executable, os.path.join(AMD, "predict-genotype.py"), "--cohort", "cohort.list", "-v", "in.vcf", "-o", "device.vcf", "--joint-ins", "--joint-prior"],
                       capture_output=True, text=True, cwd=tmp_path)
    assert p.returncode == 0, p.stderr
    monkeypatch.setenv("SVJG_PY_VCF", "1")
    monkeypatch.setattr(capi, "Context", SitePriorModelCtx)
    genotype.run_cohort(str(tmp_path / "cohort.list"), str(tmp_path / "in.vcf"), str(tmp_path / "model.vcf"), 3, 5e-5, joint_ins=True, joint_prior=True)
    capsys.readouterr()
    assert (tmp_path / "device.vcf").read_text() == (tmp_path / "model.vcf").read_text()
