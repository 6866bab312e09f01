"""svjg_genotype_cohort_sites_prior keeps a block of its own (BLOCK_COHORT_SITES_PRIOR), as tests/test_leg_blocks_gpu.py shows of the seven calls
before it: run between them on ONE context, in either order, it returns the bytes it returns on a context of its own, every other call returns
its own, and a view of the diploid call's pinned block outlives it.  Needs an MI355X: run with -m gpu."""
import pytest

from tests.test_leg_blocks_gpu import MS, ERR, R, _bytes, _call, _load, alone, case     # noqa: F401  (alone, case: the fixtures of that file)

pytestmark = pytest.mark.gpu


def _prior(ctx, c):
    return ctx.genotype_cohort_sites_prior(c["sites"], MS, ERR)


@pytest.fixture(scope="module")
def prior_alone(case):
    from svjg import capi
    ctx = capi.Context(0)
    try:
        _load(ctx, case)
        want = _bytes(_prior(ctx, case))
    finally:
        ctx.close()
    assert any(want[1]) and any(want[6]) and any(want[8])               # PLs, posterior calls, frequencies
    return want


@pytest.mark.parametrize("order", [("cohort_sites", "NEW", "cohort_prior", "sites", "NEW", "cohort", "ploidy"),
                                   ("NEW", "cohort", "cohort_sites", "NEW", "cohort_ploidy", "cohort_prior", "NEW")])
def test_the_call_in_a_block_of_its_own(case, alone, prior_alone, order):
    from svjg import capi
    ctx = capi.Context(0)
    try:
        _load(ctx, case)
        view = _call(ctx, case, "rows", view=True)[:4]
        assert _bytes(view) == alone["rows"][:4]
        for which in order:
            if which == "NEW":
                got = _bytes(_prior(ctx, case))
                assert got == prior_alone and got[:6] == alone["cohort_sites"]
            else:
                assert _bytes(_call(ctx, case, which)) == alone[which], which
            assert _bytes(view) == alone["rows"][:4], f"the view after {which}"
            assert ctx.boundary_flags(R).tobytes() == alone["rows"][4], f"the boundary bytes after {which}"
        assert _bytes(_call(ctx, case, "rows")) == alone["rows"]
    finally:
        ctx.close()
