"""One k_classify_main launch's plan on the CPU: how the text is divided among the workers (region, small chunks, grid), the occupancy cap
and the sizes of the launch's lists — the SAME functions libsvjg_hip.so compiles (svjedi-graph_amd/csrc/svjg_pass.h through tests/hostsim),
against a restatement of the formulas in Python (floats are C doubles, int() truncates as the cast does below 2^53), the properties
the kernel relies on, and one answer worked out by hand."""
import os
import random
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests.hostsim import overlap      # noqa: E402

STRIPE, SMALL_CHUNK, FIRST_SHARE = 8192, 65536, 0.85       # svjg_kernels.h: TEXT; svjg_capi.hip: SMALL_CHUNK, FIRST_CHUNK_SHARE
WORKERS = (1, 14, 3584, 4096)                              # n_cu x occupancy: one CU alone, 256 x 14 (MI355X), 256 x 16
CONFIGS2, CONFIGS3 = 2_133_165_175, 21_621_759_346         # bytes of text of bench.py's configs[2] and configs[3]


@pytest.fixture(scope="module")
def logic():
    return overlap.plan_logic()


def sizes(workers):
    switch = 8 * SMALL_CHUNK * workers                     # (an even share of 8 chunks: the chunked regime begins)
    fixed = [1, STRIPE - 1, STRIPE, STRIPE + 1, workers * STRIPE - 1, workers * STRIPE, workers * STRIPE + 1,
             switch - 1, switch, switch + 1, switch - workers, switch - workers + 1,    # (ceil: the share is 8 chunks from switch - workers + 1 on)
             2 ** 32 - 1, 2 ** 32, 2 ** 32 + 1, CONFIGS2, CONFIGS3, 2 ** 36]
    rng = random.Random(20260 + workers)
    return [n for n in fixed if n >= 1] + [rng.randrange(1, 2 ** rng.randrange(1, 37)) for _ in range(3000)]


def plan_restated(n, workers):
    share = (n + workers - 1) // workers
    region, small = (share + 15) & ~15, 0
    if share >= 8 * SMALL_CHUNK:
        region, small = (int(share * FIRST_SHARE) + 15) & ~15, SMALL_CHUNK
    region = max(region, STRIPE)
    return region, small, min((n + region - 1) // region, workers)


@pytest.mark.parametrize("workers", WORKERS)
def test_plan_is_the_restated_formulas(logic, workers):
    plan = logic[0]
    for n in sizes(workers):
        assert plan(n, workers, STRIPE, SMALL_CHUNK, FIRST_SHARE) == plan_restated(n, workers), (n, workers)


@pytest.mark.parametrize("workers", WORKERS)
def test_plan_has_what_the_kernel_relies_on(logic, workers):
    plan = logic[0]
    regimes = set()
    for n in sizes(workers):
        region, small, grid = plan(n, workers, STRIPE, SMALL_CHUNK, FIRST_SHARE)
        share = (n + workers - 1) // workers
        assert region % 16 == 0 and region >= STRIPE, (n, region)
        assert 1 <= grid <= workers, (n, grid)
        assert small in (0, SMALL_CHUNK), (n, small)
        if small == 0:
            assert grid * region >= n, (n, region, grid)           # every byte has an owner
        else:
            assert grid == workers and region <= share and region >= 0.84 * share, (n, region, grid, share)
        regimes.add((small != 0, grid == workers))
    # fewer workers at a stripe each (none fewer than one); even shares; first chunk + small chunks
    assert regimes == ({(False, False)} if workers > 1 else set()) | {(False, True), (True, True)}


def test_plan_known_answer(logic):
    """configs[2] on 256 CUs x 14 workers, by hand: share ceil(2 133 165 175 / 3584) = 595 192 >= 8 x 65 536, so the first chunk is
    int(595 192 x 0.85) = 505 913 rounded up to 16 = 505 920, small chunks of 65 536, and every one of the 3584 workers has a region"""
    plan = logic[0]
    assert (CONFIGS2 + 3583) // 3584 == 595_192
    assert plan(CONFIGS2, 3584, STRIPE, SMALL_CHUNK, FIRST_SHARE) == (505_920, 65_536, 3_584)
    # the switch itself: an even share of 8 chunks less one byte is still divided evenly
    assert plan((8 * SMALL_CHUNK - 1) * 3584, 3584, STRIPE, SMALL_CHUNK, FIRST_SHARE) == (524_288, 0, 3_584)
    assert plan((8 * SMALL_CHUNK - 1) * 3584 + 1, 3584, STRIPE, SMALL_CHUNK, FIRST_SHARE) == (445_648, 65_536, 3_584)


def test_occupancy_cap(logic):
    """LDS comes in granules: 160 KB / (lds rounded up to the granule) workgroups a CU, where the API may say one more"""
    occ = logic[1]
    assert occ(10, 15_568, 1280) == 9           # 15 568 B -> 13 granules = 16 640 B; 163 840 / 16 640 = 9
    assert occ(16, 11_520, 1280) == 14          # 9 granules exactly
    assert occ(16, 11_521, 1280) == 12          # one byte more: 10 granules
    assert occ(8, 11_520, 1280) == 8 and occ(1, 11_520, 1280) == 1      # (the API's answer holds where it is the smaller)
    assert occ(4, 200_000, 1280) == 4           # (a workgroup beyond 160 KB: the cap does not apply, the launch itself fails)
    for api in range(1, 33):
        for lds in (1, 1279, 1280, 1281, 10_240, 11_520, 12_800, 65_536, 163_840):
            assert occ(api, lds, 1280) == min(api, 163_840 // ((lds + 1279) // 1280 * 1280))


@pytest.mark.parametrize("all_slow", (False, True))
def test_list_sizes(logic, all_slow):
    """the three lists of a step-by-step call — first attempt, and after each overflow bit — and the fused pass's own"""
    _, _, first, grown, fused = logic
    rng = random.Random(7 + all_slow)
    for n in [1, 23, 24, 39, 40, 4095, 4096, 2 ** 32 + 1, CONFIGS2, CONFIGS3] + [rng.randrange(1, 2 ** 36) for _ in range(300)]:
        recs, host = rng.randrange(0, 2 ** 30), rng.randrange(0, 2 ** 20)
        deferred = n // 24 + 64 if all_slow else n // 4096 + 65536
        assert first(all_slow, True, n, recs, host) == (deferred, recs + n // 40 + 65536, host + 4096)
        assert first(all_slow, False, n, recs, host) == (deferred, 0, host + 4096)
        assert fused(all_slow, n) == (deferred, 0, 4096)
        s = first(all_slow, True, n, recs, host)
        after = recs + rng.randrange(0, 2 ** 28)
        for bits in range(8):
            want = (n // 24 + 64 if bits & 1 else s[0],
                    recs + (after - recs) * 2 + n // 24 + 64 if bits & 2 else s[1],
                    host + n // 24 + 64 if bits & 4 else s[2])
            assert grown(s, n, recs, host, after, bits) == want, (n, bits)


def test_sweep_under_sanitizers():
    """the same functions over the same kind of sweep in a stand-alone program built with AddressSanitizer and UBSan"""
    p = subprocess.run([overlap.build_main()], capture_output=True, text=True)
    assert p.returncode == 0 and p.stdout.startswith("overlap_sim ok:"), p.stdout + p.stderr
    assert "runtime error" not in p.stderr and "AddressSanitizer" not in p.stderr
