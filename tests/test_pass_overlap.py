"""The overlapped fused pass's host decisions, on the CPU: which form the next pass takes, whether svjg_run_end owes a pass its exact
path (the settle step), and what kernel_ms()[0] reports when two launches share an interval — the SAME functions libsvjg_hip.so
compiles (svjedi-graph_amd/csrc/svjg_pass.h through tests/hostsim).  The real thing on a GPU: tests/test_pass_overlap_gpu.py."""
import itertools
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests.hostsim import overlap      # noqa: E402


@pytest.fixture(scope="module")
def logic():
    return overlap.overlap_logic()


def test_form_of_the_next_pass(logic):
    """overlapped only for a context alone on its GPU, a graph whose lines are not all the exact path's, the stamps' clock, and a last
    finished pass that deferred nothing: any one of the four alone keeps the former form"""
    overlaps = logic[0]
    for comm, slow, events, deferred in itertools.product((False, True), repeat=4):
        assert overlaps(comm, slow, events, deferred) == (not (comm or slow or events or deferred))


def test_settle_step(logic):
    """the exact path is owed at svjg_run_end exactly to an overlapped pass that deferred lines and whose lists held; a list that
    overflowed repeats the pass instead (pass_repeats) — never both, never a pass of the former form (its stream ran the exact path)"""
    _, settles, _, repeats = logic
    for comm, slow, overlapped in itertools.product((False, True), repeat=3):
        for overflow in (0, 1, 4, 5):
            for n_def in (0, 1, 7, 40000, 1 << 40):
                want = overlapped and not comm and not slow and overflow == 0 and n_def != 0
                assert settles(comm, slow, overlapped, overflow, n_def) == want
                assert not (settles(comm, slow, overlapped, overflow, n_def) and repeats(comm, overflow, 0))
    assert repeats(False, 1, 0) and not settles(False, False, True, 1, 9)


def test_main_interval_on_hand_made_stamps(logic):
    """t_last(k) - max(t_first(k), t_last(k - 1)): the shared interval of two overlapped launches counts once"""
    ticks = logic[2]
    # first pass / a pass behind a host sync: no pass in front (0) -> first worker's start to last worker's end, the value of before
    assert ticks(1000, 123000, 0) == 122000
    # disjoint (one stream, or run_resident): the pass in front ended before this one's first worker started -> the same old value
    assert ticks(130000, 252000, 123000) == 122000
    assert ticks(130000, 252000, 130000) == 122000
    # overlapping: this one's first worker started under the drain of the pass in front -> from that pass's end
    assert ticks(110000, 240000, 123000) == 240000 - 123000
    # a run of overlapped passes: the reported intervals tile the time from the first start to the last end, nothing counted twice
    stamps = [(0, 1200), (1100, 2350), (2290, 3500), (3400, 4700)]
    total, prev = 0, 0
    for first, last in stamps:
        total += ticks(first, last, prev)
        prev = last
    assert total == 4700
    # fully side by side (grids smaller than the device) and this one ended first: nothing left to report, never a wrapped difference
    assert ticks(100, 900, 1000) == 0
    assert ticks(0, 0, 0) == 0
    # 64-bit stamps
    big = 1 << 62
    assert ticks(big + 10, big + 500, big + 100) == 400
