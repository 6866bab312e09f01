"""Where the rows of a genotype call lie, and how the log10(i!) table grows (svjedi-graph_amd/csrc/svjg_geno.h: rows_layout, ploidy_layout,
sites_layout, run_layout, rows_in, logfact_grow_to), on the CPU through tests/hostsim and tests/geno_sim.  svjg_genotype_view and svjg_run_end hand out pointers into these blocks and
callers keep them, so every offset is pinned to the formula the library used before the layouts had one description: the formulas are
written out HERE, as the expectation.  Besides: no two fields overlap, the last one ends inside the block, and every field is aligned
for its element type."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests.hostsim import sim     # noqa: E402
from tests.geno_sim import ploidy, site    # noqa: E402

NS = (0, 1, 2, 3, 5, 63, 64, 65, 1000)


def _check_block(fields, end):
    """fields: (name, offset, bytes, alignment) in the order they lie in a block that is `end` bytes long"""
    at = 0
    for name, off, size, align in fields:
        assert off >= at, f"{name} overlaps the field in front of it"
        assert off % align == 0, f"{name} at {off} is not {align}-byte aligned"
        at = off + size
    assert at <= end, "the last field ends behind the block"


@pytest.mark.parametrize("n", NS)
def test_step_by_step_block(n):
    L = sim.rows_layout(n)
    maxn = (35 * n + 7) & ~7
    inputs = maxn + 8
    assert L == {"pl": 0, "raw": 24 * n, "gt": 32 * n, "flags": 33 * n, "boundary": 34 * n, "maxn": maxn,
                 "slot": inputs, "type": inputs + 4 * n, "ok": inputs + 5 * n, "total": inputs + 6 * n + 64}
    _check_block([("pl", L["pl"], 24 * n, 8), ("raw", L["raw"], 8 * n, 4), ("gt", L["gt"], n, 1), ("flags", L["flags"], n, 1),
                  ("boundary", L["boundary"], n, 1), ("maxn", L["maxn"], 8, 8), ("slot", L["slot"], 4 * n, 4), ("type", L["type"], n, 1),
                  ("ok", L["ok"], n, 1)], L["total"])


@pytest.mark.parametrize("n", NS)
def test_ploidy_block(n):
    L = ploidy.layout(n)
    maxn = (83 * n + 7) & ~7
    logtab = maxn + 8                                            # the call's logarithms: 2 x 45 doubles
    slot = logtab + 720
    assert L == {"pl": 0, "raw": 72 * n, "gt": 80 * n, "flags": 81 * n, "boundary": 82 * n, "maxn": maxn, "logtab": logtab,
                 "slot": slot, "type": slot + 4 * n, "ok": slot + 5 * n, "ploidy": slot + 6 * n, "in_bytes": 720 + 7 * n,
                 "total": logtab + 720 + 7 * n + 64}
    _check_block([("pl", L["pl"], 72 * n, 8), ("raw", L["raw"], 8 * n, 4), ("gt", L["gt"], n, 1), ("flags", L["flags"], n, 1),
                  ("boundary", L["boundary"], n, 1), ("maxn", L["maxn"], 8, 8), ("logtab", L["logtab"], 720, 8), ("slot", L["slot"], 4 * n, 4),
                  ("type", L["type"], n, 1), ("ok", L["ok"], n, 1), ("ploidy", L["ploidy"], n, 1)], L["total"])
    assert L["ploidy"] + n == L["logtab"] + L["in_bytes"]        # ONE copy in covers the logarithms and the four arrays, and nothing else


@pytest.mark.parametrize("n", NS)
def test_sites_block(n):
    L = site.layout(n, 1, False, own_fields=True)
    maxn = (255 * n + 7) & ~7
    logs = maxn + 8                                              # the call's logarithms: 16 doubles
    assert L == {"pl": 0, "raw": 224 * n, "gt": 252 * n, "boundary": 254 * n, "maxn": maxn, "logs": logs, "slots": logs + 128,
                 "in_bytes": 128 + 24 * n, "total": logs + 128 + 24 * n + 64}
    _check_block([("pl", L["pl"], 224 * n, 8), ("raw", L["raw"], 28 * n, 4), ("gt", L["gt"], 2 * n, 1), ("boundary", L["boundary"], n, 1),
                  ("maxn", L["maxn"], 8, 8), ("logs", L["logs"], 128, 8), ("slots", L["slots"], 24 * n, 4)], L["total"])
    assert L["slots"] + 24 * n == L["logs"] + L["in_bytes"]      # ONE copy in covers the logarithms and the slots, and nothing else


@pytest.mark.parametrize("n", NS)
def test_fused_pass_blocks(n):
    L = sim.rows_layout(n, fused=True)
    status_bytes = sim.geno_constants()[0]                       # sizeof(DevStatus)
    guard_words = sim.pass_logic()[3]
    assert status_bytes >= 8 and guard_words == 3
    h_tail = (23 * n + 63) & ~63
    guard = 8 + ((status_bytes + 7) & ~7)
    tail_bytes = guard + 8 * guard_words
    pl64 = (tail_bytes + 63) & ~63
    assert L == {"pl32": 0, "raw": 12 * n, "gt": 20 * n, "flags": 21 * n, "boundary": 22 * n, "h_tail": h_tail, "out_bytes": h_tail + tail_bytes,
                 "maxn": 0, "status": 8, "guard": guard, "tail_bytes": tail_bytes, "pl64": pl64, "total": pl64 + 24 * n + 64,
                 "slot": 0, "type": 4 * n, "ok": 5 * n, "in_bytes": 6 * n}
    # the pinned host block the results land in, with the copy of the device block's tail behind them
    _check_block([("pl32", L["pl32"], 12 * n, 4), ("raw", L["raw"], 8 * n, 4), ("gt", L["gt"], n, 1), ("flags", L["flags"], n, 1),
                  ("boundary", L["boundary"], n, 1), ("tail", L["h_tail"], L["tail_bytes"], 8)], L["out_bytes"])
    # the device block: the tail (the status block and the guard words hold 64-bit counters), the 64-bit PLs
    _check_block([("maxn", L["maxn"], 8, 8), ("status", L["status"], status_bytes, 8), ("guard", L["guard"], 8 * guard_words, 8)], L["tail_bytes"])
    _check_block([("tail", 0, L["tail_bytes"], 8), ("pl64", L["pl64"], 24 * n, 8)], L["total"])
    assert (L["h_tail"] + L["maxn"]) % 8 == 0                    # max_n as the host reads it
    # the input block the slots share
    _check_block([("slot", L["slot"], 4 * n, 4), ("type", L["type"], n, 1), ("ok", L["ok"], n, 1)], L["in_bytes"])


def test_logfact_growth_rule():
    _, first, cap, grow_to = sim.geno_constants()
    assert first == 65536 and cap == 1 << 24
    for max_n in (1, 65535, 65536, cap - 1026, cap - 1025, cap - 1024, cap - 1):
        want = max_n + 1 + 1024 if max_n < cap - 1024 else cap
        got = grow_to(max_n)
        assert got == want and max_n < got <= cap, max_n
