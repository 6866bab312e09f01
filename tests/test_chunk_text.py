"""tests/chunk_text.py without a GPU: the texts for k_classify_main's chunked regime are what they claim to be — every feature at its
offset from its chunk boundary, the plan chunked, every kind of feature on a region end and on a small-chunk end over the set of texts
of W workers — and the two oracles agree on them (counts and line numbers by oracle/oracle_c, the JSON by oracle/oracle_py), so that
tests/test_chunked_handover_gpu.py compares the kernel with fixtures that are sound before a GPU sees them."""
import json

import numpy as np
import pytest

from tests import chunk_text as T
from tests.test_main_plan import SMALL_CHUNK, plan_restated

VARIANTS = [(W, rot, end) for W in (1, 3) for rot, end in T.variants(W)]


def test_bounds_are_the_restated_plan():
    """bounds() against plan_restated, by hand at W = 3: n = 5 520 000 -> share 1 840 000, first chunk int(1 564 000.0) = 1 564 000 (a multiple of 16)"""
    assert plan_restated(5_520_000, 3) == (1_564_000, SMALL_CHUNK, 3)
    ends_r, ends_s = T.bounds(5_520_000, 3)
    assert ends_r == [1_564_000, 3_128_000, 4_692_000]
    assert ends_s == [4_692_000 + j * 65_536 for j in range(1, 13)] and ends_s[-1] < 5_520_000 <= ends_s[-1] + 65_536
    assert T.n_chunks(5_520_000, 3) == 13
    with pytest.raises(AssertionError):
        T.bounds(8 * SMALL_CHUNK * 3 - 3, 3)                                    # (even shares: not a chunked plan)


@pytest.mark.parametrize("W", (1, 3))
def test_texts_are_what_they_claim(W):
    cases = T.cases(W)
    T.coverage(cases)
    assert {c.end for c in cases} == {"partial", "exact"}
    for c in cases:
        T.check(c)
        region, small, grid = plan_restated(len(c.text), W)
        assert small == SMALL_CHUNK and grid == W and c.chunks >= 12 and len(c.text) <= 8 << 20
        assert len(c.text) >= 8 * SMALL_CHUNK * W
        assert {sub for _, sub, _ in c.placed} >= {"5", "6"}                     # (lines beyond the stage in every text: the exact path takes them)
        print(W, c.rot, c.end, len(c.text), "bytes, plan", c.plan, c.chunks, "chunks;", " ".join(f"{sub}@{w[0]}" for _, sub, w in c.placed))


def test_check_notices_a_text_shifted_by_one_byte():
    """the conditions are read off the finished bytes: the same text with one byte more in front of it fails them"""
    c = T.build(3, 0, "partial")
    shifted = T.Case()
    shifted.__dict__.update(c.__dict__)
    shifted.text = c.text[:40].replace(b"\t", b"x\t", 1) + c.text[40:-1]          # (the same length: the plan stays)
    assert len(shifted.text) == len(c.text)
    with pytest.raises(AssertionError):
        T.check(shifted)


@pytest.mark.parametrize("W", (1, 3))
def test_texts_tell_ownership_rules_apart(W):
    """What the texts can show, counted here without a kernel: a worker owns the line starts in [lo, hi) of its chunk, and the chunks' sums are
    the oracle's n_lines.  A rule that also takes the start AT hi counts a line twice, one that leaves out the start at lo never counts it, one
    that begins a line behind every "\r" or "\n" finds an empty line inside a split "\r\n": every text of the set tells each of them from the
    right rule, at a region end or a small-chunk end."""
    for c in T.cases(W):
        _, _, n_lines, _, _ = T.oracles(W, c.rot, c.end)
        a = np.frombuffer(c.text, dtype=np.uint8)
        term = (a == 10) | ((a == 13) & (np.append(a[1:], 0) != 10))             # "\n", or a "\r" that no "\n" follows
        starts = np.concatenate(([0], np.flatnonzero(term) + 1))
        starts = starts[starts < len(a)]
        ends_r, ends_s = T.bounds(len(a), W)
        cuts = np.array([0] + ends_r + ends_s + [len(a)])
        lo, hi = cuts[:-1], cuts[1:]
        count = lambda left, right: int(sum(((starts >= l) & (starts < r)).sum() for l, r in zip(left, right)))
        assert len(starts) == n_lines == count(lo, hi)
        assert count(lo, hi + 1) > n_lines                                        # a line start exactly at a boundary: counted twice
        assert count(np.where(lo > 0, lo + 1, 0), hi) < n_lines                   # ... or never
        naive = np.flatnonzero((a == 10) | (a == 13)) + 1
        assert (naive < len(a)).sum() + 1 > n_lines                               # a "\r\n" pair somewhere: an empty line for the naive rule
        on_b = {int(b) for b in ends_r + ends_s}
        assert any(int(s) in on_b for s in starts) and any(a[b - 1] == 13 and a[b] == 10 for b in on_b)


@pytest.mark.parametrize("W,rot,end", VARIANTS + [(3, -1, "partial")])
def test_oracles_agree(W, rot, end):
    from oracle import oracle_py
    c = T.build_clean(W) if rot < 0 else T.build(W, rot, end)
    orc, want, n_lines, ref_text, py_counts = T.oracles(W, rot, end)
    assert n_lines == len(T.text_lines(c.text)) > 1000
    c_counts = {sv: (int(want[i, 0]), int(want[i, 1])) for i, sv in enumerate(orc.sv_ids) if want[i].sum()}
    assert c_counts == py_counts and want.sum() > 5000
    # the JSON holds every hit of the count vector once: as many list entries as the C oracle counted
    assert sum(a + b for a, b in oracle_py.counts_of(json.loads(ref_text)).values()) == int(want.sum())
    assert np.array_equal(T.oracles(W, rot, end)[1], want)                       # (computed once, handed out unchanged)
