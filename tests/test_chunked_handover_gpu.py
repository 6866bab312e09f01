"""k_classify_main in its CHUNKED regime — a fixed first chunk per worker, then 64 KB chunks from the counter DevStatus::next_chunk to
whoever asks next — on texts of a few megabytes: svjg_set_main_workers makes the launch plan for W = 1 or 3 workers, so the regime every
headline number runs in begins at 8 x 65 536 x W bytes instead of 1.88 GB.  tests/chunk_text.py puts a line start, a split "\r\n", a node
name, an id:f: tag, a line beyond the stage, a line that covers a whole chunk, a run of tiny lines or a path of 65..216 nodes on EVERY chunk
boundary (tests/test_chunk_text.py holds the texts to that without a GPU), and svjg_last_main_plan tells that the launch really was chunked
and how often it asked the counter.  Every comparison is exact: counts and line numbers against oracle/oracle_c, the JSON text — each hit
once, in file order, with its line's offset — against oracle/oracle_py.  Needs an MI355X: run with -m gpu."""
import numpy as np
import pytest

from tests import chunk_text as T
from tests.test_main_plan import SMALL_CHUNK

pytestmark = pytest.mark.gpu

MS, ERR = 3, 0.00005
VARIANTS = [(W, rot, end) for W in (1, 3) for rot, end in T.variants(W)]


@pytest.fixture(scope="module")
def graphs():
    from svjg.graph import Graph
    P = T.pool()
    return {all_slow: Graph(P.edges, P.alt, all_slow=all_slow) for all_slow in (False, True)}


def _context(W, g):
    from svjg import capi
    c = capi.Context(0)
    c.set_main_workers(W)
    c.load_graph(g)
    return c


def _want(W, rot, end, g):
    """(case, its bytes as an array, the C oracle's counts in the graph's slot order, n_lines, the Python oracle's JSON text)"""
    case = T.build_clean(W) if rot < 0 else T.build(W, rot, end)
    orc, want, n_lines, ref_text, _ = T.oracles(W, rot, end)
    by_slot = np.zeros((g.n_slots, 2), dtype=np.uint32)
    for i, sv in enumerate(orc.sv_ids):
        if want[i].sum():
            by_slot[g.slot_of[sv]] = want[i]
    return case, np.frombuffer(case.text, dtype=np.uint8), by_slot, n_lines, ref_text


def _chunked(c, case):
    """the last launch's plan is the restated one, chunked, and every worker ended on exactly one failing claim"""
    region, small, grid, claimed = c.last_main_plan()
    assert (region, small, grid) == case.plan and small == SMALL_CHUNK and grid == case.W
    assert claimed == case.chunks + grid, (claimed, case.chunks, grid)
    return region, small, grid, claimed


@pytest.mark.parametrize("all_slow", (False, True))
@pytest.mark.parametrize("W,rot,end", VARIANTS)
def test_boundaries(graphs, W, rot, end, all_slow, tmp_path):
    """one text of the set of W workers (the deal of the features rotated by `rot`), main kernel and exact path"""
    from svjg import capi
    g = graphs[all_slow]
    case, data, want, n_lines, ref_text = _want(W, rot, end, g)
    c = _context(W, g)
    try:
        c.upload(data)
        c.classify_resident(want_hits=True)
        plan = _chunked(c, case)
        print(f"W={W} rot={rot} end={end} all_slow={all_slow}: {len(data)} bytes, plan region={plan[0]} small = {plan[1]} grid={plan[2]}, "
              f"{plan[3]} claims ({case.chunks} chunks), kernel_ms={tuple(round(x, 4) for x in c.kernel_ms())}")
        assert np.array_equal(c.counts(), want) and want.sum() > 5000
        st, cause = c.stats(), c.defer_causes()
        assert st["n_lines"] == n_lines
        capi.write_informative_json(str(tmp_path / "o.json"), data, c.hits(), g.sv_ids)
        assert open(tmp_path / "o.json").read() == ref_text
        if not all_slow:
            # the lines beyond the stage whose tail holds "d:" took the exact path; most lines stayed in the main kernel (the generators' own
            # tests hold them to less than half: test_random_graphs, test_long_path_fuzz)
            assert cause["whole_stripe"] > 0 and st["n_deferred"] < 0.5 * n_lines, (st, cause)
    finally:
        c.close()


@pytest.mark.parametrize("W", (1, 3))
def test_both_ends_of_the_text(graphs, W):
    """the text ends without a terminator inside a partial last chunk / the small chunks end exactly at n_bytes, so that the first failing
    claim is `pos == n_bytes`"""
    g = graphs[False]
    seen = set()
    for rot, end in T.variants(W)[:2]:
        case, data, want, n_lines, _ = _want(W, rot, end, g)
        rest = len(data) - case.W * case.plan[0]
        if end == "partial":
            assert rest % SMALL_CHUNK != 0 and data[-1] not in (10, 13)
        else:
            assert rest == case.chunks * SMALL_CHUNK and data[-1] == 10
        c = _context(W, g)
        try:
            c.upload(data)
            c.classify_resident()
            print(f"W={W} end={end}: plan and claims {_chunked(c, case)}, {rest} bytes in small chunks")
            assert np.array_equal(c.counts(), want) and c.stats()["n_lines"] == n_lines
        finally:
            c.close()
        seen.add(end)
    assert seen == {"partial", "exact"}


@pytest.mark.parametrize("W", (1, 3))
def test_step_calls_repeat(graphs, W):
    """two launches into the same count vector: twice the counts, and the chunk counter starts each launch at zero"""
    g = graphs[False]
    rot, end = T.variants(W)[-1]
    case, data, want, n_lines, _ = _want(W, rot, end, g)
    c = _context(W, g)
    try:
        c.upload(data)
        for k in (1, 2):
            c.classify_resident()
            _chunked(c, case)
            assert np.array_equal(c.counts(), want * k)
        assert c.stats()["n_lines"] == 2 * n_lines
    finally:
        c.close()


class Rows:
    """one VCF row per count slot: raw[r] of a pass is the count vector's entry r"""

    def __init__(self, n_slots):
        self.sv_type = (np.arange(n_slots) % 4).astype(np.uint8)
        self.slot = np.arange(n_slots, dtype=np.uint32)
        self.ok = np.ones(n_slots, dtype=np.uint8)


def test_fused_passes(graphs):
    """Three passes with two in flight, then one run_resident, under the chunked plan: every pass's raw counts are the oracle's, its plan is
    chunked and its own status block's counter says chunks + grid — a counter not zero when a pass starts would hand out fewer chunks than
    the text has (lines never counted) and read differently here.  First on a text that defers nothing (asserted), so that all passes run in
    the overlapped form, two main kernels alive at once on a status block each; then on a text whose long lines are deferred: its first two
    passes are overlapped and settled by run_end, the others run with the exact path on their stream."""
    W = 3
    g = graphs[False]
    rows = Rows(g.n_slots)
    c = _context(W, g)
    try:
        c.set_rows(rows.sv_type, rows.slot, rows.ok)
        for rot, end, defers in ((-1, "partial", False), (0, "partial", True)):
            case, data, want, n_lines, _ = _want(W, rot, end, g)
            c.upload(data)

            def ended(got):
                raw = np.array(got[2])
                assert np.array_equal(raw, want) and want.sum() > 5000
                st = c.stats()
                assert st["n_lines"] == n_lines and (st["n_deferred"] > 0) == defers, st
                return _chunked(c, case)

            c.run_begin(MS, ERR); c.run_begin(MS, ERR)
            plans = [ended(c.run_end())]
            c.run_begin(MS, ERR)
            plans += [ended(c.run_end()), ended(c.run_end())]
            plans.append(ended(c.run_resident(MS, ERR)))
            assert np.array_equal(c.counts(), want)
            print(f"fused, defers={defers}: {len(data)} bytes, plans and claims {plans}")
    finally:
        c.close()


def test_cap_is_per_context(graphs):
    """a second context without the cap plans even shares for the same text, and counts the same"""
    from svjg import capi
    W = 3
    g = graphs[False]
    rot, end = T.variants(W)[0]
    case, data, want, n_lines, _ = _want(W, rot, end, g)
    capped = _context(W, g)
    plain = capi.Context(0)
    try:
        plain.load_graph(g)
        for c in (capped, plain):
            c.upload(data)
            c.classify_resident()
        _chunked(capped, case)
        region, small, grid, claimed = plain.last_main_plan()
        print("without the cap:", (region, small, grid, claimed))
        assert small == 0 and claimed == 0 and grid > W and grid * region >= len(data)
        assert np.array_equal(plain.counts(), want) and np.array_equal(capped.counts(), want)
        assert plain.stats()["n_lines"] == capped.stats()["n_lines"] == n_lines
        capped.set_main_workers(0)                                            # (0 takes the cap off again)
        capped.reset_counts()
        capped.classify_resident()
        assert capped.last_main_plan() == (region, small, grid, 0) and np.array_equal(capped.counts(), want)
    finally:
        capped.close()
        plain.close()
