"""Texts of a few megabytes for k_classify_main's CHUNKED regime (svjg_pass.h: main_plan with small != 0 — a fixed first chunk per worker, the
rest in 64 KB chunks to whoever asks the counter next), which begins at 8 x 65 536 x W bytes once the plan is made for W workers
(svjg_set_main_workers): every chunk boundary of such a text carries one chosen feature at a chosen offset.  TEST INFRASTRUCTURE:
tests/test_chunk_text.py (no GPU: the conditions below and the two oracles against each other), tests/test_chunked_handover_gpu.py.

The boundaries `b` of a text of n bytes (bounds): the region ends k * region, k = 1..W, and behind them the small-chunk ends
W * region + j * 65 536 that lie inside the text.  A worker owns the lines that START in its chunk.  Sub-kinds, dealt to the boundaries in turn:

  1a  a line starts exactly at b ("\n" at b - 1)         1b  a line starts at b - 1              1c  a line starts at b + 1 ("\n" at b)
  2a  "\r" at b - 1 and "\n" at b                        2b  a lone "\r" at b - 1, the next line at b
  3a  b inside a node name of a line with hits           3b  b between two nodes of such a line (b is the "<" / ">")
  4   b inside an id:f: tag: "d" at b - 1, ":" at b
  5   b inside a line longer than the 8 KB stage whose tail holds the byte pair "d:": the exact path
  6   one line of more than 2 x 64 KB covers a whole small chunk and both its ends; no line starts in that chunk
  7   b inside a run of tiny lines: more than 64 line starts in any 8 KB around b
  8   a path of 65..216 nodes straddles b
  9   the end of the text (`end`): "partial" — no terminator, inside a partial last chunk; "exact" — n - W * region is a multiple of 65 536,
      so the first failing claim lands at exactly n_bytes

Lines come from tests/graph_fuzz.make_case (hub nodes, both alleles) and tests/longpath_fuzz.make_case, on the union of their graphs (a
graph_fuzz seed whose chromosomes the long-path graph does not have).  Every feature line but the tiny runs' is a line WITH hits, so a line
counted twice or never shows in the counts.  Filler lines are padded in a trailing cg:Z: tag (the JSON text stops in front of it).

The plan depends on the length and the length on the padding: the builder chooses n FIRST (the fixed point is then the one line padded in
front of every feature, and the last line of the text), builds from left to right, and then asserts on the finished bytes that every
feature sits where it claims, that the plan is chunked (small == 65 536, grid == W) with at least 12 small chunks, and n <= 8 MB.

One text has W region ends and eight kinds of feature, so no single text can put every kind on a region end: a SET of texts per W
(variants(W): the deal rotated) does, and coverage() asserts it over the set — every kind on at least one region end and on at least one
small-chunk end."""
import functools
import io
import random

import numpy as np

from tests import graph_fuzz, longpath_fuzz
from tests.test_main_plan import SMALL_CHUNK, plan_restated

SUB = ("1a", "2a", "3a", "4", "5", "7", "8", "1b", "2b", "3b", "1c")      # dealt in turn; kind = the digit.  Kind 6 takes a chunk (two boundaries) of its own
KINDS = ("1", "2", "3", "4", "5", "6", "7", "8")
STAGE = 8192                                                            # svjg_kernels.h: TEXT
N_PARTIAL = 5_520_000                                                   # 0.15 n = 12.6 small chunks: 13, the last one partial
MAX_BYTES = 8 << 20


def bounds(n, W):
    """-> (region ends k * region for k = 1..W, small-chunk ends W * region + j * 65 536 inside the text, j >= 1), by tests/test_main_plan.py: plan_restated"""
    region, small, grid = plan_restated(n, W)
    assert small == SMALL_CHUNK and grid == W, (n, W, region, small, grid)
    return [k * region for k in range(1, W + 1)], list(range(W * region + small, n, small))


def n_chunks(n, W):
    """small chunks of the plan: successful claims of a launch (every worker adds one failing claim)"""
    region, small, grid = plan_restated(n, W)
    return -(-(n - grid * region) // small)


def variants(W):
    """the set of texts of W workers: (rotation of the deal, version of the text's end); the last one puts kind 6 on the first small chunk,
    whose lower end is the region end W * region"""
    rots = list(range(0, 7, W))                                  # seven kinds go to W region ends a text ...
    if 7 - rots[-1] > W - 1:                                     # ... but W - 1 in the last one
        rots.append(rots[-1] + W)
    return tuple((r, ("partial", "exact")[i % 2]) for i, r in enumerate(rots))


def _choose_n(W, end):
    if end == "partial":
        n = N_PARTIAL
        while not 8192 <= (n - W * plan_restated(n, W)[0]) % SMALL_CHUNK <= 57344:
            n += 20_011
        return n
    # n - W * region climbs by one per byte between its drops (region is rounded up to 16), so it meets every multiple of the chunk
    for n in range(N_PARTIAL + 100_000, N_PARTIAL + 700_000):
        if (n - W * plan_restated(n, W)[0]) % SMALL_CHUNK == 0:
            return n
    raise AssertionError("no length with an exact number of small chunks")


class Pool:
    """the lines and the graph every text of this module is made of (built once)"""

    def __init__(self):
        from oracle import oracle_py
        lp_edges, lp_alt, lp_lines, _ = longpath_fuzz.make_case(4100, n_lines=60, n_fatal=0)
        lp_chroms = {k.split("@")[0].rsplit(":", 1)[0] for k in lp_edges} | {k.split("@")[2].rsplit(":", 1)[0] for k in lp_edges}
        for seed in range(5100, 5200):
            gf_edges, gf_alt, gf_lines = graph_fuzz.make_case(seed, 1500)
            gf_chroms = {k.split("@")[0].rsplit(":", 1)[0] for k in gf_edges} | {k.split("@")[2].rsplit(":", 1)[0] for k in gf_edges}
            if not gf_chroms & lp_chroms:
                break
        else:
            raise AssertionError("no graph_fuzz seed with chromosomes of its own")
        assert not set(gf_edges) & set(lp_edges) and not set(gf_alt) & set(lp_alt)
        self.edges = {**lp_edges, **gf_edges}
        self.alt = {**lp_alt, **gf_alt}
        self.lines = [l.encode() for l in lp_lines + gf_lines]
        n_hits = [len(oracle_py.classify_line(l, self.edges, self.alt)) for l in lp_lines + gf_lines]
        self.hits = [k > 0 for k in n_hits]
        self.n_nodes = [len([s for s in l.split(b"\t")[5].replace(b"<", b">").split(b">") if s]) for l in self.lines]
        self.short = [l for l in self.lines if len(l) < 1000]
        # (a line's text goes into the JSON once per hit — a path of a hundred nodes is a megabyte of JSON —, so the filler takes one line in
        #  three hundred from those that weigh 3 KB and more there)
        weight = [len(l.split(b"cg:Z:")[0]) * k for l, k in zip(self.lines, n_hits)]
        self.plain = [l for l, w in zip(self.lines, weight) if w < 3000 and len(l) < 4000]
        self.rare = [l for l, w in zip(self.lines, weight) if not (w < 3000 and len(l) < 4000)]
        # lines with hits: plain ones of 3..40 nodes (features 1..6), and paths of 65..216 nodes (feature 8)
        self.hit_lines = [l for l, h, k in zip(self.lines, self.hits, self.n_nodes) if h and 3 <= k <= 40 and len(l) < 1500 and b"id:f:" not in l and b"cg:Z:" not in l]
        self.long_paths = [l for l, h, k in zip(self.lines, self.hits, self.n_nodes) if h and 65 <= k <= 216]
        assert len(self.hit_lines) >= 50 and len(self.long_paths) >= 8, (len(self.hit_lines), len(self.long_paths))
        # a tiny line with a hit: two neighbouring reference nodes of the long-path graph, 100 bp and more on either side
        self.tiny = None
        for key in sorted(lp_edges):
            l, sl, r, sr = key.split("@")
            if sl == sr == "+" and "." not in l.split(":")[-1] + r.split(":")[-1] and len(key) < 44:
                tl = sum(int(x.split(":")[-1].split("-")[1]) - int(x.split(":")[-1].split("-")[0]) + 1 for x in (l, r))
                line = f"t%d\t9\t0\t9\t+\t>{l}>{r}\t{tl}\t0\t{tl}\t9\t9\t%d\n"
                if oracle_py.classify_line(line % (0, 0), self.edges, self.alt):
                    self.tiny = line
                    break
        assert self.tiny and len(self.tiny) < 100


@functools.lru_cache(maxsize=None)
def pool():
    return Pool()


def _path_span(line):
    """(offset of the path column in the line, its length)"""
    cols = line.split(b"\t")
    at = sum(len(c) + 1 for c in cols[:5])
    return at, len(cols[5])


def _pad_tag(line, total):
    """the line (terminated by "\n") made `total` bytes long by a trailing cg:Z: tag"""
    k = total - len(line) - 6
    assert k >= 1, (len(line), total)
    return line[:-1] + b"\tcg:Z:" + (b"50M2D40M" * (k // 8 + 1))[:k] + b"\n"


def _feature(P, sub, i, rot):
    """-> (block of bytes, offset in the block that has to land on the boundary) for sub-kind `sub` at the i-th boundary"""
    h = P.hit_lines
    A, B = h[(7 * i + rot) % len(h)], h[(7 * i + rot + 3) % len(h)]
    if sub == "1a":
        return A, 0
    if sub == "1b":
        return A, 1
    if sub == "1c":
        return A, -1
    if sub == "2a":
        return A[:-1] + b"\r\n" + B, len(A)                         # "\r" at len(A) - 1, "\n" at len(A)
    if sub == "2b":
        return A[:-1] + b"\r" + B, len(A)                           # "\r" at len(A) - 1, B starts at len(A)
    if sub in ("3a", "3b"):
        at, ln = _path_span(A)
        path = A[at:at + ln]
        marks = [k for k in range(1, ln) if path[k] in b"<>"]      # the second node's orientation sign and those behind it
        m = marks[len(marks) // 2]
        return A, at + m + (4 if sub == "3a" else 0)               # (names are 8 bytes and longer: four behind the sign is inside one)
    if sub == "4":
        cols = A[:-1].split(b"\t")
        line = b"\t".join(cols[:12] + [b"id:f:0.9875"] + cols[12:]) + b"\n"
        return line, sum(len(c) + 1 for c in cols[:12]) + 2          # "id:f:": "d" at + 1, ":" at + 2
    if sub == "5":
        tail = (b"50M2D40M" * 3000)
        line = A[:-1] + b"\tcg:Z:" + tail[:14000] + b"\txd:Z:" + tail[:6000] + b"\n"
        return line, (len(A) + 3000, 9000, 12000, 16000)[i % 4]     # inside the first 8 KB, and at three places beyond them
    if sub == "7":
        run = b"".join((P.tiny % (k, k % 61)).encode() for k in range(400))      # 50..80 bytes a line: > 100 line starts in 8 KB
        assert len(run) > 2 * STAGE
        return run, len(run) // 2 + (0, 1, 7, 40)[i % 4]
    if sub == "8":
        L = P.long_paths[(i + rot) % len(P.long_paths)]
        at, ln = _path_span(L)
        return L, at + ln // 2
    raise AssertionError(sub)


def _chunk_line(P, i, rot):
    """feature 6: a line of 2 x 64 KB and more with hits; odd rotations: the pair "d:" in its tail (the exact path)"""
    A = P.hit_lines[(11 * i + rot) % len(P.hit_lines)]
    tail = b"50M2D40M" * 20000
    mid = b"\txd:Z:" if rot % 2 else b"50M2D4"
    return A[:-1] + b"\tcg:Z:" + tail[:66000] + mid + tail[:66000] + b"\n"


class Case:
    """one text and what the builder knows about it (build, build_clean)"""


@functools.lru_cache(maxsize=None)
def build(W, rot=0, end="partial"):
    """one text: -> Case with .text (bytes), .W, .n, .plan = (region, small, grid), .chunks, .placed = [(boundary, sub-kind, "region" | "small")],
    .edges, .alt.  The conditions of the module's docstring are asserted here, on the finished bytes."""
    P = pool()
    rng = random.Random(1000 * W + 10 * rot + (end == "exact"))
    n = _choose_n(W, end)
    region, small, grid = plan_restated(n, W)
    ends_r, ends_s = bounds(n, W)
    C = n_chunks(n, W)
    first_small = W * region
    c6 = 0 if rot == variants(W)[-1][0] else 4 + rot % 5                       # the small chunk feature 6 covers: [first_small + c6 * 65536, + 65536)
    lo6, hi6 = first_small + c6 * small, first_small + (c6 + 1) * small
    assert hi6 < n
    todo = []                                                                   # (start of the block, block, boundary, sub-kind, where)
    free = [(b, "region") for b in ends_r] + [(b, "small") for b in ends_s]
    free = [(b, w) for b, w in free if b not in (lo6, hi6)]
    six = _chunk_line(P, c6, rot)
    todo.append((lo6 - 36000 - 16 * rot, six, lo6, "6", "region" if c6 == 0 else "small"))
    for i, (b, where) in enumerate(free):
        sub = SUB[(i + rot) % len(SUB)]
        block, a = _feature(P, sub, i, rot)
        if b - a + len(block) + 6000 > n:                                       # (the last boundary may lie too close to the text's end)
            continue
        todo.append((b - a, block, b, sub, where))
    todo.sort()
    out, pos, fill = [], 0, 0
    order = list(range(len(P.plain)))
    rng.shuffle(order)

    def filler_to(target, last_terminated=True):
        """filler lines up to exactly `target`: the last of them padded"""
        nonlocal pos, fill
        assert target - pos >= 1100 or target == pos, (pos, target)
        while target - pos > 4000:
            fill += 1
            if target - pos <= 40_000:
                l = P.short[(fill * 13) % len(P.short)]
            else:
                l = P.rare[(fill // 300 * 7 + rot) % len(P.rare)] if fill % 300 == 150 else P.plain[order[fill % len(order)]]
            if len(l) < 1000 and rng.random() < 0.7:
                l = _pad_tag(l, len(l) + 7 + rng.randrange(2600))
            out.append(l); pos += len(l)
        if target > pos:
            fill += 1
            l = _pad_tag(P.short[(fill * 13) % len(P.short)], target - pos + (0 if last_terminated else 1))
            out.append(l if last_terminated else l[:-1]); pos = target

    for start, block, b, sub, where in todo:
        filler_to(start)
        out.append(block); pos += len(block)
    filler_to(n, last_terminated=end == "exact")
    text = b"".join(out)
    c = Case()
    c.text, c.W, c.n, c.plan, c.chunks, c.end, c.rot = text, W, n, (region, small, grid), C, end, rot
    c.placed = [(b, sub, where) for _, _, b, sub, where in todo] + [(hi6, "6", "small")]
    c.edges, c.alt = P.edges, P.alt
    check(c)
    return c


def _line_around(text, b):
    """(start, end) of the line that holds byte b: end = offset of its terminator (or the text's length)"""
    s = max(text.rfind(b"\n", 0, b), text.rfind(b"\r", 0, b)) + 1
    e = len(text)
    for t in (b"\n", b"\r"):
        k = text.find(t, b)
        if k >= 0:
            e = min(e, k)
    return s, e


def check(c):
    """the conditions, on the finished text: every feature sits where it claims; the plan is chunked"""
    from oracle import oracle_py
    text, W, n = c.text, c.W, len(c.text)
    assert n == c.n and n <= MAX_BYTES
    region, small, grid = plan_restated(n, W)
    assert (region, small, grid) == c.plan and small == SMALL_CHUNK and grid == W
    assert c.chunks == -(-(n - W * region) // small) >= 12
    ends_r, ends_s = bounds(n, W)
    assert len(ends_r) == W and len(ends_s) == c.chunks - 1 and all(0 < b < n for b in ends_r + ends_s)
    assert b"\n\n" not in text and b"\r\r" not in text and b"\n\r" not in text and text[:1] not in (b"\n", b"\r")      # no empty line: the reference refuses one
    nl = np.frombuffer(text, dtype=np.uint8)
    starts = np.flatnonzero((nl == 10) | ((nl == 13) & (np.append(nl[1:], 0) != 10))) + 1       # line starts behind a terminator
    is_name = lambda ch: ch not in b"<>\t\n\r"

    def hits_of(s, e):
        return oracle_py.classify_line(text[s:e].decode() + "\n", c.edges, c.alt)

    for b, sub, where in c.placed:
        assert b in (ends_r if where == "region" else ends_s), (b, sub, where)
        s, e = _line_around(text, b)
        if sub == "1a":
            assert text[b - 1] == 10 and s == b and hits_of(s, e)
        elif sub == "1b":
            assert text[b - 2] == 10 and s == b - 1 and hits_of(s, e)
        elif sub == "1c":
            assert text[b] == 10 and hits_of(b + 1, _line_around(text, b + 1)[1])
        elif sub == "2a":
            assert text[b - 1] == 13 and text[b] == 10 and hits_of(*_line_around(text, b - 2)) and hits_of(*_line_around(text, b + 1))
        elif sub == "2b":
            assert text[b - 1] == 13 and text[b] != 10 and s == b and hits_of(*_line_around(text, b - 2)) and hits_of(s, e)
        elif sub in ("3a", "3b"):
            at, ln = _path_span(text[s:e])
            assert s + at < b < s + at + ln and hits_of(s, e)
            if sub == "3a":
                assert is_name(text[b - 1]) and is_name(text[b])
            else:
                assert text[b] in b"<>" and is_name(text[b - 1])
        elif sub == "4":
            assert text[b - 3:b + 3] == b"\tid:f:" and text[b - 1] == ord("d") and text[b] == ord(":") and hits_of(s, e)
        elif sub == "5":
            assert e - s > STAGE and b"d:" in text[s + STAGE:e] and s < b < e and hits_of(s, e)
        elif sub == "6":                                                      # listed under both ends of its chunk
            lo = b - small if s < b - small else b
            assert s < lo and e > lo + small and e - s > 2 * small and hits_of(s, e)
            assert not ((starts > lo - 1) & (starts < lo + small)).any()      # no line starts in the chunk
        elif sub == "7":
            for lo, hi in ((b - STAGE // 2, b), (b, b + STAGE // 2)):          # any 8 KB around b hold one of the two halves
                assert ((starts >= lo) & (starts < hi)).sum() > 64
        elif sub == "8":
            at, ln = _path_span(text[s:e])
            k = len([x for x in text[s + at:s + at + ln].replace(b"<", b">").split(b">") if x])
            assert s + at < b < s + at + ln and 65 <= k <= 216 and hits_of(s, e)
    if c.end == "partial":
        assert text[-1] not in (10, 13) and (n - W * region) % small != 0
    else:
        assert text[-1] == 10 and (n - W * region) % small == 0 and W * region + c.chunks * small == n


@functools.lru_cache(maxsize=None)
def build_clean(W):
    """a chunked text of which the main kernel should defer NOTHING (the GPU test asserts that it does not), for the fused passes' overlapped
    form: two-node lines with hits over reference nodes of the long-path graph whose names are no substring of another name, twelve plain
    columns and a cg:Z: tag of 0..3 KB; no carriage return, no "d:", no id:f: tag, no line beyond the stage.  -> Case (no features placed)"""
    from oracle import oracle_py
    from svjg.graph import Graph, NODE_HAZARD
    P = pool()
    g = Graph(P.edges, P.alt)
    hazard = {nm for i, nm in enumerate(g.node_names) if int(g.nodes["row"][i]) & NODE_HAZARD}
    kit = []
    for key in sorted(P.edges):
        l, sl, r, sr = key.split("@")
        if sl == sr == "+" and l.startswith("chr2:") and r.startswith("chr2:") and "." not in l + r and not {l, r} & hazard:
            tl = sum(int(x.split(":")[-1].split("-")[1]) - int(x.split(":")[-1].split("-")[0]) + 1 for x in (l, r))
            line = f"c{len(kit)}\t{tl}\t0\t{tl}\t+\t>{l}>{r}\t{tl}\t0\t{tl}\t{tl}\t{tl}\t60\ttp:A:P\n"
            if oracle_py.classify_line(line, P.edges, P.alt):
                kit.append(line.encode())
        if len(kit) == 200:
            break
    assert len(kit) == 200
    rng = random.Random(77 + W)
    n = _choose_n(W, "partial")
    out, pos = [], 0
    while n - pos > 8000:
        l = kit[rng.randrange(len(kit))]
        if rng.random() < 0.8:
            l = _pad_tag(l, len(l) + 7 + rng.randrange(3000))
        out.append(l); pos += len(l)
    out.append(_pad_tag(kit[0], n - pos + 1)[:-1])
    c = Case()
    c.text, c.W, c.n, c.plan, c.chunks, c.end, c.rot, c.placed = b"".join(out), W, n, plan_restated(n, W), n_chunks(n, W), "partial", -1, []
    c.edges, c.alt = P.edges, P.alt
    check(c)
    return c


def coverage(cases):
    """over a set of texts: every kind of feature on at least one region end and on at least one small-chunk end"""
    for where in ("region", "small"):
        got = {sub[0] for c in cases for _, sub, w in c.placed if w == where}
        assert got == set(KINDS), (where, sorted(set(KINDS) - got))


def cases(W):
    return [build(W, rot, end) for rot, end in variants(W)]


def text_lines(text):
    """the lines as the reference reads them: text mode, universal newlines"""
    return io.TextIOWrapper(io.BytesIO(text), encoding="utf-8", newline=None).readlines()


@functools.lru_cache(maxsize=None)
def oracles(W, rot, end):
    """-> (COracle, counts uint64[n_sv, 2] by the C oracle, n_lines, JSON text by the Python oracle, its counts as {sv: (ref, alt)}), computed once"""
    from oracle import oracle_c, oracle_py
    c = build_clean(W) if rot < 0 else build(W, rot, end)           # (rot -1: the clean text)
    orc =oracle_c.COracle(c.edges, c.alt)
    want, _, n_lines = orc.filter(np.frombuffer(c.text, dtype=np.uint8), want_hits=False)
    want.flags.writeable = False
    d = oracle_py.classify(text_lines(c.text), c.edges, c.alt)
    return orc, want, n_lines, oracle_py.dump_informative(d), oracle_py.counts_of(d)
