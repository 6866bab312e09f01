"""svjg/filter.py: the host's part of the filter behind every way into it (classify_file, classify_sharded, classify_stream) — which lines the
host decides (resolve_host_lines), which exception the reference dies with first (reference_error, check_utf8) — against verdicts the reference
itself recorded.  Stand-in contexts classify with the host build of the exact per-line routine (tests/hostsim), line by line."""
import base64
import io
import json
import os
import re
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "svjedi-graph_amd"), os.path.join(ROOT, "tools")):
    if p not in sys.path:
        sys.path.insert(0, p)

from svjg import capi, filter as flt          # noqa: E402
from svjg.graph import Graph                   # noqa: E402
from tests.hostsim import sim                  # noqa: E402

_LINE = re.compile(rb"[^\r\n]*(?:\r\n|\r|\n)|[^\r\n]+\Z")


class _Ctx:
    """What a Context does with a text, one line at a time: counts the lines that pass, keeps the offsets of the lines it sets aside for the
    host, raises the first bad line's exception with its offset, notes a byte >= 0x80."""
    n_host = 0                                                    # lines set aside, over all contexts

    def __init__(self, device=0):
        self.device, self.hl, self.non_ascii, self.comm = device, [], False, False

    def load_graph(self, g):
        self.g = g
        self.total = np.zeros((g.n_slots, 2), dtype=np.uint64)

    def classify(self, gaf, base_offset=0, want_hits=False):
        raw = bytes(np.asarray(gaf))
        self.non_ascii |= any(b >= 0x80 for b in raw)
        lines = [(m.start(), m.group()) for m in _LINE.finditer(raw)]
        counts, excs = sim.classify_cases(self.g, [t for _, t in lines]) if lines else ([], [])
        for (off, _), c, e in zip(lines, counts, excs):
            if e is sim.HostLine:
                self.hl.append(base_offset + off)
                _Ctx.n_host += 1
            elif e is not None:
                ex = e(f"GAF line at byte offset {base_offset + off}")
                ex.svjg_offset = base_offset + off
                raise ex
            else:
                self.total += c.astype(np.uint64)

    def classify_file(self, path, offset, n_bytes, want_hits=False):
        with open(path, "rb") as fh:
            fh.seek(offset)
            self.classify(np.frombuffer(fh.read(n_bytes), dtype=np.uint8), offset, want_hits)

    def stats(self):
        return {"non_ascii": int(self.non_ascii), "n_deferred": 0, "n_hitrecs": 0}

    def counts(self):
        return self.total

    def host_lines(self):
        return np.array(self.hl, dtype=np.uint64)

    def close(self):
        pass


@pytest.fixture()
def standin(monkeypatch, tmp_path):
    def comm_init_all(ctxs):
        for c in ctxs:
            c.comm = True

    def allreduce_counts_all(ctxs):
        assert len(ctxs) == 1 or all(c.comm for c in ctxs)
        tot = sum(c.total for c in ctxs)
        for c in ctxs:
            c.total = tot.copy()
    monkeypatch.setattr(capi, "Context", _Ctx)
    monkeypatch.setattr(capi, "comm_init_all", comm_init_all)
    monkeypatch.setattr(capi, "allreduce_counts_all", allreduce_counts_all)
    monkeypatch.setattr(capi, "release_host_tables", lambda: None)
    monkeypatch.setattr(flt, "STREAM_BLOCK", 512)               # (the stream arrives in many small reads)
    monkeypatch.setenv("XDG_CACHE_HOME", str(tmp_path))          # (note_rccl_init_s)
    monkeypatch.delenv("SVJG_COMM_OVERLAP", raising=False)
    return tmp_path


DRIVERS = {
    "classify_file": lambda g, path: flt.classify_file(_Ctx(0), g, path, want_hits=False),
    "sharded [0]": lambda g, path: flt.classify_sharded(g, path, want_hits=False, devices=[0]),
    "sharded [0, 0, 0]": lambda g, path: flt.classify_sharded(g, path, want_hits=False, devices=[0, 0, 0]),
    "sharded [0, 1]": lambda g, path: flt.classify_sharded(g, path, want_hits=False, devices=[0, 1]),
    "stream": lambda g, path: flt.classify_stream(g, io.BytesIO(open(path, "rb").read()), want_hits=False),
}


def _verdict(drive, g, path):
    """-> ("ok", {sv id: [ref, alt]}) or ("died", exception class name)"""
    try:
        counts, _, _ = drive(g, path)
    except Exception as e:                                        # noqa: BLE001
        return ("died", type(e).__name__)
    return ("ok", {g.sv_ids[i]: [int(counts[i, 0]), int(counts[i, 1])] for i in np.flatnonzero(counts.sum(axis=1))})


def _graph(golden, which):
    d = f"{golden}/{which}"
    stem = "test" if which == "testdir" else "q"
    return Graph.from_files(f"{d}/{stem}_svs_edges.json", f"{d}/{stem}.gfa", native=False)


def _check(g, cases, tmp, drivers=DRIVERS):
    """cases: [(name, raw bytes, wanted verdict)] -> the mismatches of every driver"""
    bad = []
    path = str(tmp / "in.gaf")
    for name, raw, want in cases:
        with open(path, "wb") as fh:
            fh.write(raw)
        for who in drivers:
            got = _verdict(DRIVERS[who], g, path)
            if got != want:
                bad.append((name, who, want, got))
    return bad


def test_fuzz_cases_through_every_driver(golden, standin):
    """golden/fuzz: 500 mutated fragments, the reference's counts or exception class; then each fatal one between runs of good lines
    in a file cut into two shards: the first bad line in file order wins"""
    g = _graph(golden, "testdir")
    cases = json.load(open(f"{golden}/fuzz/fuzz.json"))["cases"]
    frags = [base64.b64decode(c["gaf"]) for c in cases]
    want = [("ok", c["counts"]) if c["rc"] == 0 else ("died", c["error"]) for c in cases]
    bad = _check(g, [(i, f, w) for i, (f, w) in enumerate(zip(frags, want))], standin)
    assert not bad, bad[:5]
    good = [f if f.endswith((b"\n", b"\r")) else f + b"\n" for f, c in zip(frags, cases) if c["rc"] == 0]
    pad = b"".join(good[:40])
    fatal = [(i, pad + f + (b"" if f.endswith((b"\n", b"\r")) else b"\n") + pad, ("died", c["error"]))
             for i, (f, c) in enumerate(zip(frags, cases)) if c["rc"] and c["error"] != "UnicodeDecodeError"]
    assert len(fatal) > 100
    bad = _check(g, fatal, standin, ["sharded [0, 0, 0]", "sharded [0, 1]", "stream"])
    assert not bad, bad[:5]


def test_unicode_files_through_every_driver(golden, standin):
    """golden/unicode: decimal columns in non-ASCII digits and blanks — lines the host decides and sends through the classifier again"""
    g = _graph(golden, "quirks")
    u = f"{golden}/unicode"
    man = json.load(open(f"{u}/manifest.json"))
    cases = []
    for name, m in sorted(man.items()):
        if m["rc"] == 0:
            ref = json.load(open(f"{u}/{name}.ref.json"))
            want = ("ok", {k: [len(v[0]), len(v[1])] for k, v in ref.items()})
        else:
            want = ("died", m["error"])
        cases.append((name, open(f"{u}/{name}.gaf", "rb").read(), want))
    assert len(cases) == 12
    _Ctx.n_host = 0
    bad = _check(g, cases, standin)
    assert not bad, bad
    assert _Ctx.n_host > 0                                        # (the host's int() / float() decided lines, which went through again)


def test_utf8_error_order_through_every_driver(golden, standin):
    """golden/utf8order: files that are not UTF-8 and may hold a malformed line — UnicodeDecodeError or the line's error, as the
    reference's 8 KB text-mode blocks decide"""
    g = _graph(golden, "quirks")
    cases = json.load(open(f"{golden}/utf8order/cases.json"))
    bad = _check(g, [(name, base64.b64decode(c["gaf"]), ("died", c["error"])) for name, c in sorted(cases.items())], standin)
    assert not bad, bad
