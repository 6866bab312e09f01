"""The item sets the CPU stand-ins and the device kernels are both run on, formed from tests/golden/lik/lik_products.npz (rows on which it
matters that every product c * L is rounded to a double before the exact sum; tests/golden/make_golden.py: make_lik_products).  Each set is
built once per process, with the models' answers (tests/ploidy_model.py, tests/site_model.py), and handed out unchanged."""
import functools
import os

import numpy as np

from tests import ploidy_model as PM
from tests import site_model as SM

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
E_DEEP = 5e-5                                 # err of the fused and onesided rows
PLOIDY_CASES = [("one_sided", 1), ("one_sided", 2), ("one_sided", 3), ("one_sided", 8), ("half", 1), ("half", 2), ("half", 4), ("half", 8)]


@functools.lru_cache(maxsize=None)
def fixture():
    """-> (cases int64[n, 8] = type, ref, alt, min_support, GT, three PLs; err[n]; src[n])"""
    z = np.load(f"{GOLDEN}/lik/lik_products.npz")
    cases, err, src = z["cases"], z["err"], z["src"]
    for a in (cases, err, src):
        a.flags.writeable = False
    return cases, err, src


def groups():
    """the fixture's rows by (min_support, err): [(ms, e, row indices)]"""
    cases, err, _ = fixture()
    return [(int(ms), float(e), np.flatnonzero((cases[:, 3] == ms) & (err == e))) for ms in np.unique(cases[:, 3]) for e in np.unique(err)
            if ((cases[:, 3] == ms) & (err == e)).any()]


def one_sided():
    cases, _, src = fixture()
    return np.isin(src, ("fused", "onesided"))


@functools.lru_cache(maxsize=None)
def ploidy_items(kind, P):
    """kind "one_sided": the fused and onesided rows, err 5e-5; "half": the half rows, err 0.5; all at ploidy P.
    -> [(min_support, err, rows int64[n, 4] = type, ref, alt, ploidy, the model's (gt, pls) per row)]"""
    cases, err, src = fixture()
    sel = one_sided() if kind == "one_sided" else src == "half"
    e = E_DEEP if kind == "one_sided" else 0.5
    assert sel.any() and (err[sel] == e).all()
    out = []
    for ms in np.unique(cases[sel, 3]).tolist():
        c = cases[sel & (cases[:, 3] == ms)]
        rows = np.column_stack([c[:, 0:3], np.full(len(c), P)])
        rows.flags.writeable = False
        out.append((ms, e, rows, tuple(PM.genotype(t, a, b, p, ms, e) for t, a, b, p in rows.tolist())))
    return out


@functools.lru_cache(maxsize=None)
def site_items(kind):
    """kind "one_sided": from the deep count A of every fused and onesided row the sites (0, [A, 0, ..]), (A, [0, ..]) and (0, [1, A, 0, ..]) at
    K = 2 and K = 6 (one count is not zero, or only the half that rounds to 0 beside it: the chain term T is 0), err 5e-5, min_support 3;
    "half": from every distinct (ref, alt) of the half rows the site (ref, [alt, 0]), err 0.5, min_support 0 and 3 in turn.
    -> [(min_support, err, sites, the model's (call, pls) per site)]"""
    cases, _, src = fixture()
    if kind == "one_sided":
        deep = sorted({int(max(a, b)) for a, b in cases[one_sided(), 1:3].tolist()})
        sites = [s for A in deep for K in (2, 6) for s in ((0, [A] + [0] * (K - 1)), (A, [0] * K), (0, [1, A] + [0] * (K - 2)))]
        sets = [(3, E_DEEP, sites)]
    else:
        pairs = sorted({(int(a), int(b)) for a, b in cases[src == "half", 1:3].tolist()})
        sets = [(ms, 0.5, [(a, [b, 0]) for a, b in pairs[i::2]]) for i, ms in enumerate((0, 3))]
    return [(ms, e, sites, tuple(SM.genotype(ref, alts, ms, e) for ref, alts in sites)) for ms, e, sites in sets]
