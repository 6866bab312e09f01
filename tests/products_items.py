"""The item sets the CPU stand-ins and the device kernels are both run on, formed from tests/golden/lik/lik_products.npz (rows on which it
matters that every product c * L is rounded to a double before the exact sum; tests/golden/make_golden.py: make_lik_products) and from
tests/golden/lik/site_products.npz (sites of that kind, found by search; tests/golden/make_site_products.py).  Each set is built once per
process, with the models' answers (tests/ploidy_model.py, tests/site_model.py), and handed out unchanged.  The sensitive_* functions say, by
an exact emulation of a fused multiply-add (tests/lik_model.py: FUSED_ORDERS), on which items of a set a contraction would show."""
import functools
import os
import types

import numpy as np

from tests import lik_model
from tests import ploidy_model as PM
from tests import site_model as SM

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
E_DEEP = 5e-5                                 # err of the fused and onesided rows
PLOIDY_CASES = [("one_sided", 1), ("one_sided", 2), ("one_sided", 3), ("one_sided", 5), ("one_sided", 6), ("one_sided", 7), ("one_sided", 8),
                ("half", 1), ("half", 2), ("half", 4), ("half", 6), ("half", 8)]
ORDERS = tuple(lik_model.FUSED_ORDERS)        # "first", "second": the product of a pair that is multiplied inside s = a + b
NO_CALL = 0xFF
N_COHORT_SITES = 200                          # sites of a cohort sites call (cohort_site_items)


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
    "half": from every distinct (ref, alt) of the half rows the site (ref, [alt, 0]), err 0.5, min_support 0 and 3 in turn;
    "searched": the sites of site_products.npz, one set per err (5e-5, 0.01, 0.3), K = 2..6 mixed: one deep count beside zeros or beside
    the half that rounds to 0 (T = 0 again), each with a PL that a fused product turns (sensitive_sites).
    -> [(min_support, err, sites, the model's (call, pls) per site)]"""
    cases, _, src = fixture()
    if kind == "searched":
        z = searched()
        sets = []
        for e in np.unique(z["err"]).tolist():
            at = np.flatnonzero(z["err"] == e)
            assert len(set(z["min_support"][at].tolist())) == 1
            sets.append((int(z["min_support"][at[0]]), e, [(int(z["ref"][i]), z["alt"][i, :z["K"][i]].tolist()) for i in at]))
    elif kind == "one_sided":
        deep = sorted({int(max(a, b)) for a, b in cases[one_sided(), 1:3].tolist()})
        sites = [s for A in deep for K in (2, 6) for s in ((0, [A] + [0] * (K - 1)), (A, [0] * K), (0, [1, A] + [0] * (K - 2)))]
        sets = [(3, E_DEEP, sites)]
    else:
        pairs = sorted({(int(a), int(b)) for a, b in cases[src == "half", 1:3].tolist()})
        sets = [(ms, 0.5, [(a, [b, 0]) for a, b in pairs[i::2]]) for i, ms in enumerate((0, 3))]
    return [(ms, e, sites, tuple(SM.genotype(ref, alts, ms, e) for ref, alts in sites)) for ms, e, sites in sets]


@functools.lru_cache(maxsize=None)
def searched():
    """site_products.npz as it is stored: K, err, min_support, ref, alt[n, 6], call[n, 2], pl[n, 28], orders (bit 0: "first", bit 1: "second")"""
    z = dict(np.load(f"{GOLDEN}/lik/site_products.npz"))
    for a in z.values():
        a.flags.writeable = False
    return z


def sensitive_sites(sites, want, e):
    """per site (its chain term T is 0) the orders under which a fused product changes a PL of the model's"""
    return [tuple(o for o in ORDERS if SM.fused_pls(ref, alts, e, o) != w[1]) for (ref, alts), w in zip(sites, want)]


def sensitive_rows(rows, want, ms, e, gt_only=False):
    """per row (type, ref, alt, ploidy) the orders under which a fused product changes the model's PLs or GT (gt_only: its GT)"""
    out = []
    for (t, a, b, p), w in zip(rows.tolist(), want):
        got = [PM.fused(t, a, b, p, ms, e, o) for o in ORDERS]
        out.append(tuple(o for o, g in zip(ORDERS, got) if (g[0] != w[0] if gt_only else g != (w[0], w[1]))))
    return out


def rotation(c, s):
    """row r of sample s holds the counts (and the reference's answers) of row rotation(c, s)[r]: the rows of r's own SV type (the halving
    of a count depends on it) rotated by s * (their number // 3)"""
    src_row = np.arange(len(c))
    for t in range(4):
        at = np.flatnonzero(c[:, 0] == t)
        if len(at):
            src_row[at] = np.roll(at, -s * (len(at) // 3))
    return src_row


@functools.lru_cache(maxsize=None)
def cohort_ploidy_items(kind, S, all_diploid=False):
    """The fixture's rows as cohort calls at per-sample ploidy: kind "one_sided": all fused and onesided rows in one call, err 5e-5, min_support
    3; "half": every third half row of either min_support group, err 0.5, a call each.  Sample s holds the call's rows rotated within their SV
    type (rotation).  Item (r, s), i = r * S + s: ploidy 1 + (r + 3 s) mod 8, and 0 (not genotyped) where i mod 11 == 10; all_diploid: 2 on
    every item.
    -> [namespace: ms, e, type[n], counts[n, S, 2], ploidy[n, S], on[n, S] (ploidy != 0), rows int64[m, 4] = (type, ref, alt, ploidy) of the
    items that are on, in item order, want = the model's (gt, pls) per such row, ref int64[n, S, 4] = the reference's GT and three PLs of the
    counts at ploidy 2]"""
    cases, err, src = fixture()
    if kind == "one_sided":
        sets = [(3, E_DEEP, np.flatnonzero(one_sided()))]
    else:
        sets = [(ms, 0.5, np.flatnonzero((src == "half") & (cases[:, 3] == ms))[::3]) for ms in (0, 3)]
    out = []
    for ms, e, sel in sets:
        assert len(sel) and (err[sel] == e).all()
        c = cases[sel]
        n = len(c)
        held = np.stack([c[rotation(c, s)] for s in range(S)], axis=1)             # [n, S, 8]
        i = np.arange(n * S).reshape(n, S)
        ploidy = np.where(i % 11 == 10, 0, 1 + (i // S + 3 * (i % S)) % 8).astype(np.uint8)
        if all_diploid:
            ploidy[:] = 2
        on = ploidy != 0
        rows = np.column_stack([np.broadcast_to(c[:, 0:1], (n, S))[on], held[:, :, 1:3][on], ploidy[on]]).astype(np.int64)
        want = tuple(PM.genotype(t, a, b, p, ms, e) for t, a, b, p in rows.tolist())
        item = types.SimpleNamespace(ms=ms, e=e, type=c[:, 0].astype(np.uint8), counts=held[:, :, 1:3].astype(np.uint32), ploidy=ploidy, on=on, rows=rows,
                                     want=want, ref=held[:, :, 4:8].copy())
        for a in (item.type, item.counts, item.ploidy, item.on, item.rows, item.ref):
            a.flags.writeable = False
        out.append(item)
    return out


def cohort_ploidy_expected(item):
    """the model's answers of a cohort_ploidy_items call as the call's arrays: gt[n, S] (0xFF: no call or not genotyped), site[n, 3] = NS, AN, AC"""
    gt = np.full(item.on.shape, NO_CALL, np.uint8)
    gt[item.on] = [NO_CALL if g is None else g for g, _ in item.want]
    called = gt != NO_CALL
    site = np.stack([called.sum(axis=1), np.where(called, item.ploidy, 0).sum(axis=1, dtype=np.int64), np.where(called, gt, 0).sum(axis=1, dtype=np.int64)], axis=1)
    return gt, site.astype(np.uint32)


def load_cohort(ctx, counts, present):
    """counts[S, n_slots, 2], present[S, n_slots] -> the context's cohort matrix: per sample the present slots with their counts"""
    S, n_slots = present.shape
    ctx.cohort_alloc(S, n_slots)
    for s in range(S):
        sl = np.flatnonzero(present[s]).astype(np.uint32)
        ctx.cohort_set_counts(s, sl, counts[s, sl])


def brute_site(gt, members):
    """site[n, 6, 2] = NS_j, AC_j of a cohort sites call from the items' calls gt[n, S, 2] and members[n, S]"""
    bits = (members[..., None] >> np.arange(6, dtype=np.uint8)) & 1
    sal = np.cumsum(bits, axis=-1) * bits
    called = (gt[..., 0] != NO_CALL)[..., None] & (bits != 0)
    copies = (gt[..., 0, None] == sal).astype(np.int64) + (gt[..., 1, None] == sal)
    return np.stack([called.sum(axis=1), np.where(called, copies, 0).sum(axis=1)], axis=2).astype(np.uint32)


@functools.lru_cache(maxsize=None)
def cohort_site_items(S):
    """The searched sites as cohort sites calls, one per err: N_COHORT_SITES sites of six candidates, every candidate a slot of its own.  Item
    (k, s), i = k * S + s, is one searched site of K' members embedded on K' of the six candidates chosen at random (masks with holes among
    them): the members hold the site's alt counts in candidate order, one of them its ref count and the others half of it or less; the other
    candidates are absent for that sample.  Where i mod 8 == 5 the item has one member or none: no site call.
    -> [namespace: ms, e, slots[n, 6], counts[S, n_slots, 2], present[S, n_slots], and the expected gt[n, S, 2], pl[n, S, 28], raw[n, S, 7],
    members[n, S]; site_of[n, S]: the item's index into site_items("searched")'s set, -1 without a site call]"""
    rng = np.random.default_rng(600 + S)
    out = []
    for ms, e, sites, want in site_items("searched"):
        n = N_COHORT_SITES
        slots = np.arange(n * 6, dtype=np.uint32).reshape(n, 6)
        counts, present = np.zeros((S, n * 6, 2), np.uint32), np.zeros((S, n * 6), bool)
        gt, pl, raw = np.full((n, S, 2), NO_CALL, np.uint8), np.zeros((n, S, 28), np.int64), np.zeros((n, S, 7), np.uint32)
        members, site_of = np.zeros((n, S), np.uint8), np.full((n, S), -1, np.int64)
        order = rng.permutation(len(sites))
        for k, s in np.ndindex(n, S):
            i = k * S + s
            at = int(order[i % len(sites)])
            ref, alts = sites[at]
            few = i % 8 == 5
            K = int(rng.integers(2)) if few else len(alts)
            m = sorted(rng.choice(6, K, replace=False).tolist())
            if K == 3 and 0b100101 not in members:
                m = [0, 2, 5]                                                     # (one mask with two holes for certain)
            holder = m[int(rng.integers(K))] if K else None
            for j, a in zip(m, alts):
                counts[s, slots[k, j]] = (ref if j == holder else ref // (2 + j), a)
                present[s, slots[k, j]] = True
            members[k, s] = sum(1 << j for j in m)
            if few:
                continue
            call, pls = want[at]
            site_of[k, s] = at
            pl[k, s, :len(pls)] = pls
            raw[k, s, 0], raw[k, s, 1:K + 1] = ref, alts
            if call is not None:
                gt[k, s] = call
        item = types.SimpleNamespace(ms=ms, e=e, slots=slots, counts=counts, present=present, gt=gt, pl=pl, raw=raw, members=members, site_of=site_of)
        for a in (slots, counts, present, gt, pl, raw, members, site_of):
            a.flags.writeable = False
        out.append(item)
    return out
