#!/usr/bin/env python3
"""Writes tests/golden/lik/site_products.npz: sites for geno_site (insertions that share a position) on which it matters that each product
c * L is rounded to a double BEFORE the exact sum, found by search, with the answers of the model (tests/site_model.py).  Needs neither the
reference nor a GPU.

A site has ONE deep raw count A in [2^27, 2^32) — the ref count, or one alt count (halved) — beside zeros, or beside a single alt count of 1
whose half rounds to 0: the chain term T is 0, the site is never flagged, every PL is the routine's own.  A site is kept when the model's PL
vector differs from the one a fused multiply-add would give (tests/site_model.py: fused_pls), in either order a compiler may choose
(tests/lik_model.py: FUSED_ORDERS; beside zeros the two orders give one value, beside the half they differ).  Per K in 2..6 and err in ERRS:
QUOTA sites for either order.  Most of them turn on c * L_x, the PLs of the genotypes WITHOUT the deep allele (|L_x| is 0.8 .. 5.1, a hit
costs 10^5 .. 10^6 candidates); the PL of a genotype with it turns on c * L_he or c * L_ok, whose hits cost 10^7 and, at err 5e-5, 10^10
candidates: deep counts that turn the homozygous PL are therefore searched once at err 0.01 and 0.3 and placed at every K.  Windows of consecutive counts are screened in long double (10 * (p1 + p2) within twice the deep
product's ulps of an integer) and decided in Fraction.  The file is written with fixed zip time stamps: a second run gives the same bytes.
Minutes on one core.

    python tests/golden/make_site_products.py
"""
import io
import os
import sys
import zipfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [ROOT, os.path.join(ROOT, "svjedi-graph_amd")]
from tests import site_model as SM              # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "lik", "site_products.npz")
ERRS = (5e-5, 0.01, 0.3)                        # err values of lik_products.npz's groups
MIN_SUPPORT = 3
ORDERS = ("first", "second")
QUOTA = 7                                       # per (K, err, order): 20 and more per (K, order)
L_OK_HITS = {0.01: 2, 0.3: 4}                   # deep counts that turn the homozygous PL, each placed at every K
LO, HI, WIDTH = 2**27, 2**32, 400_000
ld = np.longdouble


def site_of(K, deep_at, one_at, A):
    """(ref, alts): the deep count A at allele deep_at (0: the ref count), a raw 1 at alt allele one_at (None: zeros only)"""
    v = [0] * (K + 1)
    v[deep_at] = A
    if one_at is not None:
        v[one_at] = 1
    return v[0], v[1:]


def screen(K, deep_at, one_at, raw, e):
    """the counts of the window `raw` at which one of the site's 10 * (p1 + p2) lies within twice the deep product's ulps of an integer; each
    distinct pair of products once"""
    l_ok, l_x, l_he = SM.logs(K, e)
    deep = raw.astype(np.float64) * (0.5 if deep_at else 1.0)
    half = [0.5 if j == one_at else 0.0 for j in range(K + 1)]                   # an allele's count: [j == deep_at] * deep + half[j]
    h_all = sum(half)
    hit, seen = np.zeros(len(raw), bool), set()
    for a, b in SM.genotypes(K):
        d_own = (a == deep_at) or (b == deep_at)
        h_own = half[a] if a == b else half[a] + half[b]
        key = (d_own, h_own, a == b)
        if key in seen:
            continue
        seen.add(key)
        own, rest = (deep + h_own, h_all - h_own) if d_own else (h_own, deep + (h_all - h_own))
        p1, p2 = own * (l_ok if a == b else l_he), rest * l_x
        big, small = (p1, p2) if d_own else (p2, p1)                             # (small: one double, 0 or half a logarithm)
        v = ld(10) * (big.astype(ld) + ld(small))
        hit |= np.abs(v - np.rint(v)) <= (20 * np.spacing(np.abs(big))).astype(ld)
    return raw[hit].tolist()


def sensitive(ref, alts, e):
    """-> (the model's (call, pls), the orders under which a fused product changes a PL)"""
    want = SM.genotype(ref, alts, MIN_SUPPORT, e)
    return want, [o for o in ORDERS if SM.fused_pls(ref, alts, e, o) != want[1]]


def search_l_ok(rng, e, n):
    """n (deep_at in {0, 1}, A) at which the homozygous PL of the deep allele — the product c * L_ok — turns under "first", ref and alt side
    in turn.  K = 2 decides: the product does not depend on K"""
    out = []
    while len(out) < n:
        deep_at = len(out) % 2
        start = int(np.exp(rng.uniform(np.log(2**31), np.log(HI - WIDTH))))      # (the deepest octave: the fewest candidates a hit)
        raw = np.arange(start, start + WIDTH, dtype=np.int64)
        p = raw.astype(np.float64) * (0.5 if deep_at else 1.0) * SM.logs(2, e)[0]
        v = ld(10) * p.astype(ld)
        for A in raw[np.abs(v - np.rint(v)) <= (10 * np.spacing(np.abs(p))).astype(ld)].tolist():
            ref, alts = site_of(2, deep_at, None, A)
            want, orders = sensitive(ref, alts, e)
            at = 0 if deep_at == 0 else 2                                        # VCF order: (0, 0) is 0, (1, 1) is 2
            if "first" in orders and SM.fused_pls(ref, alts, e, "first")[at] != want[1][at] and len(out) < n:
                out.append((deep_at, A))
    return out


def search(rng, K, e):
    """sites of K alleles at err e until each order holds QUOTA of them"""
    have = {o: 0 for o in ORDERS}
    exact = [ee for ee in ERRS if SM.logs(K, ee)[1].is_integer()]            # K = 3, err 0.3: L_x = -1; K = 5, err 5e-5: L_x = -5: c * L_x is exact, only the dear hits
    quota = 0 if e in exact else QUOTA + 3 * len(exact)                      # are left there: the K's other err values take more instead
    out = []
    while any(have[o] < quota for o in ORDERS):
        deep_at = int(rng.integers(K + 1))
        others = [j for j in range(1, K + 1) if j != deep_at]
        one_at = others[int(rng.integers(len(others)))] if rng.random() < 0.4 else None
        start = int(np.exp(rng.uniform(np.log(LO), np.log(HI - WIDTH))))
        for A in screen(K, deep_at, one_at, np.arange(start, start + WIDTH, dtype=np.int64), e):
            ref, alts = site_of(K, deep_at, one_at, A)
            want, orders = sensitive(ref, alts, e)
            if any(have[o] < quota for o in orders):
                out.append((K, e, ref, alts, want, orders))
                for o in orders:
                    have[o] += 1
    return out


def write_npz(path, arrays):
    """np.savez_compressed with fixed time stamps: the same arrays give the same bytes"""
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED) as z:
        for name, a in arrays.items():
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.ascontiguousarray(a), allow_pickle=False)
            info = zipfile.ZipInfo(name + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            info.external_attr = 0o644 << 16
            z.writestr(info, buf.getvalue())


def main():
    assert np.finfo(ld).nmant >= 63                      # 10 * a double is exact in it
    rng = np.random.default_rng(1912)
    kept = []                                            # (K, err, ref, alts, the model's answer, orders)
    for e, n in L_OK_HITS.items():
        for deep_at, A in search_l_ok(rng, e, n):
            for K in range(2, 7):
                ref, alts = site_of(K, deep_at, None, A)
                want, orders = sensitive(ref, alts, e)
                assert "first" in orders
                kept.append((K, e, ref, alts, want, orders))
        print("err %g: %d deep counts that turn c * L_ok" % (e, n), flush=True)
    for K in range(2, 7):
        for e in ERRS:
            kept += search(rng, K, e)
            print("K = %d, err %g: %d sites so far" % (K, e, len(kept)), flush=True)
    n = len(kept)
    assert len({(k, e, ref, tuple(alts)) for k, e, ref, alts, _, _ in kept}) == n
    alt, call, pl = np.zeros((n, 6), np.uint32), np.full((n, 2), SM.NO_CALL, np.uint8), np.zeros((n, 28), np.int64)
    for i, (K, e, ref, alts, (w_call, w_pl), orders) in enumerate(kept):
        alt[i, :K] = alts
        pl[i, :len(w_pl)] = w_pl
        if w_call is not None:
            call[i] = w_call
    write_npz(OUT, {"K": np.array([k[0] for k in kept], np.uint8), "err": np.array([k[1] for k in kept], np.float64),
                    "min_support": np.full(n, MIN_SUPPORT, np.uint8), "ref": np.array([k[2] for k in kept], np.uint32), "alt": alt,
                    "call": call, "pl": pl, "orders": np.array([sum(1 << ORDERS.index(o) for o in k[5]) for k in kept], np.uint8)})
    for K in range(2, 7):
        print("K = %d: %s" % (K, ", ".join("%d sites sensitive to %s" % (sum(1 for k in kept if k[0] == K and o in k[5]), o) for o in ORDERS)))
    print("%s: %d sites, %d bytes" % (os.path.relpath(OUT, ROOT), n, os.path.getsize(OUT)))


if __name__ == "__main__":
    main()
