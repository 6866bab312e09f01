"""Host side of the genotyper: VCF rows -> count slots, svjg_genotype (HIP) -> VCF text.

Mirrors predict-genotype.py's decision_vcf (:89-279) for everything that is file format; the likelihood
(:281-338) and the presence gate (:216) run on the GPU.
"""
import functools
from typing import NamedTuple

import numpy as np

NONE = 0xFFFFFFFF
TYPE_CODE = {"DEL": 0, "INS": 1, "INV": 2, "BND": 3}
GT_TEXT = ("0/0", "0/1", "1/1", "./.")

FORMAT_HEADER = (
    '##FORMAT=<ID=GT,Number=1,Type=String,Description="Genotype">\n'
    '##FORMAT=<ID=DP,Number=1,Type=Float,Description="Total number of informative read alignments across all alleles (after normalization for unbalanced SVs)">\n'
    '##FORMAT=<ID=AD,Number=2,Type=Float,Description="Number of informative read alignments supporting each allele (after normalization by breakpoint number for unbalanced SVs)">\n'
    '##FORMAT=<ID=PL,Number=3,Type=Integer,Description="Phred-scaled likelihood for each genotype">\n'
    "#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\tSAMPLE\n"
)


def _info(info, label):
    """predict-genotype.py:77-87 (IndexError when the label is absent, like the reference)."""
    fields = info.split(";")
    if fields[0].startswith(label + "="):
        return info.split(label + "=")[1].split(";")[0]
    if fields[-1].startswith(label + "="):
        return info.split(";" + label + "=")[1]
    return info.split(";" + label + "=")[1].split(";")[0]


def row_key(chrom, pos, alt, info, ins_seen):
    """(svtype, sv_id, length) of one VCF row — predict-genotype.py:118-211."""
    svtype = ""
    if "SVTYPE" in info:
        svtype = info.split("SVTYPE=")[1]
        if not info.split(";")[-1].startswith("SVTYPE="):
            svtype = svtype.split(";")[0]
    end = _info(info, "END") if svtype not in ("BND", "INS") else None
    if svtype in ("DEL", "INV"):
        return svtype, "%s:%s-%s-%s" % (chrom, svtype, pos, end), int(end) - int(pos)
    if svtype == "INS":
        n = ins_seen[pos] = ins_seen.get(pos, 0) + 1        # keyed by POS only, shared by all chromosomes
        return svtype, "%s:INS-%s-%d" % (chrom, pos, n), len(alt)
    if svtype == "BND":
        for br in ("[", "]"):
            if br in alt:
                parts = [x for x in alt.split(br) if x]
                if ":" in parts[1]:
                    return svtype, "%s:BND-%s%s%s%s" % (chrom, pos, br, parts[1], br), 50
                return svtype, "%s:BND-%s%s%s%s" % (chrom, br, parts[0], br, pos), 50
        return svtype, "wrong_format", 50
    return svtype, "unsupported_type", 0


class VcfRows:
    """Input VCF split into header output lines and data rows with their count slot."""

    def __init__(self, vcf_path, slot_of, slot_is_presence=False):
        self.items = []          # ("h", text) or ("r", row index)
        self.prefix = []         # text before "\tGT:DP:AD:PL" for each data row
        self.chrom, self.pos = [], []   # CHROM and POS text of each data row (the ploidy file is matched against them)
        types, slots, oks = [], [], []
        ins_seen = {}
        with open(vcf_path) as fh:
            for line in fh:
                if line.startswith("##FORMAT"):
                    continue
                if line.startswith("##"):
                    self.items.append(("h", line))
                    continue
                if line.startswith("#C"):
                    self.items.append(("h", FORMAT_HEADER))
                    continue
                text = line.rstrip("\n")
                cols = text.split("\t")
                chrom, pos, _id, _ref, alt, _q, _f, info, *_rest = cols
                svtype, key, length = row_key(chrom, pos, alt, info, ins_seen)
                code = TYPE_CODE.get(svtype)
                types.append(code if code is not None else 0)
                oks.append((3 if slot_is_presence else 1) if (code is not None and abs(length) >= 50) else 0)
                slots.append(slot_of.get(key, NONE))
                # the first eight columns as they stand (columns 1..8 cannot hold the terminator, so the split of the
                # stripped line has the same first eight as the reference's split of the raw one)
                self.prefix.append(text if len(cols) <= 8 else "\t".join(cols[:8]))
                self.chrom.append(chrom)
                self.pos.append(pos)
                self.items.append(("r", len(types) - 1))
        self.sv_type = np.array(types, dtype=np.uint8)
        self.slot = np.array(slots, dtype=np.uint32)
        self.ok = np.array(oks, dtype=np.uint8)


def _norm_counts(svtype_code, ref, alt):
    """-> (c1, c2): the counts after the in-place normalisation of predict-genotype.py:327-338"""
    if svtype_code == 0 and ref > 0:
        return round(ref / 2, 1), alt
    if svtype_code == 1 and alt > 0:
        return ref, round(alt / 2, 1)
    return ref, alt


def _fmt_counts(svtype_code, ref, alt):
    """DP and AD text of the normalised counts (Python formatting)."""
    c1, c2 = _norm_counts(svtype_code, ref, alt)
    return str(round(c1 + c2, 3)), "%s,%s" % (c1, c2)


def _call_args(min_support, err):
    """what every genotype call starts with -> (min_support, the err to call with, bad_err).  A negative threshold: `sum(nbAln) >= minNbAln` always
    holds (predict-genotype.py:310).  bad_err: math.log10(e) / math.log10(1 - e) raise in likelihood(), i.e. only once a row gets there
    (:295-297: the reference dies at the first genotyped row), so the call runs at 0.5 and the caller raises if anything was genotyped."""
    bad_err = not (0.0 < float(err) < 1.0)
    return max(0, int(min_support)), 0.5 if bad_err else err, bad_err


# ln(z!) by Stirling's series at 60 digits: ln z! = (z + 1/2) ln z - z + ln(2 pi) / 2 + sum B_2j / (2j (2j - 1) z^(2j - 1)).  With
# z > 2000 and the terms up to B_24 the remainder is below 1e-80.
_PI = "3.14159265358979323846264338327950288419716939937510582097494459230781640628620899"
_BERNOULLI = ((1, 6), (-1, 30), (1, 42), (-1, 30), (5, 66), (-691, 2730), (7, 6), (-3617, 510), (43867, 798), (-174611, 330),
              (854513, 138), (-236364091, 2730))
_COMB_DIRECT = 2000            # min(k, n - k) up to this (or n up to 10 * this): math.comb itself is fast


def _ln_fact(z):
    from decimal import Decimal
    z = Decimal(z)
    s = (z + Decimal("0.5")) * z.ln() - z + (2 * Decimal(_PI)).ln() / 2
    zz, p = z * z, z
    for j, (a, b) in enumerate(_BERNOULLI, 1):
        s += Decimal(a) / (Decimal(b) * (2 * j) * (2 * j - 1) * p)
        p *= zz
    return s


def _log10_comb(n, k):
    """math.log10(math.comb(n, k)), the same double, without the big integer where it is slow: CPython's log10 of an int
    (mathmodule.c: loghelper) takes the int rounded to a double (PyLong_AsDouble) if that is below 2^1024, else x * 2^e with x
    the int's top 53 bits rounded half to even (_PyLong_Frexp) and returns log10(x) + log10(2.0) * e.  The int's rounding is
    taken from ln comb(n, k) at 60 digits; where that cannot decide it (the value sits at a rounding point), math.comb does."""
    import math
    from decimal import Decimal, localcontext
    if n <= 10 * _COMB_DIRECT or min(k, n - k) <= _COMB_DIRECT:
        return math.log10(math.comb(n, k))
    with localcontext() as ctx:
        ctx.prec = 60
        lnc = _ln_fact(n) - _ln_fact(k) - _ln_fact(n - k)
        ln2 = Decimal(2).ln()
        t = lnc / ln2
        e = int(t) + 1                                           # bit length: 2^(e-1) <= comb < 2^e
        m = (lnc - (e - 53) * ln2).exp()                         # comb / 2^(e-53), in [2^52, 2^53)
        mi = int(m)
        fr = m - mi
        if abs(t - int(t)) < Decimal("1e-30") or abs(t - int(t) - 1) < Decimal("1e-30") or abs(fr - Decimal("0.5")) < Decimal("1e-30"):
            return math.log10(math.comb(n, k))
    if fr > Decimal("0.5") or (fr == Decimal("0.5") and mi & 1):
        mi += 1
    if mi == 1 << 53:                                            # the rounding carried: 0.5 * 2^(e+1)
        mi, e = 1 << 52, e + 1
    if e <= 1024:
        return math.log10(math.ldexp(float(mi), e - 53))
    return math.log10(math.ldexp(float(mi), -53)) + math.log10(2.0) * e


def exact_pl(svtype_code, ref, alt, err):
    """The three PL integers of one row with the reference's own arithmetic (predict-genotype.py:284-323): double products, Decimal
    sums at precision 28, log10 of the binomial coefficient as CPython computes it for the exact integer, truncation.  For the rows
    the kernel flags as lying within 1e-6 of an integer boundary or beyond its log10(i!) table (svjg_genotype_boundary): there
    libm's log10 of a big integer — not necessarily the correctly rounded value the kernel uses — could decide the integer.  The diploid
    case of exact_pl_ploidy: lik0, lik1 (one product) and lik2 are its g = 0, 1, 2."""
    return exact_pl_ploidy(svtype_code, ref, alt, 2, err)


def recompute_flagged(sv_type, pl, raw, done, boundary, err, ploidy=None):
    """The boundary guard of every genotype call: the items that are flagged and genotyped get exact_pl_ploidy's integers, in place.  done,
    boundary, ploidy: one entry per item, of any leading shape ([n], or [n, S] in a cohort) whose first index is the row of sv_type; pl and
    raw: that shape + [>= P + 1] and + [2]; ploidy None: 2 everywhere.  -> the number of flagged items"""
    idx = np.argwhere((np.asarray(boundary) != 0) & (np.asarray(done) != 0))
    for at in map(tuple, idx):
        P = 2 if ploidy is None else int(ploidy[at])
        pl[at][:P + 1] = exact_pl_ploidy(int(sv_type[at[0]]), int(raw[at][0]), int(raw[at][1]), P, err)
    return len(idx)


def apply_boundary_guard(ctx, rows, pl, raw, done, err):
    """-> pl with the flagged rows recomputed (a copy only if a row is flagged), number of flagged rows"""
    flags = ctx.boundary_flags(len(rows.sv_type))
    if not (flags & (np.asarray(done) != 0)).any():
        return pl, 0
    pl = np.array(pl, dtype=np.int64)
    return pl, recompute_flagged(rows.sv_type, pl, raw, done, flags, err)


# ---- any ploidy from 1 to 8 (--ploidy / --ploidy-file): svjg_genotype_ploidy, Python rows and the writer below ----

MAX_PLOIDY = 8
NO_CALL = 0xFF
_PL_3 = "##FORMAT=<ID=PL,Number=3,"
_PL_G = "##FORMAT=<ID=PL,Number=G,"


def exact_pl_ploidy(svtype_code, ref, alt, ploidy, err):
    """The ploidy + 1 PL integers of one row, PL_g for g = 0..ploidy alt copies, with the reference's arithmetic generalised: a read
    shows the alt allele with probability (g (1 - e) + (P - g) e) / P.  g = 0 and g = P are the reference's lik0 and lik2, 2 g = P its
    lik1 (one product): double products, Decimal sums at precision 28, log10 of the binomial coefficient as CPython computes it for the
    exact integer, truncation.  For the rows and items the kernels flag (recompute_flagged)."""
    import math
    from decimal import Decimal, localcontext
    P = int(ploidy)
    if not 1 <= P <= MAX_PLOIDY:
        raise ValueError("ploidy %r is not in 1..%d" % (ploidy, MAX_PLOIDY))
    c1, c2 = _norm_counts(svtype_code, ref, alt)
    rc1, rc2 = int(round(c1, 0)), int(round(c2, 0))              # the rounded counts fed to comb()
    with localcontext() as ctx:
        ctx.prec = 28
        comb = Decimal(_log10_comb(rc1 + rc2, rc1))
        out = []
        for g in range(P + 1):
            if g == 0:
                lik = Decimal(c1 * math.log10(1 - err)) + Decimal(c2 * math.log10(err))
            elif g == P:
                lik = Decimal(c2 * math.log10(1 - err)) + Decimal(c1 * math.log10(err))
            elif 2 * g == P:
                lik = Decimal((c1 + c2) * math.log10(1 / 2))
            else:
                l_ref = math.log10(((P - g) * (1 - err) + g * err) / P)
                l_alt = math.log10((g * (1 - err) + (P - g) * err) / P)
                lik = Decimal(c1 * l_ref) + Decimal(c2 * l_alt)
            out.append(int(-10 * (lik + comb)))
        return out


def _plain_int(text):
    if not (text.isascii() and text.isdigit()):
        raise ValueError
    return int(text)


def _ploidy_region(f, path, no, line, forms="`CHROM PLOIDY` or `CHROM FROM TO PLOIDY`"):
    """the fields `CHROM PLOIDY` or `CHROM FROM TO PLOIDY` of line `no` of a ploidy file -> (chrom, from, to, ploidy); the one place that reads
    them, for load_ploidy_file and load_cohort_ploidy_file (forms: how the error message spells the file's lines)"""
    try:
        if len(f) == 2:
            lo = hi = None
        elif len(f) == 4:
            lo, hi = _plain_int(f[1]), _plain_int(f[2])
            if lo < 1 or hi < lo:
                raise ValueError
        else:
            raise ValueError
        p = _plain_int(f[-1])
    except ValueError:
        raise ValueError("%s:%d: expected %s: %r" % (path, no, forms, line.rstrip("\n"))) from None
    if p > MAX_PLOIDY:
        raise ValueError("%s:%d: ploidy %d is not in 0..%d" % (path, no, p, MAX_PLOIDY))
    return f[0], lo, hi, p


def load_ploidy_file(path):
    """-> [(chrom, from, to, ploidy)] in file order; from = to = None for a whole-chromosome line.  Lines: `CHROM PLOIDY` or
    `CHROM FROM TO PLOIDY`, separated by tabs or blanks, coordinates 1-based and inclusive; `#` lines and empty lines are skipped.
    ValueError for anything else, and for a ploidy outside 0..8."""
    regions = []
    with open(path) as fh:
        for no, line in enumerate(fh, 1):
            f = line.split()
            if not f or f[0].startswith("#"):
                continue
            regions.append(_ploidy_region(f, path, no, line))
    return regions


def rows_ploidy(rows, ploidy=None, regions=()):
    """the ploidy of every data row of a VcfRows: the first line of the ploidy file that matches its CHROM (and, for a region line, its POS when
    that is a plain decimal), else `ploidy`, else 2"""
    default = 2 if ploidy is None else int(ploidy)
    if not 1 <= default <= MAX_PLOIDY:
        raise ValueError("ploidy %r is not in 1..%d" % (ploidy, MAX_PLOIDY))
    by_chrom = {}
    for chrom, lo, hi, p in regions:
        by_chrom.setdefault(chrom, []).append((lo, hi, p))
    out = np.full(len(rows.chrom), default, dtype=np.uint8)
    if by_chrom:
        for r, (chrom, pos) in enumerate(zip(rows.chrom, rows.pos)):
            lines = by_chrom.get(chrom)
            if not lines:
                continue
            at = int(pos) if pos.isascii() and pos.isdigit() else None
            for lo, hi, p in lines:
                if lo is None or (at is not None and lo <= at <= hi):
                    out[r] = p
                    break
    return out


@functools.lru_cache(maxsize=None)
def gt_text_ploidy(P, g):
    """GT of g alt copies out of P: (P - g) zeros then g ones joined by `/`; a no-call: P dots"""
    if g == NO_CALL:
        return "/".join("." * P)
    return "/".join("0" * (P - g) + "1" * g)


def sample_column(svtype_code, P, g, pl, ref, alt, done, gq=None):
    """One sample column GT:DP:AD:PL of every writer.  P: the item's ploidy (0: `.:0:0,0:.`); g: the alt copies of the call, NO_CALL = 0xFF for
    none (at P >= 3 a 3 is a call: the diploid callers translate their 3 themselves); pl: at least P + 1 integers; ref, alt: the raw counts;
    done false: P dots as GT, no counts, P + 1 dots as PL.  gq (--cohort-prior; None: no such field): one more field, GQ, `.` where there is
    no call (NO_CALL)."""
    tail = "" if gq is None else ":." if gq == NO_CALL or g == NO_CALL or P == 0 or not done else ":%d" % gq
    if P == 0:
        return ".:0:0,0:." + tail
    if not done:
        return "%s:0:0,0:%s%s" % ("/".join("." * P), ",".join("." * (P + 1)), tail)
    dp, ad = _fmt_counts(svtype_code, ref, alt)
    return "%s:%s:%s:%s%s" % (gt_text_ploidy(P, g), dp, ad, ",".join(map(str, pl[:P + 1])), tail)


def _write_rows(out_path, rows, header, columns, info=None):
    """The one writer loop over a VcfRows.  header: the text that stands for FORMAT_HEADER; columns(v): FORMAT and the sample columns of data
    row v, as a list; info(v, text): the INFO column of row v from the input's (None: as it stands)."""
    with open(out_path, "w") as out:
        for kind, v in rows.items:
            if kind == "h":
                out.write(header if v is FORMAT_HEADER else v)
                continue
            prefix = rows.prefix[v]
            if info is not None:
                first7, text = prefix.rsplit("\t", 1)
                prefix = first7 + "\t" + info(v, text)
            out.write(prefix + "\t" + "\t".join(columns(v)) + "\n")


def _item_columns(rows, ploidy, gt, pl, raw, done, gq=None):
    """-> (columns(v) for _write_rows: GT:DP:AD:PL and one sample_column per sample, the number of genotyped rows per sample).  The arrays hold
    one item per row ([n]: one sample) or [n, S]; ploidy None: diploid arrays, whose gt says 3 for no call; gq ([n, S], --cohort-prior): the
    fifth field, GT:DP:AD:PL:GQ"""
    gt, pl, raw, done = np.asarray(gt), np.asarray(pl), np.asarray(raw), np.asarray(done)
    if ploidy is None:
        ploidy, gt = np.full(gt.shape, 2, np.uint8), np.where(gt == 3, NO_CALL, gt)
    ploidy = np.asarray(ploidy)
    if gt.ndim == 1:
        ploidy, gt, pl, raw, done = ploidy[:, None], gt[:, None], pl[:, None], raw[:, None], done[:, None]
    n_done = np.count_nonzero((done != 0) & (ploidy != 0), axis=0).tolist()
    if gq is not None:
        gq = np.asarray(gq)

    def columns(v):
        t = int(rows.sv_type[v])
        items = zip(ploidy[v].tolist(), gt[v].tolist(), pl[v].tolist(), raw[v].tolist(), done[v].tolist(), gq[v].tolist() if gq is not None else [None] * len(gt[v]))
        return ["GT:DP:AD:PL" if gq is None else "GT:DP:AD:PL:GQ"] + [sample_column(t, P, g, p, r[0], r[1], d, q) for P, g, p, r, d, q in items]
    return columns, n_done


def write_vcf_ploidy(out_path, rows, ploidy, gt, pl, raw, done):
    """write_vcf for rows of any ploidy: P + 1 PLs per row, `Number=G` in the PL header line; a ploidy-0 row prints `.:0:0,0:.`"""
    columns, n_done = _item_columns(rows, ploidy, gt, pl, raw, done)
    _write_rows(out_path, rows, FORMAT_HEADER.replace(_PL_3, _PL_G), columns)
    return n_done[0]


def _open_call(vcf_path, slot_of, slot_is_presence, min_support, err, native=False):
    """The opening of every single-sample driver: the rows (open_rows; native False: the Python rows) and _call_args -> (rows, min_support, the err
    to call with, check); check(genotyped) after the call: "math domain error" if err lies outside (0, 1) and any row was genotyped
    (predict-genotype.py:295-297: the reference dies at the first genotyped row)"""
    rows = open_rows(vcf_path, slot_of, slot_is_presence, native)
    min_support, call_err, bad_err = _call_args(min_support, err)

    def check(done):
        if bad_err and np.asarray(done).any():
            raise ValueError("math domain error")
    return rows, min_support, call_err, check


def genotype_with_counts_ploidy(ctx, vcf_path, slot_of, out_path, min_support, err, slot_is_presence, ploidy, ploidy_file):
    """genotype_with_counts with --ploidy and / or --ploidy-file: the Python rows, svjg_genotype_ploidy, the writer above"""
    regions = load_ploidy_file(ploidy_file) if ploidy_file is not None else ()       # (raises before any output exists)
    rows, min_support, call_err, check = _open_call(vcf_path, slot_of, slot_is_presence, min_support, err)
    pld = rows_ploidy(rows, ploidy, regions)
    gt, pl, raw, done, boundary = ctx.genotype_ploidy(rows.sv_type, rows.slot, rows.ok, pld, min_support, call_err)
    check(done)
    recompute_flagged(rows.sv_type, pl, raw, done, boundary, err, pld)
    return write_vcf_ploidy(out_path, rows, pld, gt, pl, raw, done)


# ---- insertions that share a position, genotyped together (--joint-ins): svjg_genotype_sites, Python rows and the writer below ----

MAX_SITE_ALTS = 6
JOINT_INS_PLOIDY = "--joint-ins is diploid only: it cannot be combined with --ploidy or --ploidy-file"
_PL_LINE = '##FORMAT=<ID=PL,Number=3,Type=Integer,Description="Phred-scaled likelihood for each genotype">\n'
SITE_FORMAT_LINES = (
    '##FORMAT=<ID=SGT,Number=1,Type=String,Description="Joint genotype of the insertions sharing this position: allele 0 is the reference, allele i the insertion with SAL=i">\n'
    '##FORMAT=<ID=SAL,Number=1,Type=Integer,Description="Allele number of this insertion in SGT">\n'
)


def check_single_options(ploidy=None, ploidy_file=None, joint_ins=False):
    """The rules between the options of a single-sample run (run, genotype_with_counts, predict-genotype.py): ValueError with the rule's text"""
    if joint_ins and (ploidy is not None or ploidy_file is not None):
        raise ValueError(JOINT_INS_PLOIDY)


def site_genotypes(K):
    """the genotypes {a, b} of a site of K members in VCF order: index b (b + 1) / 2 + a"""
    return [(a, b) for b in range(K + 1) for a in range(b + 1)]


def exact_pl_site(ref, alts, err):
    """The (K + 1)(K + 2) / 2 PL integers of one site (ref: the members' largest raw ref count, alts: their K raw alt counts) in VCF order,
    with the reference's arithmetic written for K alt alleles: double products, Decimal sums at precision 28, every chain term
    log10 comb(s_j, r_j) as CPython computes it for the exact integer, truncation.  For the sites svjg_genotype_sites flags."""
    import math
    from decimal import Decimal, localcontext
    K = len(alts)
    if not 2 <= K <= MAX_SITE_ALTS:
        raise ValueError("a site has 2..%d insertions, not %d" % (MAX_SITE_ALTS, K))
    c = [ref] + [round(x / 2, 1) if x > 0 else 0 for x in alts]
    r = [int(round(x, 0)) for x in c]
    N = sum(c)
    l_ok, l_x, l_he = math.log10(1 - err), math.log10(err / K), math.log10(((1 - err) + err / K) / 2)
    with localcontext() as ctx:
        ctx.prec = 28
        T, s = Decimal(0), r[0]
        for j in range(1, K + 1):
            s += r[j]
            T += Decimal(_log10_comb(s, r[j]))
        out = []
        for a, b in site_genotypes(K):
            if a == b:
                lik = Decimal(c[a] * l_ok) + Decimal((N - c[a]) * l_x)
            else:
                lik = Decimal((c[a] + c[b]) * l_he) + Decimal((N - c[a] - c[b]) * l_x)
            out.append(int(-10 * (lik + T)))
        return out


def form_sites(rows, done):
    """-> (sites, skipped): sites = lists of row indices, the INS rows the ordinary call genotyped that share CHROM and POS text, 2..6 of them in
    file order (they need not be adjacent); skipped = [(chrom, pos, count)] for the positions with more than six, which keep their own calls"""
    by_pos = {}
    for r in range(len(rows.chrom)):
        if done[r] and rows.sv_type[r] == TYPE_CODE["INS"]:
            by_pos.setdefault((rows.chrom[r], rows.pos[r]), []).append(r)
    sites = [m for m in by_pos.values() if 2 <= len(m) <= MAX_SITE_ALTS]
    skipped = [(k[0], k[1], len(m)) for k, m in by_pos.items() if len(m) > MAX_SITE_ALTS]
    return sites, skipped


def _site_slots(rows, sites):
    """the slot matrix of a site call from form_sites' lists: [n, 6], a site's rows' slots first, NONE behind them"""
    slots = np.full((len(sites), MAX_SITE_ALTS), NONE, dtype=np.uint32)
    for k, m in enumerate(sites):
        slots[k, :len(m)] = rows.slot[m]
    return slots


def _report_skipped(skipped):
    import sys
    for chrom, pos, count in skipped:
        print("--joint-ins: %s:%s has %d insertions, more than %d: they keep their independent calls" % (chrom, pos, count, MAX_SITE_ALTS), file=sys.stderr)


def recompute_flagged_sites(s_pl, s_raw, boundary, k_of, err):
    """recompute_flagged for the site calls: the flagged items get exact_pl_site's integers on their own K' = k_of[item] members, in place.
    boundary, k_of: one entry per item, [n] or [n, S] in a cohort; s_pl, s_raw: that shape + [28] and + [7].  -> the number of flagged items"""
    idx = np.argwhere(np.asarray(boundary) != 0)
    for at in map(tuple, idx):
        K = int(k_of[at])
        s_pl[at][:(K + 1) * (K + 2) // 2] = exact_pl_site(int(s_raw[at][0]), [int(x) for x in s_raw[at][1:K + 1]], err)
    return len(idx)


@functools.lru_cache(maxsize=None)
def _site_copy_sets(K, i):
    """the genotype indices of a site of K members with 0, 1 and 2 copies of allele i (the projection's three groups)"""
    return tuple(np.array([k for k, (x, y) in enumerate(site_genotypes(K)) if (x == i) + (y == i) == n], dtype=np.int64) for n in range(3))


def project_site(K, i, gt_pair, site_pl):
    """member i (1..K) of a site called gt_pair = (a, b) or (0xFF, 0xFF) -> (its copies g = 0..2, or 3 for a no-call; [PL_0, PL_1, PL_2]: the
    smallest site PL over the genotypes with exactly that many copies of allele i).  The scalar face of project_cohort_sites."""
    a, b = int(gt_pair[0]), int(gt_pair[1])
    site_pl = np.asarray(site_pl)
    return 3 if a == NO_CALL else (a == i) + (b == i), [int(site_pl[idx].min()) for idx in _site_copy_sets(K, i)]


def _member_column(svtype_code, g, pl3, ref, alt, sgt, sal):
    """a member's sample column: GT and PL the site call's projection, DP and AD the row's own, then the site call's text and the allele number"""
    return "%s:%s:%d" % (sample_column(svtype_code, 2, NO_CALL if g == 3 else g, pl3, ref, alt, True), sgt, sal)


def _sgt_text(a, b):
    return "./." if a == NO_CALL else "%d/%d" % (a, b)


def write_vcf_joint(out_path, rows, gt, pl, raw, done, member):
    """write_vcf with the members of a site printed as GT:DP:AD:PL:SGT:SAL; member: row -> (g, [three PLs], site call text, allele number)"""
    plain, n_done = _item_columns(rows, None, gt, pl, raw, done)

    def columns(v):
        if not (done[v] and v in member):
            return plain(v)
        g, pl3, sgt, sal = member[v]
        return ["GT:DP:AD:PL:SGT:SAL", _member_column(int(rows.sv_type[v]), g, pl3, int(raw[v, 0]), int(raw[v, 1]), sgt, sal)]
    _write_rows(out_path, rows, FORMAT_HEADER.replace(_PL_LINE, _PL_LINE + SITE_FORMAT_LINES), columns)
    return n_done[0]


def genotype_with_counts_joint(ctx, vcf_path, slot_of, out_path, min_support, err, slot_is_presence):
    """genotype_with_counts with --joint-ins: the Python rows, the ordinary diploid call on all of them, then ONE svjg_genotype_sites call
    over the sites of form_sites; the members' GT and PL become the site call's projection (project_cohort_sites at S = 1), DP and AD stay the row's own"""
    rows, min_support, call_err, check = _open_call(vcf_path, slot_of, slot_is_presence, min_support, err)
    gt, pl, raw, done = ctx.genotype(rows.sv_type, rows.slot, rows.ok, min_support, call_err)
    check(done)
    pl, _ = apply_boundary_guard(ctx, rows, pl, raw, done, err)
    sites, skipped = form_sites(rows, done)
    _report_skipped(skipped)
    member = {}
    if sites:
        s_gt, s_pl, s_raw, s_boundary = ctx.genotype_sites(_site_slots(rows, sites), min_support, err)
        k_of, s_pl = np.array([len(m) for m in sites]), np.array(s_pl, dtype=np.int64)
        recompute_flagged_sites(s_pl, s_raw, s_boundary, k_of, err)
        _, g, pl3, _ = project_cohort_sites(np.asarray(s_gt)[:, None], s_pl[:, None], ((1 << k_of) - 1)[:, None])      # (every named slot is a member)
        for k, m in enumerate(sites):
            sgt = _sgt_text(int(s_gt[k, 0]), int(s_gt[k, 1]))
            for j, r in enumerate(m):
                member[r] = (int(g[k, 0, j]), pl3[k, 0, j].tolist(), sgt, j + 1)
    return write_vcf_joint(out_path, rows, gt, pl, raw, done, member)


# ---- cohort (--cohort [--cohort-ploidy FILE] [--cohort-prior] | [--joint-ins]): many samples' counts, one multi-sample VCF: the three svjg_genotype_cohort* calls (and svjg_genotype_cohort_sites behind the plain one), Python rows, one driver and one writer ----

COHORT_INFO_LINES = (
    '##INFO=<ID=NS,Number=1,Type=Integer,Description="Number of samples with a called genotype">\n'
    '##INFO=<ID=AN,Number=1,Type=Integer,Description="Total number of alleles in called genotypes">\n'
    '##INFO=<ID=AC,Number=A,Type=Integer,Description="Allele count in called genotypes">\n'
    '##INFO=<ID=AF,Number=A,Type=Float,Description="Allele frequency in called genotypes: AC / AN">\n'
)
_SITE_TAGS = ("NS=", "AN=", "AC=", "AF=")
_EM_KEYS = ("EMAF", "EMNC")
_QUAL_KEYS = ("SVQ", "MLAC", "MLAF")
COHORT_ITEM_BYTES = 37             # svjg.h: what one (row, sample) item takes in a svjg_genotype_cohort call
COHORT_CALL_BYTES = 1 << 30


def load_cohort_list(path):
    """-> [(name, json_path)] in file order.  One sample per line, `NAME<TAB>PATH_TO_informative_aln.json`; `#` lines and empty lines are
    skipped; a relative path is relative to the list's directory.  ValueError naming file and line for anything else: a line without exactly
    two fields, an empty name or path, a name given twice."""
    import os
    here = os.path.dirname(os.path.abspath(path))
    out, seen = [], set()
    with open(path) as fh:
        for no, line in enumerate(fh, 1):
            text = line.rstrip("\n").rstrip("\r")
            if not text or text.startswith("#"):
                continue
            f = text.split("\t")
            if len(f) != 2 or not f[0] or not f[1]:
                raise ValueError("%s:%d: expected `NAME<TAB>PATH`: %r" % (path, no, text))
            if f[0] in seen:
                raise ValueError("%s:%d: sample name %r is given twice" % (path, no, f[0]))
            seen.add(f[0])
            out.append((f[0], f[1] if os.path.isabs(f[1]) else os.path.join(here, f[1])))
    if not out:
        raise ValueError("%s: no sample" % path)
    return out


def cohort_union(samples):
    """samples: [(keys, counts[n, 2])], one per sample -> (union of the keys in first-seen order, [(slots, counts)] per sample: the slots the
    sample has as keys, each once; a key repeated within one sample: the last one wins, like json.load)"""
    slot_of, per = {}, []
    for keys, counts in samples:
        last = {}
        for i, k in enumerate(keys):
            if k not in slot_of:
                slot_of[k] = len(slot_of)
            last[slot_of[k]] = i
        slots = np.fromiter(last.keys(), dtype=np.uint32, count=len(last))
        at = np.fromiter(last.values(), dtype=np.int64, count=len(last))
        per.append((slots, np.asarray(counts, dtype=np.uint32).reshape(-1, 2)[at]))
    return list(slot_of), per


def cohort_info(info, ns, ac, an=None, em=None, qual=None, hwe=None):
    """the INFO column of a cohort row: the input's without any NS= / AN= / AC= / AF= field (whole fields, exact key), a lone `.` replaced,
    then NS, AN (2 NS unless given: the called samples' ploidies summed, --cohort-ploidy), AC and, when AN > 0, AF = "%.6g" % (AC / AN).
    em (--cohort-prior): (f, not_converged) of the row's EM — the input's EMAF= and EMNC fields are dropped too, EMAF = "%.6g" % f follows
    unless f is NaN (no estimate), and the flag EMNC when the step cap was reached.  qual (--cohort-qual): (svq, mlac, chroms) of the row's
    allele-count posterior — the input's SVQ= / MLAC= / MLAF= fields are dropped too; behind everything else SVQ = "%.2f" % svq unless it is NaN
    (a value that prints as -0.00 prints 0.00) and, where chroms > 0, MLAC and MLAF = "%.6g" % (mlac / chroms).  hwe (--cohort-hwe):
    ((n_ref, n_het, n_alt), p_hwe, p_exchet) of the row's called diploid samples — the input's DGC= / HWE= / EXCHET= / FIS= fields are dropped too;
    behind everything else DGC always, HWE and EXCHET = "%.6g" where there is an item (n > 0), FIS = "%.6g" % hwe_fis where there is a minor
    allele (a text of -0 prints 0)"""
    keep = [f for f in info.split(";") if not f.startswith(_SITE_TAGS)]
    if em is not None:
        keep = [f for f in keep if f.split("=", 1)[0] not in _EM_KEYS]
    if qual is not None:
        keep = [f for f in keep if f.split("=", 1)[0] not in _QUAL_KEYS]
    if hwe is not None:
        keep = [f for f in keep if f.split("=", 1)[0] not in _HWE_KEYS]
    if keep == ["."]:
        keep = []
    if an is None:
        an = 2 * ns
    keep += ["NS=%d" % ns, "AN=%d" % an, "AC=%d" % ac]
    if an > 0:
        keep.append("AF=%s" % ("%.6g" % (ac / an)))
    if em is not None:
        f, not_converged = em
        if f == f:
            keep.append("EMAF=%s" % ("%.6g" % f))
        if not_converged:
            keep.append("EMNC")
    if qual is not None:
        svq, mlac, chroms = qual
        if svq == svq:
            text = "%.2f" % svq
            keep.append("SVQ=%s" % ("0.00" if text == "-0.00" else text))
        if chroms > 0:
            keep += ["MLAC=%d" % mlac, "MLAF=%s" % ("%.6g" % (mlac / chroms))]
    if hwe is not None:
        dgc, p_hwe, p_exc = hwe
        keep.append("DGC=%d,%d,%d" % tuple(dgc))
        if sum(dgc) > 0:
            keep += ["HWE=%s" % ("%.6g" % p_hwe), "EXCHET=%s" % ("%.6g" % p_exc)]
        fis = hwe_fis(*dgc)
        if fis is not None:
            text = "%.6g" % fis
            keep.append("FIS=%s" % ("0" if text == "-0" else text))
    return ";".join(keep)


class CohortCalls(NamedTuple):
    """What a cohort call gives over all rows (genotype_cohort_rows): gt, done: [n, S]; pl: [n, S, >= 3]; raw: [n, S, 2]; site: [n, 2] = NS, AC or
    [n, 3] = NS, AN, AC.  With the prior (--cohort-prior) gt and site are the posterior calls', and gq[n, S], af[n], em_steps[n] are there"""
    gt: np.ndarray; pl: np.ndarray; raw: np.ndarray; done: np.ndarray; site: np.ndarray
    gq: np.ndarray = None; af: np.ndarray = None; em_steps: np.ndarray = None


class JointMember(NamedTuple):
    """A row that is a member of a site for at least one sample (cohort_joint_sites), one entry per sample: covered[S]; g[S] and pl3[S, 3], the
    projection of the sample's site call; a[S], b[S], that call; sal[S], the row's allele number in it.  With --joint-prior g, a and b are the
    POSTERIOR site call's and sgq[S] is there"""
    covered: np.ndarray; g: np.ndarray; pl3: np.ndarray; a: np.ndarray; b: np.ndarray; sal: np.ndarray
    sgq: np.ndarray = None


class JointSites(NamedTuple):
    """cohort_joint_sites' answer: site, the plain call's with the candidate rows' NS and AC replaced; joint: row -> JointMember; em (--joint-prior):
    row -> (p_j, not_converged) of the site's EM for the rows of joint"""
    site: np.ndarray; joint: dict
    em: dict = None


def _joint_columns(rows, raw, plain, joint):
    """columns(v) of a --cohort --joint-ins run from the plain cohort's: a row of `joint` (row -> JointMember) prints GT:DP:AD:PL:SGT:SAL — a
    covered sample what write_vcf_joint prints (DP and AD stay the row's own), every other sample its independent column and `:.:.` —; every other
    row is the plain one.  With sgq (--joint-prior): GT:DP:AD:PL:SGT:SAL:SGQ, SGQ `.` beside `./.`, and `:.:.:.` behind a sample without a site"""
    raw = np.asarray(raw)

    def columns(v):
        cols = plain(v)
        if v not in joint:
            return cols
        m = joint[v]
        covered, g, p3, a, b, sal = (x.tolist() for x in m[:6])
        t = int(rows.sv_type[v])
        out = [_member_column(t, g[s], p3[s], int(raw[v, s, 0]), int(raw[v, s, 1]), _sgt_text(a[s], b[s]), sal[s]) if covered[s]
               else col + ":.:." for s, col in enumerate(cols[1:])]
        if m.sgq is None:
            return ["GT:DP:AD:PL:SGT:SAL"] + out
        sgq = m.sgq.tolist()
        return ["GT:DP:AD:PL:SGT:SAL:SGQ"] + [col + (":." if not covered[s] or a[s] == NO_CALL else ":%d" % sgq[s]) for s, col in enumerate(out)]
    return columns


def write_vcf_cohort(out_path, rows, names, calls, ploidy=None, joint=None, qual=None, hwe=None):
    """The one cohort writer: write_vcf with one column per sample of `calls` (CohortCalls), the site tags' INFO lines in front of the header and
    the tags in INFO.  ploidy ([n, S]; None: diploid arrays, `Number=3`): every item in write_vcf_ploidy's forms and `Number=G` in the PL header
    line.  calls.gq: one more FORMAT field, GQ; calls.af and em_steps: EMAF / EMNC in INFO.  joint (JointSites): its site words stand for the
    calls', the member rows are printed by _joint_columns under SITE_FORMAT_LINES; joint.em: EMAF / EMNC in the member rows' INFO, and
    SITE_PRIOR_FORMAT_LINE behind SAL's.  qual (cohort_qual_rows): (svq[n], mlac[n], chroms[n]), SVQ / MLAC / MLAF behind the other tags in INFO
    and their header lines; the QUAL column stays the input's.  hwe (cohort_hwe_rows): (counts[n, 3], p[n, 2]), DGC / HWE / EXCHET / FIS behind all
    of them and their header lines behind all other INFO lines.  -> the number of genotyped rows of every sample"""
    columns, n_done = _item_columns(rows, ploidy, calls.gt, calls.pl, calls.raw, calls.done, calls.gq)
    header = FORMAT_HEADER if ploidy is None else FORMAT_HEADER.replace(_PL_3, _PL_G)
    site, em = calls.site, None                                  # em: row -> (frequency, not_converged) for the rows that have an EM
    if joint is not None:
        site, em = joint.site, joint.em
        columns = _joint_columns(rows, calls.raw, columns, joint.joint)
        header = header.replace(_PL_LINE, _PL_LINE + SITE_FORMAT_LINES + (SITE_PRIOR_FORMAT_LINE if em is not None else ""))
    if calls.gq is not None:
        header = header.replace("#CHROM\t", _GQ_LINE + "#CHROM\t")
    if calls.af is not None:
        not_converged = (np.asarray(calls.em_steps).astype(np.int64) & EM_NOT_CONVERGED) != 0
        em = dict(enumerate(zip(np.asarray(calls.af, dtype=np.float64).tolist(), not_converged.tolist())))
    info_lines = COHORT_INFO_LINES + (COHORT_PRIOR_INFO_LINES if em is not None else "") + (COHORT_QUAL_INFO_LINES if qual is not None else "") + (
        COHORT_HWE_INFO_LINES if hwe is not None else "")
    header = info_lines + header.replace("\tFORMAT\tSAMPLE\n", "\tFORMAT\t" + "\t".join(names) + "\n")
    has_an = np.shape(site)[1] == 3

    def info(v, text):
        return cohort_info(text, int(site[v, 0]), int(site[v, -1]), int(site[v, 1]) if has_an else None, None if em is None else em.get(v),
                           None if qual is None else (float(qual[0][v]), int(qual[1][v]), int(qual[2][v])),
                           None if hwe is None else (tuple(int(x) for x in hwe[0][v]), float(hwe[1][v][0]), float(hwe[1][v][1])))
    _write_rows(out_path, rows, header, columns, info)
    return n_done


def cohort_chunk_rows(n_samples, max_ploidy=None, prior=False):
    """rows per cohort call, so that it stays under 1 GiB.  An item takes 37 bytes in svjg_genotype_cohort (max_ploidy None; svjg.h), else
    8 (max_ploidy + 1) + 12, with the prior one more and 46 a row"""
    item = COHORT_ITEM_BYTES if max_ploidy is None else 8 * (int(max_ploidy) + 1) + 12 + bool(prior)
    return max(1, COHORT_CALL_BYTES // (item * max(1, int(n_samples)) + (46 if prior else 0)))


def _join_chunks(parts):
    """the tuples of the chunks of one call -> one list of arrays over all rows, field by field (a field that is None stays None)"""
    return [None if parts[0][k] is None else np.concatenate([p[k] for p in parts]) for k in range(len(parts[0]))]


def _cohort_rows(call, rows, step, empty, min_support, err, ploidy=None):
    """The one cohort driver: the rows of a VcfRows against the context's cohort matrix in chunks of `step` rows, call(lo, hi, min_support, err) ->
    the context's tuple (gt, pl, raw, done, boundary, site[, gq, af, em_steps]) per chunk -> CohortCalls over all rows (empty: the same for no row
    at all), the flagged items recomputed (the GT does not depend on the PL integers: the site words stay as the kernel gave them)"""
    min_support, call_err, bad_err = _call_args(min_support, err)
    parts = []
    for at in range(0, len(rows.sv_type), step):
        got = call(at, at + step, min_support, call_err)
        gt, pl, raw, done, boundary, site = got[:6]
        if bad_err and done.any():
            raise ValueError("math domain error")               # (as genotype_with_counts)
        recompute_flagged(rows.sv_type[at:at + step], pl, raw, done, boundary, err, None if ploidy is None else ploidy[at:at + step])
        parts.append(CohortCalls(gt, pl, raw, done, site, *got[6:]))
    return CohortCalls(*_join_chunks(parts)) if parts else empty


def _matrix_max_ploidy(ploidy):
    """a cohort call's ploidy matrix or None -> (the matrix as the library reads it or None, max_ploidy: 2 without a matrix, else its maximum, at least 1)"""
    ploidy = None if ploidy is None else np.ascontiguousarray(ploidy, dtype=np.uint8)
    return ploidy, 2 if ploidy is None else max(1, int(ploidy.max())) if ploidy.size else 1


def genotype_cohort_rows(ctx, rows, n_samples, min_support, err, ploidy=None, prior=False, step=None):
    """The cohort call over all rows -> CohortCalls.  ploidy None and no prior: svjg_genotype_cohort, gt (3: no call), pl[n, S, 3], site[n, 2] = NS,
    AC.  ploidy[n, S]: svjg_genotype_cohort_ploidy, gt (0xFF: no call), pl[n, S, max_ploidy + 1], site[n, 3] = NS, AN, AC; max_ploidy = the
    matrix's maximum, at least 1.  prior: svjg_genotype_cohort_prior, ploidy[n, S] or None (diploid), gt = the posterior calls (0xFF: none), site
    of them, and gq[n, S], af[n], em_steps[n].  step: rows per call (None: what fits 1 GiB)"""
    S = int(n_samples)
    ploidy, max_ploidy = _matrix_max_ploidy(ploidy)
    plain = ploidy is None and not prior

    def call(lo, hi, ms, e):
        if plain:
            return ctx.genotype_cohort(rows.sv_type[lo:hi], rows.slot[lo:hi], rows.ok[lo:hi], ms, e)
        fn = ctx.genotype_cohort_prior if prior else ctx.genotype_cohort_ploidy
        return fn(rows.sv_type[lo:hi], rows.slot[lo:hi], rows.ok[lo:hi], None if ploidy is None else ploidy[lo:hi], max_ploidy, ms, e)
    empty = CohortCalls(np.zeros((0, S), np.uint8), np.zeros((0, S, max_ploidy + 1), np.int64), np.zeros((0, S, 2), np.uint32), np.zeros((0, S), np.uint8),
                        np.zeros((0, 2 if plain else 3), np.uint32), *((np.zeros((0, S), np.uint8), np.zeros(0, np.float64), np.zeros(0, np.uint32)) if prior else ()))
    if step is None:
        step = cohort_chunk_rows(S, None if plain else max_ploidy, prior)
    return _cohort_rows(call, rows, int(step), empty, min_support, err, ploidy)


# ---- cohort at per-sample ploidy (--cohort LIST --cohort-ploidy FILE): the file and the ploidy matrix of svjg_genotype_cohort_ploidy ----

COHORT_PLOIDY_FORMS = "`SAMPLE<TAB>CHROM<TAB>PLOIDY` or `SAMPLE<TAB>CHROM<TAB>FROM<TAB>TO<TAB>PLOIDY`"


def load_cohort_ploidy_file(path, names):
    """-> per sample of `names`, in their order: [(chrom, from, to, ploidy)] as load_ploidy_file gives them, the lines of the file whose first
    field is the sample's name or `*` (every sample), in file order.  Lines are TAB-separated (a sample name may hold blanks):
    `SAMPLE<TAB>CHROM<TAB>PLOIDY` or `SAMPLE<TAB>CHROM<TAB>FROM<TAB>TO<TAB>PLOIDY`, the fields behind SAMPLE under load_ploidy_file's rules
    (_ploidy_region); `#` lines and empty lines are skipped.  ValueError naming file and line for anything else, a SAMPLE that is neither `*`
    nor in `names` included."""
    at = {name: s for s, name in enumerate(names)}
    per = [[] for _ in names]
    with open(path) as fh:
        for no, line in enumerate(fh, 1):
            text = line.rstrip("\n").rstrip("\r")
            if not text.strip() or text.startswith("#"):
                continue
            f = text.split("\t")
            rest = f[1:]
            if not f[0] or any(x.split() != [x] for x in rest):    # (an empty field, or one with a blank in it: no line of a --ploidy-file says that)
                rest = []
            region = _ploidy_region(rest, path, no, line, COHORT_PLOIDY_FORMS)
            if f[0] == "*":
                for regions in per:
                    regions.append(region)
            elif f[0] in at:
                per[at[f[0]]].append(region)
            else:
                raise ValueError("%s:%d: sample %r is not in the cohort list (`*`: every sample)" % (path, no, f[0]))
    return per


def cohort_ploidy_matrix(rows, per_sample_regions):
    """ploidy[n_rows, S] uint8: column s = rows_ploidy(rows, regions=the sample's lines) — the first matching line wins, 2 where none matches.
    Samples with the same lines share one pass over the rows."""
    out = np.empty((len(rows.chrom), len(per_sample_regions)), dtype=np.uint8)
    seen = {}
    for s, regions in enumerate(per_sample_regions):
        key = tuple(regions)
        if key not in seen:
            seen[key] = rows_ploidy(rows, None, regions)
        out[:, s] = seen[key]
    return out


# ---- cohort with an allele-frequency prior (--cohort LIST --cohort-prior [--cohort-ploidy FILE]): the header lines of svjg_genotype_cohort_prior's fields ----

COHORT_PRIOR_INFO_LINES = (
    '##INFO=<ID=EMAF,Number=A,Type=Float,Description="Allele frequency estimated from all samples\' genotype likelihoods by EM under Hardy-Weinberg">\n'
    '##INFO=<ID=EMNC,Number=0,Type=Flag,Description="The EM for EMAF reached its step limit without converging">\n'
)
_GQ_LINE = '##FORMAT=<ID=GQ,Number=1,Type=Integer,Description="Genotype quality: -10 log10 of the posterior probability that the call is wrong, at most 99">\n'
EM_NOT_CONVERGED = 1 << 31         # svjg.h: bit 31 of a row's em_steps word


# ---- cohort site quality (--cohort LIST --cohort-qual [--cohort-theta X]): svjg_cohort_qual beside whichever cohort call the run makes ----

COHORT_QUAL_INFO_LINES = (
    '##INFO=<ID=SVQ,Number=1,Type=Float,Description="Site quality: -10 log10 of the posterior probability that no sample of the cohort carries the alt allele (exact allele-count posterior)">\n'
    '##INFO=<ID=MLAC,Number=A,Type=Integer,Description="Allele count at the maximum of the cohort\'s allele-count posterior">\n'
    '##INFO=<ID=MLAF,Number=A,Type=Float,Description="MLAC over the chromosomes of the samples whose reads took part">\n'
)
COHORT_QUAL_THETA = 1e-3           # the default of --cohort-theta
COHORT_QUAL_THETA_MAX = 0.05       # svjg.h: theta of svjg_cohort_qual lies in (0, 0.05]
COHORT_THETA_RANGE = "--cohort-theta: a value in (0, %g]" % COHORT_QUAL_THETA_MAX
JOINT_INS_QUAL = "--joint-ins cannot be combined with --cohort-qual: the site model there is multi-allelic"


def cohort_qual_rows(ctx, rows, n_samples, ploidy, err, theta=COHORT_QUAL_THETA, step=None):
    """svjg_cohort_qual over all rows, in the row chunks of the cohort call (step: rows per call, None: cohort_chunk_rows of the plain call — a row's
    answer depends on no other row, so any chunking gives the same bytes).  ploidy[n, S] or None (diploid) -> (qual[n], mlac[n], chroms[n])"""
    _, call_err, _ = _call_args(0, err)
    ploidy, max_ploidy = _matrix_max_ploidy(ploidy)
    if step is None:
        step = cohort_chunk_rows(n_samples, None if ploidy is None else max_ploidy)
    parts = [ctx.cohort_qual(rows.sv_type[at:at + step], rows.slot[at:at + step], rows.ok[at:at + step], None if ploidy is None else ploidy[at:at + step],
                             max_ploidy, call_err, theta) for at in range(0, len(rows.sv_type), int(step))]
    if not parts:
        return np.zeros(0, np.float64), np.zeros(0, np.uint32), np.zeros(0, np.uint32)
    return tuple(_join_chunks(parts))


# ---- cohort calls for insertions that share a position (--cohort LIST --joint-ins [--joint-prior]): svjg_genotype_cohort_sites (svjg_genotype_cohort_sites_prior) behind the plain cohort call ----

JOINT_INS_COHORT = "--joint-ins is diploid only: with --cohort it cannot be combined with --cohort-ploidy or --cohort-prior"
COHORT_SITES_ITEM_BYTES = 256      # svjg.h: what one (site, sample) item takes in a svjg_genotype_cohort_sites call,
COHORT_SITES_SITE_BYTES = 72       # and one site
JOINT_PRIOR_NEEDS = "--joint-prior needs --cohort and --joint-ins: it is the allele-frequency prior over the samples of a multi-allelic site"
COHORT_SITES_PRIOR_ITEM_BYTES = 259      # svjg.h: svjg_genotype_cohort_sites_prior adds sgt and sgq to an item,
COHORT_SITES_PRIOR_SITE_BYTES = 180      # and p[7], the step word and the posterior's NS_j, AC_j to a site
SITE_PRIOR_FORMAT_LINE = '##FORMAT=<ID=SGQ,Number=1,Type=Integer,Description="Quality of SGT under the site\'s allele frequencies: -10 log10 of the posterior probability that the joint call is wrong, at most 99">\n'


def cohort_sites_chunk(n_samples, prior=False):
    """sites per svjg_genotype_cohort_sites call (prior: svjg_genotype_cohort_sites_prior), so that it stays under 1 GiB"""
    item, site = (COHORT_SITES_PRIOR_ITEM_BYTES, COHORT_SITES_PRIOR_SITE_BYTES) if prior else (COHORT_SITES_ITEM_BYTES, COHORT_SITES_SITE_BYTES)
    fixed = 256 if prior else 0          # the pair, the logarithms, the spare bytes and the alignments of the block (the plain call's chunks stay what they were)
    return max(1, (COHORT_CALL_BYTES - fixed) // (item * max(1, int(n_samples)) + site))


def project_cohort_sites(s_gt, s_pl, members):
    """project_site for every (site, sample, candidate) at once.  s_gt[n, S, 2], s_pl[n, S, 28], members[n, S] as svjg_genotype_cohort_sites returns
    them -> (covered[n, S, 6]: the candidate is a member of the sample's site, K' >= 2; g[n, S, 6]: its copies 0..2, 3 = the site has no call;
    pl3[n, S, 6, 3]: the smallest site PL per copy number; sal[n, S, 6]: its allele number, 0 where it is absent).  numpy over the index sets of
    every (K', allele): no loop over items."""
    members = np.asarray(members)
    bits = ((members[..., None] >> np.arange(MAX_SITE_ALTS, dtype=np.uint8)) & 1).astype(np.int64)
    k_of = bits.sum(axis=-1)
    sal = np.cumsum(bits, axis=-1) * bits
    covered = (bits != 0) & (k_of[..., None] >= 2)
    a, b = np.asarray(s_gt)[..., 0, None].astype(np.int64), np.asarray(s_gt)[..., 1, None].astype(np.int64)
    g = np.where(a == NO_CALL, 3, (a == sal).astype(np.int64) + (b == sal)).astype(np.uint8)
    pl3 = np.zeros(members.shape + (MAX_SITE_ALTS, 3), dtype=np.int64)
    for K in range(2, MAX_SITE_ALTS + 1):
        of_k = covered & (k_of[..., None] == K)
        if not of_k.any():
            continue
        for i in range(1, K + 1):
            at = np.nonzero(of_k & (sal == i))
            if not len(at[0]):
                continue
            site_pl = s_pl[at[0], at[1]]
            for n, idx in enumerate(_site_copy_sets(K, i)):
                pl3[at[0], at[1], at[2], n] = site_pl[:, idx].min(axis=1)
    return covered, g, pl3, sal


def cohort_joint_sites(ctx, rows, gt, site, min_support, err, step=None, prior=False):
    """Behind the plain cohort call (gt[n, S], site[n, 2] = NS, AC): the candidate sites at the VCF level — the INS rows with ok & 1 and a slot
    that share CHROM and POS text, 2..6 of them in file order (form_sites; more than six: skipped for every sample, one stderr line) —, ONE
    svjg_genotype_cohort_sites call over them (chunks of `step` sites, None: what fits 1 GiB), the flagged items recomputed with their own K'
    (exact_pl_site), the projection.  -> JointSites: site with the candidate rows' NS and AC replaced (the kernel's sums over the covered samples
    plus the independent calls of the others) and joint, the rows covered in at least one sample.  prior (--joint-prior): svjg_genotype_cohort_sites_prior
    instead — the PLs, and so the flagged items' recomputation, are the same; g, a, b and the sums are the POSTERIOR calls', the members carry
    sgq[S], and em is there (p_j: the EM's frequency of that row's allele, NaN where no item of the site took part)"""
    min_support, call_err, _ = _call_args(min_support, err)
    sites, skipped = form_sites(rows, ((rows.ok & 1) != 0) & (rows.slot != NONE))
    _report_skipped(skipped)
    site, joint, em = np.array(site), {}, {} if prior else None
    if not sites:
        return JointSites(site, joint, em)
    slots = _site_slots(rows, sites)
    if step is None:
        step = cohort_sites_chunk(np.shape(gt)[1], prior)
    call = ctx.genotype_cohort_sites_prior if prior else ctx.genotype_cohort_sites
    got = _join_chunks([call(slots[at:at + step], min_support, call_err) for at in range(0, len(sites), int(step))])
    s_gt, s_pl, s_raw, members, boundary, s_site = got[:6]
    recompute_flagged_sites(s_pl, s_raw, boundary, ((members[..., None] >> np.arange(MAX_SITE_ALTS, dtype=np.uint8)) & 1).sum(axis=-1), err)
    sgq = None
    if prior:
        s_gt, sgq, af, em_steps, s_site = got[6:]                # (the EM never reads PLs: the posterior calls stand as the kernel gave them)
    covered, g, pl3, sal = project_cohort_sites(s_gt, s_pl, members)
    k_of = np.repeat(np.arange(len(sites)), [len(m) for m in sites])
    j_of = np.concatenate([np.arange(len(m)) for m in sites])
    r_of = np.concatenate([np.asarray(m, dtype=np.int64) for m in sites])
    cov = covered[k_of, :, j_of]                                 # [candidate rows, S]
    own = np.asarray(gt)[r_of]
    alone = (own != 3) & ~cov                                    # the samples whose item has no site there keep their independent call
    site[r_of, 0] = s_site[k_of, j_of, 0] + alone.sum(axis=1)
    site[r_of, 1] = s_site[k_of, j_of, 1] + np.where(alone, own, 0).sum(axis=1)
    for c in np.flatnonzero(cov.any(axis=1)).tolist():
        k, j = k_of[c], j_of[c]
        joint[int(r_of[c])] = JointMember(cov[c], g[k, :, j], pl3[k, :, j], s_gt[k, :, 0], s_gt[k, :, 1], sal[k, :, j], sgq[k] if prior else None)
        if prior:
            em[int(r_of[c])] = (float(af[k, 1 + j]), bool(int(em_steps[k]) & EM_NOT_CONVERGED))
    return JointSites(site, joint, em)


# ---- cohort sample QC (--cohort LIST --cohort-qc PREFIX): svjg_cohort_qc on the calls the run has made, PREFIX.samples.tsv and PREFIX.pairs.tsv ----

COHORT_QC_NEEDS = "--cohort-qc needs --cohort: it summarises the samples of a cohort run"
COHORT_QC_PREFIX = "--cohort-qc: the prefix of PREFIX.samples.tsv and PREFIX.pairs.tsv must not be empty"
QC_SAMPLES_HEADER = "#SAMPLE\tN_ELIGIBLE\tN_CALLED\tCALL_RATE\tN_CARRIER\tN_DIPLOID\tN_HET\tN_HOMALT\tHET_HOMALT\n"
QC_PAIRS_HEADER = "#SAMPLE1\tSAMPLE2\tN_BOTH\tHET1\tHET2\tHETHET\tIBS0\tKINSHIP\tRELATION\n"
KINSHIP_BOUNDS = ((2.0 ** -1.5, "DUP"), (2.0 ** -2.5, "1ST"), (2.0 ** -3.5, "2ND"), (2.0 ** -4.5, "3RD"))


def kinship(het1, het2, hethet, ibs0):
    """KING-robust (Manichaikul et al. 2010) on svjg_cohort_qc's counts of a pair, in Python integers and ONE true division:
    0.5 - (4 ibs0 + (het1 - hethet) + (het2 - hethet)) / (4 min(het1, het2)); None where that minimum is 0 (no estimate).  Equal columns: exactly 0.5"""
    het1, het2, hethet, ibs0 = int(het1), int(het2), int(hethet), int(ibs0)
    m = min(het1, het2)
    if m == 0:
        return None
    return 0.5 - (4 * ibs0 + (het1 - hethet) + (het2 - hethet)) / (4 * m)


def relation(phi):
    """the degree a kinship says, decided on the double: above 2^-1.5 DUP, 2^-2.5 1ST, 2^-3.5 2ND, 2^-4.5 3RD, else UN"""
    for bound, name in KINSHIP_BOUNDS:
        if phi > bound:
            return name
    return "UN"


def kinship_text(phi):
    """"%.4f", and 0.0000 for a value that would print -0.0000"""
    text = "%.4f" % phi
    return "0.0000" if text == "-0.0000" else text


def _ratio_text(a, b):
    return "%.6g" % (a / b) if b else "."


def _calls_chunk_rows(n_samples, per_item, row_bytes, fixed):
    """rows per call of a statistic over the run's calls (svjg_cohort_qc, svjg_cohort_hwe), so that it stays under 1 GiB and under the call's 2^32
    rows: 1 byte an item, 2 with a ploidy array, row_bytes a row beside them, `fixed` a call whatever its rows, and the block's own 256"""
    return max(1, min((1 << 32) - 1, (COHORT_CALL_BYTES - fixed - 256) // (max(1, int(n_samples)) * (2 if per_item else 1) + row_bytes)))


def cohort_qc_chunk_rows(n_samples, per_item=False):
    """rows per svjg_cohort_qc call (svjg.h: 3 bits of planes an item; 20 bytes a pair, 24 a sample, and 24 a sample for the planes' last word begun)"""
    S = max(1, int(n_samples))
    return _calls_chunk_rows(S, per_item, (3 * S + 7) // 8, 20 * (S * (S - 1) // 2) + 24 * S + 24 * S)


def _calls_chunks(call, chunk_rows, gt, done, ploidy, step):
    """The one walk of cohort_qc_rows and cohort_hwe_rows: gt with NO_CALL where done == 0 and ploidy (contiguous, or None) go to call(gt, ploidy)
    in chunks of `step` rows (None: chunk_rows(S, per_item)) -> the list of its answers, a chunk each (no row: empty)"""
    gt = np.where(np.asarray(done) != 0, np.asarray(gt, dtype=np.uint8), np.uint8(NO_CALL)).astype(np.uint8)
    n, S = gt.shape
    ploidy = None if ploidy is None else np.ascontiguousarray(ploidy, dtype=np.uint8)
    step = chunk_rows(S, ploidy is not None) if step is None else int(step)
    return [call(gt[at:at + step], None if ploidy is None else ploidy[at:at + step]) for at in range(0, n, step)]


def cohort_qc_rows(ctx, gt, done, ploidy, step=None):
    """svjg_cohort_qc over all rows of a cohort run's calls: gt[n, S] and done[n, S] as CohortCalls has them — an item with done == 0 goes in as
    0xFF, not called whatever its ploidy —, ploidy[n, S] or None (diploid).  Rows in chunks of `step` (None: cohort_qc_chunk_rows); the chunks'
    integer outputs are summed in int64, so any chunking gives the same numbers.  -> (sample[S, 6], pair[S (S - 1) / 2, 5]) int64"""
    S = np.shape(gt)[1]
    sample, pair = np.zeros((S, 6), np.int64), np.zeros((S * (S - 1) // 2, 5), np.int64)
    for s, p in _calls_chunks(ctx.cohort_qc, cohort_qc_chunk_rows, gt, done, ploidy, step):
        sample += s
        pair += np.asarray(p).reshape(-1, 5)
    return sample, pair


def printed_gt(calls, joint=None):
    """gt[n, S] as the cohort writer prints it: calls.gt, and on a row of joint.joint (--joint-ins) the projection of the site call for the samples
    the site covers (3: the site has no call), the row-by-row call for the others"""
    gt = np.array(calls.gt, dtype=np.uint8)
    if joint is not None:
        for v, m in joint.joint.items():
            gt[v] = np.where(m.covered, m.g, gt[v])
    return gt


def write_qc_samples(path, names, sample):
    """PREFIX.samples.tsv: a line per sample of the cohort list, in its order; CALL_RATE = called / eligible and HET_HOMALT = het / homalt as
    "%.6g", `.` where the denominator is 0"""
    with open(path, "w") as fh:
        fh.write(QC_SAMPLES_HEADER)
        for name, row in zip(names, np.asarray(sample).tolist()):
            eligible, called, carrier, dip, het, homalt = row
            fh.write("%s\t%d\t%d\t%s\t%d\t%d\t%d\t%d\t%s\n" % (name, eligible, called, _ratio_text(called, eligible), carrier, dip, het, homalt,
                                                                _ratio_text(het, homalt)))


def write_qc_pairs(path, names, pair):
    """PREFIX.pairs.tsv: a line per pair i < j in the order of svjg_cohort_qc's k; KINSHIP as kinship_text and RELATION from the double, both `.`
    where there is no estimate"""
    rows = np.asarray(pair).tolist()
    with open(path, "w") as fh:
        fh.write(QC_PAIRS_HEADER)
        k = 0
        for i in range(len(names)):
            for j in range(i + 1, len(names)):
                both, het1, het2, hethet, ibs0 = rows[k]
                k += 1
                phi = kinship(het1, het2, hethet, ibs0)
                fh.write("%s\t%s\t%d\t%d\t%d\t%d\t%d\t%s\t%s\n" % (names[i], names[j], both, het1, het2, hethet, ibs0,
                                                                    "." if phi is None else kinship_text(phi), "." if phi is None else relation(phi)))


# ---- cohort site test for Hardy-Weinberg equilibrium (--cohort LIST --cohort-hwe): svjg_cohort_hwe on the calls the run has made, DGC / HWE / EXCHET / FIS in INFO ----

COHORT_HWE_INFO_LINES = (
    '##INFO=<ID=DGC,Number=3,Type=Integer,Description="Genotype counts hom-ref, het, hom-alt, called diploid samples only">\n'
    '##INFO=<ID=HWE,Number=1,Type=Float,Description="Exact two-sided test of Hardy-Weinberg equilibrium (Wigginton et al. 2005), called diploid samples only">\n'
    '##INFO=<ID=EXCHET,Number=1,Type=Float,Description="Exact one-sided test for an excess of heterozygotes, called diploid samples only">\n'
    '##INFO=<ID=FIS,Number=1,Type=Float,Description="Inbreeding coefficient 1 - observed / expected heterozygotes, called diploid samples only">\n'
)
_HWE_KEYS = ("DGC", "HWE", "EXCHET", "FIS")


def hwe_fis(n_ref, n_het, n_alt):
    """the inbreeding coefficient of a row from svjg_cohort_hwe's counts, in Python integers and ONE true division: 1 - n_het 2 n / (nA nB) with
    nA = 2 n_alt + n_het, nB = 2 n_ref + n_het; None where min(nA, nB) = 0 (no minor allele: no estimate)"""
    n_ref, n_het, n_alt = int(n_ref), int(n_het), int(n_alt)
    nA, nB = 2 * n_alt + n_het, 2 * n_ref + n_het
    if min(nA, nB) == 0:
        return None
    return 1 - n_het * 2 * (n_ref + n_het + n_alt) / (nA * nB)


def cohort_hwe_chunk_rows(n_samples, per_item=False):
    """rows per svjg_cohort_hwe call (svjg.h: 28 bytes a row)"""
    return _calls_chunk_rows(n_samples, per_item, 28, 0)


def cohort_hwe_rows(ctx, gt, done, ploidy, step=None):
    """svjg_cohort_hwe over all rows of a cohort run's calls: gt[n, S] and done[n, S] as CohortCalls has them — an item with done == 0 goes in as
    0xFF, not called whatever its ploidy, as in cohort_qc_rows —, ploidy[n, S] or None (diploid).  Rows in chunks of `step` (None:
    cohort_hwe_chunk_rows), concatenated: a row's numbers do not depend on its chunk.  -> (counts[n, 3] uint32, p[n, 2] float64)"""
    parts = _calls_chunks(ctx.cohort_hwe, cohort_hwe_chunk_rows, gt, done, ploidy, step)
    return (np.concatenate([np.zeros((0, 3), np.uint32)] + [np.asarray(c, dtype=np.uint32).reshape(-1, 3) for c, _ in parts]),
            np.concatenate([np.zeros((0, 2), np.float64)] + [np.asarray(q, dtype=np.float64).reshape(-1, 2) for _, q in parts]))


def check_cohort_options(ploidy_file=None, prior=False, joint_ins=False, joint_prior=False, qual=False, theta=COHORT_QUAL_THETA, qc=None, hwe=False):
    """The rules between the options of a cohort run (run_cohort, predict-genotype.py --cohort): ValueError with the first broken rule's text
    (hwe, --cohort-hwe, stands beside every other option: no rule names it)"""
    if joint_ins and (ploidy_file is not None or prior):
        raise ValueError(JOINT_INS_COHORT)
    if joint_prior and not joint_ins:
        raise ValueError(JOINT_PRIOR_NEEDS)
    if qual and not 0.0 < theta <= COHORT_QUAL_THETA_MAX:
        raise ValueError(COHORT_THETA_RANGE)
    if joint_ins and qual:
        raise ValueError(JOINT_INS_QUAL)
    if qc is not None and not qc:
        raise ValueError(COHORT_QC_PREFIX)


def run_cohort(list_path, vcf_path, out_path, min_support=3, err=0.00005, device=0, ploidy_file=None, prior=False, joint_ins=False, qual=False,
               theta=COHORT_QUAL_THETA, joint_prior=False, qc=None, hwe=False):
    """predict-genotype.py --cohort: the samples of a cohort list (load_cohort_list), one multi-sample VCF.  Sample column s is what the
    reference writes as SAMPLE for sample s alone; INFO gains NS, AN, AC and AF.  ploidy_file (--cohort-ploidy, load_cohort_ploidy_file): a
    ploidy per sample and contig or region; column s is then what --ploidy-file with the sample's lines writes for sample s alone, and AN is
    the called samples' ploidies summed.  prior (--cohort-prior): GT is the call under the row's allele frequency, estimated from all samples by EM
    (svjg_genotype_cohort_prior), with GQ beside it and EMAF / EMNC in INFO; DP, AD and PL stay those of the plain run.  joint_ins (--joint-ins,
    diploid only: neither ploidy_file nor prior): the insertions that share a position are genotyped together per sample (cohort_joint_sites);
    column s is then what --joint-ins writes for sample s alone, but for `:.:.` behind a sample that has no site on a row another sample has one
    on, and for a position with more than six candidate rows, which is skipped for EVERY sample.  qual (--cohort-qual, theta: --cohort-theta; with
    any of the above but joint_ins): INFO gains SVQ, MLAC and MLAF of the row's exact allele-count posterior (svjg_cohort_qual); every other byte
    of the file stays what it is without it.  joint_prior (--joint-prior, with joint_ins only): the samples of a site inform each other — the
    frequencies of the site's alleles by EM (svjg_genotype_cohort_sites_prior); a member row prints GT:DP:AD:PL:SGT:SAL:SGQ with GT the projection of the
    POSTERIOR site call and SGT that call, NS / AC / AN / AF come from the posterior calls, EMAF and EMNC follow them; every non-member row stays the
    plain cohort row.  qc (--cohort-qc PREFIX, with any of the above): svjg_cohort_qc on the calls the file prints (printed_gt, calls.done) — with prior the
    posterior calls, with joint_ins a member row's projected site calls — and, once the VCF has been written, PREFIX.samples.tsv (write_qc_samples) and PREFIX.pairs.tsv
    (write_qc_pairs); no byte of the VCF changes.  hwe (--cohort-hwe, with any of the above): svjg_cohort_hwe on the same printed calls; INFO gains DGC, HWE,
    EXCHET and FIS behind every other tag (cohort_info), the header their four lines; every other byte stays what it is without it.
    -> the number of genotyped rows of every sample"""
    from . import capi, filter as flt
    check_cohort_options(ploidy_file, prior, joint_ins, joint_prior, qual, theta, qc, hwe)     # (before anything is read, asked of the device or written)
    samples = load_cohort_list(list_path)                       # (raises before any output exists)
    names = [name for name, _ in samples]
    regions = load_cohort_ploidy_file(ploidy_file, names) if ploidy_file is not None else None   # (so does this)
    loaded = []
    for _, path in samples:
        got = flt.read_handoff(path)                             # left by our filter-alignments.py for exactly this file, else None
        loaded.append(got if got is not None else capi.count_informative_json(path))
    keys, per = cohort_union(loaded)
    rows = open_rows(vcf_path, keys, native=False)
    ploidy = cohort_ploidy_matrix(rows, regions) if regions is not None else None
    ctx = capi.Context(device)
    try:
        ctx.cohort_alloc(len(samples), len(keys))
        for s, (slots, counts) in enumerate(per):
            ctx.cohort_set_counts(s, slots, counts)
        calls = genotype_cohort_rows(ctx, rows, len(samples), min_support, err, ploidy, prior)
        joint = cohort_joint_sites(ctx, rows, calls.gt, calls.site, min_support, err, prior=joint_prior) if joint_ins else None
        site_qual = cohort_qual_rows(ctx, rows, len(samples), ploidy, err, theta) if qual else None
        printed = printed_gt(calls, joint) if qc is not None or hwe else None
        qc_counts = cohort_qc_rows(ctx, printed, calls.done, ploidy) if qc is not None else None
        site_hwe = cohort_hwe_rows(ctx, printed, calls.done, ploidy) if hwe else None
    finally:
        ctx.close()
    n_done = write_vcf_cohort(out_path, rows, names, calls, ploidy, joint, site_qual, site_hwe)
    if qc is not None:
        write_qc_samples(qc + ".samples.tsv", names, qc_counts[0])
        write_qc_pairs(qc + ".pairs.tsv", names, qc_counts[1])
    for name, n in zip(names, n_done):
        print("Genotyped svs (%s): %d" % (name, n))
    return n_done


def write_vcf(out_path, rows, gt, pl, raw, done):
    columns, n_done = _item_columns(rows, None, gt, pl, raw, done)
    _write_rows(out_path, rows, FORMAT_HEADER, columns)
    return n_done[0]


def open_rows(vcf_path, slot_of, slot_is_presence=False, native=True):
    """The rows of the VCF with their count slots: the native reader (libsvjg_host, svjg_vcf_load) for ordinary files, the
    Python rows above (the semantics, and what raises the reference's exceptions) for everything it declines.
    slot_of: dict key -> slot, or a list of keys (slot = index; a repeated key: the last one wins, like json.load).
    SVJG_PY_VCF=1, or native False, forces the Python rows."""
    import os
    from . import capi
    if native and not os.environ.get("SVJG_PY_VCF"):
        slots = np.fromiter(slot_of.values(), dtype=np.uint32, count=len(slot_of)) if isinstance(slot_of, dict) else None
        rows = capi.vcf_load_native(vcf_path, slot_of, slots, slot_is_presence)      # (a dict gives its keys)
        if rows is not None:
            return rows
    if not isinstance(slot_of, dict):
        slot_of = {k: i for i, k in enumerate(slot_of)}
    return VcfRows(vcf_path, slot_of, slot_is_presence)


def genotype_with_counts(ctx, vcf_path, slot_of, out_path, min_support=3, err=0.00005, slot_is_presence=False, ploidy=None, ploidy_file=None,
                         joint_ins=False):
    """Counts already live in the context (fused path, or set_counts): parse, run the kernel, write.  ploidy (1..8, every row) and / or
    ploidy_file (per contig or region, load_ploidy_file): genotype_with_counts_ploidy; joint_ins (insertions that share a position are
    genotyped together, diploid only): genotype_with_counts_joint; with none of them, the diploid path below."""
    check_single_options(ploidy, ploidy_file, joint_ins)         # (before anything is asked of the device or written)
    if joint_ins:
        return genotype_with_counts_joint(ctx, vcf_path, slot_of, out_path, min_support, err, slot_is_presence)
    if ploidy is not None or ploidy_file is not None:
        return genotype_with_counts_ploidy(ctx, vcf_path, slot_of, out_path, min_support, err, slot_is_presence, ploidy, ploidy_file)
    rows, min_support, call_err, check = _open_call(vcf_path, slot_of, slot_is_presence, min_support, err, native=True)
    gt, pl, raw, done = ctx.genotype(rows.sv_type, rows.slot, rows.ok, min_support, call_err, reuse_outputs=True)   # views: written out right away
    check(done)
    pl, _ = apply_boundary_guard(ctx, rows, pl, raw, done, err)
    if isinstance(rows, VcfRows):
        return write_vcf(out_path, rows, gt, pl, raw, done)
    try:
        return rows.write(out_path, gt, pl, raw, done)
    finally:
        rows.close()


def run(json_path, vcf_path, out_path, min_support=3, err=0.00005, device=0, ploidy=None, ploidy_file=None, joint_ins=False):
    """predict-genotype.py main(): counts come from the informative-alignment JSON."""
    from . import capi, filter as flt
    check_single_options(ploidy, ploidy_file, joint_ins)
    got = flt.read_handoff(json_path)                            # left by our filter-alignments.py for exactly this file, else None
    if got is None:
        got = capi.count_informative_json(json_path)             # len() of the two lists of every key (:219-226)
    keys, counts = got                                           # (a repeated key: the last one wins, like json.load — open_rows)
    ctx = capi.Context(device)
    try:
        ctx.alloc_counts(len(keys))
        ctx.set_counts(counts)
        n = genotype_with_counts(ctx, vcf_path, list(keys), out_path, min_support, err, slot_is_presence=True, ploidy=ploidy, ploidy_file=ploidy_file,
                                 joint_ins=joint_ins)
    finally:
        ctx.close()
    print("Genotyped svs: " + str(n))
    return n
