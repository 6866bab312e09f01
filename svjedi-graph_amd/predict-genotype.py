#!/usr/bin/env python3
"""Drop-in for SVJedi-graph's predict-genotype.py (same flags, same files) running on an MI355X.

    predict-genotype.py -d P_informative_aln.json -v VCF --minsupport N -o P_genotype.vcf   (svjedi-graph.py:124)
    predict-genotype.py --cohort LIST -v VCF --minsupport N -o COHORT_genotype.vcf          (extension: one column per sample)
    predict-genotype.py --cohort LIST --cohort-ploidy FILE -v VCF ...                       (extension: a ploidy per sample and contig or region)
    predict-genotype.py --cohort LIST --cohort-prior [--cohort-ploidy FILE] -v VCF ...      (extension: calls under the cohort's allele frequency, with GQ)
    predict-genotype.py --cohort LIST --joint-ins -v VCF ...                                (extension: insertions that share a position, together per sample)
    predict-genotype.py --cohort LIST --joint-ins --joint-prior -v VCF ...                  (extension: the samples of such a site inform each other, with SGQ)
    predict-genotype.py --cohort LIST --cohort-qual [--cohort-theta X] -v VCF ...           (extension: SVQ / MLAC / MLAF, the cohort's exact allele-count posterior)
    predict-genotype.py --cohort LIST --cohort-qc PREFIX -v VCF ...                         (extension: PREFIX.samples.tsv and PREFIX.pairs.tsv, per-sample sums and pairwise kinship)
    predict-genotype.py --cohort LIST --cohort-hwe -v VCF ...                               (extension: DGC / HWE / EXCHET / FIS, the exact test of Hardy-Weinberg equilibrium per site)
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))


def main():
    ap = argparse.ArgumentParser(description="Structural variations genotyping using long reads")
    # -d stays required when --cohort is absent: every command line of the reference parses, and fails, as before
    ap.add_argument("-d", "--aln", metavar="<alndict>", nargs=1, required=not any(a == "--cohort" or a.startswith("--cohort=") for a in sys.argv[1:]))
    ap.add_argument("-v", "--vcf", metavar="<vcffile>", help="vcf format", required=True)
    ap.add_argument("-o", "--output", metavar="<output>", nargs=1, help="output file")
    ap.add_argument("-e", "--err", nargs=1, type=float, help="allele error probability")
    ap.add_argument("-ms", "--minsupport", metavar="<minNbAln>", type=int, default=3,
                    help="Minimum number of alignments to genotype a SV (default: 3>=)")
    ap.add_argument("--ploidy", metavar="<ploidy>", type=int, choices=range(1, 9),
                    help="ploidy of every SV, 1..8 (extension; default: the reference's diploid model)")
    ap.add_argument("--ploidy-file", metavar="<ploidyfile>",
                    help="per-contig or per-region ploidy, 0..8: lines `CHROM PLOIDY` or `CHROM FROM TO PLOIDY` (extension)")
    ap.add_argument("--joint-ins", action="store_true",
                    help="genotype insertions that share a CHROM and POS together, 2..6 per site, diploid only (extension).  With --cohort: per "
                         "sample, over the rows that sample has counts for; a position with more than six such rows in the VCF is skipped for "
                         "every sample (a single-sample run forms a site there when at most six of them are present in that sample)")
    ap.add_argument("--joint-prior", action="store_true",
                    help="with --cohort --joint-ins: estimate the frequencies of a site's alleles from all samples by EM under Hardy-Weinberg and call "
                         "every sample's site at the maximum of likelihood x prior; member rows gain SGQ, INFO gains EMAF and EMNC, DP / AD / PL stay "
                         "as without it (extension)")
    ap.add_argument("--cohort", metavar="<samplelist>",
                    help="many samples, one multi-sample VCF with NS / AN / AC / AF in INFO: lines `NAME<TAB>PATH_TO_informative_aln.json` "
                         "(extension; takes the place of -d; diploid, row by row, unless --cohort-ploidy is given; --joint-ins genotypes "
                         "insertions that share a position together)")
    ap.add_argument("--cohort-ploidy", metavar="<cohortploidyfile>",
                    help="with --cohort: per-sample ploidy, 0..8, TAB-separated lines `SAMPLE<TAB>CHROM<TAB>PLOIDY` or "
                         "`SAMPLE<TAB>CHROM<TAB>FROM<TAB>TO<TAB>PLOIDY`, SAMPLE a name of the list or `*`; the first matching line wins, 2 otherwise (extension)")
    ap.add_argument("--cohort-prior", action="store_true",
                    help="with --cohort: estimate each row's allele frequency from all samples by EM under Hardy-Weinberg and call every sample at "
                         "the maximum of likelihood x prior; FORMAT gains GQ, INFO gains EMAF and EMNC, DP / AD / PL stay as without it (extension)")
    ap.add_argument("--cohort-qual", action="store_true",
                    help="with --cohort: INFO gains SVQ, the site quality (-10 log10 of the posterior probability that no sample carries the alt "
                         "allele, from the exact allele-count posterior over all samples' likelihoods), and MLAC / MLAF at the posterior's maximum; "
                         "the QUAL column and everything else stay as without it; not with --joint-ins (extension)")
    ap.add_argument("--cohort-theta", metavar="<theta>", type=float,
                    help="with --cohort-qual: the prior of k alt copies in the cohort is theta / k, a value in (0, 0.05] (default: 0.001)")
    ap.add_argument("--cohort-qc", metavar="<prefix>",
                    help="with --cohort, beside any other cohort option: write <prefix>.samples.tsv (per sample: eligible, called, carrier, diploid, het and "
                         "hom-alt rows, call rate, het / hom-alt) and <prefix>.pairs.tsv (per pair of samples: the KING-robust kinship over the rows both "
                         "are diploid on, and DUP / 1ST / 2ND / 3RD / UN) from the run's calls; the VCF stays byte for byte what it is without it (extension)")
    ap.add_argument("--cohort-hwe", action="store_true",
                    help="with --cohort, beside any other cohort option: INFO gains DGC (hom-ref, het and hom-alt calls), HWE (the exact two-sided test "
                         "of Hardy-Weinberg equilibrium), EXCHET (the one-sided test for an excess of heterozygotes) and FIS, over the called diploid "
                         "samples of each row, from the calls the file prints; everything else stays as without it (extension)")
    args = ap.parse_args()
    if args.cohort is not None and args.aln is not None:
        ap.error("exactly one of -d and --cohort")
    if args.cohort is not None and (args.ploidy is not None or args.ploidy_file is not None):
        ap.error("--cohort is diploid, row by row: it cannot be combined with --ploidy or --ploidy-file "
                 "(per-sample ploidy in a cohort: --cohort-ploidy)")
    from svjg import genotype
    single = dict(ploidy=args.ploidy, ploidy_file=args.ploidy_file, joint_ins=args.joint_ins)
    cohort = dict(ploidy_file=args.cohort_ploidy, prior=args.cohort_prior, joint_ins=args.joint_ins, joint_prior=args.joint_prior, qual=args.cohort_qual,
                  theta=genotype.COHORT_QUAL_THETA if args.cohort_theta is None else args.cohort_theta, qc=args.cohort_qc, hwe=args.cohort_hwe)
    try:                                                         # the rules between the options themselves are the library's: one text each
        if args.cohort is None:
            for flag, given in (("--cohort-ploidy", args.cohort_ploidy is not None), ("--cohort-prior", args.cohort_prior)):
                if given:
                    ap.error(flag + " needs --cohort")
            genotype.check_single_options(**single)
            for flag, given in (("--joint-prior", args.joint_prior), ("--cohort-qual", args.cohort_qual), ("--cohort-hwe", args.cohort_hwe)):
                if given:
                    ap.error(flag + " needs --cohort")
            if args.cohort_qc is not None:
                ap.error(genotype.COHORT_QC_NEEDS)
        else:
            genotype.check_cohort_options(**cohort)
    except ValueError as e:
        ap.error(str(e))
    if args.cohort_theta is not None and not args.cohort_qual:
        ap.error("--cohort-theta needs --cohort-qual")
    out = "genotype_results.txt" if args.output is None else args.output[0]
    err = args.err[0] if args.err is not None else 0.00005
    if args.cohort is not None:
        genotype.run_cohort(args.cohort, args.vcf, out, args.minsupport, err, **cohort)
        return
    genotype.run(args.aln[0], args.vcf, out, args.minsupport, err, **single)


if __name__ == "__main__":
    main()
