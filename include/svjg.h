/* svjg.h — C ABI of libsvjg_hip.so: the MI355X (gfx950) implementation of SVJedi-graph's
 * alignment-classification + genotype-likelihood hot path.
 *
 * The reference (SandraLouise/SVJedi-graph) has no FFI for this path: its boundary is two Python
 * scripts run as shell commands (svjedi-graph.py:114-115, :124-125).  The drop-in scripts in
 * svjedi-graph_amd/ keep that command-line / file contract and call the entry points below through
 * ctypes (svjedi-graph_amd/svjg/capi.py).  Each entry point names the reference code it replaces.
 *
 * Conventions: every function returns 0 on success and a negative SVJG_E_* code on failure (message via
 * svjg_last_error).  The caller owns every host buffer it passes in or out; the library owns all device
 * memory.  Calls on one context must be serialised by the caller.  All structs are fixed-width
 * little-endian PODs.  No exceptions or aborts cross the boundary.  There is no CPU fallback: without a
 * GPU svjg_init fails with SVJG_E_NO_DEVICE.
 */
#ifndef SVJG_H
#define SVJG_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SVJG_ABI_VERSION 1

/* error codes (negative returns) */
#define SVJG_E_NO_DEVICE   (-1)   /* no usable HIP device */
#define SVJG_E_HIP         (-2)   /* a HIP runtime call failed */
#define SVJG_E_ARG         (-3)   /* bad argument / call order */
#define SVJG_E_NOMEM       (-4)
#define SVJG_E_RCCL        (-5)
#define SVJG_E_IO          (-6)   /* the GAF file could not be opened / read (svjg_gaf_upload_file) */
/* The input made the reference raise (it would exit 1, svjedi-graph.py:117-118).  svjg_input_error()
 * tells which Python exception and at which byte offset of the GAF. */
#define SVJG_E_INPUT       (-10)
#define SVJG_E_OVERFLOW    (-12)  /* 2^32 or more informative alignments for one SV (the count fields are 32 bits wide) */

/* exception class the reference would have died with (svjg_input_error) */
#define SVJG_EXC_NONE            0
#define SVJG_EXC_VALUE_ERROR     1   /* int()/float() of a column, too few columns (filter-alignments.py:185-194) */
#define SVJG_EXC_INDEX_ERROR     2   /* empty path column, unoriented multi-node path, node name without '-' */
#define SVJG_EXC_KEY_ERROR       3   /* alt node missing from the GFA (filter-alignments.py:346) */
#define SVJG_EXC_ZERO_DIVISION   4   /* Alen == 0 without an id:f: tag (filter-alignments.py:196) */
/* Not an exception: int() / float() / str.rstrip() of the reference also take non-ASCII digits and blanks (Unicode categories Nd,
 * Zs, ...), which the kernels do not read.  A line whose decimal column or id:f: value fails the ASCII rules AND holds a byte
 * >= 0x80 is neither counted nor an error: its offset goes to a list (svjg_get_host_lines) and the host decides with Python's
 * own int() / float() (svjedi-graph_amd/svjg/filter.py: resolve_host_lines), resubmitting an ASCII spelling of the line if the
 * reference accepts it. */
#define SVJG_EXC_ASK_HOST        5
/* -O / --dover given (SVJG_GRAPH_DOVER_LIST): argparse hands the reference a LIST, and the first comparison with it — the left
 * overlap of the first link that has a candidate SV, after the node lengths of that sum were looked up — dies with
 * TypeError (filter-alignments.py:52-57, :88, :153 -> :269). */
#define SVJG_EXC_TYPE_ERROR      6

typedef struct svjg_ctx svjg_ctx;

/* ---- graph tables (built on the host by svjedi-graph_amd/svjg/graph.py) ---------------------------
 * They replace d_link_sv (filter-alignments.py:95-98), alt_node_len (:103-113) and the node-name
 * arithmetic of get_node_start/end/len (:328-349).
 *
 * Nodes are sorted by `key` = chrom_idx << 48 | pos << 16 | kind << 15 | cnt
 *   reference node "chrom:start-end": pos = start, kind = 0, cnt = 0, aux = end
 *   alt node       "chrom:pos.cnt"  : pos = pos,   kind = 1, cnt = cnt, aux = sequence length
 *                                     (SVJG_LEN_UNKNOWN if the GFA has no S-line for it)
 * row   = first entry of this node's links in the edge array (rows are contiguous, node n's links are
 *         [row(n), row(n+1)); the node array carries one sentinel element at the end)
 * flags = SVJG_NODE_HAZARD if the node's name is a proper substring of another node name of the graph
 *         (the strand quirk of filter-alignments.py:206 can then depend on the other nodes of the path)
 */
#define SVJG_LEN_UNKNOWN 0xFFFFFFFFu
#define SVJG_NODE_HAZARD 1u

typedef struct {
    uint64_t key;
    uint32_t aux;
    uint32_t row;      /* bit 31 = SVJG_NODE_HAZARD, bits 0..30 = row */
} svjg_node;

/* One directed link query (left node = the row it sits in).  The host stores, for every key K of
 * *_svs_edges.json and its reversed form R (filter-alignments.py:221-225), the concatenation
 * d[K] ++ d[R] under K and d[R] ++ d[K] under R, so that ONE probe per path step returns exactly what
 * the reference collects with its two dictionary probes (:141-153), multiplicities included.
 *   meta bit 0 = strand of the left node  (1 = '-'), bit 1 = strand of the right node, bits 2.. = n_hits
 *   n_hits <= 2: h0, h1 are the hits;  n_hits > 2: h0 = first index into the hit array
 *   a hit is slot << 1 | allele
 */
typedef struct {
    uint32_t right;
    uint32_t meta;
    uint32_t h0;
    uint32_t h1;
} svjg_edge;

/* chromosome dictionary: names concatenated in `chrom_names`, chrom i = [chrom_off[i], chrom_off[i+1]);
 * chrom_node_lo[i] .. chrom_node_lo[i+1] is its node range. */
typedef struct {
    const svjg_node *nodes;        uint64_t n_nodes;       /* without the sentinel; nodes[n_nodes] is the sentinel */
    const svjg_edge *edges;        uint64_t n_edges;
    const uint32_t  *hits;         uint64_t n_hits;        /* overflow hit lists */
    const char      *chrom_names;  const uint32_t *chrom_off;  const uint32_t *chrom_node_lo;  uint32_t n_chrom;
    uint32_t         n_slots;      /* number of distinct sv_id keys = length of the count vector */
    uint32_t         d_over;       /* minimum breakpoint overlap, 100 (filter-alignments.py:56,88) */
    uint32_t         flags;        /* SVJG_GRAPH_* */
} svjg_graph;

#define SVJG_GRAPH_ALL_SLOW 1u     /* route every alignment through the exact string path (debug / odd names) */
/* The reference was given -O: d_over is a list there, and the first link with a candidate SV whose left-overlap sum can be formed
 * raises TypeError (SVJG_EXC_TYPE_ERROR).  Every line takes the exact path (the flag implies SVJG_GRAPH_ALL_SLOW); lines in front
 * of that link are classified — and may raise — as usual, and a file without such a link is written as the reference writes it. */
#define SVJG_GRAPH_DOVER_LIST 16u

/* One informative (alignment, SV) pair: what filter-alignments.py:163-166 appends, run-length encoded —
 * n_ref / n_alt = how many times the line is appended to the ref / alt list of that SV. */
typedef struct {
    uint64_t line_start;           /* byte offset of the line in the GAF given to svjg_classify */
    uint32_t slot;
    uint16_t n_ref;
    uint16_t n_alt;
} svjg_hitrec;

typedef struct {
    uint64_t n_lines;              /* GAF lines seen */
    uint64_t n_deferred;           /* lines that took the exact string path */
    uint64_t n_hitrecs;
    uint64_t non_ascii;            /* 1 if any byte >= 0x80 was seen (host must validate UTF-8 like the reference's text-mode read) */
} svjg_stats;

/* ---- lifecycle ---------------------------------------------------------------------------------- */
int  svjg_abi_version(void);
int  svjg_device_count(void);
int  svjg_init(int device, svjg_ctx **out);
void svjg_destroy(svjg_ctx *ctx);
const char *svjg_last_error(const svjg_ctx *ctx);          /* ctx may be NULL: error of the last failed svjg_init */

/* ---- graph (filter-alignments.py:95-113) ---------------------------------------------------------- */
int svjg_load_graph(svjg_ctx *ctx, const svjg_graph *g);
/* The lookup tables the kernels use are derived from `g` on the host (seconds for a graph of 500 k SVs) and kept for the next
 * svjg_load_graph of the same graph in this process (one context per GPU: they are built once); this drops the kept copy. */
void svjg_release_host_tables(void);

/* ---- alignments (filter-alignments.py:123-166) ----------------------------------------------------
 * svjg_gaf_upload copies a GAF byte buffer to HBM (the PCIe leg); svjg_classify_resident runs the kernels
 * over the resident buffer and ADDS to the per-SV counts; svjg_classify = upload + classify_resident.
 * `base_offset` is added to the line offsets reported in hit records / input errors (for chunked files).
 * Lines end at \n, \r\n or a lone \r and the last line may be unterminated, as in Python's text mode.
 * The _file forms take the bytes [offset, offset + n_bytes) of the file itself (the `for line in aln_file` of
 * filter-alignments.py:123-126 without a host copy of the text): feeder threads pread() pieces into pinned buffers
 * that go to HBM while the next pieces are read; svjg_classify_file uses `offset` as base_offset. */
int svjg_gaf_upload(svjg_ctx *ctx, const char *gaf, uint64_t n_bytes);
int svjg_gaf_upload_file(svjg_ctx *ctx, const char *path, uint64_t offset, uint64_t n_bytes);
/* The resident text in pieces (a text larger than the caller wants to hold on the host: the 21.6 GB of BASELINE configs[3] on one
 * GPU): piece [offset, offset + n_bytes) of a text of at most capacity_bytes; the call with offset 0 sizes the buffer, the one
 * with last != 0 ends the text at offset + n_bytes and makes it resident.  Pieces go in ascending order and may be cut anywhere
 * (the text as a whole ends at a line end or without a terminator, like a file: filter-alignments.py:123-126). */
int svjg_gaf_upload_part(svjg_ctx *ctx, const char *gaf, uint64_t n_bytes, uint64_t offset, uint64_t capacity_bytes, int last);
int svjg_classify_resident(svjg_ctx *ctx, uint64_t base_offset, int want_hits);
int svjg_classify(svjg_ctx *ctx, const char *gaf, uint64_t n_bytes, uint64_t base_offset, int want_hits);
int svjg_classify_file(svjg_ctx *ctx, const char *path, uint64_t offset, uint64_t n_bytes, int want_hits);
int svjg_reset_counts(svjg_ctx *ctx);
int svjg_get_stats(svjg_ctx *ctx, svjg_stats *out);
int svjg_input_error(svjg_ctx *ctx, int *exc_class, uint64_t *line_offset);
/* Why lines took the exact string path since the last svjg_reset_counts (their sum is svjg_stats.n_deferred):
 * out[0] columns that are not twelve plain ones (blanks, signs, too few, Alen = 0, ...), [1] a 64-byte span of the line holds the
 * byte pair "d:" and the line is not decided in the main kernel (an id:f: tag, filter-alignments.py:193-196, whose value is not a
 * plain decimal, or several pairs in the line's spans), [2] a path of 4 Gbp and more (the main kernel's path sums are 32 bits wide; paths of
 * up to 216 nodes — more marks than that and the line's stripe cannot list it: [4] — stay in the main kernel), [3] a node name
 * the kernel's name table does not hold (not in the graph, a substring of another name, longer than 48 bytes, alt node without a
 * length), [4] whole stripes of 8 KB (more than 64 lines or 216 orientation marks, a line whose columns and path run beyond 8 KB or whose tail beyond them is not plain, SVJG_GRAPH_ALL_SLOW / _DOVER_LIST),
 * [5..7] reserved (0). */
int svjg_get_defer_causes(svjg_ctx *ctx, uint64_t *out8);

/* counts: out[slot*2 + 0] = ref, out[slot*2 + 1] = alt  (= len() of the two lists of
 * dict_of_informative_aln[sv_id], filter-alignments.py:163-166) */
int svjg_get_counts(svjg_ctx *ctx, uint32_t *out, uint32_t n_slots);
int svjg_set_counts(svjg_ctx *ctx, const uint32_t *in, uint32_t n_slots);   /* predict-genotype.py run stand-alone from a JSON */
/* size the count vector without a graph (stand-alone predict-genotype.py: counts come from the JSON) */
int svjg_alloc_counts(svjg_ctx *ctx, uint32_t n_slots);
/* hit records accumulated since the last svjg_reset_counts, unordered; copy at most `cap` */
int svjg_get_hits(svjg_ctx *ctx, svjg_hitrec *out, uint64_t cap, uint64_t *n);
/* byte offsets (base_offset included) of the lines set aside for the host since the last svjg_reset_counts (SVJG_EXC_ASK_HOST),
 * unordered; copy at most `cap`, *n = how many there are */
int svjg_get_host_lines(svjg_ctx *ctx, uint64_t *out, uint64_t cap, uint64_t *n);

/* ---- multi-GPU: one process per GPU, one all-reduce of the count vector over RCCL/xGMI ------------- */
int svjg_comm_unique_id(char *out128);                                      /* rank 0, then broadcast by the launcher */
int svjg_comm_init(svjg_ctx *ctx, const char *id128, int n_ranks, int rank);
int svjg_allreduce_counts(svjg_ctx *ctx);
/* ---- multi-GPU, one process (what the drop-in filter-alignments.py does with the GPUs it sees): one context per device,
 * communicators from ncclCommInitAll, the same all-reduce issued for every context; n == 1 is allowed (no collective).
 * Both all-reduce forms fail with SVJG_E_OVERFLOW when a per-SV count cannot be represented (>= 2^32). */
int svjg_comm_init_all(svjg_ctx *const *ctxs, int n);
/* What went wrong in the last failed svjg_comm_init_all (NUL terminated, at most cap bytes).  That call may run in a thread of its own beside
 * other calls on the same contexts, so it never writes a context's svjg_last_error. */
int svjg_comm_error(char *out, uint64_t cap);
/* Where the fused pass (svjg_run_begin) enqueues its all-reduce: 0 (default) on the compute stream, between this pass's kernels and
 * the next pass's; 1 on the second stream, in front of the pass's genotype kernel (bench.py measures both on a multi-GPU box). */
int svjg_comm_set_stream(svjg_ctx *ctx, int second_stream);
int svjg_allreduce_counts_all(svjg_ctx *const *ctxs, int n);

/* ---- genotypes (predict-genotype.py:216-227 gate, :281-325 likelihood) -----------------------------
 * Per VCF row r: sv_type[r] in {0 DEL, 1 INS, 2 INV, 3 BND}; slot[r] = count slot or 0xFFFFFFFF when the
 * row's sv_id is not a key of the edge table; ok[r] bit 0 = the reference's type/length gate (:216) passed,
 * bit 1 = a valid slot alone proves the sv_id is a key of the informative dict (counts loaded from a JSON).
 * Outputs: gt[r] in {0 "0/0", 1 "0/1", 2 "1/1", 3 "./."}, pl[r*3..] = the three PL integers,
 * raw[r*2..] = raw (ref, alt) counts, genotyped[r] = 1 if the row went through likelihood()
 * (i.e. counted by "Genotyped svs", :229).  Rows with genotyped = 0 print "./.:0:0,0:.,.,." (:237-239). */
int svjg_genotype(svjg_ctx *ctx, const uint8_t *sv_type, const uint32_t *slot, const uint8_t *ok,
                  uint64_t n_rows, uint32_t min_support, double err,
                  uint8_t *gt, int64_t *pl, uint32_t *raw, uint8_t *genotyped);
/* PL boundary guard.  The reference adds Decimal(math.log10(math.comb(rc1 + rc2, rc1))) to the three likelihoods
 * (predict-genotype.py:313): libm's log10 of an exact big integer, a double that need not be the correctly rounded logarithm the
 * kernel works with (double-double table of log10(i!)).  The two agree on every known answer, but a difference in the last
 * places, times ten, right next to an integer would turn a PL by one: out[r] = 1 for the rows of the last svjg_genotype /
 * svjg_genotype_view call in which one of the three -10 * (lik + comb) lies within 1e-6 of an integer.  The caller recomputes
 * those rows (a few per million) with the reference's own arithmetic: svjedi-graph_amd/svjg/genotype.py: exact_pl. */
int svjg_genotype_boundary(svjg_ctx *ctx, uint8_t *out, uint64_t n_rows);
/* The same without the copy into caller buffers: the four pointers look into the context's pinned host block (where the
 * device wrote the results) and stay valid until the next svjg_genotype / svjg_genotype_view / svjg_destroy on `ctx`. */
int svjg_genotype_view(svjg_ctx *ctx, const uint8_t *sv_type, const uint32_t *slot, const uint8_t *ok,
                       uint64_t n_rows, uint32_t min_support, double err,
                       const uint8_t **gt, const int64_t **pl, const uint32_t **raw, const uint8_t **genotyped);
/* The table the binomial term of every genotype call comes from: log10(i!) in double-double, entry i = (hi, lo), built on the device
 * with the device's log10 (k_logfact_*), 65 536 entries at a context's first genotype call, rebuilt larger inside a call that meets
 * n = r1 + r2 beyond it, never more than 2^24 entries (256 MB).
 *   svjg_logfact_reserve  afterwards the table holds at least `entries` (capped at 2^24, rounded up to a multiple of 1024).  It never
 *                         shrinks the table and does nothing when it is large enough already.  Before a rebuild the context's streams
 *                         drain: a pass in flight still reads the old table.  Called once behind svjg_init it takes the build (and a
 *                         later growth) out of the first genotype call, e.g. one that is timed.
 *   svjg_logfact_read     out[k*2], out[k*2+1] = hi, lo of entry first + k, k < n, copied synchronously; *entries (may be NULL) = the
 *                         table's size, 0 while none has been built.  n = 0 with out = NULL asks for the size alone.  SVJG_E_ARG with a
 *                         message in svjg_last_error: first + n beyond the size, out = NULL with n > 0.
 * Read-only access for tests and diagnostics (tests/test_logfact_gpu.py pins every entry): nothing in the product reads the table back. */
int svjg_logfact_reserve(svjg_ctx *ctx, uint32_t entries);
int svjg_logfact_read(svjg_ctx *ctx, uint32_t first, uint32_t n, double *out, uint32_t *entries);

/* Any ploidy from 1 to SVJG_MAX_PLOIDY, row by row: ploidy[r] in 0..SVJG_MAX_PLOIDY beside the three inputs of svjg_genotype.  A row of
 * ploidy P has P + 1 genotypes, g = 0..P alt copies; a read shows the alt allele with probability (g (1 - e) + (P - g) e) / P, which at
 * P = 2 is the reference's likelihood() term for term.  Outputs: gt[r] = alt copies of the call (0xFF = no call), pl[r*9..] = PL_0..PL_P in
 * that order (entries beyond a row's ploidy = 0), raw and genotyped as svjg_genotype; boundary[r] = 1 where one of the P + 1 values lies within
 * 1e-6 of an integer (what svjg_genotype_boundary reports for svjg_genotype; this call neither reads nor changes that state, nor the views of
 * svjg_genotype_view): recompute such rows with svjedi-graph_amd/svjg/genotype.py: exact_pl_ploidy.  A row with ploidy 0 is never genotyped
 * (genotyped = 0, raw = 0,0).  SVJG_E_ARG: a ploidy above SVJG_MAX_PLOIDY (found before any launch), a null array, no counts yet, a slot out
 * of range. */
#define SVJG_MAX_PLOIDY 8
int svjg_genotype_ploidy(svjg_ctx *ctx, const uint8_t *sv_type, const uint32_t *slot, const uint8_t *ok, const uint8_t *ploidy,
                         uint64_t n_rows, uint32_t min_support, double err,
                         uint8_t *gt, int64_t *pl, uint32_t *raw, uint8_t *genotyped, uint8_t *boundary);

/* Insertions that share a CHROM and POS, genotyped together (diploid; --joint-ins).  A site has K = 2..SVJG_MAX_SITE_ALTS members; slots holds
 * SVJG_MAX_SITE_ALTS count slots per site, the members first, 0xFFFFFFFF behind them.  Allele 0 is the reference, allele j the j-th member;
 * c_0 = the largest raw ref count of the members, c_j = alt_j / 2, N their sum.  The genotypes {a, b}, 0 <= a <= b <= K, in VCF order
 * b (b + 1) / 2 + a: a read shows an allele with probability q(.|a) / 2 + q(.|b) / 2, q = 1 - e for the haplotype's own allele and e / K for each
 * other one, i.e. lik = c_a log10(1 - e) + (N - c_a) log10(e / K) for a = b and (c_a + c_b) log10(((1 - e) + e / K) / 2) + (N - c_a - c_b) log10(e / K)
 * for a < b; the coefficient term is the chain of binomial terms log10 comb(s_j, r_j) over the rounded counts, s_j = r_0 + .. + r_j.  At K = 1
 * this is the reference's likelihood().  Outputs per site: gt[2] = the pair (a, b) that alone attains the maximum, 0xFF, 0xFF on a tie or when
 * N is below min_support; pl[SVJG_SITE_GENOTYPES] = the PLs in that order, 0 beyond the site's (K + 1)(K + 2) / 2; raw[7] = the ref maximum and
 * alt_1..alt_6; boundary = 1 where one of the values lies within 2.5e-6 of an integer or s_K >= 2^24: recompute such sites with
 * svjedi-graph_amd/svjg/genotype.py: exact_pl_site.  The call neither reads nor changes what svjg_genotype_view and svjg_genotype_boundary hand
 * out.  n_sites = 0 returns 0.  SVJG_E_ARG, all found before any launch: a site with fewer than two members, a hole in front of a member, a slot
 * out of range, a slot twice in one site, a null array, no counts yet.  svjg_last_kernel_ms reports the kernel's time as genotype_ms; no timing
 * of this kernel has been measured beyond the first reading recorded with the change that added it. */
#define SVJG_MAX_SITE_ALTS 6
#define SVJG_SITE_GENOTYPES 28
int svjg_genotype_sites(svjg_ctx *ctx, const uint32_t *slots, uint64_t n_sites, uint32_t min_support, double err,
                        uint8_t *gt, int64_t *pl, uint32_t *raw, uint8_t *boundary);

/* ---- cohort: many samples' counts, one row set, one multi-sample call (--cohort) -----------------------------------------
 * A count matrix of n_samples x n_slots lives in the context, slot-major: cm[slot * n_samples + s], packed ref | alt << 32 like the count
 * vector, with a presence byte beside each entry.  Slot-major because the genotype kernel's neighbouring lanes are neighbouring samples of one
 * row: they read the counts and write their results coalesced.  The presence byte says that the slot's sv_id is a key of THAT sample's JSON
 * (predict-genotype.py:216): a key with two empty lists is genotyped, an absent key is not.
 *   svjg_cohort_alloc        a zeroed matrix (counts and presence); a second call replaces it.  SVJG_E_ARG: n_samples = 0; SVJG_E_NOMEM: the
 *                            n_samples x n_slots x 9 bytes cannot be had.
 *   svjg_cohort_set_counts   sparse: the n slots the sample has as keys, counts[k*2..] = (ref, alt) of slots[k]; their presence is set, every
 *                            other slot of the sample is cleared and absent.  SVJG_E_ARG, found before any launch: no matrix, sample or slot
 *                            out of range, a slot named twice, null arrays with n > 0.
 *   svjg_cohort_store_counts the context's current count vector (what the classify kernels have just accumulated) -> column `sample`, device
 *                            to device by a small transposing kernel; presence = (ref | alt) != 0, the rule of svjg_genotype's gate when ok
 *                            bit 1 is clear.  Classify S GAFs in a loop on one graph and genotype them without any JSON.  SVJG_E_ARG: no
 *                            matrix, sample out of range, the count vector's length is not the matrix's n_slots.
 *   svjg_cohort_get_counts   one sample back (out[slot*2..] as svjg_get_counts, present[slot]); n_slots must be the matrix's.
 *
 * svjg_genotype_cohort: per item (r, s) what svjg_genotype does per row, gate included, with the presence test in place of the count test: the
 * item is genotyped iff ok[r] & 1, slot[r] != 0xFFFFFFFF and present[slot[r]][s].  ok bit 1 is IGNORED here (the presence byte says it per
 * sample).  An item that is not genotyped has gt = 3, zero PLs, raw = 0,0.  Outputs, [n_rows][n_samples] row-major: gt, pl (3 x int64), raw
 * (2 x uint32), genotyped, boundary (as svjg_genotype_boundary: recompute such items with svjedi-graph_amd/svjg/genotype.py: exact_pl); and
 * site[r*2..] = NS (the samples with gt != 3) and AC (the sum of their alt copies) of row r, summed in integers in the same launch (wave
 * ballots, one 64-bit atomic per row and wave), so they are equal from run to run; AN = 2 NS.  The call works in a block of its own: it
 * neither reads nor changes what svjg_genotype_view and svjg_genotype_boundary hand out, nor the count vector.  The caller bounds memory by
 * calling with row chunks (37 bytes per item on the device and on the host).  n_rows = 0 returns 0.  SVJG_E_ARG: no matrix, a null array; a
 * row naming a slot >= the matrix's n_slots is reported after the pass, as svjg_genotype reports it.  svjg_last_kernel_ms reports the kernel
 * as genotype_ms.  Measured once, with the change that added it (one MI355X, 100 000 rows x 64 samples, counts 0..60, e = 5e-5, median of 30
 * calls behind 5, alternated twice with the loop in one process): 0.165 / 0.165 ms for the one launch, against 0.956 / 0.951 ms of kernels summed
 * and 21.4 / 21.4 ms of wall time for 64 x (svjg_set_counts + svjg_genotype); nothing else about this kernel has been measured. */
int svjg_cohort_alloc(svjg_ctx *ctx, uint32_t n_samples, uint32_t n_slots);
int svjg_cohort_set_counts(svjg_ctx *ctx, uint32_t sample, const uint32_t *slots, const uint32_t *counts, uint64_t n);
int svjg_cohort_store_counts(svjg_ctx *ctx, uint32_t sample);
int svjg_cohort_get_counts(svjg_ctx *ctx, uint32_t sample, uint32_t *out, uint8_t *present, uint32_t n_slots);
int svjg_genotype_cohort(svjg_ctx *ctx, const uint8_t *sv_type, const uint32_t *slot, const uint8_t *ok,
                         uint64_t n_rows, uint32_t min_support, double err,
                         uint8_t *gt, int64_t *pl, uint32_t *raw, uint8_t *genotyped, uint8_t *boundary, uint32_t *site);

/* svjg_genotype_cohort_ploidy: the cohort call at a ploidy per (row, sample) item (--cohort-ploidy): ploidy[r*n_samples + s] in 0..max_ploidy,
 * max_ploidy in 1..SVJG_MAX_PLOIDY.  Per item what svjg_genotype_ploidy does per row, with svjg_genotype_cohort's gate plus the ploidy byte: the
 * item is genotyped iff ok[r] & 1, slot[r] != 0xFFFFFFFF, present[slot[r]][s] and 1 <= ploidy <= max_ploidy (ok bit 1 is IGNORED; ploidy 0: never
 * genotyped).  An item that is not genotyped has gt = 0xFF, zero PLs, raw = 0,0, boundary = 0.  Outputs, [n_rows][n_samples] row-major: gt = alt
 * copies of the call (0xFF = no call); pl = max_ploidy + 1 int64 per item, PL_0..PL_P then zeros — the stride is the CALL's, so a human cohort
 * (max_ploidy 2) moves 24 bytes of PLs per item like the diploid call, not 72 —; raw, genotyped as svjg_genotype_cohort; boundary as
 * svjg_genotype_ploidy's: recompute flagged items with svjedi-graph_amd/svjg/genotype.py: exact_pl_ploidy.  site[r*3..] = NS (the items with
 * gt != 0xFF), AN (the sum of their ploidies) and AC (the sum of their alt copies) of row r, summed in integers in the same launch (nine wave ballots,
 * at most two 64-bit atomics per row and wave), so they are equal from run to run.  The call works in a block of its own: it neither reads nor
 * changes the count vector, what svjg_genotype_view and svjg_genotype_boundary hand out, or the block of svjg_genotype_cohort.  The caller bounds
 * memory by calling with row chunks (8 (max_ploidy + 1) + 12 bytes per item).  n_rows = 0 returns 0.  SVJG_E_ARG with a message in
 * svjg_last_error, all found before any launch: no matrix, a null array, max_ploidy outside 1..SVJG_MAX_PLOIDY, a ploidy byte above max_ploidy,
 * n_rows x n_samples beyond 2^40, a matrix of 2^28 samples or more (AN must fit 32 bits); a row naming a slot >= the matrix's n_slots is reported
 * after the pass, as svjg_genotype reports it.  svjg_last_kernel_ms reports the kernel as genotype_ms.
 * Measured once, with the change that added it (one MI355X, 2026-10-19, tools/cohort_ploidy_timing.py: 100 000 rows x 64 samples, counts 0..60,
 * e = 5e-5, median of 30 calls behind 5, the legs alternated twice in one process): 0.191 / 0.191 ms for the one launch with ploidies 0 / 1 / 2 by
 * row class and sex at max_ploidy 2, 0.451 / 0.452 ms with ploidies 1..8 at max_ploidy 8; svjg_genotype_cohort on the same matrix 0.166 / 0.165 ms;
 * the loop 64 x (svjg_set_counts + svjg_genotype_ploidy) with the same ploidies 1.267 / 1.266 ms and 1.563 / 1.572 ms of kernels summed, 118 / 120 ms
 * and 134 / 135 ms of wall time.  One call from Python took 35.5 / 37.0 ms (226 MB to the host) and 77.2 / 78.3 ms (533 MB).  Nothing else about
 * this kernel has been measured. */
int svjg_genotype_cohort_ploidy(svjg_ctx *ctx, const uint8_t *sv_type, const uint32_t *slot, const uint8_t *ok,
                                const uint8_t *ploidy /* [n_rows][n_samples] */, uint32_t max_ploidy, uint64_t n_rows,
                                uint32_t min_support, double err,
                                uint8_t *gt, int64_t *pl /* [n_rows][n_samples][max_ploidy+1] */, uint32_t *raw,
                                uint8_t *genotyped, uint8_t *boundary, uint32_t *site /* [n_rows][3] = NS, AN, AC */);

/* svjg_genotype_cohort_prior: the cohort call with an allele-frequency prior (--cohort-prior).  The arguments of svjg_genotype_cohort_ploidy,
 * with `ploidy` nullable: NULL = every item diploid, max_ploidy must be 2, and the first launch is svjg_genotype_cohort's kernel.  pl, raw,
 * genotyped and boundary are exactly what svjg_genotype_cohort / svjg_genotype_cohort_ploidy return on the same inputs (pl: max_ploidy + 1 per
 * item).  Behind that kernel, on the same stream, a second one estimates every row's alt-allele frequency f from all its samples' likelihoods by
 * EM under Hardy-Weinberg and calls each item at the maximum of likelihood x prior (the model: DESIGN.md 4.3, svjg_geno.h):
 *   gt        [n_rows][n_samples]  alt copies of the POSTERIOR call, 0xFF = no call (in both modes: never 3 for "no call")
 *   gq        [n_rows][n_samples]  min(99, int(-10 log10(1 - q_best))), 0xFF where gt is 0xFF
 *   af        [n_rows]             the row's f; NaN: no item took part (genotyped and with a read), no estimate
 *   em_steps  [n_rows]             EM steps taken (0..128) in the low bits; bit 31 set: 128 steps without |f' - f| <= 1e-9 ("not converged")
 *   site      [n_rows][3]          NS, AN, AC of the posterior calls, summed in integers
 * No atomics take part in the second kernel (a row lies within one wave; its sums go through a fixed butterfly): equal bytes from run to run.
 * The call works in a block of its own (8 (max_ploidy + 1) + 13 bytes per item, 46 per row).  n_rows = 0 returns 0.  SVJG_E_ARG with a
 * message, all found before any launch: as svjg_genotype_cohort_ploidy, and ploidy == NULL with max_ploidy != 2.  svjg_last_kernel_ms reports
 * both kernels together as genotype_ms.
 * The items of a lane beyond its first (more than 64 samples) keep their weights in LDS across the EM steps, up to 256 samples; beyond, they are
 * recomputed at every step.  SVJG_PRIOR_STAGE=recompute / lds in the environment forces one way (for tools/cohort_prior_timing.py).
 * Measured once, with the change that added it (one MI355X, 2026-10-19, ROCm 7.2.0, tools/cohort_prior_timing.py: 100 000 rows, counts 0..60,
 * e = 5e-5, median of 30 calls behind 5, the legs alternated twice in one process; genotype_ms, both kernels): 64 samples 0.730 / 0.730 ms against
 * 0.159 / 0.160 ms of svjg_genotype_cohort alone (+0.571 / +0.570 ms; 4.79 EM steps a row, 7 at the most); 64 samples with ploidies 1..8 at
 * max_ploidy 8 1.419 / 1.419 ms against 0.456 / 0.456 ms of svjg_genotype_cohort_ploidy (+0.963 / +0.963 ms; 8.82 steps, at most 12); 4 samples
 * 0.084 / 0.084 ms against 0.029 / 0.029 ms (+0.055 ms; 2.64 steps, at most 18); 256 samples 2.549 / 2.549 ms against 0.597 / 0.597 ms (+1.952 ms;
 * 4.90 steps, at most 6), and 3.685 / 3.692 ms with the further items recomputed instead of staged in LDS.  A call from Python took 32.6 / 29.7 ms at
 * 64 samples (30.5 / 30.8 ms without the prior): the copies to the host dominate either way.  Nothing else about this kernel has been measured. */
int svjg_genotype_cohort_prior(svjg_ctx *ctx, const uint8_t *sv_type, const uint32_t *slot, const uint8_t *ok,
                               const uint8_t *ploidy /* [n_rows][n_samples], or NULL */, uint32_t max_ploidy, uint64_t n_rows,
                               uint32_t min_support, double err,
                               uint8_t *gt, int64_t *pl /* [n_rows][n_samples][max_ploidy+1] */, uint32_t *raw,
                               uint8_t *genotyped, uint8_t *boundary, uint32_t *site /* [n_rows][3] = NS, AN, AC */,
                               uint8_t *gq, double *af, uint32_t *em_steps);

/* svjg_genotype_cohort_sites: svjg_genotype_sites for every sample of the cohort matrix in one launch (--cohort --joint-ins; diploid).  slots holds
 * SVJG_MAX_SITE_ALTS CANDIDATE slots of the matrix per site (the rows of the merged catalogue at one CHROM and POS), the candidates first, 0xFFFFFFFF
 * behind them, checked as svjg_genotype_sites checks its members (2..6, no hole, each below the matrix's n_slots, none twice).  An item is (site k,
 * sample s): sample s's site consists of the candidates whose presence byte is set for s, in candidate order, numbered 1..K' — the members
 * svjg_genotype_sites would be given in a single-sample run of s — with c_0 = the largest raw ref count over THOSE members.  Outputs,
 * [n_sites][n_samples] row-major: gt[2], pl[SVJG_SITE_GENOTYPES], raw[7] and boundary exactly what svjg_genotype_sites returns for the item's members
 * (recompute flagged items with svjedi-graph_amd/svjg/genotype.py: exact_pl_site on the item's own K' alt counts); members = a byte whose bit j says
 * that candidate j took part.  An item with K' < 2 has no site call: gt = 0xFF, 0xFF, zero PLs, raw = 0, boundary = 0, and members still names the
 * candidate that was present, if any.  site[k*12 + j*2..] = NS_j, AC_j of candidate j of site k: the items with a site call of which j is a member, and
 * the copies of j's allele in those calls, summed in integers in the same launch (three wave ballots a candidate, one 64-bit atomic per candidate,
 * site and wave), so they are equal from run to run.  The call reads the cohort matrix and not the count vector, and works in a block of its own: it
 * neither reads nor changes the other calls' blocks, what svjg_genotype_view and svjg_genotype_boundary hand out, or the count vector.  The caller
 * bounds memory by calling with site chunks (256 bytes per item, 72 per site, on the device and on the host).  n_sites = 0 returns 0.  SVJG_E_ARG with
 * a message in svjg_last_error, all found before any launch: no matrix, a null array, a malformed site, n_sites x n_samples beyond 2^40.
 * svjg_last_kernel_ms reports the kernel as genotype_ms.
 * Measured once, with the change that added it (one MI355X, 2026-10-20, ROCm 7.2.0, tools/cohort_sites_timing.py: 10 000 sites x 64 samples, K mixed
 * 2..6, presence 0.9, counts 0..60, e = 5e-5, median of 30 calls behind 5, the legs alternated twice in one process): 0.129 / 0.129 ms for the one
 * launch, against 1.910 / 1.919 ms of kernels summed and 20.0 / 20.7 ms of wall time for the loop 64 x (svjg_set_counts + svjg_genotype_sites) on the
 * same columns; one call from Python took 18.6 / 18.6 ms (164 MB to the host).  Nothing else about this kernel has been measured. */
int svjg_genotype_cohort_sites(svjg_ctx *ctx, const uint32_t *slots /* [n_sites][SVJG_MAX_SITE_ALTS] */, uint64_t n_sites, uint32_t min_support, double err,
                               uint8_t *gt /* [n_sites][n_samples][2] */, int64_t *pl /* [n_sites][n_samples][SVJG_SITE_GENOTYPES] */,
                               uint32_t *raw /* [n_sites][n_samples][7] */, uint8_t *members, uint8_t *boundary,
                               uint32_t *site /* [n_sites][SVJG_MAX_SITE_ALTS][2] = NS_j, AC_j */);

/* svjg_genotype_cohort_sites_prior: svjg_genotype_cohort_sites, and behind it in the same call the samples of a SITE inform each other
 * (--cohort --joint-ins --joint-prior): the frequencies p_0..p_C of the site's alleles (0 the reference, j candidate j) are estimated by EM under
 * Hardy-Weinberg over the items that have a site (K' >= 2) and a read, from p_j = 1 / (C + 1), until max_j |p_j' - p_j| <= 1e-9 or 128 steps; each
 * item is then called at the maximum of likelihood x prior over the genotypes on the reference and ITS OWN members (the model, the fixed-point
 * caveat for samples with a subset of the candidates, and how the kernel divides the work: svjg_geno.h).  gt, pl, raw, members,
 * boundary and site are bit for bit what svjg_genotype_cohort_sites returns.  Added: sgt[2] = the posterior call in the item's member numbering (gt's
 * convention), 0xFF, 0xFF: no call (a tie, below min_support, no site or no read); sgq = min(99, int(-10 log10(sum of the other posteriors))), 0xFF
 * beside a no-call; af[k*7 + j] = p_j (0 beyond C; all NaN where no item took part); em_steps[k]: the steps taken, bit 31 set: not converged;
 * psite[k*12 + j*2..] = NS_j, AC_j of the posterior calls.  No atomics: equal bytes from run to run.  A block of its own: it neither reads nor
 * changes another call's block or views.  Checks and errors as svjg_genotype_cohort_sites (the added arrays must not be null), all before any
 * launch; 259 bytes per item and 180 per site.  svjg_last_kernel_ms reports both kernels together as genotype_ms.
 * Measured once, with the change that added it (one MI355X, 2026-10-21, ROCm 7.2.0, tools/cohort_sites_prior_timing.py: 10 000 sites, K mixed 2..6,
 * presence 0.9, counts 0..60, e = 5e-5, median of 30 calls behind 5, the legs alternated twice in one process): 0.614 / 0.615 ms for both kernels at 64
 * samples against 0.129 / 0.128 ms of svjg_genotype_cohort_sites alone (6.49 steps a site, at most 13), 2.560 / 2.559 against 0.540 / 0.540 ms at 256
 * (6.06 steps, at most 9).  Nothing else about this kernel has been measured. */
int svjg_genotype_cohort_sites_prior(svjg_ctx *ctx, const uint32_t *slots /* [n_sites][SVJG_MAX_SITE_ALTS] */, uint64_t n_sites, uint32_t min_support,
                                     double err, uint8_t *gt, int64_t *pl, uint32_t *raw, uint8_t *members, uint8_t *boundary, uint32_t *site,
                                     uint8_t *sgt /* [n_sites][n_samples][2] */, uint8_t *sgq /* [n_sites][n_samples] */, double *af /* [n_sites][7] */,
                                     uint32_t *em_steps /* [n_sites] */, uint32_t *psite /* [n_sites][SVJG_MAX_SITE_ALTS][2] */);

/* svjg_cohort_qual: the site quality of every row of a cohort (--cohort-qual): how sure are we that at least one alt copy exists in the cohort.
 *   The exact allele-count posterior (the "exact model" of Li 2011): the samples' genotype likelihoods folded in one by one into y_k, the
 *   likelihood of k alt copies among the M chromosomes folded in so far, in its normalised form, rescaled by exact powers of two;
 *   prior phi_k = theta / k (k >= 1), phi_0 = 1 - theta H_M; qual = -10 log10 of the posterior of k = 0, mlac = the k at the posterior's maximum.
 *   The model in full: DESIGN.md 4.3 "Site quality (k_cohort_qual)" and svjg_geno.h.
 * It reads the cohort matrix, not the count vector.  Item (r, s) takes part iff ok[r] & 1, slot[r] != 0xFFFFFFFF, present[slot[r]][s], its ploidy
 * is in 1..max_ploidy (ploidy == NULL: 2 everywhere, max_ploidy must be 2) and it has a read.  There is no min_support: support gates calls, not
 * likelihoods, as in the EM of svjg_genotype_cohort_prior.  Outputs per row: chroms = M, the chromosomes of the items that took part; mlac in
 * 0..M; qual >= 0, NaN (and mlac = 0, chroms = 0) where no item took part.  No atomic takes part in an output (a row lies within one wave, every
 * sum over k goes through a fixed butterfly): equal bytes from run to run.  The call works in a block of its own (16 bytes a row, the ploidy
 * bytes, 8 (M_max + 1) + 720 bytes of tables): it neither reads nor changes any other call's block or views.  n_rows = 0 returns 0.  SVJG_E_ARG
 * with a message in svjg_last_error, all found before any launch: no matrix, a null array, max_ploidy outside 1..SVJG_MAX_PLOIDY, ploidy == NULL with
 * max_ploidy != 2, a ploidy byte above max_ploidy, n_samples x max_ploidy above SVJG_QUAL_MAX_CHROMS (the row's 2 (M_max + 1) doubles live in one
 * block's LDS: 65.6 KB at 2 048 diploid samples), theta not in (0, 0.05] (0.05 H_4096 < 1: phi_0 > 0), n_rows x n_samples beyond 2^40; a row
 * naming a slot >= the matrix's n_slots is reported after the pass, as svjg_genotype reports it.  svjg_last_kernel_ms reports the kernel as
 * genotype_ms.
 * Measured once, with the change that added it (one MI355X, 2026-10-20, ROCm 7.2.0, tools/cohort_qual_timing.py: counts 0..60, e = 5e-5, theta = 1e-3,
 * median of 30 calls behind 5, run twice in one process; genotype_ms): 100 000 rows x 64 samples diploid 8.565 / 8.550 ms; the same matrix with
 * ploidies 1..8 at max_ploidy 8 15.065 / 15.033 ms; 2 000 rows x 1 024 samples diploid 20.509 / 20.511 ms.  A first reading: nothing is compared
 * against it, and nothing else has been measured. */
#define SVJG_QUAL_MAX_CHROMS 4096
int svjg_cohort_qual(svjg_ctx *ctx, const uint8_t *sv_type, const uint32_t *slot, const uint8_t *ok,
                     const uint8_t *ploidy /* [n_rows][n_samples], or NULL */, uint32_t max_ploidy, uint64_t n_rows, double err, double theta,
                     double *qual, uint32_t *mlac, uint32_t *chroms);

/* svjg_cohort_qc: the samples of a cohort, from the calls a cohort run has made (--cohort-qc): six sums per sample and five per pair of samples,
 * the counts of the KING-robust kinship estimator (Manichaikul et al. 2010).  Integers only.  gt[n_rows][n_samples] = the calls, ploidy the same
 * shape or NULL (2 everywhere); with g the call and P the ploidy of an item: eligible P >= 1; called: eligible and g <= P (both no-call codes of
 * the library, 3 and 0xFF, are "g > P"); carrier: called and g >= 1; dip: called and P = 2; het: dip and g = 1; homalt: dip and g = 2; homref: dip
 * and g = 0.  Outputs, uint32 sums over the rows:
 *   sample [n_samples][6]                     eligible, called, carrier, dip, het, homalt
 *   pair   [n_samples (n_samples - 1) / 2][5] for i < j at k = i n_samples - i (i + 1) / 2 + (j - i - 1): both = sum dip_i dip_j, het1 = sum het_i dip_j,
 *                                             het2 = sum dip_i het_j, hethet = sum het_i het_j, ibs0 = sum (homref_i homalt_j + homalt_i homref_j)
 * Only diploid items enter a pair.  The kinship is the host's: with m = min(het1, het2), phi = 0.5 - (4 ibs0 + (het1 - hethet) + (het2 - hethet)) / (4 m),
 * no estimate where m = 0 (svjedi-graph_amd/svjg/genotype.py: kinship).  A first kernel turns the bytes into bit planes of 64 rows a word and sums
 * the samples' counts (integer atomics), a second one takes the pairs tile by tile with ANDs and popcounts and writes every pair once: no float,
 * equal bytes from run to run, and sums over row chunks add up to the sums of one call.  The call neither needs nor reads the cohort matrix, the
 * count vector or the log10(i!) table's values, and works in a block of its own: it neither reads nor changes any other call's block or views.
 * The caller bounds memory by calling with row chunks: 1 byte per item (2 with a ploidy array) on the device and the host, 3 bits per item of
 * planes on the device, 20 bytes per pair and 24 per sample.  n_rows = 0 returns 0 with zeroed outputs; n_samples = 1 is valid and writes no pair
 * (pair may be NULL).  SVJG_E_ARG with a message in svjg_last_error, all found before any launch: a null gt or sample, a null pair with
 * n_samples >= 2, n_samples = 0 or above SVJG_QC_MAX_SAMPLES (the pair array is then at most 42 MB; the sample count svjg_cohort_qual admits for
 * diploids), n_rows x n_samples beyond 2^40, n_rows >= 2^32 (a sum must fit 32 bits).  svjg_last_kernel_ms reports both kernels together as
 * genotype_ms.
 * Measured once, with the change that added it (one MI355X, 2026-10-21, ROCm 7.2.0, tools/cohort_qc_timing.py: 10 000 rows, calls 0 / 1 / 2 / none at
 * 0.45 / 0.3 / 0.15 / 0.1, no ploidy array, median of 10 calls behind 3, run twice in one process; genotype_ms, the memset and both kernels):
 * 64 samples (2 016 pairs) 0.215 / 0.217 ms, 256 samples (32 640 pairs) 0.230 / 0.230 ms, 2 048 samples (2 096 128 pairs) 0.538 / 0.538 ms; a call
 * from Python took 0.32 / 0.32, 0.43 / 0.43 and 7.4 / 7.3 ms (42 MB of pairs to the host), the numpy model of tests/cohort_qc_model.py (float64 matrix
 * products on the same machine's CPUs) 12, 36 and 608 ms, and every call's outputs equalled it.  With 8 words instead of 2 to a lane of the first
 * kernel the three shapes took 0.306, 0.353 and 0.657 ms (20 waves at 64 samples).  A first reading: nothing is compared against it, and nothing
 * else has been measured. */
#define SVJG_QC_MAX_SAMPLES 2048
int svjg_cohort_qc(svjg_ctx *ctx, const uint8_t *gt /* [n_rows][n_samples] */, const uint8_t *ploidy /* [n_rows][n_samples], or NULL */,
                   uint64_t n_rows, uint32_t n_samples, uint32_t *sample /* [n_samples][6] */, uint32_t *pair /* [n_samples (n_samples - 1) / 2][5] */);

/* svjg_cohort_hwe: the sites of a cohort, from the calls a cohort run has made (--cohort-hwe): do a row's genotypes fit Hardy-Weinberg
 * proportions?  gt[n_rows][n_samples] = the calls, ploidy the same shape or NULL (2 everywhere).  An item enters iff it is a called diploid item,
 * the dip predicate of svjg_cohort_qc: P = 2 and g <= 2 (haploid, polyploid and ploidy-0 items and both no-call codes drop out).  Per row:
 * counts[r][3] = n_ref, n_het, n_alt, the entering items with g = 0, 1, 2; n their sum, nA = 2 n_alt + n_het, nB = 2 n_ref + n_het, m = min(nA, nB).
 * For every h of m's parity in 0..m, with a = (m - h) / 2 and b = (2 n - m - h) / 2, the weight is w(h) = 2^h n! / (a! h! b!), the number of ways to
 * have h heterozygotes among n diploids with m minor alleles (Wigginton et al. 2005).  p[r][0] = HWE, the two-sided exact test: the sum of w(h)
 * over the h with w(h) 10^7 <= w(n_het) (10^7 + 1) — the 1e-7 slack is the tie rule of R's fisher.test: exact ties occur — over the sum of all
 * w(h); p[r][1] = EXCHET, the one-sided test for excess heterozygotes: the sum over h >= n_het over the same total.  m = 0: both exactly 1.0;
 * n = 0: both NaN.  The model in Python integers is tests/cohort_hwe_model.py; the device forms log10 w(h) in double-double from the log10(i!)
 * table, every term relative to the h next to the mean nA nB / (2 n - 1), and sums doubles in a fixed order: within 1e-9 relative of the model
 * wherever the model is at least 1e-280 and no weight lies within 1e-8 of the tie rule's edge (asserted; the observed maximum is in DESIGN 4.3),
 * below that a value of at most 1e-279, possibly 0.  One kernel, one row a wave segment, no atomics: equal bytes from run to run, and a row's bytes
 * do not depend on the rows around it or on how the caller chunks the rows.  The call reads the log10(i!) table — it reserves 2 n_samples + 1
 * entries through svjg_logfact_reserve's path before it launches — and neither needs nor reads the cohort matrix or the count vector; it works
 * in a block of its own: it neither reads nor changes any other call's block or views.  The caller bounds memory by calling with row chunks:
 * 1 byte per item (2 with a ploidy array) and 28 bytes per row, on the device and the host.  n_rows = 0 returns 0 and writes nothing.
 * SVJG_E_ARG with a message in svjg_last_error, all found before any launch: a null gt, counts or p, n_samples = 0 or above
 * SVJG_HWE_MAX_SAMPLES, n_rows x n_samples beyond 2^40, n_rows >= 2^32.  svjg_last_kernel_ms reports the kernel as genotype_ms.
 * Measured once, with the change that added it (one MI355X, 2026-10-21, ROCm 7.2.0, tools/cohort_hwe_timing.py: genotypes in Hardy-Weinberg
 * proportions at a frequency per row in 0.01 .. 0.5, no ploidy array, median of 10 calls behind 3, run twice in one process; genotype_ms, the
 * kernel): 100 000 rows x 64 samples 0.163 / 0.159 ms, 10 000 rows x 2 048 samples 0.087 / 0.087 ms; a call from Python took 0.55 / 0.55 and
 * 0.79 / 0.79 ms, the host harness (tests/geno_sim, the same routines with g++ -O2, one thread) 305 and 218 ms for the same call, and the device's
 * p-values lay within 2.1e-15 and 5.6e-15 relative of the harness's.  A first reading: nothing is compared against it, and nothing else has
 * been measured. */
#define SVJG_HWE_MAX_SAMPLES 65536
int svjg_cohort_hwe(svjg_ctx *ctx, const uint8_t *gt /* [n_rows][n_samples] */, const uint8_t *ploidy /* [n_rows][n_samples], or NULL */,
                    uint64_t n_rows, uint32_t n_samples, uint32_t *counts /* [n_rows][3]: n_ref, n_het, n_alt */, double *p /* [n_rows][2]: HWE, EXCHET */);

/* ---- the whole pass in one call (what a fused svjedi-graph run and bench.py do per batch) -----------------------------------
 * svjg_set_rows copies the three per-row input arrays of svjg_genotype to the device once (they stay until the next
 * svjg_set_rows / svjg_destroy).  svjg_run_resident then does, for the resident text of svjg_gaf_upload and those rows:
 * svjg_reset_counts, svjg_classify_resident(base_offset, no hit records), svjg_allreduce_counts if the context has a
 * communicator, svjg_genotype — enqueued back to back with ONE host wait at the end (filter-alignments.py:123-166 and
 * predict-genotype.py:216-227, :281-325 with the counts handed over in HBM instead of through the JSON file).
 * Results land in the context's pinned host block, valid until the next svjg_run_resident / svjg_set_rows / svjg_destroy:
 * gt[r], raw[r*2..] as svjg_genotype; pl[r*3..] = the PLs as 32-bit integers; flags[r] bit 0 = genotyped, bit 1 = a PL of the
 * row does not fit 32 bits (ask svjg_genotype for the 64-bit values: it needs > 4e7 informative alignments for one SV);
 * boundary[r] as svjg_genotype_boundary. */
int svjg_set_rows(svjg_ctx *ctx, const uint8_t *sv_type, const uint32_t *slot, const uint8_t *ok, uint64_t n_rows);
int svjg_run_resident(svjg_ctx *ctx, uint64_t base_offset, uint32_t min_support, double err,
                      const uint8_t **gt, const int32_t **pl, const uint32_t **raw, const uint8_t **flags, const uint8_t **boundary);
/* The same in two halves, for a loop over batches: svjg_run_begin enqueues a pass (kernels on a compute stream of the context, its
 * genotypes and the hand-over of its results to pinned host memory on a low-priority stream) and returns; svjg_run_end waits for the
 * OLDEST pass in flight and hands out its results (valid until the second svjg_run_begin after it).  At most two passes are in flight,
 * so the results of pass k cross PCIe while pass k + 1 computes: begin(0); for k: begin(k + 1); end() -> results of k; ...; end().
 * A context without a communicator alternates its passes between two compute streams: the classify kernel of pass k + 1 starts in the
 * slots that of pass k vacates; lines such a pass defers are classified by svjg_run_end (same results; svjg_pass.h). */
int svjg_run_begin(svjg_ctx *ctx, uint64_t base_offset, uint32_t min_support, double err);
int svjg_run_end(svjg_ctx *ctx, const uint8_t **gt, const int32_t **pl, const uint32_t **raw, const uint8_t **flags, const uint8_t **boundary);

/* ---- host-side writer of <prefix>_informative_aln.json (libsvjg_host.so, no GPU involved) -----------------
 * Byte-identical to json.dumps(dict_of_informative_aln, sort_keys=True, indent=4) (filter-alignments.py:174-175)
 * from the hit records: sv_ids[slot] is the key of each count slot, `gaf` the same bytes that were classified. */
int svjg_write_informative_json(const char *path, const char *gaf, uint64_t n_bytes, const svjg_hitrec *recs,
                                uint64_t n_recs, const char *const *sv_ids, uint32_t n_slots, int n_threads);

/* Reader side for a stand-alone predict-genotype.py (json.load at predict-genotype.py:67-68, then only len() of the two
 * lists of each key, :219-226): one scan of the JSON text -> keys (unescaped UTF-8, NUL separated, file order) and
 * the two list lengths per key.  Buffers are malloc'd by the library and released with svjg_host_free. */
int svjg_count_informative_json(const char *path, char **keys_out, uint64_t *keys_len, uint64_t **counts_out, uint64_t *n_keys);
void svjg_host_free(void *p);

/* ---- native loader of the graph inputs (libsvjg_host.so, no GPU involved) ---------------------------------------
 * Fast path of svjedi-graph_amd/svjg/graph.py for the files construct-graph.py writes: <prefix>_svs_edges.json
 * (filter-alignments.py:95-98) and the alt-node S-lines of the GFA (:103-113) -> the svjg_graph tables above.
 * Returns SVJG_E_UNSUPPORTED for anything it does not recognise (escapes / non-ASCII in strings, duplicate keys, odd
 * node names, ...): the caller then uses the Python loader, which holds the semantics and raises what it raises. */
#define SVJG_E_UNSUPPORTED (-11)
typedef struct svjg_hostgraph svjg_hostgraph;
int  svjg_graph_load(const char *edges_json_path, const char *gfa_path, svjg_hostgraph **out);
const svjg_graph *svjg_graph_view(const svjg_hostgraph *g);           /* d_over = 100, flags = 0: the caller may copy and adjust */
int  svjg_graph_info(const svjg_hostgraph *g, const char **sv_ids_blob, uint64_t *sv_ids_len, uint32_t *n_hazard);   /* sv_ids: NUL-terminated, slot order */
void svjg_graph_free(svjg_hostgraph *g);

/* ---- native VCF rows (libsvjg_host.so, no GPU) ----------------------------------------------------
 * Fast path of svjedi-graph_amd/svjg/genotype.py for ordinary files: every data row's sv_id key (predict-genotype.py:118-211)
 * looked up among `n_keys` NUL-terminated keys (slots[i] = count slot of key i, NULL: slot = i; a repeated key: the last
 * wins, like json.load) -> the three input arrays of svjg_genotype; svjg_vcf_write then produces the output file
 * (predict-genotype.py:102-115, :248-271) from svjg_genotype's results.  slot_is_presence: ok = 3 instead of 1 (the
 * count table IS the JSON: svjg_genotype's gate bit 1).  SVJG_E_UNSUPPORTED for anything but plain ASCII rows with plain
 * decimal POS / END (and for every row the reference would crash on): the caller then runs the Python path. */
typedef struct svjg_vcf svjg_vcf;
int  svjg_vcf_load(const char *vcf_path, const char *keys_blob, uint64_t blob_len, const uint32_t *slots, uint32_t n_keys,
                   int slot_is_presence, svjg_vcf **out);
int  svjg_vcf_arrays(const svjg_vcf *v, const uint8_t **sv_type, const uint32_t **slot, const uint8_t **ok, uint64_t *n_rows);
int  svjg_vcf_write(const svjg_vcf *v, const char *out_path, const uint8_t *gt, const int64_t *pl, const uint32_t *raw,
                    const uint8_t *genotyped, uint64_t *n_genotyped);
void svjg_vcf_free(svjg_vcf *v);

/* ---- measurement hooks (bench.py): time of the kernels of the last classify / genotype.  HIP events, except in a fused pass
 * (svjg_run_begin): there the classify kernels leave time stamps of the device's constant-rate clock in the pass's status block — no
 * event record stands between two passes' kernels —; SVJG_KERNEL_MS=events in the environment puts the event pair back, and
 * svjg_last_main_ms then gives both readings of the same launch (by_events = 0 without it).  classify_main_ms of a fused pass k is
 * t_last(k) - max(t_first(k), t_last(k - 1)) when pass k was enqueued with pass k - 1 still in flight: the interval two overlapped
 * launches share is counted once, so the passes' figures add up to the time the device spent on them. ---- */
int svjg_last_kernel_ms(svjg_ctx *ctx, float *classify_main_ms, float *classify_slow_ms, float *genotype_ms);
int svjg_last_main_ms(svjg_ctx *ctx, float *by_stamps, float *by_events);
int svjg_sync(svjg_ctx *ctx);
/* ---- test hooks: k_classify_main's chunked regime (a first chunk per worker, then 64 KB chunks from one counter) begins at an even share
 * of 8 x 64 KB, 1.88 GB of text on 256 CUs x 14 workers.  svjg_set_main_workers caps the workers the launch plan is made for at
 * min(CUs x occupancy, workers) on this context (0, the default: no cap), for the step-by-step calls and the fused pass alike: with 3
 * workers the regime begins at 1.5 MB.  svjg_last_main_plan gives the plan of the last k_classify_main launch that finished on this context
 * (of a fused pass: the pass svjg_run_end last returned) — bytes of a worker's first chunk, bytes of a small chunk (0: even shares or
 * stripes), workers launched — and how often that launch asked the chunk counter (every worker ends on one claim at or behind the text's
 * end); all zero before the first launch.  Any pointer may be NULL. ---- */
int svjg_set_main_workers(svjg_ctx *ctx, uint32_t workers);
int svjg_last_main_plan(svjg_ctx *ctx, uint64_t *region, uint64_t *small, uint32_t *grid, uint64_t *chunks_claimed);
/* what plain streams of n_bytes reach on this GPU right now (16 B per lane, non-temporal, four in flight per lane; best of three), in
 * GB/s: copy = a device-to-device copy, bytes read + bytes written per second; read = a kernel that only reads (and folds what it read
 * into one word) — the measured ceilings bench.py reports beside the 8 TB/s of the data sheet.  Either pointer may be NULL. */
int svjg_copy_rate(svjg_ctx *ctx, uint64_t n_bytes, double *copy_gb_per_s, double *read_gb_per_s);

#ifdef __cplusplus
}
#endif
#endif
