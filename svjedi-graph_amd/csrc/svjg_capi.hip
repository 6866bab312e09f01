// libsvjg_hip.so — host side of the C ABI declared in include/svjg.h.
// One context = one MI355X; two compute streams (the second only carries every other overlapped fused pass: svjg_pass.h) and a low-priority one
// for a pass's genotypes and tail; kernels live in svjg_kernels.h.
#include "svjg_kernels.h"
#include "svjg_host_tables.h"
#include "svjg_pass.h"
#include "svjg_own.h"
#include <rccl/rccl.h>
#include <errno.h>
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <fcntl.h>
#include <unistd.h>
#include <string>
#include <thread>
#include <vector>

using namespace svjg;
typedef struct svjg_ctx svjg_ctx;

static thread_local std::string g_init_error;

// The main kernel's tables (perfect hash of the node names, link table) are built on the host from the graph: 0.25 s at 100 k SVs,
// 2.5 s at 500 k.  A process that gives several contexts the same graph (one per GPU: filter-alignments.py, bench.py --gpus N)
// builds them once: the most recent build is kept, keyed by the sizes and two digests of everything the build reads (graph_digest); the contexts' loads may come from several threads at once (the first builds, the others wait for it).
#include <memory>
#include <mutex>
namespace {
struct TablesCache {
    std::mutex mu;
    uint64_t key[6] = {0, 0, 0, 0, 0, 0};
    std::shared_ptr<const KernelTables> kt;
} g_tables;

uint64_t fold64(const void *p, size_t n, uint64_t h) {
    const uint8_t *b = (const uint8_t *)p;
    for (size_t i = 0; i + 8 <= n; i += 8) { uint64_t w; memcpy(&w, b + i, 8); h = (h ^ w) * 0x9E3779B97F4A7C15ull; h ^= h >> 29; }
    if (n & 7) { uint64_t w = 0; memcpy(&w, b + (n & ~(size_t)7), n & 7); h = (h ^ w ^ ((uint64_t)(n & 7) << 56)) * 0x9E3779B97F4A7C15ull; h ^= h >> 29; }   // (the last n % 8 bytes count too)
    return h;
}

// everything build_kernel_tables reads — node, edge and hit arrays, the chromosome names' BYTES (every node name is spelled from
// them), chrom_off, chrom_node_lo, d_over, flags — under two seeds.  No addresses: a freed graph's arrays are handed out again.
uint64_t graph_digest(const svjg_graph &g, uint64_t seed) {
    uint64_t h = seed;
    h = fold64(g.nodes, (size_t)(g.n_nodes + 1) * sizeof(svjg_node), h);
    h = fold64(g.edges, (size_t)g.n_edges * sizeof(svjg_edge), h ^ g.n_edges);
    h = fold64(g.hits, (size_t)g.n_hits * sizeof(uint32_t), h ^ g.n_hits);
    h = fold64(g.chrom_off, (size_t)(g.n_chrom + 1) * sizeof(uint32_t), h ^ g.n_chrom);
    h = fold64(g.chrom_node_lo, (size_t)(g.n_chrom + 1) * sizeof(uint32_t), h);
    h = fold64(g.chrom_names, (size_t)g.chrom_off[g.n_chrom], h);
    const uint64_t tail[3] = {g.d_over, g.flags, g.n_slots};
    return fold64(tail, sizeof tail, h);
}

std::shared_ptr<const KernelTables> kernel_tables_for(const svjg_graph &g) {
    const uint64_t key[6] = {g.n_nodes, g.n_edges, g.n_hits, g.n_chrom, graph_digest(g, 1), graph_digest(g, 0xD6E8FEB86659FD93ull)};
    std::lock_guard<std::mutex> lk(g_tables.mu);              // (held while building: a second loader of the same graph waits, then reuses)
    if (!g_tables.kt || memcmp(key, g_tables.key, sizeof key) != 0) {
        g_tables.kt = std::make_shared<const KernelTables>(build_kernel_tables(g));
        memcpy(g_tables.key, key, sizeof key);
    }
    return g_tables.kt;
}
}  // namespace

extern "C" void svjg_release_host_tables(void) {
    std::lock_guard<std::mutex> lk(g_tables.mu);
    g_tables.kt.reset();
    memset(g_tables.key, 0, sizeof g_tables.key);
}

// ingest geometry: a file range goes to HBM through pinned buffers filled by STAGE_THREADS host threads (page cache ->
// pinned piece by pread -> asynchronous copy on the thread's stream; the next piece is read while the previous one is on
// the bus)
constexpr int STAGE_THREADS = 4;
constexpr uint64_t STAGE_PIECE = 8ull << 20;

// The device block of a step-by-step genotype call and its pinned host twin (genotype_leg).  Every call has a block of its own: svjg_genotype_view
// hands out pointers into BLOCK_ROWS' twin and svjg_genotype_boundary reads it later, and both must survive calls of the other ten.
// A fused pass's slot holds the same pair (RunSlot).
struct LegBlock { DevBuf<uint8_t> d;  PinBuf h; };
enum { BLOCK_ROWS, BLOCK_PLOIDY, BLOCK_SITES, BLOCK_COHORT, BLOCK_COHORT_PLOIDY, BLOCK_COHORT_PRIOR, BLOCK_COHORT_SITES, BLOCK_COHORT_QUAL, BLOCK_COHORT_SITES_PRIOR, BLOCK_COHORT_QC, BLOCK_COHORT_HWE, LEG_BLOCKS };   // eleven, a call each (svjg_geno.h: LegSpan): rows_layout, ploidy_layout, sites_layout, cohort_layout for the three cohort blocks, sites_layout again, qual_layout, sites_layout with its prior switch, qc_layout, hwe_layout

// slots the passes of svjg_run_begin rotate through: two may be in flight, and the one the NEXT pass will use is zeroed while the newest computes
constexpr int RUN_SLOTS = 3;

// What one k_classify_main launch, and the k_classify_exact behind it, may write into.  Two main kernels may be alive at once (consecutive
// overlapped passes), and a launch shares NONE of this with the launch beside it: count vector and status block (the slot's), the two lists
// (the slot's), the workers' scratch words (the compute stream's).  Text and graph tables are read-only; a fused pass writes no hit records
// (want_hits 0).  The step-by-step calls have one set (step_targets), every fused pass its slot's (slot_targets); main_launch_setup fills
// ClassifyArgs from a set, and nobody assigns one of these fields of ClassifyArgs afterwards.
struct PassTargets {
    unsigned long long *counts;  DevStatus *st;
    uint64_t *deferred;  uint64_t deferred_cap;
    uint64_t *host;  uint64_t host_cap;              // offsets of the lines set aside for the host (SVJG_EXC_ASK_HOST)
    svjg_hitrec *recs;  uint64_t rec_cap;
    int scratch;                                     // the compute stream the launch runs on (0: stream, 1: stream2): svjg_ctx::d_long[scratch]
};

// The graph on the device: the tables svjg_load_graph uploads and the two count vectors (counts: what the API works on; snap: what an overflowed classify
// attempt is rolled back to).  free_graph resets it; GraphView gv looks into it.
struct GraphTables {
    DevBuf<svjg_node> nodes;  DevBuf<svjg_edge> edges;  DevBuf<uint32_t> hits;
    DevBuf<uint8_t> cnames;  DevBuf<uint32_t> coff, clo, chash, names, links, nok;  DevBuf<uint16_t> disp;  DevBuf<uint32_t> ihits, pfx;
    DevBuf<unsigned long long> counts, snap;
};

// Every allocation, event and stream is an owner (svjg_own.h) and goes with the context; members are destroyed last to first, so the streams stand first: buffers and events go before them.
struct svjg_ctx {
    Stream stream, copy_stream;
    // The second compute stream: overlapped fused passes alternate between `stream` and it, everything else runs on `stream`.
    // second_busy: stream2 holds work `stream` is not ordered behind; first_dirty: `stream` holds work other than overlapped passes that
    // stream2 is not ordered behind (serial_enter / svjg_run_begin order them, ev_join[i] recorded on stream i).
    Stream stream2;
    Stream stage_stream[STAGE_THREADS];  // ingest: each feeder thread with a copy stream of its own
    Event ev_join[2];
    bool second_busy = false, first_dirty = false;
    Event ev[6];
    int device = 0;
    int wall_khz = 0;                    // rate of wall_clock64(), the clock of the kernels' time stamps
    int n_cu = 256;
    int occ_main = 0;                    // workgroups of k_classify_main one CU holds
    uint32_t main_workers = 0;           // svjg_set_main_workers: the plan is made for at most that many workers (0: no cap; a test hook)
    MainPlan last_plan{0, 0, 0};  uint64_t last_claimed = 0;   // svjg_last_main_plan: the last k_classify_main launch that finished, and its status block's next_chunk
    std::string err;
    // graph
    bool have_graph = false, have_counts = false;
    GraphTables graph;
    GraphView gv{};
    uint32_t gflags = 0, n_slots = 0;
    // text
    DevBuf<uint8_t> d_gaf;  uint64_t gaf_bytes = 0;  bool have_gaf = false;
    // ingest: pinned staging buffers, two per feeder thread
    PinBuf h_stage[STAGE_THREADS * 2];
    Event stage_ev[STAGE_THREADS * 2];
    // outputs
    DevBuf<uint64_t> d_deferred;
    DevBuf<svjg_hitrec> d_recs;
    DevBuf<uint64_t> d_host;             // offsets of the lines set aside for the host (SVJG_EXC_ASK_HOST)
    DevBuf<DevStatus> d_st;
    DevBuf<unsigned long long> d_dbg;
    DevBuf<uint32_t> d_long[2];          // LONG_WORDS words per worker of k_classify_main (ClassifyArgs::long_pre), [k]: of the launches on compute stream k — two main kernels may be alive at once, worker numbers are per launch (scratch_words)
    const uint64_t *host_lines_src = nullptr;  uint64_t host_lines_cap = 0;   // the list hs().n_host counts (svjg_get_host_lines): d_host (nullptr), or the last finished pass's own
    PinBuf h_stp;                        // host twin of d_st in pinned memory: the status copies are asynchronous in both directions; [1]: a fresh status (svjg_init)
    DevStatus &hs(int k = 0) { return ((DevStatus *)h_stp.p)[k]; }
    uint64_t total_deferred = 0;
    // genotype scratch
    DevBuf<dd> d_logfact, d_bsum;  uint32_t logfact_n = 0;
    LegBlock leg[LEG_BLOCKS];
    uint64_t geno_rows = 0;                              // rows of the last svjg_genotype / svjg_genotype_view (svjg_genotype_boundary)
    // cohort: the slot-major count matrix (svjg_cohort_alloc: counts, then the presence bytes, ONE allocation) and the dense vector a sample's
    // column is staged in
    DevBuf<uint8_t> d_cm;  uint8_t *d_cpresent = nullptr;  uint32_t cohort_samples = 0, cohort_slots = 0;
    unsigned long long *cm() const { return (unsigned long long *)d_cm.p; }
    DevBuf<uint8_t> d_cstage;
    // resident VCF rows of svjg_set_rows / svjg_run_resident: device block d (results, row inputs) and the pinned host block h the results land in
    struct RunSlot : LegBlock {
        void *h_dev = nullptr;           // the pinned block as the device sees it
        DevBuf<unsigned long long> counts;   // the pass's own count vector (+ guard words): the next pass may zero its own while this one is genotyped
        Event ev[6], computed, copied;
        uint64_t base_offset = 0;  uint32_t min_support = 0;  double err = 0;  bool had_text = false, slow_end_own = false, timed_by_events = false;
        // the pass's own lists (two main kernels may be alive at once): deferred lines, lines for the host; sized in pass_lists, while no pass uses the slot
        DevBuf<uint64_t> deferred, host;
        bool overlapped = false;         // the pass's form (svjg_pass.h: pass_overlaps): no exact-path launch on its stream, svjg_run_end settles it
        bool inflight = false;           // begun, not yet ended
        bool settled = false;            // settle_pass has looked at it; geno_owed: it ran the exact path, the genotypes are owed once more
        bool geno_owed = false;  float ms_settle = 0;
        bool chained = false;            // another pass was in flight when this one was enqueued: its main kernel may have started under that one's drain
        hipStream_t on = nullptr;        // the compute stream of its kernels
        ClassifyArgs cargs{};            // its k_classify_main's arguments (the settle step's k_classify_exact takes the same)
        uint32_t grid = 0;               // ... and its workers (svjg_last_main_plan)
        bool clean = false;              // the pass before has already zeroed this slot's vector, status block and max_n (k_classify_exact)
    } run[RUN_SLOTS];
    int run_head = 0, run_tail = 0, run_inflight = 0;
    uint64_t pass_seq = 0;                               // passes begun: an overlapped pass k runs on compute stream k mod 2
    bool last_pass_deferred = false;                     // the last pass that finished deferred lines (pass_overlaps)
    uint64_t prev_t_last = 0;                            // t_last of the last finished pass's main kernel (pass_main_ticks); 0: none since the last host sync
    int counts_in_slot = -1;                             // >= 0: the newest counts live in that slot's vector, not yet in graph.counts (fetch_slot_counts)
    DevBuf<uint8_t> d_run_in;  uint64_t run_rows = 0;  bool have_rows = false;
    // timing of the last calls
    float ms_main = 0, ms_slow = 0, ms_geno = 0;
    float ms_main_stamps = 0, ms_main_events = 0;   // the last fused pass's k_classify_main by the device's clock / by the event pair (svjg_last_main_ms)
    // rccl
    ncclComm_t comm = nullptr;
    bool allreduce_second = false;       // svjg_comm_set_stream
    uint64_t part_total = 0, part_need = 0, part_next = 0;   // svjg_gaf_upload_part
};

#define HIPCHK(ctx, call)                                                                         \
    do {                                                                                          \
        hipError_t e_ = (call);                                                                   \
        if (e_ != hipSuccess) {                                                                   \
            (ctx)->err = std::string(#call) + ": " + hipGetErrorString(e_);                       \
            return SVJG_E_HIP;                                                                    \
        }                                                                                         \
    } while (0)

extern "C" int svjg_abi_version(void) { return SVJG_ABI_VERSION; }

extern "C" int svjg_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

extern "C" const char *svjg_last_error(const svjg_ctx *ctx) { return ctx ? ctx->err.c_str() : g_init_error.c_str(); }

extern "C" int svjg_init(int device, svjg_ctx **out) {
    if (!out) return SVJG_E_ARG;
    *out = nullptr;
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess || n <= 0) {
        g_init_error = "no HIP device visible (libsvjg_hip has no CPU fallback)";
        return SVJG_E_NO_DEVICE;
    }
    if (device < 0 || device >= n) { g_init_error = "device index out of range"; return SVJG_E_ARG; }
    svjg_ctx *c = new svjg_ctx();
    c->device = device;
    if (hipSetDevice(device) != hipSuccess || c->stream.create() != hipSuccess || c->stream2.create() != hipSuccess ||
        c->ev_join[0].create(hipEventDisableTiming) != hipSuccess || c->ev_join[1].create(hipEventDisableTiming) != hipSuccess) {
        g_init_error = "hipSetDevice / hipStreamCreate failed";
        delete c;                                                 // (with whatever it made so far, here and below)
        return SVJG_E_HIP;
    }
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, device) == hipSuccess) c->n_cu = prop.multiProcessorCount;
    if (hipDeviceGetAttribute(&c->wall_khz, hipDeviceAttributeWallClockRate, device) != hipSuccess || c->wall_khz < 1) c->wall_khz = 0;
    for (auto &ev : c->ev) (void)ev.create();
    if (c->d_dbg.reserve(DBG_WORDS) != hipSuccess || c->d_st.reserve(1) != hipSuccess || c->h_stp.reserve(2 * sizeof(DevStatus), hipHostMallocDefault) != hipSuccess) {
        g_init_error = "hipMalloc failed";
        delete c;
        return SVJG_E_NOMEM;
    }
    memset(c->h_stp, 0, 2 * sizeof(DevStatus));
    c->hs(1).err = ~0ull;                                     // [1]: a fresh status, never written again (reset_status copies from it without a sync)
    hipFuncSetAttribute((const void *)k_classify_main, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
    *out = c;
    return 0;
}

static void free_graph(svjg_ctx *c) {
    c->graph = GraphTables{};
    c->have_graph = false; c->have_counts = false;
    for (auto &r : c->run) r.clean = false;                   // (the next graph's vector may be longer than what was zeroed)
}

extern "C" void svjg_destroy(svjg_ctx *c) {
    if (!c) return;
    hipSetDevice(c->device);
    if (c->stream) hipStreamSynchronize(c->stream);
    if (c->stream2) hipStreamSynchronize(c->stream2);
    if (c->copy_stream) hipStreamSynchronize(c->copy_stream);
    if (c->comm) ncclCommDestroy(c->comm);
    delete c;
}

// ---- the two compute streams ----
// Everything but an overlapped fused pass runs on c->stream and begins with serial_enter: c->stream then comes behind whatever stream2 holds
// (a pass's main kernel, a settle step), and the next pass that goes to stream2 will come behind this work (svjg_run_begin).
static int serial_enter(svjg_ctx *c) {
    if (c->second_busy) {
        HIPCHK(c, hipEventRecord(c->ev_join[1], c->stream2));
        HIPCHK(c, hipStreamWaitEvent(c->stream, c->ev_join[1], 0));
        c->second_busy = false;
    }
    c->first_dirty = true;
    return 0;
}
// the host waits for both (a buffer is about to be freed, the caller wants everything done)
static int sync_compute(svjg_ctx *c) {
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (c->stream2) HIPCHK(c, hipStreamSynchronize(c->stream2));
    c->second_busy = false; c->first_dirty = false; c->prev_t_last = 0;
    return 0;
}

template <class T>
static int upload(svjg_ctx *c, DevBuf<T> &dst, const T *src, uint64_t n, uint64_t extra = 0) {
    HIPCHK(c, dst.reserve(n + extra + 1));
    if (n) HIPCHK(c, hipMemcpyAsync(dst, src, n * sizeof(T), hipMemcpyHostToDevice, c->stream));
    return 0;
}

#ifndef SVJG_SMALL_CHUNK
#define SVJG_SMALL_CHUNK 65536
#endif
#ifndef SVJG_FIRST_SHARE
#define SVJG_FIRST_SHARE 0.85
#endif
constexpr uint64_t SMALL_CHUNK = SVJG_SMALL_CHUNK;            // bytes (multiple of 16)
constexpr double FIRST_CHUNK_SHARE = SVJG_FIRST_SHARE;       // of an even share of the text

// the count vector and its guard words (svjg_pass.h), in bytes
static uint64_t counts_bytes(const svjg_ctx *c) { return ((uint64_t)c->n_slots + GUARD_WORDS) * 8; }
// graph.counts and the snapshot an overflowed classify attempt is rolled back to
static int alloc_count_vectors(svjg_ctx *c, GraphTables &t, uint32_t n_slots) {
    HIPCHK(c, t.counts.reserve((uint64_t)n_slots + GUARD_WORDS));
    HIPCHK(c, t.snap.reserve((uint64_t)n_slots + GUARD_WORDS));
    return 0;
}
// blocks of tpb over n items, 1 to 1024 (the kernels stride)
static uint32_t capped_grid(uint64_t n, uint32_t tpb = TPB) { const uint64_t g = (n + tpb - 1) / tpb; return g > 1024 ? 1024u : g < 1 ? 1u : (uint32_t)g; }

static int reset_status(svjg_ctx *c, bool all) {
    if (all) {                                                // from the constant copy: the host's own status may be written again at once
        c->hs() = c->hs(1); c->total_deferred = 0;
        HIPCHK(c, hipMemcpyAsync(c->d_st, &c->hs(1), sizeof(DevStatus), hipMemcpyHostToDevice, c->stream));
        return 0;
    }
    // (every earlier writer of hs() on the stream — the status read-backs — was followed by a synchronisation)
    c->hs().n_deferred = 0; c->hs().overflow = 0; c->hs().next_chunk = 0;
    HIPCHK(c, hipMemcpyAsync(c->d_st, &c->hs(), sizeof(DevStatus), hipMemcpyHostToDevice, c->stream));
    return 0;
}

// the graph's tables and count vectors into `t`, the view of them into c->gv (the copies on c->stream, waited for)
static int upload_graph(svjg_ctx *c, const svjg_graph *g, GraphTables &t) {
    int rc;
    if ((rc = upload(c, t.nodes, g->nodes, g->n_nodes + 1))) return rc;
    if ((rc = upload(c, t.edges, g->edges, g->n_edges))) return rc;
    if ((rc = upload(c, t.hits, g->hits, g->n_hits))) return rc;
    if ((rc = upload(c, t.cnames, (const uint8_t *)g->chrom_names, g->chrom_off[g->n_chrom], 8))) return rc;
    if ((rc = upload(c, t.coff, g->chrom_off, g->n_chrom + 1))) return rc;
    if ((rc = upload(c, t.clo, g->chrom_node_lo, g->n_chrom + 1))) return rc;
    std::vector<uint32_t> hash = build_chrom_hash(*g);
    if ((rc = upload(c, t.chash, hash.data(), hash.size()))) return rc;
    const std::shared_ptr<const KernelTables> ktp = kernel_tables_for(*g);   // (built once per graph and process)
    const KernelTables &kt = *ktp;
    if ((rc = upload(c, t.names, kt.names.data(), kt.names.size()))) return rc;
    if ((rc = upload(c, t.links, kt.links.data(), kt.links.size()))) return rc;
    if ((rc = upload(c, t.disp, kt.disp.data(), kt.disp.size()))) return rc;
    if ((rc = upload(c, t.ihits, kt.ihits.data(), kt.ihits.size()))) return rc;
    if ((rc = upload(c, t.nok, kt.node_of_kid.data(), kt.node_of_kid.size()))) return rc;
    if (!kt.name_pfx.empty() && (rc = upload(c, t.pfx, kt.name_pfx.data(), kt.name_pfx.size()))) return rc;   // (names of 49..64 bytes: rare)
    HIPCHK(c, hipStreamSynchronize(c->stream));           // `hash` and `kt` are locals
    c->gv.nodes = t.nodes; c->gv.n_nodes = (uint32_t)g->n_nodes; c->gv.edges = t.edges; c->gv.hits = t.hits;
    c->gv.chrom_names = t.cnames; c->gv.chrom_off = t.coff; c->gv.chrom_lo = t.clo; c->gv.chrom_hash = t.chash;
    c->gv.n_chrom = g->n_chrom; c->gv.hash_mask = (uint32_t)hash.size() - 1; c->gv.d_over = g->d_over;
    c->gv.dover_list = (g->flags & SVJG_GRAPH_DOVER_LIST) ? 1u : 0u;
    c->gv.name_pfx = t.pfx;
    c->gv.node_of_kid = t.nok; c->gv.name_tab = t.names; c->gv.name_ihits = t.ihits; c->gv.name_disp = t.disp; c->gv.name_slots = kt.name_slots; c->gv.name_buckets = kt.name_buckets;
    c->gv.name_complete = (kt.names_left_out == 0 && kt.names_skipped == 0) ? 1u : 0u;
    c->gv.link_tab = t.links; c->gv.link_mask = kt.link_mask; c->gv.link_seed = kt.link_seed;
    c->gflags = g->flags;
    if (g->flags & SVJG_GRAPH_DOVER_LIST) c->gflags |= SVJG_GRAPH_ALL_SLOW;   // (the exact routine knows where the reference's TypeError sits)
    if (kt.links_left_out) c->gflags |= SVJG_GRAPH_ALL_SLOW;   // a link the main kernel could not find would be a silent miss
    return alloc_count_vectors(c, t, g->n_slots);
}

extern "C" int svjg_load_graph(svjg_ctx *c, const svjg_graph *g) {
    if (!c || !g || !g->nodes || !g->chrom_off || !g->chrom_node_lo) return SVJG_E_ARG;
    if (g->n_nodes >= 0x7FFFFFFFull || g->n_edges >= 0x7FFFFFFFull || g->n_chrom >= 65535) { c->err = "graph too large"; return SVJG_E_ARG; }
    if (g->d_over >= 0x80000000u) { c->err = "d_over too large"; return SVJG_E_ARG; }   // (the overlap sums of the main kernel are 32 bits wide)
    HIPCHK(c, hipSetDevice(c->device));
    free_graph(c);                                            // (first: the old graph and the new one are never both on the device)
    GraphTables t;                                            // a failure midway leaves nothing behind: t goes, behind whatever is still being copied into it
    if (const int rc = upload_graph(c, g, t)) { hipStreamSynchronize(c->stream); return rc; }
    c->graph = std::move(t);
    c->n_slots = g->n_slots; c->have_counts = true; c->have_graph = true;
    return svjg_reset_counts(c);
}

extern "C" int svjg_alloc_counts(svjg_ctx *c, uint32_t n_slots) {
    if (!c) return SVJG_E_ARG;
    HIPCHK(c, hipSetDevice(c->device));
    free_graph(c);
    if (const int rc = alloc_count_vectors(c, c->graph, n_slots)) return rc;
    c->n_slots = n_slots; c->have_counts = true;
    return svjg_reset_counts(c);
}

extern "C" int svjg_reset_counts(svjg_ctx *c) {
    if (!c || !c->have_counts) return SVJG_E_ARG;
    c->counts_in_slot = -1;
    HIPCHK(c, hipSetDevice(c->device));
    { const int rc0 = serial_enter(c); if (rc0) return rc0; }
    HIPCHK(c, hipMemsetAsync(c->graph.counts, 0, counts_bytes(c), c->stream));
    return reset_status(c, true);                             // (nothing to wait for: the next call on the stream comes behind both)
}

// room for n bytes of text plus the zero padding the kernels read past the end without bounds tests
static int gaf_reserve(svjg_ctx *c, uint64_t n, uint64_t *need_out) {
    const uint64_t need = ((n + 15) & ~15ull) + TEXT + 64;
    if (need > c->d_gaf.cap) {
        { const int rc0 = sync_compute(c); if (rc0) return rc0; }     // (both compute streams read the text)
        c->d_gaf.release();                                           // (first: the old text and the new one are never both on the device)
        HIPCHK(c, c->d_gaf.reserve(need));
    }
    *need_out = need;
    return 0;
}

// bytes [offset, offset + n) of the open file -> d_gaf through the pinned staging buffers
static int staged_upload(svjg_ctx *c, int fd, uint64_t offset, uint64_t n, uint64_t dst_off = 0) {
    for (int i = 0; i < STAGE_THREADS * 2; ++i) {
        HIPCHK(c, c->h_stage[i].reserve(STAGE_PIECE, hipHostMallocDefault));
        HIPCHK(c, c->stage_ev[i].create(hipEventDisableTiming));
    }
    for (int t = 0; t < STAGE_THREADS; ++t) HIPCHK(c, c->stage_stream[t].create(hipStreamNonBlocking));
    const uint64_t n_pieces = (n + STAGE_PIECE - 1) / STAGE_PIECE;
    std::string errs[STAGE_THREADS];
    int rcs[STAGE_THREADS] = {};
    auto feeder = [&](int t) {
        auto fail = [&](int rc, const std::string &m) { rcs[t] = rc; errs[t] = m; };
        if (hipSetDevice(c->device) != hipSuccess) return fail(SVJG_E_HIP, "hipSetDevice in an ingest thread");
        bool used[2] = {false, false};
        uint64_t k = 0;
        for (uint64_t p = (uint64_t)t; p < n_pieces && !rcs[t]; p += STAGE_THREADS, ++k) {
            const int b = t * 2 + (int)(k & 1);
            const uint64_t a = p * STAGE_PIECE, len = n - a < STAGE_PIECE ? n - a : STAGE_PIECE;
            if (used[k & 1] && hipEventSynchronize(c->stage_ev[b]) != hipSuccess) return fail(SVJG_E_HIP, "hipEventSynchronize (ingest)");
            for (uint64_t got = 0; got < len;) {
                const ssize_t r = pread(fd, c->h_stage[b] + got, len - got, (off_t)(offset + a + got));
                if (r <= 0) return fail(SVJG_E_IO, r == 0 ? "the GAF file is shorter than announced" : std::string("pread: ") + strerror(errno));
                got += (uint64_t)r;
            }
            if (hipMemcpyAsync(c->d_gaf + dst_off + a, c->h_stage[b], len, hipMemcpyHostToDevice, c->stage_stream[t]) != hipSuccess ||
                hipEventRecord(c->stage_ev[b], c->stage_stream[t]) != hipSuccess) return fail(SVJG_E_HIP, "hipMemcpyAsync (ingest)");
            used[k & 1] = true;
        }
        if (hipStreamSynchronize(c->stage_stream[t]) != hipSuccess) fail(SVJG_E_HIP, "hipStreamSynchronize (ingest)");
    };
    std::vector<std::thread> th;
    for (int t = 1; t < STAGE_THREADS; ++t) th.emplace_back(feeder, t);
    feeder(0);
    for (auto &x : th) x.join();
    for (int t = 0; t < STAGE_THREADS; ++t)
        if (rcs[t]) { c->err = errs[t]; return rcs[t]; }
    return 0;
}

static int gaf_finish(svjg_ctx *c, uint64_t n, uint64_t need) {
    HIPCHK(c, hipMemsetAsync(c->d_gaf + n, 0, need - n, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    c->gaf_bytes = n;
    c->have_gaf = true;
    return 0;
}

extern "C" int svjg_gaf_upload(svjg_ctx *c, const char *gaf, uint64_t n) {
    if (!c || (n && !gaf)) return SVJG_E_ARG;
    if (c->run_inflight) { c->err = "svjg_gaf_upload with a pass in flight (svjg_run_end first: a repeat of that pass would read the new text)"; return SVJG_E_ARG; }
    HIPCHK(c, hipSetDevice(c->device));
    uint64_t need;
    int rc = gaf_reserve(c, n, &need);
    if (rc) return rc;
    c->have_gaf = false;
    if (n) HIPCHK(c, hipMemcpyAsync(c->d_gaf, gaf, n, hipMemcpyHostToDevice, c->stream));   // (the runtime stages pageable memory itself: 47 GB/s measured)
    return gaf_finish(c, n, need);
}

extern "C" int svjg_gaf_upload_part(svjg_ctx *c, const char *gaf, uint64_t n, uint64_t offset, uint64_t capacity, int last) {
    if (!c || (n && !gaf) || n > capacity || offset > capacity - n) return SVJG_E_ARG;
    if (c->run_inflight) { c->err = "svjg_gaf_upload_part with a pass in flight (svjg_run_end first)"; return SVJG_E_ARG; }
    HIPCHK(c, hipSetDevice(c->device));
    if (offset == 0) {
        int rc = gaf_reserve(c, capacity, &c->part_need);
        if (rc) return rc;
        c->have_gaf = false; c->part_total = capacity; c->part_next = 0;
    }
    if (capacity != c->part_total || offset != c->part_next || c->have_gaf) { c->err = "svjg_gaf_upload_part: pieces go in ascending order, the first at offset 0"; return SVJG_E_ARG; }
    if (n) HIPCHK(c, hipMemcpyAsync(c->d_gaf + offset, gaf, n, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));               // (the caller's buffer may go away)
    c->part_next = offset + n;
    if (last) return gaf_finish(c, c->part_next, c->part_need);   // (zero padding from the text's end to the end of the buffer)
    return 0;
}

extern "C" int svjg_gaf_upload_file(svjg_ctx *c, const char *path, uint64_t offset, uint64_t n) {
    if (!c || !path) return SVJG_E_ARG;
    if (c->run_inflight) { c->err = "svjg_gaf_upload_file with a pass in flight (svjg_run_end first)"; return SVJG_E_ARG; }
    HIPCHK(c, hipSetDevice(c->device));
    uint64_t need;
    int rc = gaf_reserve(c, n, &need);
    if (rc) return rc;
    c->have_gaf = false;
    if (n) {
        const int fd = open(path, O_RDONLY | O_CLOEXEC);
        if (fd < 0) { c->err = std::string("open ") + path + ": " + strerror(errno); return SVJG_E_IO; }
        rc = staged_upload(c, fd, offset, n);
        close(fd);
        if (rc) return rc;
    }
    return gaf_finish(c, n, need);
}

// Room in a device buffer the kernels of this context may still be using (DevBuf::reserve): the contents, if kept, are copied on c->stream, and the
// old block is freed once nothing enqueued anywhere still uses it.
struct ComputeIdle {
    const svjg_ctx *c;
    hipError_t operator()() const {
        const hipError_t e = hipStreamSynchronize(c->stream);
        return e == hipSuccess && c->second_busy ? hipStreamSynchronize(c->stream2) : e;
    }
};
template <class T>
static int ensure(svjg_ctx *c, DevBuf<T> &b, uint64_t want, bool keep) {
    HIPCHK(c, b.reserve(want, keep, c->stream, ComputeIdle{c}));
    return 0;
}

// The passes of svjg_run_begin keep their counts in vectors of their own; the rest of the API works on graph.counts: the newest pass's
// vector is copied there when someone asks for it (svjg_get_counts, svjg_genotype, svjg_classify adding to it, ...).
static int settle_pass(svjg_ctx *c, svjg_ctx::RunSlot &r);
static int fetch_slot_counts(svjg_ctx *c) {
    if (c->counts_in_slot < 0) return 0;
    const int k = c->counts_in_slot;
    c->counts_in_slot = -1;
    HIPCHK(c, hipSetDevice(c->device));
    // an overlapped pass still in flight has no exact-path hits in its vector until it is settled: do that now (a host wait for the pass; svjg_run_end
    // then finds it settled), so that the counts handed out are the whole pass's, as they were when the exact path ran on the stream
    if (c->run[k].inflight && c->run[k].overlapped) { const int rc0 = settle_pass(c, c->run[k]); if (rc0) return rc0; }
    { const int rc0 = serial_enter(c); if (rc0) return rc0; }      // (the pass that uses this slot next may run on stream2: it comes behind the copy)
    if (c->run[k].copied) HIPCHK(c, hipStreamWaitEvent(c->stream, c->run[k].copied, 0));   // (the pass's all-reduce runs on the second stream)
    HIPCHK(c, hipMemcpyAsync(c->graph.counts, c->run[k].counts, counts_bytes(c), hipMemcpyDeviceToDevice, c->stream));
    return 0;
}

// the two sets of targets there are, each from its fields in this one place: the step-by-step calls' (the context's own lists, graph.counts, on c->stream) ...
static PassTargets step_targets(const svjg_ctx *c) { return PassTargets{c->graph.counts, c->d_st, c->d_deferred, c->d_deferred.cap, c->d_host, c->d_host.cap, c->d_recs, c->d_recs.cap, 0}; }
// ... and a fused pass's: everything its slot's (the status block lies in the slot's row block: its tail goes to the host in one small copy)
static PassTargets slot_targets(const svjg_ctx *c, const svjg_ctx::RunSlot &r, const RunLayout &L) {
    return PassTargets{r.counts, (DevStatus *)((uint8_t *)r.d + L.status), r.deferred, r.deferred.cap, r.host, r.host.cap, nullptr, 0, r.on == c->stream2 ? 1 : 0};
}

// the scratch words of the launches on compute stream k, allocated at the stream's first launch (the second block: only a context that overlaps
// passes has one); nullptr: no memory.  Both are freed where the occupancy becomes known (main_launch_setup).
static uint32_t *scratch_words(svjg_ctx *c, int k) {
    if (!c->d_long[k] && c->d_long[k].reserve((uint64_t)c->n_cu * (uint64_t)c->occ_main * LONG_WORDS) != hipSuccess) (void)hipGetLastError();
    return c->d_long[k];
}

#ifdef SVJG_ABLATE
// ablation knobs (measurement builds only): ClassifyArgs::diag from SVJG_DIAG; the occupancy the API gave, printed, and SVJG_OCC in its place
static uint32_t ablate_diag() { const char *dg = getenv("SVJG_DIAG"); return dg ? (uint32_t)atoi(dg) : 0u; }
static void ablate_occupancy(svjg_ctx *c, int occ, size_t lds) { const char *oc = getenv("SVJG_OCC"); fprintf(stderr, "[svjg diag] occupancy API: %d workgroups of %u threads per CU (LDS %zu)\n", occ, WG, lds); if (oc && atoi(oc) > 0) c->occ_main = atoi(oc); }
#endif

// arguments and geometry of one k_classify_main launch over the lines of the resident text that lie in [begin, end), writing into `t`
static int main_launch_setup(svjg_ctx *c, const PassTargets &t, uint64_t begin, uint64_t end, uint64_t base_offset, int want_hits, ClassifyArgs &a, uint32_t &grid, size_t &lds) {
    a.gaf = c->d_gaf; a.begin = begin; a.n_bytes = end; a.base_offset = base_offset; a.g = c->gv;
    a.all_slow = (c->gflags & SVJG_GRAPH_ALL_SLOW) != 0; a.want_hits = want_hits != 0;
#ifdef SVJG_ABLATE
    a.diag = ablate_diag();
#endif
    a.counts = t.counts; a.st = t.st; a.deferred = t.deferred; a.deferred_cap = t.deferred_cap;
    a.host_lines = t.host; a.host_cap = t.host_cap; a.recs = t.recs; a.rec_cap = t.rec_cap; a.dbg = c->d_dbg;
    lds = LDS_MAIN;
    if (c->occ_main < 1) {                                // persistent grid: every CU filled to what LDS / registers admit (asked once)
        int occ = 0;
        if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&occ, k_classify_main, (int)WG, lds) != hipSuccess || occ < 1) occ = 1;
        c->occ_main = occ = main_occupancy(occ, lds, LDS_GRANULE);
        for (auto &w : c->d_long) w.release();
#ifdef SVJG_ABLATE
        ablate_occupancy(c, occ, lds);
#endif
    }
    if (!(a.long_pre = scratch_words(c, t.scratch))) { c->err = "no memory for the workers' scratch words"; return SVJG_E_NOMEM; }
    uint64_t workers = (uint64_t)c->n_cu * (uint64_t)c->occ_main;     // (the scratch words are sized by this, whatever the cap)
    if (c->main_workers && c->main_workers < workers) workers = c->main_workers;
    const MainPlan p = main_plan(end - begin, workers, TEXT, SMALL_CHUNK, FIRST_CHUNK_SHARE);
    a.region = p.region; a.small = p.small; grid = p.grid;
    return 0;
}

// The exact path's one launch, k_classify_exact behind a k_classify_main with the same arguments: its blocks take the wave role up to
// `wave_rounds` rounds of deferred lines, the lane role beyond, and zero `nx` for the fused pass after this one (NextPass{}: nothing).
// The two callers' limits were measured apart; making them one needs a crossover measurement and is not part of unifying the kernels.
constexpr uint64_t EXACT_ROUND_PER_CU = 4;      // lines a CU in a round: the grid of the former one-wave-per-line kernel, now only the limits' unit
constexpr uint64_t STEP_WAVE_ROUNDS = 30;       // classify_range: the roles met at ~31 k lines on 256 CUs (profiles/r04/experiments/exact_path.txt)
constexpr uint64_t FUSED_WAVE_ROUNDS = 16;      // svjg_run_begin: r07 (profiles/r07/experiments/pass_tail.txt)
static int launch_exact(svjg_ctx *c, const ClassifyArgs &a, uint64_t wave_rounds, const NextPass &nx, hipStream_t on = nullptr, unsigned long long *t_begin = nullptr) {
    const uint64_t wave_limit = wave_rounds * EXACT_ROUND_PER_CU * (uint64_t)c->n_cu;
    hipLaunchKernelGGL(k_classify_exact, dim3((uint32_t)c->n_cu * EXACT_BLOCKS_PER_CU), dim3(EXACT_TPB), 0, on ? on : c->stream, a, wave_limit, nx, t_begin);
    HIPCHK(c, hipGetLastError());
    return 0;
}

// k_classify_main on `on`, for the step-by-step calls and the fused pass alike; ev (or nullptr): an event pair recorded around it
static int enqueue_main(svjg_ctx *c, hipStream_t on, const ClassifyArgs &a, uint32_t grid, size_t lds, Event *ev) {
    if (ev) HIPCHK(c, hipEventRecord(ev[0], on));
    hipLaunchKernelGGL(k_classify_main, dim3(grid), dim3(WG), lds, on, a);
    HIPCHK(c, hipGetLastError());
    if (ev) HIPCHK(c, hipEventRecord(ev[1], on));
    return 0;
}

#ifdef SVJG_TIMING
// measurement only (SVJG_DIAG & 16): what the kernels of a step-by-step call left in d_dbg, behind the main kernel / behind the exact path
static int timing_print_main(svjg_ctx *c) {
    unsigned long long d[16];
    HIPCHK(c, hipMemcpy(d, c->d_dbg, sizeof d, hipMemcpyDeviceToHost));
    fprintf(stderr, "[svjg diag] sub-passes of long lines: first sweep counting %llu, first sweep measuring only %llu, second sweep %llu; nodes in sub-passes %llu\n", d[12], d[13], d[14], d[15]);
    fprintf(stderr, "[svjg diag] wave time per phase (sum over waves, counter ticks)  A+B1 %llu  prefix %llu  B2 %llu  R1 %llu  NP: lists %llu  names+disp %llu  records %llu  scan+search %llu  links+atomics %llu  R6+end %llu;  passes %llu (sub-passes of long lines %llu), nodes in them %llu\n",
            d[0], d[1], d[2], d[3], d[8], d[9], d[4], 0ull, d[6], d[7], d[10], d[11], d[5]);
    return 0;
}
static int timing_print_exact(svjg_ctx *c) {
    unsigned long long d[8];
    HIPCHK(c, hipMemcpy(d, c->d_dbg + 16, sizeof d, hipMemcpyDeviceToHost));
    fprintf(stderr, "[svjg diag] one wave per line, the longest any line took per step (counter ticks): terminator + staging %llu  per-line part %llu  piece table %llu  nodes %llu  links %llu\n",
            d[0], d[1], d[2], d[3], d[4]);
    unsigned long long l[5];
    HIPCHK(c, hipMemcpy(l, c->d_dbg + 24, sizeof l, hipMemcpyDeviceToHost));
    fprintf(stderr, "[svjg diag] one lane per line, ticks summed over the blocks of 64 lines: terminators + staging %llu  per-line part %llu  nodes %llu  links %llu  rest %llu\n",
            l[0], l[1], l[2], l[3], l[4]);
    return 0;
}
#endif

// the lines of the resident text that lie in [begin, end): begin is a line start, end the byte behind a terminator (or the text's end)
static int classify_range(svjg_ctx *c, uint64_t begin, uint64_t end, uint64_t base_offset, int want_hits) {
    HIPCHK(c, hipSetDevice(c->device));
    { const int rc0 = fetch_slot_counts(c); if (rc0) return rc0; }
    { const int rc0 = serial_enter(c); if (rc0) return rc0; }
    c->host_lines_src = nullptr;                                  // (d_host, wherever ensure() puts it)
    if (end <= begin) return 0;
    const uint64_t n = end - begin;
    ListSizes want = lists_first((c->gflags & SVJG_GRAPH_ALL_SLOW) != 0, want_hits != 0, n, c->hs());
    int rc;
    for (int attempt = 0; attempt < 3; ++attempt) {
        if ((rc = ensure(c, c->d_deferred, want.deferred, false))) return rc;
        if ((rc = ensure(c, c->d_host, want.host, true))) return rc;
        if (want_hits && (rc = ensure(c, c->d_recs, want.recs, true))) return rc;
        // snapshot so that an overflowed attempt can be rolled back
        HIPCHK(c, hipMemcpyAsync(c->graph.snap, c->graph.counts, counts_bytes(c), hipMemcpyDeviceToDevice, c->stream));
        DevStatus before = c->hs();
        if ((rc = reset_status(c, false))) return rc;
        ClassifyArgs a{};
        uint32_t grid = 0;  size_t lds = 0;
        if ((rc = main_launch_setup(c, step_targets(c), begin, end, base_offset, want_hits, a, grid, lds))) return rc;
#ifdef SVJG_TIMING
        if (a.diag & 16u) HIPCHK(c, hipMemsetAsync(c->d_dbg, 0, 32 * 8, c->stream));
#endif
        if ((rc = enqueue_main(c, c->stream, a, grid, lds, c->ev))) return rc;
        HIPCHK(c, hipMemcpyAsync(&c->hs(), c->d_st, sizeof(DevStatus), hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
        c->last_plan = MainPlan{a.region, a.small, grid}; c->last_claimed = c->hs().next_chunk;
        const uint64_t n_def = c->hs().n_deferred;
#ifdef SVJG_TIMING
        if ((a.diag & 16u) && (rc = timing_print_main(c))) return rc;
#endif
        c->ms_slow = 0;
        if (n_def && !(c->hs().overflow & 1u)) {
            HIPCHK(c, hipEventRecord(c->ev[2], c->stream));
            if ((rc = launch_exact(c, a, STEP_WAVE_ROUNDS, NextPass{}))) return rc;
            HIPCHK(c, hipEventRecord(c->ev[3], c->stream));
            HIPCHK(c, hipMemcpyAsync(&c->hs(), c->d_st, sizeof(DevStatus), hipMemcpyDeviceToHost, c->stream));
            HIPCHK(c, hipStreamSynchronize(c->stream));
            HIPCHK(c, hipEventElapsedTime(&c->ms_slow, c->ev[2], c->ev[3]));
#ifdef SVJG_TIMING
            if ((a.diag & 16u) && (rc = timing_print_exact(c))) return rc;
#endif
        }
        HIPCHK(c, hipEventElapsedTime(&c->ms_main, c->ev[0], c->ev[1]));
        if (!c->hs().overflow) {
            c->total_deferred += n_def;                               // lines that took the exact path
            break;
        }
        // roll back and retry with worst-case buffers
        if (attempt == 2) { c->err = "output buffers overflowed repeatedly"; return SVJG_E_NOMEM; }
        want = lists_grown(want, n, before, c->hs());
        HIPCHK(c, hipMemcpyAsync(c->graph.counts, c->graph.snap, counts_bytes(c), hipMemcpyDeviceToDevice, c->stream));
        uint64_t keep_err = before.err;
        c->hs() = before; c->hs().err = keep_err;
    }
    if (c->hs().err != ~0ull) return SVJG_E_INPUT;
    return 0;
}

extern "C" int svjg_classify_resident(svjg_ctx *c, uint64_t base_offset, int want_hits) {
    if (!c || !c->have_graph || !c->have_gaf) { if (c) c->err = "classify needs a graph and an uploaded GAF"; return SVJG_E_ARG; }
    return classify_range(c, 0, c->gaf_bytes, base_offset, want_hits);
}

// Upload and classify overlapped: the text goes to HBM in pieces of PIPE_BYTES cut behind line terminators; while the kernels
// work on piece k (this thread, the context's stream), a helper thread copies piece k + 1 (its own streams).  Every piece gets
// PIPE_GAP zero bytes behind it in the device buffer (the kernels read past the end of their text without bounds tests), so
// piece k sits at device offset cut[k] + k * PIPE_GAP and offsets are reported through a per-piece base.
// `fetch(dst_off, src_off, len)` moves bytes [src_off, src_off + len) of the source to d_gaf + dst_off and returns when
// they are there; `last_cut(lo, hi)` = offset behind the last terminator in [lo, hi) of the source, or lo if there is none.
constexpr uint64_t PIPE_BYTES = 128ull << 20;
constexpr uint64_t PIPE_GAP = ((uint64_t)TEXT + 64 + 15) & ~15ull;
template <class Fetch, class Cut>
static int classify_pipelined(svjg_ctx *c, uint64_t n, uint64_t base_offset, int want_hits, Fetch fetch, Cut last_cut) {
    HIPCHK(c, hipSetDevice(c->device));
    std::vector<uint64_t> cuts{0};
    while (cuts.back() < n) {
        const uint64_t lo = cuts.back(), hi = lo + PIPE_BYTES < n ? lo + PIPE_BYTES : n;
        uint64_t cut = hi == n ? n : last_cut(lo, hi);
        if (cut <= lo) cut = hi == n ? n : last_cut(lo, n);               // a line longer than a piece: up to the next terminator behind it
        if (cut <= lo) cut = n;
        cuts.push_back(cut);
    }
    const size_t n_pieces = cuts.size() - 1;
    auto dev_off = [&](size_t k) { return ((cuts[k] + 15) & ~15ull) + k * PIPE_GAP; };   // 16-byte aligned, >= PIPE_GAP - 15 zero bytes in front
    uint64_t need;
    int rc = gaf_reserve(c, dev_off(n_pieces - 1) + (cuts[n_pieces] - cuts[n_pieces - 1]), &need);
    if (rc) return rc;
    c->have_gaf = false;
    for (size_t k = 0; k < n_pieces; ++k) {                                // zero padding behind every piece
        const uint64_t e = dev_off(k) + (cuts[k + 1] - cuts[k]);
        const uint64_t upto = k + 1 < n_pieces ? dev_off(k + 1) : need;
        HIPCHK(c, hipMemsetAsync(c->d_gaf + e, 0, upto - e, c->stream));
    }
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if ((rc = fetch(dev_off(0), 0, cuts[1]))) return rc;
    for (size_t k = 0; k < n_pieces; ++k) {
        int rc_up = 0;
        std::thread up;
        if (k + 1 < n_pieces) up = std::thread([&, k] { rc_up = fetch(dev_off(k + 1), cuts[k + 1], cuts[k + 2] - cuts[k + 1]); });
        // (reported offsets = base + device offset: the base of a piece takes its place in the buffer out again; unsigned wrap-around is fine)
        rc = classify_range(c, dev_off(k), dev_off(k) + (cuts[k + 1] - cuts[k]), base_offset + cuts[k] - dev_off(k), want_hits);
        if (up.joinable()) up.join();
        if (rc) return rc;
        if (rc_up) return rc_up;
    }
    // (the buffer now holds the pieces with gaps: not a resident text for svjg_classify_resident)
    c->gaf_bytes = 0;
    return 0;
}

extern "C" int svjg_classify(svjg_ctx *c, const char *gaf, uint64_t n, uint64_t base_offset, int want_hits) {
    if (!c || (n && !gaf)) return SVJG_E_ARG;
    if (!c->have_graph) { c->err = "classify needs a graph"; return SVJG_E_ARG; }
    if (n == 0) return svjg_gaf_upload(c, gaf, 0);
    std::string uerr;
    auto fetch = [&](uint64_t dst, uint64_t src, uint64_t len) -> int {
        if (hipSetDevice(c->device) != hipSuccess) { uerr = "hipSetDevice (upload thread)"; return SVJG_E_HIP; }
        if (c->copy_stream.create(hipStreamNonBlocking) != hipSuccess) { uerr = "hipStreamCreate (upload)"; return SVJG_E_HIP; }
        if (hipMemcpyAsync(c->d_gaf + dst, gaf + src, len, hipMemcpyHostToDevice, c->copy_stream) != hipSuccess ||
            hipStreamSynchronize(c->copy_stream) != hipSuccess) { uerr = "hipMemcpyAsync (upload)"; return SVJG_E_HIP; }
        return 0;
    };
    auto last_cut = [&](uint64_t lo, uint64_t hi) -> uint64_t {
        if (hi == n) {                                                     // forward: the first terminator at or behind lo
            for (uint64_t p = lo; p < n; ++p) if (gaf[p] == '\n') return p + 1;
            return lo;
        }
        const void *q = memrchr(gaf + lo, '\n', hi - lo);
        return q ? (uint64_t)((const char *)q - gaf) + 1 : lo;
    };
    const int rc = classify_pipelined(c, n, base_offset, want_hits, fetch, last_cut);
    if (rc && !uerr.empty()) c->err = uerr;
    return rc;
}

extern "C" int svjg_classify_file(svjg_ctx *c, const char *path, uint64_t offset, uint64_t n, int want_hits) {
    if (!c || !path) return SVJG_E_ARG;
    if (!c->have_graph) { c->err = "classify needs a graph"; return SVJG_E_ARG; }
    if (n == 0) return svjg_gaf_upload(c, nullptr, 0);
    const int fd = open(path, O_RDONLY | O_CLOEXEC);
    if (fd < 0) { c->err = std::string("open ") + path + ": " + strerror(errno); return SVJG_E_IO; }
    auto fetch = [&](uint64_t dst, uint64_t src, uint64_t len) -> int { return staged_upload(c, fd, offset + src, len, dst); };
    auto last_cut = [&](uint64_t lo, uint64_t hi) -> uint64_t {
        std::vector<char> buf(1 << 20);
        if (hi == n && lo) {                                               // forward: the first terminator at or behind lo
            for (uint64_t p = lo; p < n;) {
                const ssize_t r = pread(fd, buf.data(), buf.size(), (off_t)(offset + p));
                if (r <= 0) break;
                const void *q = memchr(buf.data(), '\n', (size_t)r);
                if (q) return p + (uint64_t)((const char *)q - buf.data()) + 1;
                p += (uint64_t)r;
            }
            return lo;
        }
        for (uint64_t e = hi; e > lo;) {                                   // backward from hi
            const uint64_t b = e - lo > buf.size() ? e - buf.size() : lo;
            const ssize_t r = pread(fd, buf.data(), e - b, (off_t)(offset + b));
            if (r != (ssize_t)(e - b)) break;
            const void *q = memrchr(buf.data(), '\n', (size_t)r);
            if (q) return b + (uint64_t)((const char *)q - buf.data()) + 1;
            e = b;
        }
        return lo;
    };
    const int rc = classify_pipelined(c, n, offset, want_hits, fetch, last_cut);
    close(fd);
    return rc;
}

extern "C" int svjg_get_stats(svjg_ctx *c, svjg_stats *out) {
    if (!c || !out) return SVJG_E_ARG;
    out->n_lines = c->hs().n_lines; out->n_deferred = c->total_deferred; out->n_hitrecs = c->hs().n_recs; out->non_ascii = c->hs().non_ascii;
    return 0;
}

extern "C" int svjg_get_defer_causes(svjg_ctx *c, uint64_t *out8) {
    if (!c || !out8) return SVJG_E_ARG;
    for (int i = 0; i < 8; ++i) out8[i] = c->hs().cause[i];
    return 0;
}

extern "C" int svjg_input_error(svjg_ctx *c, int *cls, uint64_t *off) {
    if (!c || !cls || !off) return SVJG_E_ARG;
    if (c->hs().err == ~0ull) { *cls = SVJG_EXC_NONE; *off = 0; }
    else { *cls = (int)(c->hs().err & 7); *off = c->hs().err >> 3; }
    return 0;
}

extern "C" int svjg_get_counts(svjg_ctx *c, uint32_t *out, uint32_t n_slots) {
    if (!c || !c->have_counts || !out || n_slots != c->n_slots) return SVJG_E_ARG;
    HIPCHK(c, hipSetDevice(c->device));
    { const int rc0 = fetch_slot_counts(c); if (rc0) return rc0; }
    std::vector<unsigned long long> tmp(n_slots);
    if (n_slots) HIPCHK(c, hipMemcpyAsync(tmp.data(), c->graph.counts, (uint64_t)n_slots * 8, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    for (uint32_t i = 0; i < n_slots; ++i) { out[2 * i] = (uint32_t)tmp[i]; out[2 * i + 1] = (uint32_t)(tmp[i] >> 32); }
    return 0;
}

extern "C" int svjg_set_counts(svjg_ctx *c, const uint32_t *in, uint32_t n_slots) {
    if (!c || !c->have_counts || !in || n_slots != c->n_slots) return SVJG_E_ARG;
    c->counts_in_slot = -1;
    HIPCHK(c, hipSetDevice(c->device));
    std::vector<unsigned long long> tmp(n_slots);
    for (uint32_t i = 0; i < n_slots; ++i) tmp[i] = (unsigned long long)in[2 * i] | ((unsigned long long)in[2 * i + 1] << 32);
    if (n_slots) HIPCHK(c, hipMemcpyAsync(c->graph.counts, tmp.data(), (uint64_t)n_slots * 8, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return 0;
}

extern "C" int svjg_get_host_lines(svjg_ctx *c, uint64_t *out, uint64_t cap, uint64_t *n) {
    if (!c || !n) return SVJG_E_ARG;
    HIPCHK(c, hipSetDevice(c->device));
    *n = c->hs().n_host;
    const uint64_t held = c->host_lines_src ? c->host_lines_cap : c->d_host.cap;       // (never beyond the list itself)
    uint64_t have = c->hs().n_host < cap ? c->hs().n_host : cap;
    if (have > held) have = held;
    if (have && !out) return SVJG_E_ARG;
    if (have) HIPCHK(c, hipMemcpyAsync(out, c->host_lines_src ? c->host_lines_src : c->d_host, have * sizeof(uint64_t), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return 0;
}

extern "C" int svjg_get_hits(svjg_ctx *c, svjg_hitrec *out, uint64_t cap, uint64_t *n) {
    if (!c || !n) return SVJG_E_ARG;
    HIPCHK(c, hipSetDevice(c->device));
    uint64_t have = c->hs().n_recs < cap ? c->hs().n_recs : cap;
    if (have && !out) return SVJG_E_ARG;
    if (have) HIPCHK(c, hipMemcpyAsync(out, c->d_recs, have * sizeof(svjg_hitrec), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    *n = have;
    return 0;
}

// ---- multi-GPU ------------------------------------------------------------------------------------------

extern "C" int svjg_comm_unique_id(char *out128) {
    if (!out128) return SVJG_E_ARG;
    static_assert(sizeof(ncclUniqueId) == 128, "ncclUniqueId is 128 bytes");
    ncclUniqueId id;
    if (ncclGetUniqueId(&id) != ncclSuccess) return SVJG_E_RCCL;
    memcpy(out128, &id, 128);
    return 0;
}

extern "C" int svjg_comm_init(svjg_ctx *c, const char *id128, int n_ranks, int rank) {
    if (!c || !id128 || n_ranks < 1 || rank < 0 || rank >= n_ranks) return SVJG_E_ARG;
    HIPCHK(c, hipSetDevice(c->device));
    ncclUniqueId id;
    memcpy(&id, id128, 128);
    ncclResult_t r = ncclCommInitRank(&c->comm, n_ranks, id, rank);
    if (r != ncclSuccess) { c->err = std::string("ncclCommInitRank: ") + ncclGetErrorString(r); c->comm = nullptr; return SVJG_E_RCCL; }
    return 0;
}

extern "C" int svjg_comm_set_stream(svjg_ctx *c, int second_stream) {
    if (!c) return SVJG_E_ARG;
    if (c->run_inflight) { c->err = "svjg_comm_set_stream with a pass in flight"; return SVJG_E_ARG; }
    c->allreduce_second = second_stream != 0;
    return 0;
}

// the guard elements behind the count vector (svjg_pass.h) <- largest ref / alt field, and — st given: a fused pass — whether this
// rank's pass must be repeated (k_counts_guard)
static int launch_guard(svjg_ctx *c, unsigned long long *counts = nullptr, hipStream_t stream = nullptr, const DevStatus *st = nullptr) {
    if (!counts) counts = c->graph.counts;
    if (!stream) stream = c->stream;
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipMemsetAsync(counts + c->n_slots, 0, GUARD_WORDS * 8, stream));
    if (c->n_slots || st) {
        hipLaunchKernelGGL(k_counts_guard, dim3(capped_grid(c->n_slots)), dim3(TPB), 0, stream, counts, c->n_slots, st);
        HIPCHK(c, hipGetLastError());
    }
    return 0;
}
static int check_guard(svjg_ctx *c) {
    unsigned long long g[GUARD_WORDS] = {0, 0, 0};
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipMemcpyAsync(g, c->graph.counts + c->n_slots, sizeof g, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (pass_counts_overflowed(g[GUARD_MAX_REF], g[GUARD_MAX_ALT])) { c->err = "more than 2^32 informative alignments for one SV"; return SVJG_E_OVERFLOW; }
    return 0;
}

// the path's only collective: sum of the per-SV count vector (packed ref | alt << 32 as one u64 each, plus the two guard elements)
extern "C" int svjg_allreduce_counts(svjg_ctx *c) {
    if (!c || !c->have_counts) return SVJG_E_ARG;
    { const int rc0 = fetch_slot_counts(c); if (rc0) return rc0; }
    if (!c->comm) { c->err = "svjg_comm_init has not been called"; return SVJG_E_ARG; }
    int rc = launch_guard(c);
    if (rc) return rc;
    ncclResult_t r = ncclAllReduce(c->graph.counts, c->graph.counts, (size_t)c->n_slots + GUARD_WORDS, ncclUint64, ncclSum, c->comm, c->stream);
    if (r != ncclSuccess) { c->err = std::string("ncclAllReduce: ") + ncclGetErrorString(r); return SVJG_E_RCCL; }
    return check_guard(c);
}

// One process, several GPUs (the drop-in filter-alignments.py): one communicator per context from ncclCommInitAll, then the same
// all-reduce issued for every context between ncclGroupStart / ncclGroupEnd.  n == 1: only the overflow guard runs.
// svjg_comm_init_all may run in a thread of its own beside calls on the same contexts (svjg/filter.py: _CommInit), so what goes wrong in it
// is NOT written into a context's error string (another thread may be writing that): it has a message buffer of its own.
static std::mutex g_comm_err_mu;
static std::string g_comm_err;
static void comm_err_set(const std::string &m) { std::lock_guard<std::mutex> lk(g_comm_err_mu); g_comm_err = m; }
extern "C" int svjg_comm_error(char *out, uint64_t cap) {
    if (!out || !cap) return SVJG_E_ARG;
    std::lock_guard<std::mutex> lk(g_comm_err_mu);
    const size_t n = g_comm_err.size() < cap - 1 ? g_comm_err.size() : (size_t)cap - 1;
    memcpy(out, g_comm_err.data(), n); out[n] = 0;
    return 0;
}

extern "C" int svjg_comm_init_all(svjg_ctx *const *ctxs, int n) {
    if (!ctxs || n < 1 || n > 64) return SVJG_E_ARG;
    for (int i = 0; i < n; ++i) if (!ctxs[i]) return SVJG_E_ARG;
    if (n == 1) return 0;
    int devs[64];
    ncclComm_t comms[64];
    for (int i = 0; i < n; ++i) {
        devs[i] = ctxs[i]->device;
        for (int j = 0; j < i; ++j) if (devs[j] == devs[i]) { comm_err_set("svjg_comm_init_all: one context per device"); return SVJG_E_ARG; }
    }
    ncclResult_t r = ncclCommInitAll(comms, n, devs);
    if (r != ncclSuccess) { comm_err_set(std::string("ncclCommInitAll: ") + ncclGetErrorString(r)); return SVJG_E_RCCL; }
    for (int i = 0; i < n; ++i) {
        if (ctxs[i]->comm) ncclCommDestroy(ctxs[i]->comm);
        ctxs[i]->comm = comms[i];
    }
    return 0;
}

extern "C" int svjg_allreduce_counts_all(svjg_ctx *const *ctxs, int n) {
    if (!ctxs || n < 1 || n > 64) return SVJG_E_ARG;
    for (int i = 0; i < n; ++i) {
        if (!ctxs[i] || !ctxs[i]->have_counts || ctxs[i]->n_slots != ctxs[0]->n_slots) return SVJG_E_ARG;
        if (n > 1 && !ctxs[i]->comm) { ctxs[0]->err = "svjg_comm_init_all has not been called"; return SVJG_E_ARG; }
    }
    int rc;
    for (int i = 0; i < n; ++i) if ((rc = fetch_slot_counts(ctxs[i])) || (rc = launch_guard(ctxs[i]))) { if (i) ctxs[0]->err = ctxs[i]->err; return rc; }
    if (n > 1) {
        ncclResult_t r = ncclGroupStart();
        for (int i = 0; i < n && r == ncclSuccess; ++i) {
            svjg_ctx *c = ctxs[i];
            if (hipSetDevice(c->device) != hipSuccess) { ctxs[0]->err = "hipSetDevice"; ncclGroupEnd(); return SVJG_E_HIP; }
            r = ncclAllReduce(c->graph.counts, c->graph.counts, (size_t)c->n_slots + GUARD_WORDS, ncclUint64, ncclSum, c->comm, c->stream);
        }
        const ncclResult_t r2 = ncclGroupEnd();
        if (r == ncclSuccess) r = r2;
        if (r != ncclSuccess) { ctxs[0]->err = std::string("ncclAllReduce (group): ") + ncclGetErrorString(r); return SVJG_E_RCCL; }
    }
    for (int i = 0; i < n; ++i) if ((rc = check_guard(ctxs[i]))) { if (i) ctxs[0]->err = ctxs[i]->err; return rc; }
    return 0;
}

// ---- genotypes -----------------------------------------------------------------------------------------

// table of log10(i!) in double-double for the binomial term, at least `upto` entries and at most LOGFACT_CAP (svjg_geno.h: rows beyond
// the cap are recomputed on the host) (kernels on the context's stream; no host wait)
static int build_logfact(svjg_ctx *c, uint32_t upto) {
    static_assert(LF_BLOCK == LOGFACT_BLOCK, "svjg_kernels.h and svjg_geno.h disagree");
    const uint32_t want = logfact_built(upto);
    { const int rc0 = serial_enter(c); if (rc0) return rc0; }
    c->d_logfact.release(); c->d_bsum.release(); c->logfact_n = 0;      // (the callers have waited for whatever used the old table)
    HIPCHK(c, c->d_logfact.reserve(want));
    HIPCHK(c, c->d_bsum.reserve(want / LF_BLOCK));
    hipLaunchKernelGGL(k_logfact_local, dim3(want / LF_BLOCK), dim3(LF_BLOCK), 0, c->stream, c->d_logfact, c->d_bsum, want);
    hipLaunchKernelGGL(k_logfact_bsum, dim3(1), dim3(64), 0, c->stream, c->d_bsum, want / LF_BLOCK);
    hipLaunchKernelGGL(k_logfact_add, dim3(want / LF_BLOCK), dim3(LF_BLOCK), 0, c->stream, c->d_logfact, c->d_bsum, want);
    HIPCHK(c, hipGetLastError());
    c->logfact_n = want;
    return 0;
}

// ---- one genotype leg, for the step-by-step calls (genotype_leg) and the fused pass alike ----
// k_genotype's arguments but where the results go (the callers' layouts, svjg_geno.h); p: device block with the rows' inputs at I
static GenoArgs geno_args(const svjg_ctx *c, const unsigned long long *counts, const uint8_t *p, const RowsIn &I, uint64_t n_rows, uint32_t min_support, double err) {
    GenoArgs a{};
    a.counts = counts; a.slot = (const uint32_t *)(p + I.slot); a.sv_type = p + I.type; a.ok = p + I.ok; a.n_rows = n_rows; a.n_slots = c->n_slots;
    a.min_support = min_support; a.logfact = c->d_logfact; a.logfact_n = c->logfact_n;
    a.l_ok = log10(1.0 - err); a.l_err = log10(err); a.l_half = log10(1.0 / 2.0);     // host libm, as CPython's math.log10
    return a;
}
// the same with the results in the block too: L is a RowsLayout, a PloidyLayout or a CohortLayout (the same five outputs and the pair)
template <class Layout>
static GenoArgs block_geno_args(const svjg_ctx *c, const unsigned long long *counts, uint8_t *base, const Layout &L, uint64_t n_rows, uint32_t min_support, double err) {
    GenoArgs a = geno_args(c, counts, base, L.in, n_rows, min_support, err);
    a.pl = (int64_t *)(base + L.pl); a.raw = (uint32_t *)(base + L.raw); a.gt = base + L.gt; a.genotyped = base + L.flags;
    a.boundary = base + L.boundary; a.max_n = (unsigned int *)(base + L.maxn);
    return a;
}

// all rows with the table at hand, blocks of TPB on the compute stream (a fused pass's FIRST launch is svjg_run_begin's own)
static int launch_genotype(svjg_ctx *c, GenoArgs &a) {
    a.logfact = c->d_logfact; a.logfact_n = c->logfact_n;
    HIPCHK(c, hipMemsetAsync(a.max_n, 0, 8, c->stream));
    hipLaunchKernelGGL(k_genotype, dim3((uint32_t)((a.n_rows + TPB - 1) / TPB)), dim3(TPB), 0, c->stream, a);
    HIPCHK(c, hipGetLastError());
    return 0;
}

// Behind a launch, its max_n pair on the host (h_maxn): [1] a row names a slot out of range, [0] the largest n = ref + alt beyond
// the log10(i!) table.  Only then (first call, or a deeper sample than ever before) the table is rebuilt, the rows run again, `bytes` from
// d_back come back to h_back (what the caller reads, the pair included) and the check repeats.  relaunch_first: the launch itself is still
// owed (svjg_run_end behind a repeated pass).  max_n is the maximum over ALL rows, so one growth is enough; the second only guards this reasoning.
// launch(): the kernel over all its items again with the table at hand; it zeroes again whatever the kernel adds to (launch_genotype,
// launch_ploidy, launch_sites, launch_cohort).
template <class Launch>
static int settle_launch(svjg_ctx *c, const unsigned int *h_maxn, void *h_back, const void *d_back, uint64_t bytes, bool relaunch_first, Launch launch) {
    for (int growths = 0;; relaunch_first = false) {
        if (!relaunch_first) {
            if (h_maxn[1]) { c->err = "slot out of range"; return SVJG_E_ARG; }   // (checked by the kernel, row by row)
            if (h_maxn[0] == 0) return 0;                        // every row found its binomial term
            if (growths++ == 2) { c->err = "log10(i!) table could not be sized"; return SVJG_E_HIP; }
            { const int rc0 = sync_compute(c); if (rc0) return rc0; }   // (a pass already enqueued still uses the old table: it drains first)
            if (c->copy_stream) HIPCHK(c, hipStreamSynchronize(c->copy_stream));
            if (const int rc = build_logfact(c, logfact_grow_to(h_maxn[0]))) return rc;
        }
        if (const int rc = launch()) return rc;
        HIPCHK(c, hipMemcpyAsync(h_back, d_back, bytes, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
    }
}

// The host leg of a step-by-step call, on the compute stream: the call's block b and its pinned twin sized for S; fill(hb) stages the inputs into the
// twin's input region; ONE copy in; the first table, if the context has none; launch(base) runs the call's kernel over all items of the device block
// `base` with the table at hand; ONE copy out of the outputs and the max_n pair, which then lie in the twin; settle_launch (launch(base) again behind
// every growth of the table).  ms_geno: the event pair around the FIRST launch (and the table's build, if any), read once the results are settled.
template <class Fill, class Launch>
static int genotype_leg(svjg_ctx *c, LegBlock &b, const LegSpan &S, Fill fill, Launch launch) {
    int rc;
    if ((rc = ensure(c, b.d, S.total, false))) return rc;
    HIPCHK(c, b.h.reserve(S.total, hipHostMallocDefault));
    uint8_t *base = b.d, *hb = b.h;
    fill(hb);
    HIPCHK(c, hipMemcpyAsync(base + S.in_at, hb + S.in_at, S.in_bytes, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipEventRecord(c->ev[4], c->stream));
    if (c->logfact_n == 0 && (rc = build_logfact(c, logfact_first()))) return rc;
    if ((rc = launch(base))) return rc;
    HIPCHK(c, hipEventRecord(c->ev[5], c->stream));
    HIPCHK(c, hipMemcpyAsync(hb, base, S.maxn + 8, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if ((rc = settle_launch(c, (const unsigned int *)(hb + S.maxn), hb, base, S.maxn + 8, false, [&] { return launch(base); }))) return rc;
    HIPCHK(c, hipEventElapsedTime(&c->ms_geno, c->ev[4], c->ev[5]));
    return 0;
}

static void stage_rows(uint8_t *hb, const RowsIn &I, const uint8_t *sv_type, const uint32_t *slot, const uint8_t *ok, uint64_t n_rows) {   // a call's three input arrays into the pinned block
    memcpy(hb + I.slot, slot, n_rows * 4); memcpy(hb + I.type, sv_type, n_rows); memcpy(hb + I.ok, ok, n_rows);
}

// results of all rows -> the pinned host block BLOCK_ROWS (rows_layout)
static int genotype_rows(svjg_ctx *c, const uint8_t *sv_type, const uint32_t *slot, const uint8_t *ok, uint64_t n_rows, uint32_t min_support, double err) {
    HIPCHK(c, hipSetDevice(c->device));
    { const int rc0 = fetch_slot_counts(c); if (rc0) return rc0; }
    const RowsLayout L = rows_layout(n_rows);
    return genotype_leg(c, c->leg[BLOCK_ROWS], L,
        [&](uint8_t *hb) { stage_rows(hb, L.in, sv_type, slot, ok, n_rows); c->geno_rows = n_rows; },   // (from here on the block is this call's)
        [&](uint8_t *base) { GenoArgs a = block_geno_args(c, c->graph.counts, base, L, n_rows, min_support, err); return launch_genotype(c, a); });
}

// The results where the device's copy left them: the four pointers look into the context's pinned host block and stay
// valid until the next svjg_genotype / svjg_genotype_view / svjg_destroy on this context.
extern "C" int svjg_genotype_view(svjg_ctx *c, const uint8_t *sv_type, const uint32_t *slot, const uint8_t *ok, uint64_t n_rows,
                                  uint32_t min_support, double err, const uint8_t **gt, const int64_t **pl, const uint32_t **raw,
                                  const uint8_t **genotyped) {
    if (!c || !c->have_counts || !gt || !pl || !raw || !genotyped) return SVJG_E_ARG;
    *gt = nullptr; *pl = nullptr; *raw = nullptr; *genotyped = nullptr;
    if (n_rows == 0) return 0;
    if (!sv_type || !slot || !ok) return SVJG_E_ARG;
    const int rc = genotype_rows(c, sv_type, slot, ok, n_rows, min_support, err);
    if (rc) return rc;
    const uint8_t *hb = c->leg[BLOCK_ROWS].h;
    const RowsLayout L = rows_layout(n_rows);
    *pl = (const int64_t *)(hb + L.pl); *raw = (const uint32_t *)(hb + L.raw); *gt = hb + L.gt; *genotyped = hb + L.flags;
    return 0;
}

// The same, copied into the caller's arrays.
extern "C" int svjg_genotype(svjg_ctx *c, const uint8_t *sv_type, const uint32_t *slot, const uint8_t *ok, uint64_t n_rows,
                             uint32_t min_support, double err, uint8_t *gt, int64_t *pl, uint32_t *raw, uint8_t *genotyped) {
    if (n_rows && (!gt || !pl || !raw || !genotyped)) return SVJG_E_ARG;
    const uint8_t *v_gt, *v_done; const int64_t *v_pl; const uint32_t *v_raw;
    const int rc = svjg_genotype_view(c, sv_type, slot, ok, n_rows, min_support, err, &v_gt, &v_pl, &v_raw, &v_done);   // (checks the rest)
    if (rc || !n_rows) return rc;
    memcpy(pl, v_pl, n_rows * 3 * sizeof *pl); memcpy(raw, v_raw, n_rows * 2 * sizeof *raw); memcpy(gt, v_gt, n_rows); memcpy(genotyped, v_done, n_rows);
    return 0;
}

// Any ploidy from 1 to SVJG_MAX_PLOIDY per row (k_genotype_ploidy; svjg.h), through genotype_leg in BLOCK_PLOIDY: the call's logarithms and the
// rows' ploidies go in with the three input arrays.
static int launch_ploidy(svjg_ctx *c, GenoPloidyArgs &p) {
    p.g.logfact = c->d_logfact; p.g.logfact_n = c->logfact_n;
    HIPCHK(c, hipMemsetAsync(p.g.max_n, 0, 8, c->stream));
    hipLaunchKernelGGL(k_genotype_ploidy, dim3((uint32_t)((p.g.n_rows + TPB - 1) / TPB)), dim3(TPB), 0, c->stream, p);
    HIPCHK(c, hipGetLastError());
    return 0;
}

extern "C" int svjg_genotype_ploidy(svjg_ctx *c, const uint8_t *sv_type, const uint32_t *slot, const uint8_t *ok, const uint8_t *ploidy,
                                    uint64_t n_rows, uint32_t min_support, double err, uint8_t *gt, int64_t *pl, uint32_t *raw,
                                    uint8_t *genotyped, uint8_t *boundary) {
    if (!c || !c->have_counts) return SVJG_E_ARG;
    if (n_rows == 0) return 0;
    if (!sv_type || !slot || !ok || !ploidy || !gt || !pl || !raw || !genotyped || !boundary) return SVJG_E_ARG;
    for (uint64_t r = 0; r < n_rows; ++r)
        if (ploidy[r] > SVJG_MAX_PLOIDY) { c->err = "ploidy above SVJG_MAX_PLOIDY"; return SVJG_E_ARG; }
    static_assert(SVJG_MAX_PLOIDY == MAX_PLOIDY, "svjg.h and svjg_geno.h disagree");
    HIPCHK(c, hipSetDevice(c->device));
    { const int rc0 = fetch_slot_counts(c); if (rc0) return rc0; }
    const PloidyLayout L = ploidy_layout(n_rows);
    const int rc = genotype_leg(c, c->leg[BLOCK_PLOIDY], L,
        [&](uint8_t *hb) { ploidy_log_table(err, (double *)(hb + L.logtab)); stage_rows(hb, L.in, sv_type, slot, ok, n_rows); memcpy(hb + L.ploidy, ploidy, n_rows); },   // (the logarithms by the host's libm, as geno_args' three)
        [&](uint8_t *base) {
            GenoPloidyArgs p{block_geno_args(c, c->graph.counts, base, L, n_rows, min_support, err), base + L.ploidy, (const double *)(base + L.logtab)};
            return launch_ploidy(c, p);
        });
    if (rc) return rc;
    const uint8_t *hb = c->leg[BLOCK_PLOIDY].h;
    memcpy(pl, hb + L.pl, n_rows * (MAX_PLOIDY + 1) * sizeof *pl); memcpy(raw, hb + L.raw, n_rows * 2 * sizeof *raw);
    memcpy(gt, hb + L.gt, n_rows); memcpy(genotyped, hb + L.flags, n_rows); memcpy(boundary, hb + L.boundary, n_rows);
    return 0;
}

// Insertions that share a position, genotyped together (svjg.h), through genotype_leg by ONE leg, sites_call: svjg_genotype_sites in BLOCK_SITES
// (k_genotype_sites on the count vector) and svjg_genotype_cohort_sites in BLOCK_COHORT_SITES (k_genotype_cohort_sites on the cohort matrix; it reads
// nothing else of the context), and svjg_genotype_cohort_sites_prior in BLOCK_COHORT_SITES_PRIOR (the same kernel with k_cohort_sites_prior enqueued
// behind it: launch_sites_prior).  launch_sites: all items with the table at hand.  The cohort's site words lie right in front of the max_n pair
// (sites_layout): ONE memset zeroes both in front of EVERY launch, as launch_cohort's.  Blocks: capped_grid(n_sites) for the single-sample kernel;
// the cohort kernel takes 104 VGPRs (the compiler's resource remark), so a SIMD holds 512 / 104 = four of its waves and a unit four
// blocks of four waves; the rest in strides of the grid.
constexpr uint64_t COHORT_SITES_WAVES = 4;
static int launch_sites(svjg_ctx *c, GenoCohortSitesArgs &p, bool cohort) {
    GenoSitesArgs &a = p.g;
    a.logfact = c->d_logfact; a.logfact_n = c->logfact_n;
    if (cohort) {
        HIPCHK(c, hipMemsetAsync(p.site, 0, a.n_sites * MAX_SITE_ALTS * 8 + 8, c->stream));
        const uint64_t n_items = a.n_sites * p.n_samples, blocks = (n_items + TPB - 1) / TPB, cap = (uint64_t)c->n_cu * COHORT_SITES_WAVES;
        hipLaunchKernelGGL(k_genotype_cohort_sites, dim3((uint32_t)(blocks < cap ? blocks : cap)), dim3(TPB), 0, c->stream, p);
    } else {
        HIPCHK(c, hipMemsetAsync(a.max_n, 0, 8, c->stream));
        hipLaunchKernelGGL(k_genotype_sites, dim3(capped_grid(a.n_sites)), dim3(TPB), 0, c->stream, a);
    }
    HIPCHK(c, hipGetLastError());
    return 0;
}

// k_cohort_sites_prior on what the cohort sites kernel left in the block.  Blocks of SITES_PRIOR_TPB = two waves, a site a segment of a wave
// (svjg_geno.h: segment_grid).
static int launch_sites_prior(svjg_ctx *c, CohortSitesPriorArgs &p) {
    const uint32_t grid = segment_grid(p.n_sites, p.n_samples, SITES_PRIOR_TPB, (uint32_t)c->n_cu, SITES_PRIOR_BLOCKS_PER_CU);
    hipLaunchKernelGGL(k_cohort_sites_prior, dim3(grid), dim3(SITES_PRIOR_TPB), 0, c->stream, p);
    HIPCHK(c, hipGetLastError());
    return 0;
}

// what a caller can get wrong about its sites: 2..MAX_SITE_ALTS slots below n_slots, no hole, none twice
static int check_sites(svjg_ctx *c, const uint32_t *slots, uint64_t n_sites, uint32_t n_slots) {
    for (uint64_t s = 0; s < n_sites; ++s) {
        const uint32_t *m = slots + s * MAX_SITE_ALTS;
        uint32_t K = 0;
        for (uint32_t j = 0; j < MAX_SITE_ALTS; ++j) {
            if (m[j] == NONE32) continue;
            if (j != K) { c->err = "site with a hole in front of a member"; return SVJG_E_ARG; }
            if (m[j] >= n_slots) { c->err = "slot out of range"; return SVJG_E_ARG; }
            for (uint32_t i = 0; i < j; ++i) if (m[i] == m[j]) { c->err = "slot twice in one site"; return SVJG_E_ARG; }
            ++K;
        }
        if (K < 2) { c->err = "site with fewer than two members"; return SVJG_E_ARG; }
    }
    return 0;
}

// The host leg of both: the checks of the call's kind (all of them before any launch), the call's logarithms by the host's libm and the sites' slots in, the kernel of the call's kind, the copy out.  members, site: the cohort's only.
static int sites_call(svjg_ctx *c, int block, const uint32_t *slots, uint64_t n_sites, uint32_t min_support, double err,
                      uint8_t *gt, int64_t *pl, uint32_t *raw, uint8_t *members, uint8_t *boundary, uint32_t *site,
                      uint8_t *sgt = nullptr, uint8_t *sgq = nullptr, double *af = nullptr, uint32_t *em_steps = nullptr, uint32_t *psite = nullptr) {
    static_assert(SVJG_MAX_SITE_ALTS == MAX_SITE_ALTS && SVJG_SITE_GENOTYPES == SITE_GENOTYPES, "svjg.h and svjg_geno.h disagree");
    const bool prior = block == BLOCK_COHORT_SITES_PRIOR, cohort = prior || block == BLOCK_COHORT_SITES;   // (prior: k_cohort_sites_prior behind the cohort kernel, in a block of its own)
    if (!c || (!cohort && !c->have_counts)) return SVJG_E_ARG;
    if (cohort && !c->d_cm) { c->err = "no cohort matrix"; return SVJG_E_ARG; }
    if (n_sites == 0) return 0;
    if (!slots || !gt || !pl || !raw || !boundary || (cohort && (!members || !site)) || (prior && (!sgt || !sgq || !af || !em_steps || !psite))) { if (cohort) c->err = "a null array"; return SVJG_E_ARG; }
    const uint64_t S = cohort ? c->cohort_samples : 1;
    if (cohort && n_sites > (1ull << 40) / S) { c->err = "too many items for one call: genotype the sites in chunks"; return SVJG_E_ARG; }
    if (const int rc0 = check_sites(c, slots, n_sites, cohort ? c->cohort_slots : c->n_slots)) return rc0;
    HIPCHK(c, hipSetDevice(c->device));
    if (!cohort) { const int rc0 = fetch_slot_counts(c); if (rc0) return rc0; }
    const SitesLayout L = sites_layout(n_sites, S, cohort, prior);
    const int rc = genotype_leg(c, c->leg[block], L,
        [&](uint8_t *hb) { site_log_table(err, (double *)(hb + L.logs)); memcpy(hb + L.slots, slots, n_sites * MAX_SITE_ALTS * 4); },
        [&](uint8_t *base) {
            GenoCohortSitesArgs p{};
            GenoSitesArgs &a = p.g;
            a.counts = cohort ? c->cm() : c->graph.counts; a.n_slots = cohort ? c->cohort_slots : c->n_slots;
            a.slots = (const uint32_t *)(base + L.slots); a.n_sites = n_sites; a.min_support = min_support; a.logs = (const double *)(base + L.logs);
            a.pl = (int64_t *)(base + L.pl); a.raw = (uint32_t *)(base + L.raw); a.gt = base + L.gt; a.boundary = base + L.boundary;
            a.max_n = (unsigned int *)(base + L.maxn);
            p.present = c->d_cpresent; p.n_samples = (uint32_t)S; p.members = base + L.members; p.site = (unsigned long long *)(base + L.site);
            if (const int rc1 = launch_sites(c, p, cohort)) return rc1;
            if (!prior) return 0;
            CohortSitesPriorArgs q{a.raw, p.members, a.slots, a.logs, n_sites, (uint32_t)S, min_support,
                                   base + L.sgt, base + L.sgq, (double *)(base + L.af), (uint32_t *)(base + L.steps), (uint32_t *)(base + L.psite)};
            return launch_sites_prior(c, q);
        });
    if (rc) return rc;
    const uint8_t *hb = c->leg[block].h;
    const uint64_t n = n_sites * S;
    memcpy(pl, hb + L.pl, n * SITE_GENOTYPES * sizeof *pl); memcpy(raw, hb + L.raw, n * (MAX_SITE_ALTS + 1) * sizeof *raw);
    memcpy(gt, hb + L.gt, n * 2); memcpy(boundary, hb + L.boundary, n);
    if (cohort) { memcpy(members, hb + L.members, n); memcpy(site, hb + L.site, n_sites * MAX_SITE_ALTS * 8); }   // (NS_j, AC_j: the two halves of the kernel's one word a candidate)
    if (prior) {
        memcpy(sgt, hb + L.sgt, n * 2); memcpy(sgq, hb + L.sgq, n); memcpy(af, hb + L.af, n_sites * SITE_ALLELES * sizeof *af);
        memcpy(em_steps, hb + L.steps, n_sites * sizeof *em_steps); memcpy(psite, hb + L.psite, n_sites * MAX_SITE_ALTS * 2 * sizeof *psite);
    }
    return 0;
}

extern "C" int svjg_genotype_sites(svjg_ctx *c, const uint32_t *slots, uint64_t n_sites, uint32_t min_support, double err,
                                   uint8_t *gt, int64_t *pl, uint32_t *raw, uint8_t *boundary) {
    return sites_call(c, BLOCK_SITES, slots, n_sites, min_support, err, gt, pl, raw, nullptr, boundary, nullptr);
}

extern "C" int svjg_genotype_cohort_sites(svjg_ctx *c, const uint32_t *slots, uint64_t n_sites, uint32_t min_support, double err,
                                          uint8_t *gt, int64_t *pl, uint32_t *raw, uint8_t *members, uint8_t *boundary, uint32_t *site) {
    return sites_call(c, BLOCK_COHORT_SITES, slots, n_sites, min_support, err, gt, pl, raw, members, boundary, site);
}

extern "C" int svjg_genotype_cohort_sites_prior(svjg_ctx *c, const uint32_t *slots, uint64_t n_sites, uint32_t min_support, double err,
                                                uint8_t *gt, int64_t *pl, uint32_t *raw, uint8_t *members, uint8_t *boundary, uint32_t *site,
                                                uint8_t *sgt, uint8_t *sgq, double *af, uint32_t *em_steps, uint32_t *psite) {
    return sites_call(c, BLOCK_COHORT_SITES_PRIOR, slots, n_sites, min_support, err, gt, pl, raw, members, boundary, site, sgt, sgq, af, em_steps, psite);
}

// ---- cohort: many samples' counts against one row set (svjg.h) -------------------------------------------------------------
// The matrix is slot-major (cm[slot * S + s]) so that k_genotype_cohort, whose neighbouring lanes are neighbouring samples of one row, reads
// the counts and the presence bytes coalesced.  A sample's column goes in and out through a dense vector and a small transposing kernel.
extern "C" int svjg_cohort_alloc(svjg_ctx *c, uint32_t n_samples, uint32_t n_slots) {
    if (!c) return SVJG_E_ARG;
    if (n_samples == 0) { c->err = "a cohort has at least one sample"; return SVJG_E_ARG; }
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    c->d_cm.release(); c->d_cpresent = nullptr; c->cohort_samples = c->cohort_slots = 0;
    const uint64_t n = (uint64_t)n_samples * n_slots;             // (< 2^64; times nine it is below 2^68: checked)
    if (n > (1ull << 60) || c->d_cm.reserve(n * 9 + 8) != hipSuccess) { (void)hipGetLastError(); c->err = "no memory for the cohort matrix"; return SVJG_E_NOMEM; }
    c->d_cpresent = c->d_cm + n * 8;
    c->cohort_samples = n_samples; c->cohort_slots = n_slots;
    HIPCHK(c, hipMemsetAsync(c->d_cm, 0, n * 9 + 8, c->stream));
    return 0;
}

// the staging vector of one column: [ counts 8 | present 1 ] x n_slots
static int cohort_stage(svjg_ctx *c) { return ensure(c, c->d_cstage, (uint64_t)c->cohort_slots * 9 + 16, false); }

extern "C" int svjg_cohort_set_counts(svjg_ctx *c, uint32_t sample, const uint32_t *slots, const uint32_t *counts, uint64_t n) {
    if (!c) return SVJG_E_ARG;
    if (!c->d_cm) { c->err = "no cohort matrix"; return SVJG_E_ARG; }
    if (sample >= c->cohort_samples) { c->err = "sample out of range"; return SVJG_E_ARG; }
    if (n && (!slots || !counts)) return SVJG_E_ARG;
    const uint32_t ns = c->cohort_slots;
    std::vector<unsigned long long> col((size_t)ns + 1, 0ull);
    std::vector<uint8_t> pres((size_t)ns + 1, 0);
    for (uint64_t k = 0; k < n; ++k) {
        const uint32_t sl = slots[k];
        if (sl >= ns) { c->err = "slot out of range"; return SVJG_E_ARG; }
        if (pres[sl]) { c->err = "slot named twice"; return SVJG_E_ARG; }
        pres[sl] = 1;
        col[sl] = (unsigned long long)counts[2 * k] | ((unsigned long long)counts[2 * k + 1] << 32);
    }
    HIPCHK(c, hipSetDevice(c->device));
    if (ns == 0) return 0;
    if (const int rc = cohort_stage(c)) return rc;
    unsigned long long *d_col = (unsigned long long *)c->d_cstage.p; uint8_t *d_pres = c->d_cstage + (uint64_t)ns * 8;
    HIPCHK(c, hipMemcpyAsync(d_col, col.data(), (uint64_t)ns * 8, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(d_pres, pres.data(), ns, hipMemcpyHostToDevice, c->stream));
    hipLaunchKernelGGL(k_cohort_store, dim3(capped_grid(ns)), dim3(TPB), 0, c->stream, c->cm(), c->d_cpresent, c->cohort_samples, sample, d_col, d_pres, ns);
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipStreamSynchronize(c->stream));                   // `col` and `pres` are locals
    return 0;
}

extern "C" int svjg_cohort_store_counts(svjg_ctx *c, uint32_t sample) {
    if (!c) return SVJG_E_ARG;
    if (!c->d_cm) { c->err = "no cohort matrix"; return SVJG_E_ARG; }
    if (sample >= c->cohort_samples) { c->err = "sample out of range"; return SVJG_E_ARG; }
    if (!c->have_counts || c->n_slots != c->cohort_slots) { c->err = "the count vector and the cohort matrix differ in their slots"; return SVJG_E_ARG; }
    HIPCHK(c, hipSetDevice(c->device));
    { const int rc0 = fetch_slot_counts(c); if (rc0) return rc0; }
    if (c->n_slots == 0) return 0;
    hipLaunchKernelGGL(k_cohort_store, dim3(capped_grid(c->n_slots)), dim3(TPB), 0, c->stream, c->cm(), c->d_cpresent, c->cohort_samples, sample,
                       (const unsigned long long *)c->graph.counts, (const uint8_t *)nullptr, c->n_slots);
    HIPCHK(c, hipGetLastError());
    return 0;
}

extern "C" int svjg_cohort_get_counts(svjg_ctx *c, uint32_t sample, uint32_t *out, uint8_t *present, uint32_t n_slots) {
    if (!c) return SVJG_E_ARG;
    if (!c->d_cm) { c->err = "no cohort matrix"; return SVJG_E_ARG; }
    if (sample >= c->cohort_samples) { c->err = "sample out of range"; return SVJG_E_ARG; }
    if (n_slots != c->cohort_slots || (n_slots && (!out || !present))) return SVJG_E_ARG;
    HIPCHK(c, hipSetDevice(c->device));
    if (n_slots == 0) return 0;
    if (const int rc = cohort_stage(c)) return rc;
    unsigned long long *d_col = (unsigned long long *)c->d_cstage.p; uint8_t *d_pres = c->d_cstage + (uint64_t)n_slots * 8;
    hipLaunchKernelGGL(k_cohort_load, dim3(capped_grid(n_slots)), dim3(TPB), 0, c->stream, (const unsigned long long *)c->cm(), (const uint8_t *)c->d_cpresent,
                       c->cohort_samples, sample, d_col, d_pres, n_slots);
    HIPCHK(c, hipGetLastError());
    std::vector<unsigned long long> tmp(n_slots);
    HIPCHK(c, hipMemcpyAsync(tmp.data(), d_col, (uint64_t)n_slots * 8, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipMemcpyAsync(present, d_pres, n_slots, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    for (uint32_t i = 0; i < n_slots; ++i) { out[2 * i] = (uint32_t)tmp[i]; out[2 * i + 1] = (uint32_t)(tmp[i] >> 32); }
    return 0;
}

// The three cohort calls go through genotype_leg, each in its own block (svjg.h: a call does not disturb another's), by ONE leg: cohort_call.
// launch_cohort: all items with the table at hand.  The site words lie right in front of the max_n pair (cohort_layout): both are zeroed in front
// of EVERY launch — settle_launch runs the kernel over all items again after the table grew, and the atomics would add to the first launch's sums.
// Blocks: a block is four waves, one per SIMD, and a SIMD holds min(8, 512 / VGPRs) waves of a kernel: eight of k_genotype_cohort (64 VGPRs:
// svjg.h), five of k_genotype_cohort_ploidy (96 VGPRs: the compiler's resource remark); the rest in strides of the grid.
constexpr uint64_t COHORT_PLOIDY_WAVES = 5;
static int launch_cohort(svjg_ctx *c, GenoCohortArgs &p, bool per_item) {
    p.g.logfact = c->d_logfact; p.g.logfact_n = c->logfact_n;
    HIPCHK(c, hipMemsetAsync(p.site, 0, p.g.n_rows * (per_item ? 16 : 8) + 8, c->stream));
    const uint64_t n_items = p.g.n_rows * p.n_samples, blocks = (n_items + TPB - 1) / TPB, cap = (uint64_t)c->n_cu * (per_item ? COHORT_PLOIDY_WAVES : 8);
    const dim3 grid((uint32_t)(blocks < cap ? blocks : cap));
    if (per_item) hipLaunchKernelGGL(k_genotype_cohort_ploidy, grid, dim3(TPB), 0, c->stream, p);
    else hipLaunchKernelGGL(k_genotype_cohort, grid, dim3(TPB), 0, c->stream, p);
    HIPCHK(c, hipGetLastError());
    return 0;
}

// k_cohort_prior on what the cohort kernel left in the block.  Blocks of four waves, a row a segment of a wave (svjg_geno.h: segment_grid).
constexpr bool PRIOR_STAGE_DEFAULT = true;                          // measured: see k_cohort_prior
static int launch_cohort_prior(svjg_ctx *c, CohortPriorArgs &p) {
    const char *e = getenv("SVJG_PRIOR_STAGE");                   // "lds" / "recompute": the other way for the items beyond a lane's first (tools/cohort_prior_timing.py)
    const uint64_t further = (p.n_samples + 63) / 64 - 1;
    p.staged = PRIOR_STAGE_DEFAULT ? (uint32_t)(further < PRIOR_STAGE_MAX ? further : PRIOR_STAGE_MAX) : 0u;
    if (e && !strcmp(e, "recompute")) p.staged = 0;
    if (e && !strcmp(e, "lds")) p.staged = (uint32_t)(further < PRIOR_STAGE_MAX ? further : PRIOR_STAGE_MAX);
    const uint32_t grid = segment_grid(p.n_rows, p.n_samples, TPB, (uint32_t)c->n_cu, PRIOR_BLOCKS_PER_CU);
    hipLaunchKernelGGL(k_cohort_prior, dim3(grid), dim3(TPB), prior_stage_bytes(p.staged, TPB), c->stream, p);
    HIPCHK(c, hipGetLastError());
    return 0;
}

// max_ploidy of a cohort call (cohort_call, svjg_cohort_qual): in range, and 2 where no array says otherwise; no item's ploidy above it
static int check_max_ploidy(svjg_ctx *c, const uint8_t *ploidy, uint32_t max_ploidy) {
    if (max_ploidy < 1 || max_ploidy > MAX_PLOIDY) { c->err = "max_ploidy is not in 1..SVJG_MAX_PLOIDY"; return SVJG_E_ARG; }
    if (!ploidy && max_ploidy != 2) { c->err = "without a ploidy array every item is diploid: max_ploidy must be 2"; return SVJG_E_ARG; }
    return 0;
}
static int check_item_ploidy(svjg_ctx *c, const uint8_t *ploidy, uint64_t n, uint32_t max_ploidy) {
    for (uint64_t i = 0; ploidy && i < n; ++i)
        if (ploidy[i] > max_ploidy) { c->err = "ploidy above max_ploidy"; return SVJG_E_ARG; }
    return 0;
}

// The host leg of svjg_genotype_cohort (block BLOCK_COHORT: ploidy NULL, max_ploidy 2), svjg_genotype_cohort_ploidy (BLOCK_COHORT_PLOIDY: a
// ploidy per item) and svjg_genotype_cohort_prior (BLOCK_COHORT_PRIOR: ploidy or NULL, gq / af / em_steps): the checks, the call's logarithms
// (by the host's libm, as geno_args' three) and ploidy bytes in with the three input arrays, the cohort kernel of the call's kind — the table's
// grow-and-rerun is the leg's — with k_cohort_prior behind it, the copy out.  site: NS, AC (BLOCK_COHORT) or NS, AN, AC per row.
static int cohort_call(svjg_ctx *c, int block, const uint8_t *sv_type, const uint32_t *slot, const uint8_t *ok, const uint8_t *ploidy, uint32_t max_ploidy,
                       uint64_t n_rows, uint32_t min_support, double err, uint8_t *gt, int64_t *pl, uint32_t *raw, uint8_t *genotyped, uint8_t *boundary,
                       uint32_t *site, uint8_t *gq, double *af, uint32_t *em_steps) {
    const bool prior = block == BLOCK_COHORT_PRIOR, per_item = ploidy != nullptr;
    if (!c) return SVJG_E_ARG;
    if (!c->d_cm) { c->err = "no cohort matrix"; return SVJG_E_ARG; }
    if (n_rows == 0) return 0;
    if (!sv_type || !slot || !ok || (!ploidy && block == BLOCK_COHORT_PLOIDY) || !gt || !pl || !raw || !genotyped || !boundary || !site ||
        (prior && (!gq || !af || !em_steps))) { c->err = "a null array"; return SVJG_E_ARG; }
    if (const int rc0 = check_max_ploidy(c, ploidy, max_ploidy)) return rc0;
    const uint64_t S = c->cohort_samples;
    if (block != BLOCK_COHORT && S >= (1ull << 28)) { c->err = "too many samples: AN would not fit 32 bits"; return SVJG_E_ARG; }
    if (n_rows > (1ull << 40) / S) { c->err = "too many items for one call: genotype the rows in chunks"; return SVJG_E_ARG; }
    const uint64_t n = n_rows * S;
    if (const int rc0 = check_item_ploidy(c, ploidy, n, max_ploidy)) return rc0;
    HIPCHK(c, hipSetDevice(c->device));
    const CohortLayout L = cohort_layout(n_rows, S, max_ploidy, per_item, prior);
    const int rc = genotype_leg(c, c->leg[block], L,
        [&](uint8_t *hb) {
            if (per_item || prior) ploidy_log_table(err, (double *)(hb + L.logtab));
            stage_rows(hb, L.in, sv_type, slot, ok, n_rows);
            if (ploidy) memcpy(hb + L.ploidy, ploidy, n);
        },
        [&](uint8_t *base) {
            GenoCohortArgs g{block_geno_args(c, c->cm(), base, L, n_rows, min_support, err), c->d_cpresent, c->cohort_samples, (unsigned long long *)(base + L.site),
                             base + L.ploidy, (const double *)(base + L.logtab), max_ploidy};
            g.g.n_slots = c->cohort_slots;                        // (the matrix's slots, not the count vector's)
            if (const int rc1 = launch_cohort(c, g, per_item)) return rc1;
            if (!prior) return 0;
            CohortPriorArgs p{(const uint32_t *)(base + L.raw), base + L.flags, ploidy ? base + L.ploidy : nullptr, base + L.in.type,
                              (const double *)(base + L.logtab), n_rows, c->cohort_samples, min_support,
                              base + L.gt, base + L.gq, (double *)(base + L.af), (uint32_t *)(base + L.steps), (uint32_t *)(base + L.psite), 0u};
            return launch_cohort_prior(c, p);
        });
    if (rc) return rc;
    const uint8_t *hb = c->leg[block].h;
    memcpy(pl, hb + L.pl, n * (max_ploidy + 1) * sizeof *pl); memcpy(raw, hb + L.raw, n * 2 * sizeof *raw);
    memcpy(gt, hb + L.gt, n); memcpy(genotyped, hb + L.flags, n); memcpy(boundary, hb + L.boundary, n);
    if (prior) {
        memcpy(gq, hb + L.gq, n); memcpy(af, hb + L.af, n_rows * sizeof *af); memcpy(em_steps, hb + L.steps, n_rows * sizeof *em_steps);
        memcpy(site, hb + L.psite, n_rows * 3 * sizeof *site);
    } else if (per_item) {
        const uint64_t *w = (const uint64_t *)(hb + L.site);      // the kernel's two words a row: NS | AC << 32, AN
        for (uint64_t r = 0; r < n_rows; ++r) { site[r * 3] = (uint32_t)w[r * 2]; site[r * 3 + 1] = (uint32_t)w[r * 2 + 1]; site[r * 3 + 2] = (uint32_t)(w[r * 2] >> 32); }
    } else memcpy(site, hb + L.site, n_rows * 8);                 // NS, AC: the two halves of the kernel's one word a row
    return 0;
}

extern "C" int svjg_genotype_cohort(svjg_ctx *c, const uint8_t *sv_type, const uint32_t *slot, const uint8_t *ok, uint64_t n_rows,
                                    uint32_t min_support, double err, uint8_t *gt, int64_t *pl, uint32_t *raw, uint8_t *genotyped,
                                    uint8_t *boundary, uint32_t *site) {
    return cohort_call(c, BLOCK_COHORT, sv_type, slot, ok, nullptr, 2, n_rows, min_support, err, gt, pl, raw, genotyped, boundary, site, nullptr, nullptr, nullptr);
}

extern "C" int svjg_genotype_cohort_ploidy(svjg_ctx *c, const uint8_t *sv_type, const uint32_t *slot, const uint8_t *ok, const uint8_t *ploidy,
                                           uint32_t max_ploidy, uint64_t n_rows, uint32_t min_support, double err, uint8_t *gt, int64_t *pl,
                                           uint32_t *raw, uint8_t *genotyped, uint8_t *boundary, uint32_t *site) {
    return cohort_call(c, BLOCK_COHORT_PLOIDY, sv_type, slot, ok, ploidy, max_ploidy, n_rows, min_support, err, gt, pl, raw, genotyped, boundary, site, nullptr, nullptr, nullptr);
}

extern "C" int svjg_genotype_cohort_prior(svjg_ctx *c, const uint8_t *sv_type, const uint32_t *slot, const uint8_t *ok, const uint8_t *ploidy,
                                          uint32_t max_ploidy, uint64_t n_rows, uint32_t min_support, double err, uint8_t *gt, int64_t *pl,
                                          uint32_t *raw, uint8_t *genotyped, uint8_t *boundary, uint32_t *site, uint8_t *gq, double *af,
                                          uint32_t *em_steps) {
    return cohort_call(c, BLOCK_COHORT_PRIOR, sv_type, slot, ok, ploidy, max_ploidy, n_rows, min_support, err, gt, pl, raw, genotyped, boundary, site, gq, af, em_steps);
}

// ---- cohort site quality (svjg.h: svjg_cohort_qual; the model: svjg_geno.h) ----
// Through genotype_leg in BLOCK_COHORT_QUAL, a block of its own: the call's logarithms, the harmonic numbers H_0..H_m_max (both by the host, in
// doubles) and the ploidy bytes go in with the three input arrays; k_cohort_qual; qual, mlac and chroms come out.  The kernel reads no log10(i!)
// table and never asks for a larger one (the leg builds the first one for a context without, as for every call): the max_n pair carries the gate's
// "slot out of range" word only.  Blocks: one wave each; a unit holds
// what its LDS admits (160 KiB over the block's request, qual_lds_bytes + the 720 bytes of the staged logarithms), its registers (118 VGPRs: four
// waves a SIMD, 16 a unit) and the 32-wave cap; the rest in strides of the grid.  A request beyond 64 KiB (m_max > 4050) is announced to the
// runtime first.
constexpr uint64_t QUAL_WAVES_PER_CU = 16;
static int launch_cohort_qual(svjg_ctx *c, CohortQualArgs &p) {
    HIPCHK(c, hipMemsetAsync(p.g.max_n, 0, 8, c->stream));
    const uint32_t lds = qual_lds_bytes(p.m_max);
    if (lds + 2 * PLOIDY_TAB * 8 > 65536) HIPCHK(c, hipFuncSetAttribute((const void *)k_cohort_qual, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    const uint64_t fit = (160u * 1024u) / (lds + 2 * PLOIDY_TAB * 8), per_cu = fit < QUAL_WAVES_PER_CU ? (fit ? fit : 1) : QUAL_WAVES_PER_CU;
    const uint64_t cap = (uint64_t)c->n_cu * per_cu;
    hipLaunchKernelGGL(k_cohort_qual, dim3((uint32_t)(p.g.n_rows < cap ? p.g.n_rows : cap)), dim3(QUAL_TPB), lds, c->stream, p);
    HIPCHK(c, hipGetLastError());
    return 0;
}

extern "C" int svjg_cohort_qual(svjg_ctx *c, const uint8_t *sv_type, const uint32_t *slot, const uint8_t *ok, const uint8_t *ploidy, uint32_t max_ploidy,
                                uint64_t n_rows, double err, double theta, double *qual, uint32_t *mlac, uint32_t *chroms) {
    if (!c) return SVJG_E_ARG;
    if (!c->d_cm) { c->err = "no cohort matrix"; return SVJG_E_ARG; }
    if (n_rows == 0) return 0;
    if (!sv_type || !slot || !ok || !qual || !mlac || !chroms) { c->err = "a null array"; return SVJG_E_ARG; }
    if (const int rc0 = check_max_ploidy(c, ploidy, max_ploidy)) return rc0;
    const uint64_t S = c->cohort_samples;
    static_assert(SVJG_QUAL_MAX_CHROMS == QUAL_MAX_CHROMS, "svjg.h and svjg_geno.h disagree");
    if (S * max_ploidy > QUAL_MAX_CHROMS) { c->err = "too many chromosomes for the site quality: n_samples * max_ploidy is above SVJG_QUAL_MAX_CHROMS = 4096"; return SVJG_E_ARG; }
    if (!(theta > 0.0 && theta <= QUAL_THETA_MAX)) { c->err = "theta is not in (0, 0.05]"; return SVJG_E_ARG; }
    if (n_rows > (1ull << 40) / S) { c->err = "too many items for one call: take the rows in chunks"; return SVJG_E_ARG; }
    const uint64_t n = n_rows * S;
    if (const int rc0 = check_item_ploidy(c, ploidy, n, max_ploidy)) return rc0;
    HIPCHK(c, hipSetDevice(c->device));
    const uint32_t m_max = (uint32_t)(S * max_ploidy);
    const QualLayout L = qual_layout(n_rows, S, m_max, ploidy != nullptr);
    const int rc = genotype_leg(c, c->leg[BLOCK_COHORT_QUAL], L,
        [&](uint8_t *hb) {
            ploidy_log_table(err, (double *)(hb + L.logtab));
            qual_harmonic(m_max, (double *)(hb + L.harm));
            stage_rows(hb, L.in, sv_type, slot, ok, n_rows);
            if (ploidy) memcpy(hb + L.ploidy, ploidy, n);
        },
        [&](uint8_t *base) {
            CohortQualArgs p{geno_args(c, c->cm(), base, L.in, n_rows, 0, err), c->d_cpresent, c->cohort_samples, ploidy ? base + L.ploidy : nullptr,
                             (const double *)(base + L.logtab), (const double *)(base + L.harm), max_ploidy, m_max, qual_rescale_every(m_max, max_ploidy), theta,
                             (double *)(base + L.qual), (uint32_t *)(base + L.mlac), (uint32_t *)(base + L.chroms)};
            p.g.n_slots = c->cohort_slots;                        // (the matrix's slots, not the count vector's)
            p.g.max_n = (unsigned int *)(base + L.maxn);
            return launch_cohort_qual(c, p);
        });
    if (rc) return rc;
    const uint8_t *hb = c->leg[BLOCK_COHORT_QUAL].h;
    memcpy(qual, hb + L.qual, n_rows * sizeof *qual); memcpy(mlac, hb + L.mlac, n_rows * sizeof *mlac); memcpy(chroms, hb + L.chroms, n_rows * sizeof *chroms);
    return 0;
}

// ---- the calls that take the run's calls, gt[n_rows, S] and ploidy[n_rows, S] or NULL (svjg_cohort_qc, svjg_cohort_hwe) ----
// They read neither the cohort matrix nor the count vector, and their max_n pair stays zero: the leg never runs their kernels twice.  check_calls: their checks, in this order
// (max_samples with limit_err, and rows_err: the call's own; arrays: gt and the call's outputs are there).  calls_leg: genotype_leg in the call's own block, laid out by L
// (a CallsIn: calls_in); the n = n_rows * S call bytes (and the ploidy bytes) go in.
static int check_calls(svjg_ctx *c, uint64_t S, uint64_t max_samples, const char *limit_err, bool arrays, uint64_t n_rows, const char *rows_err) {
    if (S == 0) { c->err = "no sample"; return SVJG_E_ARG; }
    if (S > max_samples) { c->err = limit_err; return SVJG_E_ARG; }
    if (!arrays) { c->err = "a null array"; return SVJG_E_ARG; }
    if (n_rows >= (1ull << 32)) { c->err = rows_err; return SVJG_E_ARG; }
    if (n_rows > (1ull << 40) / S) { c->err = "too many items for one call: take the rows in chunks"; return SVJG_E_ARG; }
    return 0;
}
template <class Layout, class Launch>
static int calls_leg(svjg_ctx *c, int block, const Layout &L, const uint8_t *gt, const uint8_t *ploidy, uint64_t n, Launch launch) {
    HIPCHK(c, hipSetDevice(c->device));
    return genotype_leg(c, c->leg[block], L, [&](uint8_t *hb) { stage_calls(hb, L, gt, ploidy, n); }, launch);
}

// ---- cohort sample QC (svjg.h: svjg_cohort_qc; the model, the planes and the tiles: svjg_geno.h) ----
// Through calls_leg in BLOCK_COHORT_QC: ONE memset zeroes sample[] and the max_n pair behind it; k_qc_planes over the units, k_qc_pairs over the
// tiles (S >= 2), both in strides of a grid of at most QC_BLOCKS_PER_CU blocks a unit (svjg_geno.h); pair[] and sample[] come out.  Neither
// kernel reads the log10(i!) table.
static int launch_cohort_qc(svjg_ctx *c, const QcArgs &p) {
    HIPCHK(c, hipMemsetAsync(p.sample, 0, (uint64_t)p.S * 4 * QC_CLASSES + 8, c->stream));      // (the max_n pair lies right behind sample[]: qc_layout)
    const uint64_t cap = (uint64_t)c->n_cu * QC_BLOCKS_PER_CU, blocks = (qc_plane_units(p.n_words, p.S) + TPB - 1) / TPB;
    hipLaunchKernelGGL(k_qc_planes, dim3((uint32_t)(blocks < cap ? blocks : cap)), dim3(TPB), 0, c->stream, p);
    HIPCHK(c, hipGetLastError());
    const uint64_t tiles = qc_tiles(p.S);
    if (tiles) {
        hipLaunchKernelGGL(k_qc_pairs, dim3((uint32_t)(tiles < cap ? tiles : cap)), dim3(TPB), 0, c->stream, p);
        HIPCHK(c, hipGetLastError());
    }
    return 0;
}

extern "C" int svjg_cohort_qc(svjg_ctx *c, const uint8_t *gt, const uint8_t *ploidy, uint64_t n_rows, uint32_t n_samples, uint32_t *sample, uint32_t *pair) {
    if (!c) return SVJG_E_ARG;
    static_assert(SVJG_QC_MAX_SAMPLES == QC_MAX_SAMPLES, "svjg.h and svjg_geno.h disagree");
    const uint64_t S = n_samples, n_pairs = qc_pairs(S);
    if (const int rc0 = check_calls(c, S, QC_MAX_SAMPLES, "too many samples for the pair table: n_samples is above SVJG_QC_MAX_SAMPLES = 2048", gt && sample && (pair || S < 2),
                                    n_rows, "too many rows for 32-bit sums: take the rows in chunks")) return rc0;
    if (n_rows == 0) {
        memset(sample, 0, S * QC_CLASSES * sizeof *sample);
        if (n_pairs) memset(pair, 0, n_pairs * QC_PAIR_COUNTS * sizeof *pair);
        return 0;
    }
    const QcLayout L = qc_layout(n_rows, S, ploidy != nullptr);
    const int rc = calls_leg(c, BLOCK_COHORT_QC, L, gt, ploidy, n_rows * S,
        [&](uint8_t *base) {
            const QcArgs p{base + L.gt, ploidy ? base + L.ploidy : nullptr, n_rows, qc_words(n_rows), n_samples, (uint64_t *)(base + L.planes),
                           (uint32_t *)(base + L.sample), (uint32_t *)(base + L.pair)};
            return launch_cohort_qc(c, p);
        });
    if (rc) return rc;
    const uint8_t *hb = c->leg[BLOCK_COHORT_QC].h;
    memcpy(sample, hb + L.sample, S * QC_CLASSES * sizeof *sample);
    if (n_pairs) memcpy(pair, hb + L.pair, n_pairs * QC_PAIR_COUNTS * sizeof *pair);
    return 0;
}

// ---- cohort site test for Hardy-Weinberg equilibrium (svjg.h: svjg_cohort_hwe; the model and the routines: svjg_geno.h) ----
// Through calls_leg in BLOCK_COHORT_HWE: k_cohort_hwe over the rows — blocks of four waves, a row a segment of a wave (svjg_geno.h: segment_grid)
// —, p[] and counts[] come out.  The table's 2 S + 1 entries are reserved in front of the leg (svjg_logfact_reserve: the growth path of every
// caller), so the kernel meets no n beyond it and the max_n pair, zeroed here, stays zero.
static int launch_cohort_hwe(svjg_ctx *c, HweArgs &p, unsigned int *max_n) {
    p.logfact = c->d_logfact;
    HIPCHK(c, hipMemsetAsync(max_n, 0, 8, c->stream));
    hipLaunchKernelGGL(k_cohort_hwe, dim3(segment_grid(p.n_rows, p.S, TPB, (uint32_t)c->n_cu, HWE_BLOCKS_PER_CU)), dim3(TPB), 0, c->stream, p);
    HIPCHK(c, hipGetLastError());
    return 0;
}

extern "C" int svjg_cohort_hwe(svjg_ctx *c, const uint8_t *gt, const uint8_t *ploidy, uint64_t n_rows, uint32_t n_samples, uint32_t *counts, double *p) {
    if (!c) return SVJG_E_ARG;
    static_assert(SVJG_HWE_MAX_SAMPLES == HWE_MAX_SAMPLES, "svjg.h and svjg_geno.h disagree");
    const uint64_t S = n_samples;
    if (const int rc0 = check_calls(c, S, HWE_MAX_SAMPLES, "too many samples: n_samples is above SVJG_HWE_MAX_SAMPLES = 65536", gt && counts && p,
                                    n_rows, "too many rows for one call: take the rows in chunks")) return rc0;
    if (n_rows == 0) return 0;
    const uint32_t entries = 2 * n_samples + 1;          // (a context without a table gets the first one of every leg, never a smaller one)
    if (const int rc = svjg_logfact_reserve(c, entries > logfact_first() ? entries : logfact_first())) return rc;
    const HweLayout L = hwe_layout(n_rows, S, ploidy != nullptr);
    const int rc = calls_leg(c, BLOCK_COHORT_HWE, L, gt, ploidy, n_rows * S,
        [&](uint8_t *base) {
            HweArgs a{base + L.gt, ploidy ? base + L.ploidy : nullptr, n_rows, n_samples, nullptr, (uint32_t *)(base + L.counts), (double *)(base + L.p)};
            return launch_cohort_hwe(c, a, (unsigned int *)(base + L.maxn));
        });
    if (rc) return rc;
    const uint8_t *hb = c->leg[BLOCK_COHORT_HWE].h;
    memcpy(counts, hb + L.counts, n_rows * 3 * sizeof *counts); memcpy(p, hb + L.p, n_rows * 2 * sizeof *p);
    return 0;
}

// ---- the whole pass in one call, one host wait; two passes in flight ------------------------------------------------------
// svjg_set_rows leaves the VCF rows' three input arrays on the device.  svjg_run_begin enqueues a pass — back to back on the
// context's stream, no host round trip in between: zero counts, classify the resident text (the exact-path kernel takes the
// number of deferred lines from the device), the count all-reduce when the context has a communicator, genotype every row — and,
// on a second stream behind an event, the copy of the results (PLs as 32-bit integers) and of the pass's status block into pinned
// host memory.  svjg_run_end waits for the OLDEST pass in flight, checks what the host used to decide between the kernels
// (a list that overflowed, more deferred lines than one wave per line is good for, a log10(i!) table too short: the pass is then
// repeated the slow way) and hands out its results.  Up to two passes may be in flight: the results of pass k travel over PCIe
// while pass k + 1 computes.  The passes rotate through RUN_SLOTS = 3 slots (count vector, status block, result blocks): the slot
// behind the newest pass is used by no pass in flight, and the newest pass's exact-path kernel zeroes it for the pass to come.
// svjg_run_resident = begin + end.  Where a slot's results, its tail and the 64-bit PLs lie: run_layout (svjg_geno.h).

// SVJG_KERNEL_MS=events (read once): the fused pass's kernels timed by HIP events around them, as before r07
static bool kernel_ms_by_events(const svjg_ctx *c) {
    static const bool env_events = [] { const char *e = getenv("SVJG_KERNEL_MS"); return e && !strcmp(e, "events"); }();
    return env_events || c->wall_khz == 0;
}

extern "C" int svjg_set_rows(svjg_ctx *c, const uint8_t *sv_type, const uint32_t *slot, const uint8_t *ok, uint64_t n_rows) {
    if (!c || (n_rows && (!sv_type || !slot || !ok))) return SVJG_E_ARG;
    if (c->run_inflight) { c->err = "svjg_set_rows with a pass in flight"; return SVJG_E_ARG; }
    if (!c->have_counts) { c->err = "svjg_set_rows needs the count vector (svjg_load_graph / svjg_alloc_counts first)"; return SVJG_E_ARG; }
    { const int rc0 = fetch_slot_counts(c); if (rc0) return rc0; }
    HIPCHK(c, hipSetDevice(c->device));
    const RunLayout L = run_layout(n_rows);
    const RowsIn I = rows_in(n_rows);
    int rc;
    if ((rc = ensure(c, c->d_run_in, I.bytes + 64, false))) return rc;
    for (int k = 0; k < RUN_SLOTS; ++k) {
        svjg_ctx::RunSlot &r = c->run[k];
        r.clean = false;                                      // (the blocks may move)
        if ((rc = ensure(c, r.d, L.total, false))) return rc;
        HIPCHK(c, r.h.reserve(L.out_bytes, hipHostMallocMapped));
        HIPCHK(c, hipHostGetDevicePointer(&r.h_dev, r.h, 0));
        if ((rc = ensure(c, r.counts, (uint64_t)c->n_slots + GUARD_WORDS, false))) return rc;
        for (auto &e : r.ev) HIPCHK(c, e.create());
        HIPCHK(c, r.computed.create());                               // (with a time stamp: under SVJG_KERNEL_MS=events it also ends the exact-path kernel's interval)
        HIPCHK(c, r.copied.create(hipEventDisableTiming));
    }
    if (!c->copy_stream) {                                    // (the lowest priority there is: what runs on it must not take issue slots from the classify kernel)
        int least = 0, greatest = 0;
        if (hipDeviceGetStreamPriorityRange(&least, &greatest) != hipSuccess) least = 0;
        HIPCHK(c, c->copy_stream.create(hipStreamNonBlocking, least));
    }
    uint8_t *in = c->d_run_in;
    if (n_rows) {
        HIPCHK(c, hipMemcpyAsync(in + I.slot, slot, n_rows * 4, hipMemcpyHostToDevice, c->stream));
        HIPCHK(c, hipMemcpyAsync(in + I.type, sv_type, n_rows, hipMemcpyHostToDevice, c->stream));
        HIPCHK(c, hipMemcpyAsync(in + I.ok, ok, n_rows, hipMemcpyHostToDevice, c->stream));
    }
    HIPCHK(c, hipStreamSynchronize(c->stream));               // (the caller's arrays may go away)
    c->run_rows = n_rows; c->have_rows = true;
    return 0;
}

static GenoArgs run_geno_args(svjg_ctx *c, const svjg_ctx::RunSlot &r, const RunLayout &L, uint32_t min_support, double err, const unsigned long long *counts) {
    uint8_t *base = r.d, *hostb = (uint8_t *)r.h_dev;
    GenoArgs a = geno_args(c, counts, c->d_run_in, rows_in(c->run_rows), c->run_rows, min_support, err);
    a.gt = hostb + L.gt; a.pl = (int64_t *)(base + L.pl64); a.raw = (uint32_t *)(hostb + L.raw); a.genotyped = hostb + L.flags;
    a.pl32 = (int32_t *)(hostb + L.pl32); a.boundary = hostb + L.boundary; a.max_n = (unsigned int *)(base + L.maxn);
    return a;
}

// ---- svjg_run_begin's steps, in the order it takes them: what they enqueue, on which stream, is the design ----

// (a slot's count vector, status block and max_n as what a k_step_reset or a k_classify_exact zeroes)
static NextPass slot_reset_args(const svjg_ctx::RunSlot &s, const RunLayout &L, uint64_t words) {
    return NextPass{s.counts, words, (DevStatus *)((uint8_t *)s.d + L.status), (unsigned int *)((uint8_t *)s.d + L.maxn)};
}

// the slot's own lists (no pass in flight uses this slot: the host has ended the pass that last did)
static int pass_lists(svjg_ctx *c, svjg_ctx::RunSlot &r, uint64_t n) {
    const ListSizes want = lists_fused((c->gflags & SVJG_GRAPH_ALL_SLOW) != 0, n);
    if (const int rc = ensure(c, r.deferred, want.deferred, false)) return rc;
    return ensure(c, r.host, want.host, false);
}

// The pass's form and compute stream (svjg_pass.h).  Overlapped: pass k on stream k mod 2 — k_step_reset of its OWN slot in one-wave blocks
// (early: behind the main kernel of pass k - 2, beside that of pass k - 1), k_classify_main, the `computed` record, and nothing else: what
// was deferred is settled by svjg_run_end.  Otherwise, as before r11: on c->stream, k_classify_exact behind the main kernel.
static int pass_form_and_stream(svjg_ctx *c, svjg_ctx::RunSlot &r) {
    r.overlapped = pass_overlaps(c->comm != nullptr, (c->gflags & SVJG_GRAPH_ALL_SLOW) != 0, kernel_ms_by_events(c), c->last_pass_deferred);
    r.on = (r.overlapped && (c->pass_seq & 1)) ? c->stream2 : c->stream;
    ++c->pass_seq;
    r.chained = c->run_inflight > 0;
    r.inflight = false; r.settled = false; r.geno_owed = false; r.ms_settle = 0;
    if (!r.overlapped) return serial_enter(c);                    // (behind an overlapped pass on stream2: its `computed` is that stream's tail)
    if (c->first_dirty) {                                         // stream2 behind what c->stream holds beside overlapped passes (a pass in the other form, a step-by-step call)
        HIPCHK(c, hipEventRecord(c->ev_join[0], c->stream));
        HIPCHK(c, hipStreamWaitEvent(c->stream2, c->ev_join[0], 0));
        c->first_dirty = false;
    }
    if (r.on == c->stream2) c->second_busy = true;
    return 0;
}

// k_step_reset of the pass's own slot, unless the pass before has zeroed it: an overlapped pass; the first pass behind svjg_set_rows /
// svjg_load_graph, or behind a pass without text
static void pass_reset(svjg_ctx::RunSlot &r, const RunLayout &L, uint64_t words) {
    if (!r.clean) {
        const uint32_t rb = r.overlapped ? 64u : TPB;            // (one-wave blocks find room beside fourteen classify workers a CU)
        hipLaunchKernelGGL(k_step_reset, dim3(capped_grid(words, rb)), dim3(rb), 0, r.on, slot_reset_args(r, L, words));
    }
    r.clean = false;
}

#ifdef SVJG_ENDTIMES
// measurement only: how long before the launch's last worker the others ended
static int endtimes_print(svjg_ctx *c) {
    static unsigned long long d[DBG_WORDS];
    HIPCHK(c, hipMemcpy(d, c->d_dbg, sizeof d, hipMemcpyDeviceToHost));
    const unsigned long long nw = d[ENDT_N], span = c->hs().t_last - c->hs().t_first;
    const double us = c->wall_khz ? 1e3 / c->wall_khz : 0.0;
    double q[3] = {0, 0, 0};                                  // quartiles of (t_last - end), from the histogram (bucket centres)
    unsigned long long seen = 0;
    for (uint32_t b = 0, k = 0; b < ENDT_BUCKETS && k < 3; ++b)
        for (seen += d[ENDT_HIST + b]; k < 3 && seen * 4 >= nw * (k + 1) && nw; ++k) q[2 - k] = ((double)span - (b + 0.5) * ENDT_TICKS) * us;
    fprintf(stderr, "[svjg endtimes] %llu workers, launch %.1f us; a worker ended before the last one: mean %.1f us, quartiles %.1f / %.1f / %.1f us; ended in the last 20/50/100/200 us:",
            nw, span * us, nw ? ((double)span - (double)d[ENDT_SUM] / nw) * us : 0.0, q[0], q[1], q[2]);
    for (const double w : {20.0, 50.0, 100.0, 200.0}) {
        unsigned long long in = 0;
        for (uint32_t b = 0; b < ENDT_BUCKETS; ++b) if (((double)span - (b + 1.0) * ENDT_TICKS) * us < w) in += d[ENDT_HIST + b];
        fprintf(stderr, " %llu", in);
    }
    fprintf(stderr, "\n");
    return 0;
}
#endif

// k_classify_main over the whole resident text into the slot's targets; its arguments stay in r.cargs (the settle step's k_classify_exact takes
// the same).  SVJG_KERNEL_MS=events: its time from an event pair around it, as before r07 (two barrier packets a pass; for comparing the two
// clocks: svjg_last_main_ms).  Otherwise from the time stamps the kernel leaves in the pass's status block.
static int pass_main(svjg_ctx *c, svjg_ctx::RunSlot &r, const RunLayout &L, uint64_t n) {
    uint32_t grid = 0;  size_t lds = 0;
    r.cargs = ClassifyArgs{};
    if (const int rc = main_launch_setup(c, slot_targets(c, r, L), 0, n, r.base_offset, 0, r.cargs, grid, lds)) return rc;
    r.grid = grid;
#ifdef SVJG_ENDTIMES
    HIPCHK(c, hipMemsetAsync(c->d_dbg + ENDT_SUM, 0, (DBG_WORDS - ENDT_SUM) * 8, r.on));   // (one launch at a time: svjg_run_resident)
#endif
    return enqueue_main(c, r.on, r.cargs, grid, lds, r.timed_by_events ? r.ev : nullptr);
}

// Between this k_classify_main and the next pass's the compute stream carries ONE launch and ONE event record (`computed`):
//   k_classify_exact  the exact path, the number of deferred lines read on the device (launch_exact above).  So whatever a shard defers
//                     is counted before the pass's all-reduce; only a LIST that overflowed makes the pass repeat (svjg_pass.h).  The same
//                     blocks zero what the NEXT pass starts from — the count vector, status block and max_n of the slot behind this
//                     one, which no pass in flight uses: two are in flight at most, the slots are three — so the next pass launches no
//                     k_step_reset.
// Before r07 there were three launches (two exact-path kernels, k_step_reset) and three event records; the timeline of both:
// profiles/r07/experiments/pass_tail.txt.
// An OVERLAPPED pass has none of this: its stream carries k_step_reset, k_classify_main and `computed`, so that the next pass's workers —
// on the other stream — move into the slots this one's vacate; 53 760 B of LDS a block would only be there when THAT pass drains.
static int pass_exact_and_next(svjg_ctx *c, const svjg_ctx::RunSlot &r, const RunLayout &L, uint64_t words) {
    svjg_ctx::RunSlot &nxt = c->run[(c->run_head + 1) % RUN_SLOTS];
    const NextPass nx = (nxt.d && nxt.counts && nxt.counts.cap >= words) ? slot_reset_args(nxt, L, words) : NextPass{};
    if (const int rc = launch_exact(c, r.cargs, FUSED_WAVE_ROUNDS, nx)) return rc;
    nxt.clean = nx.counts != nullptr;
    return 0;
}

// The count all-reduce of this pass — every rank issues its collectives in the same order, one per pass — runs on the compute
// stream, between this pass's kernels and the next pass's: the classify kernel fills every CU (fourteen workers take 126 of a
// CU's 128 LDS granules and all the registers of two SIMDs), so a collective's workgroups find no room beside it and one queued
// on the second stream would only start when the NEXT pass's classify kernel drains — and hold back this pass's results, which
// the host waits for before it may enqueue the pass after.  (SVJG_ALLREDUCE_STREAM=second puts it there all the same: for a
// measurement on a multi-GPU box.)
static bool allreduce_on_second(const svjg_ctx *c) {
    static const bool env_second = [] { const char *e = getenv("SVJG_ALLREDUCE_STREAM"); return e && !strcmp(e, "second"); }();
    return env_second || c->allreduce_second;
}
static int pass_allreduce(svjg_ctx *c, svjg_ctx::RunSlot &r, const RunLayout &L, hipStream_t st) {
    // (the exact-path kernel's interval must not hold the collective: under a communicator it gets an end event of its own — 6 us of a
    //  multi-GPU pass, none of a one-GPU pass, whose interval `computed` ends)
    if (st == c->stream && r.had_text && r.timed_by_events) { HIPCHK(c, hipEventRecord(r.ev[2], c->stream)); r.slow_end_own = true; }
    if (const int rc = launch_guard(c, r.counts, st, (DevStatus *)((uint8_t *)r.d + L.status))) return rc;   // (guard word 2: "this rank's lists overflowed")
    ncclResult_t nr = ncclAllReduce(r.counts, r.counts, (size_t)c->n_slots + GUARD_WORDS, ncclUint64, ncclSum, c->comm, st);
    if (nr != ncclSuccess) { c->err = std::string("ncclAllReduce: ") + ncclGetErrorString(nr); return SVJG_E_RCCL; }
    HIPCHK(c, hipMemcpyAsync((uint8_t *)r.d + L.guard, r.counts + c->n_slots, GUARD_WORDS * 8, hipMemcpyDeviceToDevice, st));
    return 0;
}

// SVJG_GENO_GRID / SVJG_GENO_BLOCK: measurement only (read at every pass)
static void geno_grid_override(uint32_t &gb, uint32_t &gg) {
    if (const char *e = getenv("SVJG_GENO_BLOCK")) if (atoi(e) > 0) gb = (uint32_t)atoi(e);
    if (const char *e = getenv("SVJG_GENO_GRID")) if (atoi(e) > 0) gg = (uint32_t)atoi(e);
}
// Behind `computed`, on the second (low-priority) stream, the genotypes: one wave per CU (see k_genotype) fits beside the classify workers;
// the kernel writes its results straight into the pinned host block — they cross PCIe as they are produced —, which takes ~45 us for
// 100 k rows.  Meanwhile the compute stream already runs the next pass (that one zeroes and fills ITS count vector).
static int pass_genotypes(svjg_ctx *c, svjg_ctx::RunSlot &r, const GenoArgs &ga, uint64_t n_rows) {
    HIPCHK(c, hipEventRecord(r.ev[4], c->copy_stream));
    uint32_t gb = 64, gg = (uint32_t)c->n_cu;
    geno_grid_override(gb, gg);
    if (gb > TPB) gb = TPB;
    if ((uint64_t)gg * gb > n_rows + gb) gg = (uint32_t)((n_rows + gb - 1) / gb);
    hipLaunchKernelGGL(k_genotype, dim3(gg), dim3(gb), 0, c->copy_stream, ga);
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipEventRecord(r.ev[5], c->copy_stream));
    return 0;
}

// the pass's tail: max_n, status, guard words — one wave that writes them into the mapped host block, as k_genotype does its results (a
// hipMemcpyAsync here is the runtime's copy kernel, whose 256-thread blocks wait for the next pass's classify kernel to drain); then `copied`
static int pass_tail(svjg_ctx *c, svjg_ctx::RunSlot &r, const RunLayout &L) {
    static_assert(sizeof(DevStatus) % 8 == 0, "the tail is copied in 8-byte words");
    hipLaunchKernelGGL(k_pass_tail, dim3(1), dim3(64), 0, c->copy_stream, (unsigned long long *)((uint8_t *)r.h_dev + L.h_tail), (const unsigned long long *)r.d.p, (uint32_t)(L.tail_bytes / 8));
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipEventRecord(r.copied, c->copy_stream));
    return 0;
}

extern "C" int svjg_run_begin(svjg_ctx *c, uint64_t base_offset, uint32_t min_support, double err) {
    if (!c) return SVJG_E_ARG;
    if (!c->have_graph || !c->have_gaf) { c->err = "svjg_run_begin needs a graph and an uploaded GAF"; return SVJG_E_ARG; }
    if (!c->have_rows) { c->err = "svjg_set_rows has not been called"; return SVJG_E_ARG; }
    if (c->run_inflight >= 2) { c->err = "two passes are in flight: svjg_run_end first"; return SVJG_E_ARG; }
    HIPCHK(c, hipSetDevice(c->device));
    const uint64_t n = c->gaf_bytes, n_rows = c->run_rows, words = (uint64_t)c->n_slots + GUARD_WORDS;
    const RunLayout L = run_layout(n_rows);
    svjg_ctx::RunSlot &r = c->run[c->run_head];
    int rc;
    if ((rc = pass_lists(c, r, n))) return rc;
    if (c->logfact_n == 0 && (rc = build_logfact(c, logfact_first()))) return rc;
    if ((rc = pass_form_and_stream(c, r))) return rc;
    r.base_offset = base_offset; r.min_support = min_support; r.err = err;
    r.had_text = n != 0; r.timed_by_events = kernel_ms_by_events(c); r.slow_end_own = false;
    if (r.counts.cap < words) { c->err = "svjg_set_rows must follow svjg_load_graph"; return SVJG_E_ARG; }
    pass_reset(r, L, words);
    if (n && (rc = pass_main(c, r, L, n))) return rc;
    if (n && !r.overlapped && (rc = pass_exact_and_next(c, r, L, words))) return rc;
    const bool second = allreduce_on_second(c);
    if (c->comm && !second && (rc = pass_allreduce(c, r, L, c->stream))) return rc;
    HIPCHK(c, hipEventRecord(r.computed, r.on));
    HIPCHK(c, hipStreamWaitEvent(c->copy_stream, r.computed, 0));
    if (c->comm && second && (rc = pass_allreduce(c, r, L, c->copy_stream))) return rc;
    if (n_rows && (rc = pass_genotypes(c, r, run_geno_args(c, r, L, min_support, err, r.counts), n_rows))) return rc;
    if ((rc = pass_tail(c, r, L))) return rc;
    c->counts_in_slot = c->run_head;
    r.inflight = true;
    c->run_head = (c->run_head + 1) % RUN_SLOTS; ++c->run_inflight;
    return 0;
}

// The settle step of an overlapped pass (svjg_pass.h: pass_settles_exact), once per pass: wait for the pass's tail; if it deferred lines and its lists
// held, k_classify_exact on the pass's own deferred list into the pass's own count vector, behind its main kernel's stream (the blocks find their LDS
// when the NEXT pass's classify kernel drains), and the status block once more into the pass's pinned tail — overflow bits the exact path set (the
// list of lines for the host) included: svjg_run_end reads them there and repeats the pass.  t_first, which is kept, gives way to the launch's own
// start for the copy: ms_settle is first block in to last block out.  Called by svjg_run_end, and ahead of it by whoever asks for the pass's counts.
static int settle_pass(svjg_ctx *c, svjg_ctx::RunSlot &r) {
    if (r.settled) return 0;
    HIPCHK(c, hipEventSynchronize(r.copied));
    r.settled = true;
    const RunLayout L = run_layout(c->run_rows);
    DevStatus *d_st = (DevStatus *)((uint8_t *)r.d + L.status);
    DevStatus *h_st = (DevStatus *)((uint8_t *)r.h + L.h_tail + L.status);
    if (!r.had_text || !pass_settles_exact(c->comm != nullptr, (c->gflags & SVJG_GRAPH_ALL_SLOW) != 0, r.overlapped, h_st->overflow, h_st->n_deferred)) return 0;
    const unsigned long long t_main_first = h_st->t_first;
    HIPCHK(c, hipMemsetAsync(&d_st->t_first, 0xFF, 8, r.on));
    if (const int rc = launch_exact(c, r.cargs, FUSED_WAVE_ROUNDS, NextPass{}, r.on, &d_st->t_first)) return rc;
    HIPCHK(c, hipMemcpyAsync(h_st, d_st, sizeof(DevStatus), hipMemcpyDeviceToHost, r.on));
    HIPCHK(c, hipStreamSynchronize(r.on));
    if (c->wall_khz && h_st->t_exact > h_st->t_first) r.ms_settle = (float)(h_st->t_exact - h_st->t_first) / (float)c->wall_khz;
    h_st->t_first = t_main_first;
    r.geno_owed = true;
    return 0;
}

// ---- svjg_run_end's steps ----

// The finished pass's times.  By the device's clock: first worker's start to last worker's end, and from there to the end of the last block of
// the exact path that had work (never the all-reduce).  wall_clock64() counts at wall_khz.
static int pass_times(svjg_ctx *c, svjg_ctx::RunSlot &r) {
    c->ms_slow = 0;
    if (!r.had_text) return 0;
    const DevStatus &t = c->hs();
    const float per_tick = c->wall_khz ? 1.0f / (float)c->wall_khz : 0.0f;
    // (overlapped launches: the interval this one shares with the pass in front of it counts once — pass_main_ticks)
    c->ms_main_stamps = (float)pass_main_ticks(t.t_first, t.t_last, r.chained ? c->prev_t_last : 0) * per_tick;
    c->prev_t_last = t.t_last;
    c->ms_main_events = 0;
    c->ms_main = c->ms_main_stamps;
    if (r.geno_owed) c->ms_slow = r.ms_settle;            // (the settle step's launch, long behind t_last)
    else if (t.n_deferred && t.t_exact > t.t_last) c->ms_slow = (float)(t.t_exact - t.t_last) * per_tick;
    if (r.timed_by_events) {
        HIPCHK(c, hipEventElapsedTime(&c->ms_main_events, r.ev[0], r.ev[1]));
        c->ms_main = c->ms_main_events;
        if (t.n_deferred) HIPCHK(c, hipEventElapsedTime(&c->ms_slow, r.ev[1], r.slow_end_own ? r.ev[2] : r.computed));   // (the exact-path kernel alone: never the all-reduce)
    }
#ifdef SVJG_ENDTIMES
    if (const int rc = endtimes_print(c)) return rc;
#endif
    return 0;
}

// What the host would have decided in between: repeat the pass, let it stand, or refuse it.  `gd`: the pass's guard words (meaningful under
// a communicator: the sums over the ranks).  repeated: the pass was repeated step by step, its counts are in graph.counts.
static int pass_verdict(svjg_ctx *c, const svjg_ctx::RunSlot &r, const unsigned long long *gd, uint64_t n, bool &repeated) {
    repeated = false;
    if (pass_repeats(c->comm != nullptr, c->hs().overflow, gd[GUARD_REPEAT])) {
        // a list of this rank — or, under a communicator, of ANY rank (svjg_pass.h: the ranks decide together, so all of them issue the
        // one more all-reduce below) — was too short: the pass again, step by step (classify_range sizes the lists and
        // retries), behind whatever is enqueued already.  The all-reduce is issued even when this rank's text turns out to be malformed:
        // its peers are waiting in theirs.
        int rc;
        if ((rc = svjg_reset_counts(c))) return rc;
        rc = classify_range(c, 0, n, r.base_offset, 0);
        if (rc && rc != SVJG_E_INPUT) return rc;
        if (c->comm) { const std::string keep = c->err; const int rc2 = svjg_allreduce_counts(c); if (rc2 && !rc) return rc2; if (rc) c->err = keep; }
        if (rc) return rc;
        repeated = true;
    } else {
        c->total_deferred = c->hs().n_deferred;
        if (c->hs().err != ~0ull) return SVJG_E_INPUT;
        if (c->comm && pass_counts_overflowed(gd[GUARD_MAX_REF], gd[GUARD_MAX_ALT])) { c->err = "more than 2^32 informative alignments for one SV"; return SVJG_E_OVERFLOW; }
    }
    // (either way: lines the kernels set aside for the host are neither counted nor fatal — the caller has to know)
    if (c->hs().n_host) { c->err = "the text holds lines only the host can decide (non-ASCII digits in a decimal column: svjg_get_host_lines); classify it with svjg_classify"; return SVJG_E_ARG; }
    return 0;
}

extern "C" int svjg_run_end(svjg_ctx *c, const uint8_t **gt, const int32_t **pl, const uint32_t **raw, const uint8_t **flags, const uint8_t **boundary) {
    if (!c || !gt || !pl || !raw || !flags || !boundary) return SVJG_E_ARG;
    *gt = nullptr; *pl = nullptr; *raw = nullptr; *flags = nullptr; *boundary = nullptr;
    if (!c->run_inflight) { c->err = "no pass in flight"; return SVJG_E_ARG; }
    HIPCHK(c, hipSetDevice(c->device));
    svjg_ctx::RunSlot &r = c->run[c->run_tail];
    c->run_tail = (c->run_tail + 1) % RUN_SLOTS; --c->run_inflight;
    const uint64_t n = c->gaf_bytes, n_rows = c->run_rows;
    const RunLayout L = run_layout(n_rows);
    uint8_t *hb = (uint8_t *)r.h;
    int rc;
    HIPCHK(c, hipEventSynchronize(r.copied));                              // the pass's one host wait
    r.inflight = false;
    if ((rc = settle_pass(c, r))) return rc;                               // (an overlapped pass that deferred lines: one more; nothing if somebody asked for its counts before)
    const uint8_t *tail = hb + L.h_tail;
    c->hs() = *(const DevStatus *)(tail + L.status);
    if (r.had_text) { c->last_plan = MainPlan{r.cargs.region, r.cargs.small, r.grid}; c->last_claimed = c->hs().next_chunk; }
    if ((rc = pass_times(c, r))) return rc;
    if (n_rows) HIPCHK(c, hipEventElapsedTime(&c->ms_geno, r.ev[4], r.ev[5]));
    c->last_pass_deferred = r.had_text && c->hs().n_deferred != 0;
    c->host_lines_src = r.host; c->host_lines_cap = r.host.cap;
    bool repeated = false;
    if ((rc = pass_verdict(c, r, (const unsigned long long *)(tail + L.guard), n, repeated))) return rc;
    if (n_rows) {                                                 // the genotypes once more where they are owed: a repeated pass, a settle step, a log10(i!) table too short
        GenoArgs ga = run_geno_args(c, r, L, r.min_support, r.err, repeated ? c->graph.counts : r.counts);
        uint8_t *h_maxn = hb + L.h_tail + L.maxn;                 // (the results are already in the mapped host block: only the pair comes back)
        if ((rc = settle_launch(c, (const unsigned int *)h_maxn, h_maxn, (const uint8_t *)r.d + L.maxn, 8, repeated || r.geno_owed, [&] { return launch_genotype(c, ga); }))) return rc;
    }
    *pl = (const int32_t *)(hb + L.pl32); *raw = (const uint32_t *)(hb + L.raw); *gt = hb + L.gt; *flags = hb + L.flags; *boundary = hb + L.boundary;
    return 0;
}


extern "C" int svjg_run_resident(svjg_ctx *c, uint64_t base_offset, uint32_t min_support, double err,
                                 const uint8_t **gt, const int32_t **pl, const uint32_t **raw, const uint8_t **flags, const uint8_t **boundary) {
    if (!c || !gt || !pl || !raw || !flags || !boundary) return SVJG_E_ARG;
    if (c->run_inflight) { c->err = "svjg_run_resident with a pass in flight (svjg_run_end first)"; return SVJG_E_ARG; }
    const int rc = svjg_run_begin(c, base_offset, min_support, err);
    if (rc) return rc;
    return svjg_run_end(c, gt, pl, raw, flags, boundary);
}

// which rows of the last svjg_genotype / svjg_genotype_view call lie so close to a PL's integer boundary that the caller should
// recompute them with the reference's own arithmetic (predict-genotype.py:313: log10 of an exact big integer)
extern "C" int svjg_genotype_boundary(svjg_ctx *c, uint8_t *out, uint64_t n_rows) {
    const uint8_t *hb = c ? c->leg[BLOCK_ROWS].h.p : nullptr;
    if (!hb || (n_rows && !out) || n_rows != c->geno_rows) return SVJG_E_ARG;
    memcpy(out, hb + rows_layout(n_rows).boundary, n_rows);
    return 0;
}

// ---- the log10(i!) table from outside: build it ahead of a first call, read it back (svjg.h) ----

extern "C" int svjg_logfact_reserve(svjg_ctx *c, uint32_t entries) {
    if (!c) return SVJG_E_ARG;
    const uint32_t want = logfact_reserve_to(c->logfact_n, entries);
    if (!want) return 0;
    HIPCHK(c, hipSetDevice(c->device));
    { const int rc0 = sync_compute(c); if (rc0) return rc0; }      // (as settle_launch: a pass already enqueued still uses the old table)
    if (c->copy_stream) HIPCHK(c, hipStreamSynchronize(c->copy_stream));
    return build_logfact(c, want);
}

extern "C" int svjg_logfact_read(svjg_ctx *c, uint32_t first, uint32_t n, double *out, uint32_t *entries) {
    if (!c) return SVJG_E_ARG;
    if (entries) *entries = c->logfact_n;
    if ((uint64_t)first + n > c->logfact_n) {
        c->err = "svjg_logfact_read: entries " + std::to_string(first) + " .. " + std::to_string((uint64_t)first + n) + " of a table of " + std::to_string(c->logfact_n);
        return SVJG_E_ARG;
    }
    if (n == 0) return 0;
    if (!out) { c->err = "svjg_logfact_read: no buffer"; return SVJG_E_ARG; }
    static_assert(sizeof(dd) == 2 * sizeof(double), "an entry is a (hi, lo) pair");
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipMemcpyAsync(out, c->d_logfact + first, (uint64_t)n * sizeof(dd), hipMemcpyDeviceToHost, c->stream));   // (behind the build, on its stream)
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return 0;
}

extern "C" int svjg_last_kernel_ms(svjg_ctx *c, float *m, float *s, float *g) {
    if (!c) return SVJG_E_ARG;
    if (m) *m = c->ms_main;
    if (s) *s = c->ms_slow;
    if (g) *g = c->ms_geno;
    return 0;
}

extern "C" int svjg_last_main_ms(svjg_ctx *c, float *by_stamps, float *by_events) {
    if (!c) return SVJG_E_ARG;
    if (by_stamps) *by_stamps = c->ms_main_stamps;
    if (by_events) *by_events = c->ms_main_events;
    return 0;
}

extern "C" int svjg_copy_rate(svjg_ctx *c, uint64_t n_bytes, double *copy_gb_per_s, double *read_gb_per_s) {
    if (!c || n_bytes < (1u << 20)) return SVJG_E_ARG;
    HIPCHK(c, hipSetDevice(c->device));
    n_bytes &= ~4095ull;
    DevBuf<uint4> src, dst;
    if (src.reserve(n_bytes / 16) != hipSuccess || dst.reserve(n_bytes / 16) != hipSuccess) { c->err = "svjg_copy_rate: no memory for the two buffers"; return SVJG_E_NOMEM; }
    HIPCHK(c, hipMemsetAsync(src, 0x5A, n_bytes, c->stream));
    HIPCHK(c, hipMemsetAsync(dst, 0, n_bytes, c->stream));
    const uint32_t grid = (uint32_t)c->n_cu * 16;
    for (int what = 0; what < 2; ++what) {
        double *out = what ? read_gb_per_s : copy_gb_per_s;
        if (!out) continue;
        float best = 0;
        for (int i = 0; i < 4; ++i) {                          // (the first run warms up)
            HIPCHK(c, hipEventRecord(c->ev[2], c->stream));
            if (what) hipLaunchKernelGGL(k_read16, dim3(grid), dim3(TPB), 0, c->stream, dst, src, n_bytes / 16);
            else hipLaunchKernelGGL(k_copy16, dim3(grid), dim3(TPB), 0, c->stream, dst, src, n_bytes / 16);
            HIPCHK(c, hipGetLastError());
            HIPCHK(c, hipEventRecord(c->ev[3], c->stream));
            HIPCHK(c, hipStreamSynchronize(c->stream));
            float ms = 0;
            HIPCHK(c, hipEventElapsedTime(&ms, c->ev[2], c->ev[3]));
            if (i && (best == 0 || ms < best)) best = ms;
        }
        *out = best > 0 ? (what ? 1.0 : 2.0) * (double)n_bytes / (best * 1e-3) / 1e9 : 0.0;
    }
    return 0;
}

extern "C" int svjg_set_main_workers(svjg_ctx *c, uint32_t workers) {
    if (!c) return SVJG_E_ARG;
    c->main_workers = workers;
    return 0;
}

extern "C" int svjg_last_main_plan(svjg_ctx *c, uint64_t *region, uint64_t *small, uint32_t *grid, uint64_t *chunks_claimed) {
    if (!c) return SVJG_E_ARG;
    if (region) *region = c->last_plan.region;
    if (small) *small = c->last_plan.small;
    if (grid) *grid = c->last_plan.grid;
    if (chunks_claimed) *chunks_claimed = c->last_claimed;
    return 0;
}

extern "C" int svjg_sync(svjg_ctx *c) {
    if (!c) return SVJG_E_ARG;
    HIPCHK(c, hipSetDevice(c->device));
    return sync_compute(c);                                       // (both compute streams)
}
