// TEST HARNESS ONLY (never shipped, never loaded by the product): everything of svjg_geno.h that a kernel runs per lane, per item or per row,
// compiled with g++ into ONE library and driven from numpy (tests/geno_sim/*.py), a topic a file: ploidy, site, cohort, prior, qual, site_prior, qc, hwe.  A new
// routine in svjg_geno.h gets an export here.  With -DGENO_SIM_MAIN it is a stand-alone program (for -fsanitize=address,undefined):
// `_geno_sim_main <topic>` runs that topic's seeded checks.
#define SVJG_HD inline
#include "../../svjedi-graph_amd/csrc/svjg_geno.h"
#include "../host_logfact.h"
#include <math.h>
#include <stdio.h>
#include <string.h>
#include <algorithm>
#include <initializer_list>
#include <vector>

using namespace svjg;

extern "C" void genosim_logfact(dd *tab, uint32_t n) { host_logfact(tab, n); }

// Where the blocks of a call lie, names included: every layout's fields are written ONCE, here, each with its name, and the caller builds its
// dict from what comes back.  p: max_ploidy (cohort), m_max (qual).  flags: sites 1 = the cohort call, 2 = without the fields that only the
// cohort call has, 4 = the prior, 8 = the prior's fields listed (as 0) though the call is without it: with neither 4 nor 8 they are left out
// (marked in the list); cohort 1 = per item, 2 = prior; qual, qc, hwe 1 = per item.  -> the number of fields written to names_out / at_out (at most LAYOUT_MAX_FIELDS)
enum { LAYOUT_ROWS, LAYOUT_PLOIDY, LAYOUT_SITES, LAYOUT_COHORT, LAYOUT_QUAL, LAYOUT_QC, LAYOUT_HWE, LAYOUT_MAX_FIELDS = 32 };
struct LayoutField { const char *name; uint64_t at; bool left_out = false; };
#define F(field) {#field, L.field}
#define IN_FIELDS {"slot", L.in.slot}, {"type", L.in.type}, {"ok", L.in.ok}
extern "C" int genosim_layout(int kind, uint64_t n, uint64_t S, uint32_t p, int flags, const char **names_out, uint64_t *at_out) {
    std::vector<LayoutField> v;
    if (kind == LAYOUT_ROWS) {
        const RowsLayout L = rows_layout(n);
        v = {F(pl), F(raw), F(gt), F(flags), F(boundary), F(maxn), IN_FIELDS, F(total)};
    } else if (kind == LAYOUT_PLOIDY) {
        const PloidyLayout L = ploidy_layout(n);
        v = {F(pl), F(raw), F(gt), F(flags), F(boundary), F(maxn), F(logtab), IN_FIELDS, F(ploidy), F(in_bytes), F(total)};
    } else if (kind == LAYOUT_SITES) {
        const SitesLayout L = sites_layout(n, S, (flags & 1) != 0, (flags & 4) != 0);
        const bool own = (flags & 2) != 0, plain = (flags & 12) == 0;
        v = {F(pl), F(raw), F(gt), {"members", L.members, own}, F(boundary), {"sgt", L.sgt, plain}, {"sgq", L.sgq, plain}, {"af", L.af, plain},
             {"psite", L.psite, plain}, {"steps", L.steps, plain}, {"site", L.site, own}, F(maxn), {"in_at", L.in_at, own}, F(logs), F(slots),
             F(in_bytes), F(total)};
    } else if (kind == LAYOUT_COHORT) {
        const CohortLayout L = cohort_layout(n, S, p, (flags & 1) != 0, (flags & 2) != 0);
        v = {F(pl), F(raw), F(gt), F(flags), F(boundary), F(gq), F(af), F(psite), F(steps), F(site), F(maxn), F(in_at), F(logtab), IN_FIELDS,
             F(ploidy), F(total), F(in_bytes)};
    } else if (kind == LAYOUT_QUAL) {
        const QualLayout L = qual_layout(n, S, p, (flags & 1) != 0);
        v = {F(qual), F(mlac), F(chroms), F(maxn), F(in_at), F(logtab), F(harm), IN_FIELDS, F(ploidy), F(total)};
    } else if (kind == LAYOUT_QC) {
        const QcLayout L = qc_layout(n, S, (flags & 1) != 0);
        v = {F(pair), F(sample), F(maxn), F(in_at), F(in_bytes), F(gt), F(ploidy), F(planes), F(total)};
    } else if (kind == LAYOUT_HWE) {
        const HweLayout L = hwe_layout(n, S, (flags & 1) != 0);
        v = {F(p), F(counts), F(maxn), F(in_at), F(in_bytes), F(gt), F(ploidy), F(total)};
    }
    int count = 0;
    for (const LayoutField &f : v) if (!f.left_out) { names_out[count] = f.name; at_out[count++] = f.at; }
    return count;
}
#undef F
#undef IN_FIELDS

#ifdef GENO_SIM_MAIN
// the offsets alone, in the order above (what the programs' layout checks index)
static void layout_at(int kind, uint64_t n, uint64_t S, uint32_t p, int flags, uint64_t *at) {
    const char *names[LAYOUT_MAX_FIELDS];
    genosim_layout(kind, n, S, p, flags, names, at);
}
// the programs' one generator (xorshift64)
static uint64_t rng_state = 88172645463325252ull;
static uint64_t rnd() { uint64_t &x = rng_state; x ^= x << 13; x ^= x >> 7; x ^= x << 17; return x; }
#endif

// The levels m = 1, 2, ..., width / 2 of the xor butterfly (svjg_kernels.h: prior_segment_sum) over `lanes` lanes of N values each, v[lane][N]
// flat: at every level a lane adds its partner's value of the level before, own value first.  lanes is a multiple of width.
template <uint32_t N, class T> static void butterfly(T *v, uint32_t lanes, uint32_t width) {
    T old[64 * N];
    for (uint32_t m = 1; m < width; m <<= 1) {
        memcpy(old, v, lanes * N * sizeof(T));
        for (uint32_t l = 0; l < lanes; ++l) for (uint32_t a = 0; a < N; ++a) v[l * N + a] = old[l * N + a] + old[(l ^ m) * N + a];
    }
}

// A sum over S items in the order of k_cohort_prior and k_cohort_sites_prior, N doubles a lane: lane j of W = prior_segment_width(S) lanes adds its
// items j, j + 64, j + 128, ... to zeros in that order (add(s, v) adds item s to v[N]; every summand is >= +0.0, so the first one keeps its bits);
// then the levels m = 1, 2, ..., W / 2 of the xor butterfly, every lane adding its partner's value of the level before; lanes at or beyond S hold
// 0.0.  -> x[N], lane 0's
template <uint32_t N, class Add> static void wave_sum(uint64_t S, Add add, double *x) {
    const uint32_t W = prior_segment_width(S);
    double v[64][N] = {};
    for (uint32_t j = 0; j < W; ++j) for (uint64_t s = j; s < S; s += 64) add(s, v[j]);
    butterfly<N>(&v[0][0], W, W);
    memcpy(x, v[0], sizeof v[0]);
}

// What the runs of whole kernels (qc.inc, hwe.inc) share: the lanes of a block (svjg_kernels.h: TPB); a call's block with every byte poisoned, so
// that a word the run never wrote would show; and whether the block's max_n pair stayed zero, as it must where the leg never runs a kernel twice.
constexpr uint32_t SIM_TPB = 256;
static std::vector<uint64_t> poisoned_block(uint64_t total) { return std::vector<uint64_t>((total + 7) / 8, 0xA5A5A5A5A5A5A5A5ull); }
static bool maxn_stayed_zero(const uint8_t *base, uint64_t maxn) { uint32_t w[2]; memcpy(w, base + maxn, sizeof w); return !(w[0] | w[1]); }

#include "ploidy.inc"
#include "site.inc"
#include "cohort.inc"
#include "prior.inc"
#include "qual.inc"
#include "site_prior.inc"
#include "qc.inc"
#include "hwe.inc"

#ifdef GENO_SIM_MAIN
int main(int argc, char **argv) {
    const struct { const char *topic; int (*run)(); } topics[] = {{"ploidy", main_ploidy}, {"site", main_site}, {"cohort", main_cohort}, {"prior", main_prior},
                                                                 {"qual", main_qual}, {"site_prior", main_site_prior}, {"qc", main_qc}, {"hwe", main_hwe}};
    for (const auto &t : topics) if (argc == 2 && !strcmp(argv[1], t.topic)) return t.run();
    fprintf(stderr, "usage: %s ploidy|site|cohort|prior|qual|site_prior|qc|hwe\n", argv[0]);
    return 2;
}
#endif
