// TEST HARNESS ONLY (never shipped, never loaded by the product): everything of svjg_geno.h that a kernel runs per lane, per item or per row,
// compiled with g++ into ONE library and driven from numpy (tests/geno_sim/*.py), a topic a file: ploidy, site, cohort, prior, qual, site_prior.  A new
// routine in svjg_geno.h gets an export here.  With -DGENO_SIM_MAIN it is a stand-alone program (for -fsanitize=address,undefined):
// `_geno_sim_main <topic>` runs that topic's seeded checks.
#define SVJG_HD inline
#include "../../svjedi-graph_amd/csrc/svjg_geno.h"
#include "../host_logfact.h"
#include <math.h>
#include <stdio.h>
#include <string.h>
#include <initializer_list>
#include <vector>

using namespace svjg;

extern "C" void genosim_logfact(dd *tab, uint32_t n) { host_logfact(tab, n); }

// Where the blocks of a call lie, names included: every layout's fields are written ONCE, here, each with its name, and the caller builds its
// dict from what comes back.  p: max_ploidy (cohort), m_max (qual).  flags: sites 1 = the cohort call, 2 = without the fields that only the
// cohort call has, 4 = the prior, 8 = the prior's fields listed (as 0) though the call is without it: with neither 4 nor 8 they are left out
// (marked in the list); cohort 1 = per item, 2 = prior; qual 1 = per item.  -> the number of fields written to names_out / at_out (at most LAYOUT_MAX_FIELDS)
enum { LAYOUT_ROWS, LAYOUT_PLOIDY, LAYOUT_SITES, LAYOUT_COHORT, LAYOUT_QUAL, LAYOUT_MAX_FIELDS = 32 };
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
#endif

// A sum over S items in the order of k_cohort_prior and k_cohort_sites_prior, N doubles a lane: lane j of W = prior_segment_width(S) lanes adds its
// items j, j + 64, j + 128, ... to zeros in that order (add(s, v) adds item s to v[N]; every summand is >= +0.0, so the first one keeps its bits);
// then the levels m = 1, 2, ..., W / 2 of the xor butterfly, every lane adding its partner's value of the level before; lanes at or beyond S hold
// 0.0.  -> x[N], lane 0's
template <uint32_t N, class Add> static void wave_sum(uint64_t S, Add add, double *x) {
    const uint32_t W = prior_segment_width(S);
    double v[64][N] = {}, u[64][N];
    for (uint32_t j = 0; j < W; ++j) for (uint64_t s = j; s < S; s += 64) add(s, v[j]);
    for (uint32_t m = 1; m < W; m <<= 1) {
        for (uint32_t j = 0; j < W; ++j) for (uint32_t a = 0; a < N; ++a) u[j][a] = v[j][a] + v[j ^ m][a];
        memcpy(v, u, W * sizeof v[0]);
    }
    memcpy(x, v[0], sizeof v[0]);
}

#include "ploidy.inc"
#include "site.inc"
#include "cohort.inc"
#include "prior.inc"
#include "qual.inc"
#include "site_prior.inc"

#ifdef GENO_SIM_MAIN
int main(int argc, char **argv) {
    const struct { const char *topic; int (*run)(); } topics[] = {{"ploidy", main_ploidy}, {"site", main_site}, {"cohort", main_cohort}, {"prior", main_prior},
                                                                 {"qual", main_qual}, {"site_prior", main_site_prior}};
    for (const auto &t : topics) if (argc == 2 && !strcmp(argv[1], t.topic)) return t.run();
    fprintf(stderr, "usage: %s ploidy|site|cohort|prior|qual|site_prior\n", argv[0]);
    return 2;
}
#endif
