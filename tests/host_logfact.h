// TEST HARNESS ONLY (never shipped): the log10(i!) table of k_logfact_* with the HOST libm's log10 (not the device's), summed in order in
// double-double (the kernels sum in blocks: the association differs, both far below the guard's budget).  Included behind svjg_geno.h by the two
// harness libraries (tests/hostsim, tests/geno_sim), which must build one table: tests/test_logfact.py holds them byte-equal.
#pragma once
#include <math.h>

inline void host_logfact(svjg::dd *tab, uint32_t n) {
    svjg::dd run{0.0, 0.0};
    for (uint32_t i = 0; i < n; ++i) { if (i >= 2) run = svjg::dd_add(run, svjg::dd{log10((double)i), 0.0}); tab[i] = run; }
}
