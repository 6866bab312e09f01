// The per-row routines of the cohort site quality (svjg_geno.h: qual_load, qual_den, qual_fold, qual_rescale_every, qual_term, qual_best,
// qual_finish, qual_harmonic), and a row run with its sums over k sequentially or in k_cohort_qual's order (genosim_qual_row's wave arm:
// lane-strided partials in increasing k, then the xor butterfly over 64 lanes).  Topic `qual` of the stand-alone program runs random rows and
// checks what holds without a model.

// One row of S samples: raw[S][2], done[S] (the gate's outcome), ploidy[S] or NULL (2 everywhere); max_ploidy as the call's (it sizes the row and
// sets the rescaling's cadence) -> *qual (NaN: no item took part), *mlac, *chroms.  every: 0 = qual_rescale_every of the call, else that many
// steps between two rescalings (the answer must not depend on it beyond rounding: the tests say so)
static void row_qual(bool wave, uint32_t sv_type, const uint32_t *raw, const uint8_t *done, const uint8_t *ploidy, uint64_t S, uint32_t max_ploidy, double err,
                     double theta, uint32_t every, double *qual, uint32_t *mlac, uint32_t *chroms) {
    double tab[2 * PLOIDY_TAB];
    ploidy_log_table(err, tab);
    const uint32_t m_max = (uint32_t)(S * max_ploidy);
    std::vector<double> harm(m_max + 1), ya(m_max + 1, 0.0), yb(m_max + 1, 0.0);
    qual_harmonic(m_max, harm.data());
    if (!every) every = qual_rescale_every(m_max, max_ploidy);
    double *cur = ya.data(), *nxt = yb.data();
    cur[0] = 1.0;
    uint32_t M = 0, since = 0;
    int64_t E = 0;
    dd D0{0.0, 0.0};
    for (uint64_t s = 0; s < S; ++s) {
        const uint32_t P = done[s] ? (ploidy ? ploidy[s] : 2u) : 0u;
        QualItem it;
        qual_load(sv_type, raw[s * 2], raw[s * 2 + 1], P <= max_ploidy ? P : 0u, tab, it);
        if (it.it.P == 0 || M + it.it.P > m_max) continue;
        D0 = dd_add(D0, it.d0);
        const uint32_t Mn = M + it.it.P;
        const double den = qual_den(Mn, it.it.P);
        for (uint32_t k = 0; k <= Mn; ++k) nxt[k] = qual_fold(it.it, cur, M, Mn, k, den);
        M = Mn;
        { double *t = cur; cur = nxt; nxt = t; }
        if (++since == every) {
            since = 0;
            double m = 0.0;
            for (uint32_t k = 0; k <= M; ++k) m = fmax(m, cur[k]);               // (a maximum does not depend on the order)
            if (m > 0.0) {
                const int e = ilogb(m);
                const double sc = ldexp(1.0, -e);
                for (uint32_t k = 0; k <= M; ++k) cur[k] *= sc;
                E -= e;
            }
        }
    }
    const double phi0 = qual_phi0(theta, harm[M]);
    double T = 0.0;
    QualBest best{-1.0, 0u};
    if (wave) {
        double v[64], u[64]; QualBest b[64], c[64];
        for (uint32_t j = 0; j < 64; ++j) {                                       // lane j: k = j, j + 64, ...
            v[j] = 0.0; b[j] = QualBest{-1.0, 0u};
            for (uint32_t k = j; k <= M; k += 64) { const double t = qual_term(theta, phi0, k, cur[k]); v[j] += t; b[j] = qual_best(b[j], QualBest{t, k}); }
        }
        for (uint32_t m = 1; m < 64; m <<= 1) {                                   // the butterfly: every lane combines with its partner's value of the level before
            for (uint32_t j = 0; j < 64; ++j) { u[j] = v[j] + v[j ^ m]; c[j] = qual_best(b[j], b[j ^ m]); }
            for (uint32_t j = 0; j < 64; ++j) { v[j] = u[j]; b[j] = c[j]; }
        }
        T = v[0]; best = b[0];
    } else
        for (uint32_t k = 0; k <= M; ++k) { const double t = qual_term(theta, phi0, k, cur[k]); T += t; best = qual_best(best, QualBest{t, k}); }
    *chroms = M;
    *mlac = M ? best.k : 0u;
    *qual = M ? qual_finish(phi0, D0, T, E) : NAN;
}

extern "C" void genosim_qual_row(int wave, uint32_t sv_type, const uint32_t *raw, const uint8_t *done, const uint8_t *ploidy, uint64_t S, uint32_t max_ploidy, double err,
                                 double theta, uint32_t every, double *qual, uint32_t *mlac, uint32_t *chroms) {
    row_qual(wave != 0, sv_type, raw, done, ploidy, S, max_ploidy, err, theta, every, qual, mlac, chroms);
}

// the item of a sample: w[9] = C(P, g) 10^d_g, d0 as its two doubles -> the ploidy the recurrence sees (0: it takes no part)
extern "C" uint32_t genosim_qual_item(uint32_t sv_type, uint32_t ref, uint32_t alt, uint32_t P, double err, double *w, double *d0) {
    double tab[2 * PLOIDY_TAB];
    ploidy_log_table(err, tab);
    QualItem it;
    qual_load(sv_type, ref, alt, P, tab, it);
    for (uint32_t g = 0; g <= MAX_PLOIDY; ++g) w[g] = it.it.w[g];
    d0[0] = it.d0.hi; d0[1] = it.d0.lo;
    return it.it.P;
}

extern "C" uint32_t genosim_qual_every(uint32_t m_max, uint32_t max_ploidy) { return qual_rescale_every(m_max, max_ploidy); }
extern "C" void genosim_qual_constants(double *out) { out[0] = QUAL_ABS; out[1] = QUAL_REL; out[2] = QUAL_ABS_MEASURED; out[3] = QUAL_REL_MEASURED; out[4] = QUAL_MAX_CHROMS; out[5] = QUAL_THETA_MAX; }

#ifdef GENO_SIM_MAIN
static int main_qual() {
    const uint64_t sizes[14] = {1, 2, 3, 8, 9, 17, 31, 32, 33, 63, 64, 65, 200, 600};
    uint64_t rows = 0, bad = 0, x = 88172645463325252ull;
    auto next = [&] { x ^= x << 13; x ^= x >> 7; x ^= x << 17; return x; };
    for (uint64_t S : sizes)
        for (int mode = 0; mode < 3; ++mode)                                          // diploid, mixed ploidy 0..8, deep counts
            for (int k = 0; k < (S > 100 ? 4 : 30); ++k) {
                std::vector<uint32_t> raw(S * 2); std::vector<uint8_t> done(S), pld(S);
                uint32_t m_part = 0;
                for (uint64_t s = 0; s < S; ++s) {
                    const uint64_t v = next();
                    raw[s * 2] = (uint32_t)(v % (mode == 2 ? 5001 : (v >> 40) % 3 ? 61 : 5)); raw[s * 2 + 1] = (uint32_t)((v >> 16) % ((v >> 44) % 3 ? 61 : 5));
                    done[s] = (v >> 32) % 5 != 0; pld[s] = (uint8_t)((v >> 36) % 9);
                    if (done[s] && raw[s * 2] + raw[s * 2 + 1]) m_part += mode == 1 ? pld[s] : 2u;
                }
                const uint32_t type = (uint32_t)(next() % 4), mp = mode == 1 ? 8u : 2u;
                const uint8_t *pl = mode == 1 ? pld.data() : nullptr;
                double q[4]; uint32_t ml[4], ch[4];
                genosim_qual_row(0, type, raw.data(), done.data(), pl, S, mp, 5e-5, 1e-3, 0, &q[0], &ml[0], &ch[0]);
                genosim_qual_row(1, type, raw.data(), done.data(), pl, S, mp, 5e-5, 1e-3, 0, &q[1], &ml[1], &ch[1]);
                genosim_qual_row(1, type, raw.data(), done.data(), pl, S, mp, 5e-5, 1e-3, 1, &q[2], &ml[2], &ch[2]);      // a rescaling behind every step
                genosim_qual_row(1, type, raw.data(), done.data(), pl, S, mp, 5e-5, 1e-3, 0, &q[3], &ml[3], &ch[3]);
                ++rows;
                for (int i = 0; i < 4; ++i) {
                    if (ch[i] != m_part || ml[i] > ch[i]) ++bad;
                    if (m_part ? !(q[i] >= 0.0 && q[i] < 1e9) : !(q[i] != q[i] && ml[i] == 0)) ++bad;
                }
                if (m_part && (q[1] != q[3] || ml[1] != ml[3])) ++bad;                                              // the same call again: the same bits
                if (m_part && (fabs(q[0] - q[1]) > 1e-9 + 1e-12 * q[1] || fabs(q[2] - q[1]) > 1e-9 + 1e-12 * q[1])) ++bad;   // orders and cadences agree but for rounding
            }
    for (uint64_t n_rows : {1, 7, 1000}) for (uint64_t S : {1, 3, 64, 65}) for (uint32_t mp : {1u, 2u, 8u}) for (int per : {0, 1}) {
        uint64_t L[12];
        layout_at(LAYOUT_QUAL, n_rows, S, (uint32_t)(S * mp), per, L);
        if (L[0] != 0 || L[1] != 8 * n_rows || L[2] != 12 * n_rows || L[3] % 8 || L[3] < 16 * n_rows || L[4] != L[3] + 8 || L[5] != L[4] || L[6] != L[5] + 720
            || L[7] != L[6] + 8 * (S * mp + 1) || L[10] != L[7] + 6 * n_rows || L[11] != L[10] + (per ? n_rows * S : 0) + 64) ++bad;
    }
    // The shapes that max_ploidy and the ploidy array decide: the sex pattern (0 / 1 / 2 under max_ploidy 2), haploid with absent items (max_ploidy
    // 1) and 0..mp at mp = 3..7, on both sides of 64 and 128 entries and at several hundred chromosomes; 512 samples of ploidy 8 with one read
    // each (M = QUAL_MAX_CHROMS, cadence 4).  Each array is called at its own max_ploidy and at 8: the rows are sized differently, the bits are equal.
    const uint64_t shape_sizes[10] = {20, 33, 63, 64, 65, 128, 129, 300, 600, 512};
    for (uint64_t S : shape_sizes)
        for (uint32_t mp = 1; mp <= 8; ++mp) {
            if (S == 512 ? mp != 8 : (mp == 8 || (S * 8 > QUAL_MAX_CHROMS && mp > 2))) continue;
            for (int k = 0; k < (S > 100 ? 2 : 10); ++k) {
                std::vector<uint32_t> raw(S * 2); std::vector<uint8_t> done(S), pld(S);
                uint32_t m_part = 0;
                for (uint64_t s = 0; s < S; ++s) {
                    const uint64_t v = next();
                    const bool shallow = S >= 300;
                    raw[s * 2] = shallow ? (v % 7 != 0) : (uint32_t)(v % ((v >> 40) % 3 ? 61 : 5)); raw[s * 2 + 1] = shallow ? 1u - raw[s * 2] : (uint32_t)((v >> 16) % ((v >> 44) % 3 ? 61 : 5));
                    done[s] = S == 512 || (v >> 32) % 5 != 0;
                    pld[s] = S == 512 ? 8 : mp == 2 ? (uint8_t)((v >> 36) % 3) : mp == 1 ? (uint8_t)((v >> 36) % 10 != 0) : (uint8_t)((v >> 36) % (mp + 1));
                    if (done[s] && raw[s * 2] + raw[s * 2 + 1]) m_part += pld[s];
                }
                const uint32_t type = (uint32_t)(next() % 4), wide = S * 8 <= QUAL_MAX_CHROMS ? 8u : mp;
                double q[3]; uint32_t ml[3], ch[3];
                genosim_qual_row(0, type, raw.data(), done.data(), pld.data(), S, mp, 5e-5, 1e-3, 0, &q[0], &ml[0], &ch[0]);
                genosim_qual_row(1, type, raw.data(), done.data(), pld.data(), S, mp, 5e-5, 1e-3, 0, &q[1], &ml[1], &ch[1]);
                genosim_qual_row(1, type, raw.data(), done.data(), pld.data(), S, wide, 5e-5, 1e-3, 0, &q[2], &ml[2], &ch[2]);
                ++rows;
                for (int i = 0; i < 3; ++i) {
                    if (ch[i] != m_part || ml[i] > ch[i]) ++bad;
                    if (m_part ? !(q[i] >= 0.0 && q[i] < 1e9) : !(q[i] != q[i] && ml[i] == 0)) ++bad;
                }
                if (m_part && (q[1] != q[2] || ml[1] != ml[2])) ++bad;                                              // the same bits under a wider max_ploidy
                if (m_part && fabs(q[0] - q[1]) > 1e-9 + 1e-12 * q[1]) ++bad;
                if (S == 512 && ch[1] != QUAL_MAX_CHROMS) ++bad;
            }
        }
    if (genosim_qual_every(1024, 8) != 5 || genosim_qual_every(512, 8) != 6 || genosim_qual_every(63, 1) != 85 || genosim_qual_every(64, 1) != 73) ++bad;
    if (genosim_qual_every(4096, 8) != 4 || genosim_qual_every(4096, 2) != 19 || genosim_qual_every(128, 2) != 32 || genosim_qual_every(1, 1) != 512) ++bad;
    printf("cohort_qual_sim %s: %llu rows, %llu checks failed\n", bad ? "FAILED" : "ok", (unsigned long long)rows, (unsigned long long)bad);
    return bad ? 1 : 0;
}
#endif
