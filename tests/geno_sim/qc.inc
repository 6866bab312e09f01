// The cohort sample QC (svjg_geno.h: qc_class, qc_plane_words, qc_pair_word, the stage slots and the tiles are the kernels' own code) inside a plain
// C++ restatement of the two kernels' loops over blocks, waves and lanes (k_qc_planes, k_qc_pairs of svjg_kernels.h), in a block laid out by
// qc_layout.  Topic `qc` of the stand-alone program runs seeded random calls against a brute-force count.

extern "C" void genosim_qc_constants(uint32_t *out) {
    const uint32_t v[9] = {QC_TI, QC_TJ, QC_STAGE_WORDS, QC_MAX_SAMPLES, QC_RI, QC_PLANE_WORDS, QC_WAVES, QC_LDS_SLOTS, QC_BLOCKS_PER_CU};
    memcpy(out, v, sizeof v);
}
extern "C" uint32_t genosim_qc_class(uint32_t g, uint32_t P) { return qc_class(g, P); }
extern "C" uint32_t genosim_qc_tiles(uint32_t S) { return qc_tiles(S); }
extern "C" void genosim_qc_tile_at(uint32_t t, uint32_t S, uint32_t *ij) { qc_tile_at(t, S, ij[0], ij[1]); }
extern "C" void genosim_qc_pair_word(const uint64_t *i3, const uint64_t *j3, uint32_t *c) { qc_pair_word(i3[0], i3[1], i3[2], j3[0], j3[1], j3[2], c); }

// Both kernels over a call, with grids of grid_planes / grid_pairs blocks (0: one block a unit of work, the uncapped launch).  -> 0, or a code:
// 1 a store outside the block's field, 2 a pair written twice or never, 3 a plane word never written, 4 a bit set behind the last row.
extern "C" int genosim_qc_run(const uint8_t *gt, const uint8_t *ploidy, uint64_t n_rows, uint32_t S, uint32_t grid_planes, uint32_t grid_pairs,
                         uint32_t *sample, uint32_t *pair) {
    const QcLayout L = qc_layout(n_rows, S, ploidy != nullptr);
    const uint64_t n = n_rows * S, n_words = qc_words(n_rows), n_pairs = qc_pairs(S), n_plane_words = QC_PLANES * n_words * S;
    std::vector<uint64_t> block = poisoned_block(L.total);
    uint8_t *base = (uint8_t *)block.data();
    stage_calls(base, L, gt, ploidy, n);
    const uint8_t *d_gt = base + L.gt, *d_ploidy = ploidy ? base + L.ploidy : nullptr;
    uint64_t *planes = (uint64_t *)(base + L.planes);
    uint32_t *d_sample = (uint32_t *)(base + L.sample), *d_pair = (uint32_t *)(base + L.pair);
    if (L.planes + n_plane_words * 8 + 64 != L.total || L.sample + (uint64_t)S * 24 != L.maxn || L.pair + n_pairs * 20 > L.sample) return 1;
    memset(base + L.sample, 0, (uint64_t)S * 24 + 8);                                       // the launch's ONE memset
    std::vector<uint8_t> plane_written(n_plane_words, 0), pair_written(n_pairs, 0);

    // k_qc_planes
    const uint64_t units = qc_plane_units(n_words, S);
    const uint64_t gp = grid_planes ? grid_planes : (units + SIM_TPB - 1) / SIM_TPB;
    for (uint64_t b = 0; b < gp; ++b)
        for (uint32_t th = 0; th < SIM_TPB; ++th)
            for (uint64_t u = b * SIM_TPB + th; u < units; u += gp * SIM_TPB) {
                const uint64_t chunk = u / S, s = u % S;
                const uint64_t w_begin = chunk * QC_PLANE_WORDS, w_end = w_begin + QC_PLANE_WORDS < n_words ? w_begin + QC_PLANE_WORDS : n_words;
                uint32_t cnt[QC_CLASSES] = {};
                for (uint64_t w = w_begin; w < w_end; ++w) {
                    uint64_t word[QC_CLASSES];
                    qc_plane_words(d_gt, d_ploidy, n_rows, S, w, s, word);
                    for (uint32_t q = 0; q < QC_CLASSES; ++q) {
                        cnt[q] += (uint32_t)__builtin_popcountll(word[q]);
                        if (w == n_words - 1 && (n_rows & 63) && (word[q] >> (n_rows & 63))) return 4;
                    }
                    for (uint32_t k = 0; k < QC_PLANES; ++k) {
                        const uint64_t at = qc_plane_at(k, w, s, n_words, S);
                        if (at >= n_plane_words) return 1;
                        planes[at] = word[QC_DIP + k]; plane_written[at] = 1;
                    }
                }
                for (uint32_t q = 0; q < QC_CLASSES; ++q) d_sample[s * QC_CLASSES + q] += cnt[q];
            }
    for (uint8_t w : plane_written) if (!w) return 3;

    // k_qc_pairs
    const uint32_t n_tiles = qc_tiles(S), gq = grid_pairs ? grid_pairs : n_tiles;
    std::vector<uint64_t> lds(QC_LDS_SLOTS);
    std::vector<uint32_t> acc((size_t)SIM_TPB * QC_RI * QC_PAIR_COUNTS);
    for (uint32_t b = 0; b < gq; ++b)
        for (uint32_t t = b; t < n_tiles; t += gq) {
            uint32_t ti, tj;
            qc_tile_at(t, S, ti, tj);
            if (ti >= qc_tiles_i(S) || tj >= qc_tiles_j(S)) return 1;
            const uint32_t i0 = ti * QC_TI, j0 = tj * QC_TJ;
            std::fill(acc.begin(), acc.end(), 0u);
            for (uint64_t w0 = 0; w0 < n_words; w0 += QC_STAGE_WORDS) {
                for (uint32_t th = 0; th < SIM_TPB; ++th)
                    for (uint32_t e = th; e < QC_LDS_SLOTS; e += SIM_TPB) lds[e] = qc_stage_word(planes, e, i0, j0, w0, n_words, S);
                const uint32_t nw = n_words - w0 < QC_STAGE_WORDS ? (uint32_t)(n_words - w0) : QC_STAGE_WORDS;
                for (uint32_t th = 0; th < SIM_TPB; ++th) {
                    const uint32_t lane = th & 63u, wave = th >> 6, iw = i0 + wave * QC_RI;
                    if (!(iw < j0 + QC_TJ - 1)) continue;
                    for (uint32_t w = 0; w < nw; ++w)
                        for (uint32_t a = 0; a < QC_RI; ++a) {
                            const uint32_t x = wave * QC_RI + a;
                            qc_pair_word(lds[qc_lds_i(0, w, x)], lds[qc_lds_i(1, w, x)], lds[qc_lds_i(2, w, x)],
                                         lds[qc_lds_j(0, w, lane)], lds[qc_lds_j(1, w, lane)], lds[qc_lds_j(2, w, lane)], &acc[((size_t)th * QC_RI + a) * QC_PAIR_COUNTS]);
                        }
                }
            }
            for (uint32_t th = 0; th < SIM_TPB; ++th) {
                const uint32_t lane = th & 63u, wave = th >> 6, j = j0 + lane;
                if (!(j < S)) continue;
                for (uint32_t a = 0; a < QC_RI; ++a) {
                    const uint32_t i = i0 + wave * QC_RI + a;
                    if (!(i < j)) continue;
                    const uint64_t k = qc_pair_at(i, j, S);
                    if (k >= n_pairs) return 1;
                    if (pair_written[k]++) return 2;
                    memcpy(d_pair + k * QC_PAIR_COUNTS, &acc[((size_t)th * QC_RI + a) * QC_PAIR_COUNTS], QC_PAIR_COUNTS * 4);
                }
            }
        }
    for (uint8_t w : pair_written) if (w != 1) return 2;
    if (!maxn_stayed_zero(base, L.maxn)) return 1;
    memcpy(sample, d_sample, (uint64_t)S * 24);
    if (n_pairs) memcpy(pair, d_pair, n_pairs * 20);
    return 0;
}

#ifdef GENO_SIM_MAIN
// the definitions item by item and pair by pair
static int qc_brute(const std::vector<uint8_t> &gt, const uint8_t *ploidy, uint64_t R, uint32_t S, const std::vector<uint32_t> &sample, const std::vector<uint32_t> &pair) {
    for (uint32_t s = 0; s < S; ++s) {
        uint32_t want[6] = {};
        for (uint64_t r = 0; r < R; ++r) {
            const uint32_t g = gt[r * S + s], P = ploidy ? ploidy[r * S + s] : 2u;
            const bool el = P >= 1, ca = el && g <= P, di = ca && P == 2;
            want[0] += el; want[1] += ca; want[2] += ca && g >= 1; want[3] += di; want[4] += di && g == 1; want[5] += di && g == 2;
        }
        if (memcmp(want, &sample[s * 6], sizeof want)) return 1;
    }
    uint64_t k = 0;
    for (uint32_t i = 0; i < S; ++i)
        for (uint32_t j = i + 1; j < S; ++j, ++k) {
            uint32_t want[5] = {};
            for (uint64_t r = 0; r < R; ++r) {
                const uint32_t gi = gt[r * S + i], gj = gt[r * S + j], Pi = ploidy ? ploidy[r * S + i] : 2u, Pj = ploidy ? ploidy[r * S + j] : 2u;
                const bool di = Pi == 2 && gi <= 2, dj = Pj == 2 && gj <= 2;
                want[0] += di && dj; want[1] += di && dj && gi == 1; want[2] += di && dj && gj == 1; want[3] += di && dj && gi == 1 && gj == 1;
                want[4] += di && dj && ((gi == 0 && gj == 2) || (gi == 2 && gj == 0));
            }
            if (memcmp(want, &pair[k * 5], sizeof want)) return 1;
        }
    return 0;
}

static int main_qc() {
    const uint32_t sizes[] = {1, 2, 3, QC_TJ - 1, QC_TJ, QC_TJ + 1, 2 * QC_TJ + 2};
    const uint64_t rows[] = {1, 63, 64, 65, 64 * QC_STAGE_WORDS - 1, 64 * QC_STAGE_WORDS + 1};
    int cases = 0;
    for (uint32_t S : sizes)
        for (uint64_t R : rows)
            for (int mode = 0; mode < 3; ++mode) {           // no ploidy array, all 2, mixed 0..8
                std::vector<uint8_t> gt(R * S), pl(R * S);
                for (auto &g : gt) { const uint32_t v = rnd() % 10; g = v == 9 ? 0xFF : (uint8_t)v; }
                for (auto &p : pl) p = mode == 1 ? 2 : (uint8_t)(rnd() % 9);
                if (mode != 2) for (auto &g : gt) if (g != 0xFF && rnd() % 4) g %= 4;      // mostly 0..3 where every item is diploid
                std::vector<uint32_t> sample(S * 6), pair(qc_pairs(S) * 5 + 1);
                const uint8_t *ploidy = mode ? pl.data() : nullptr;
                const int rc = genosim_qc_run(gt.data(), ploidy, R, S, cases % 2 ? 3 : 0, cases % 3 ? 2 : 0, sample.data(), pair.data());
                if (rc) { fprintf(stderr, "qc_sim: code %d at S %u rows %llu mode %d\n", rc, S, (unsigned long long)R, mode); return 1; }
                if (qc_brute(gt, ploidy, R, S, sample, pair)) { fprintf(stderr, "qc_sim: counts differ at S %u rows %llu mode %d\n", S, (unsigned long long)R, mode); return 1; }
                ++cases;
            }
    printf("qc_sim ok: %d cases\n", cases);
    return 0;
}
#endif
