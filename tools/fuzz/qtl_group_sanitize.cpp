// qtl_group_sanitize.cpp -- a stand-alone program for an AddressSanitizer / UndefinedBehaviorSanitizer run of the HOST half of the grouped cis-sQTL
// permutation pass: rgx_cohort_qtl_permute_grouped_host with its threads (the member lists, a group a task, the shared per-series beta
// approximation) on planted tables, under several groupings -- runs of rows, interleaved groups, empty groups, rows in no group --, checked against
// rgx_cohort_qtl_permute_host of the same table by the max identity.  No device is touched.  Build and run (tools/fuzz/README.md):
//   cd regtools_amd/csrc && hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -Xarch_host -fsanitize=address,undefined \
//       -Xarch_host -fno-sanitize-recover=undefined -I../../include -o /tmp/qtl_group_sanitize ../../tools/fuzz/qtl_group_sanitize.cpp \
//       $(the .hip and .cpp files of the Makefile's library line) -ldl -lpthread && /tmp/qtl_group_sanitize
// Prints one line per table and grouping and "ok"; any sanitizer report ends it with a non-zero status.
#include "regtools_amd.h"

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <numeric>
#include <vector>

namespace {
uint64_t state = 0x2545F4914F6CDD1Dull;
uint64_t draw() { state ^= state << 13; state ^= state >> 7; state ^= state << 17; return state; }
double uniform() { return (double)(draw() >> 11) * 0x1p-53; }

// S samples, K rows, V variants on one contig; every third row follows the dosage of a variant inside its window; missing dosages, a constant variant
int table(uint32_t S, uint32_t K, uint32_t V, uint32_t n_cov, uint32_t B, uint64_t seed) {
    std::vector<double> X((size_t)K * S), cov((size_t)n_cov * S);
    std::vector<int8_t> dosage((size_t)V * S);
    std::vector<uint32_t> tid(V, 0), pos(V), rank2((size_t)K * S);
    std::vector<rgx_qtl_region> regions(K);
    for (uint32_t v = 0; v < V; ++v) {
        pos[v] = 100 + 700 * v;
        for (uint32_t s = 0; s < S; ++s) dosage[(size_t)v * S + s] = uniform() < 0.03 ? -1 : (int8_t)((uniform() < 0.4) + (uniform() < 0.4));
        dosage[(size_t)v * S] = 0; dosage[(size_t)v * S + 1] = 2;
    }
    if (V > 2) for (uint32_t s = 0; s < S; ++s) dosage[(size_t)2 * S + s] = 1;
    for (double &c : cov) c = uniform() - 0.5;
    for (uint32_t k = 0; k < K; ++k) {
        const uint32_t anchor = V ? (uint32_t)(draw() % V) : 0;
        regions[k] = {0, V ? pos[anchor] + 50 : 1, V ? pos[anchor] + 300 : 2};
        for (uint32_t s = 0; s < S; ++s) {
            double x = uniform() + uniform() + uniform() - 1.5;
            if (k % 3 == 0 && V) x += 0.9 * std::max<int>(dosage[(size_t)anchor * S + s], 0);
            X[(size_t)k * S + s] = x;
        }
    }
    if (K > 1) regions[K - 1] = {0, 700 * V + 50000, 700 * V + 50100};           // a row out of every variant's reach
    // twice the rank of every entry inside its column (no ties among the draws)
    std::vector<uint32_t> order(K);
    for (uint32_t s = 0; s < S; ++s) {
        std::iota(order.begin(), order.end(), 0u);
        std::sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) { return X[(size_t)a * S + s] < X[(size_t)b * S + s]; });
        for (uint32_t i = 0; i < K; ++i) rank2[(size_t)order[i] * S + s] = 2 * (i + 1);
    }
    rgx_pheno_table ph{};
    ph.n_rows = K; ph.n_samples = S; ph.rank2 = rank2.data();
    std::vector<uint16_t> perm(((size_t)B + 1) * S);
    char err[512] = {0};
    if (rgx_qtl_permutations(S, B, seed, perm.data(), err, sizeof err) != RGX_OK) { fprintf(stderr, "%s", err); return 1; }
    rgx_qtl_perm_result *u = nullptr;
    if (rgx_cohort_qtl_permute_host(&ph, regions.data(), V, tid.data(), pos.data(), dosage.data(), n_cov, cov.data(), 1000, B, perm.data(), &u, err,
                                    sizeof err) != RGX_OK) { fprintf(stderr, "%s", err); return 1; }
    // groupings: 0 = runs of 1 .. 5 rows, 1 = rows dealt into 4 groups with every seventh row in none and two empty groups behind them,
    // 2 = every row its own group, 3 = no row in any group
    for (int kind = 0; kind < 4; ++kind) {
        std::vector<uint32_t> group(K);
        uint32_t G = 0;
        if (kind == 0) { for (uint32_t k = 0; k < K; ++G) for (uint32_t n = 1 + (uint32_t)(draw() % 5); n && k < K; --n) group[k++] = G; }
        else if (kind == 1) { G = 6; for (uint32_t k = 0; k < K; ++k) group[k] = k % 7 == 3 ? RGX_NO_GROUP : k % 4; }
        else if (kind == 2) { G = K; for (uint32_t k = 0; k < K; ++k) group[k] = k; }
        else { G = 3; for (uint32_t k = 0; k < K; ++k) group[k] = RGX_NO_GROUP; }
        rgx_qtl_group_result *q = nullptr;
        if (rgx_cohort_qtl_permute_grouped_host(&ph, regions.data(), V, tid.data(), pos.data(), dosage.data(), n_cov, cov.data(), 1000, B, perm.data(), G,
                                                group.data(), &q, err, sizeof err) != RGX_OK) { fprintf(stderr, "%s", err); return 1; }
        uint64_t with = 0, fitted = 0;
        for (uint32_t g = 0; g < q->n_groups; ++g) {
            uint64_t n_cis = 0;
            for (uint32_t b = 0; b <= B; ++b) {
                uint64_t top = 0;
                for (uint32_t i = q->grp_begin[g]; i < q->grp_begin[g + 1]; ++i) {
                    uint64_t bits; memcpy(&bits, &u->perm_r[q->grp_row[i] * ((size_t)B + 1) + b], 8);
                    top = std::max(top, bits);
                    if (!b) n_cis += u->n_cis[q->grp_row[i]];
                }
                uint64_t got; memcpy(&got, &q->perm_r[g * ((size_t)B + 1) + b], 8);
                if (got != top) { fprintf(stderr, "grouping %d, group %u, permutation %u: not the largest of its members\n", kind, g, b); return 1; }
            }
            if (n_cis != q->group_n_cis[g] || (n_cis == 0) != (q->best_row[g] == RGX_NO_PAIR)) {
                fprintf(stderr, "grouping %d, group %u: its pairs are not its members'\n", kind, g); return 1; }
            if (n_cis) { ++with; fitted += q->beta_status[g] == 0; if (q->n_ge[g] < u->n_ge[q->best_row[g]]) { fprintf(stderr, "n_ge fell\n"); return 1; } }
        }
        printf("%u x %u x %u, %u covariates, %u permutations, grouping %d: %u groups, %llu pairs, %llu groups with pairs, %llu fitted\n", S, K, V, n_cov, B,
               kind, G, (unsigned long long)q->n_pairs, (unsigned long long)with, (unsigned long long)fitted);
        fflush(stdout);
        rgx_cohort_qtl_group_free(q);
    }
    rgx_cohort_qtl_perm_free(u);
    return 0;
}
}  // namespace

// Every result here stays below 64 KiB: the library keeps released blocks of that size and more for later tables until the process ends
// (block_give, api_ctx.cpp), and LeakSanitizer, which stays on, would report that cache at exit.
int main() {
    if (table(64, 30, 40, 2, 199, 5) || table(17, 9, 12, 0, 7, 1) || table(70, 40, 3, 3, 1, 2) || table(9, 50, 400, 1, 130, 3)) return 1;
    printf("ok\n");
    fflush(stdout);
    return 0;
}
