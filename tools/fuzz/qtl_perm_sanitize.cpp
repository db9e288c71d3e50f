// qtl_perm_sanitize.cpp -- a stand-alone program for an AddressSanitizer / UndefinedBehaviorSanitizer run of the HOST half of the cis-sQTL permutation
// pass: rgx_qtl_permutations, rgx_cohort_qtl_permute_host (steps (1)-(6), the permuted chains, the threaded beta approximation), rgx_qtl_beta_fit and
// the special functions, on a planted table.  No device is touched.  Build and run (tools/fuzz/README.md):
//   cd regtools_amd/csrc && hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -Xarch_host -fsanitize=address,undefined \
//       -Xarch_host -fno-sanitize-recover=undefined -I../../include -o /tmp/qtl_perm_sanitize ../../tools/fuzz/qtl_perm_sanitize.cpp \
//       $(the .hip and .cpp files of the Makefile's library line) -ldl -lpthread && /tmp/qtl_perm_sanitize
// Prints one line per table and "ok"; any sanitizer report ends it with a non-zero status.
#include "regtools_amd.h"

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
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
    rgx_qtl_perm_result *q = nullptr;
    if (rgx_cohort_qtl_permute_host(&ph, regions.data(), V, tid.data(), pos.data(), dosage.data(), n_cov, cov.data(), 1000, B, perm.data(), &q, err,
                                    sizeof err) != RGX_OK) { fprintf(stderr, "%s", err); return 1; }
    uint64_t with = 0, fitted = 0, least = B;
    std::vector<double> p(B);
    for (uint64_t k = 0; k < q->n_rows; ++k) {
        if (!q->n_cis[k]) continue;
        ++with; fitted += q->beta_status[k] == 0; least = std::min<uint64_t>(least, q->n_ge[k]);
        for (uint32_t b = 1; b <= B; ++b) {
            const double pb = rgx_qtl_pvalue(rgx_qtl_tstat(q->perm_r[k * ((size_t)B + 1) + b], q->dof), q->dof);
            p[b - 1] = std::min(std::max(pb, 2.2250738585072014e-308), 1.0 - 0x1p-53);
        }
        double a = 0, b2 = 0;
        const int status = rgx_qtl_beta_fit(p.data(), B, &a, &b2);
        if (status != q->beta_status[k] || (status != 2 && (a != q->beta_shape1[k] || b2 != q->beta_shape2[k]))) {
            fprintf(stderr, "row %llu: the fit of its own p differs from the result's\n", (unsigned long long)k); return 1; }
    }
    printf("%u x %u x %u, %u covariates, %u permutations: %llu pairs, %llu rows with pairs, %llu fitted, least n_ge %llu\n", S, K, V, n_cov, B,
           (unsigned long long)q->n_pairs, (unsigned long long)with, (unsigned long long)fitted, (unsigned long long)least);
    fflush(stdout);
    rgx_cohort_qtl_perm_free(q);
    return 0;
}
}  // namespace

// Every result here stays below 64 KiB: the library keeps released blocks of that size and more for later tables until the process ends
// (block_give, api_ctx.cpp), and LeakSanitizer, which stays on, would report that cache at exit.
int main() {
    if (table(64, 30, 40, 2, 199, 5) || table(17, 9, 12, 0, 7, 1) || table(70, 40, 3, 3, 1, 2) || table(9, 50, 400, 1, 130, 3)) return 1;
    double sum = 0;
    for (double x : {1e-3, 0.5, 1.0, 2.5, 10.0, 1e3, 1e6}) sum += rgx_qtl_digamma(x) + rgx_qtl_trigamma(x);
    for (double a : {0.3, 1.0, 2.5, 40.0, 900.0}) for (double b : {0.3, 1.0, 2.5, 40.0, 900.0}) for (double x : {0.0, 1e-12, 1e-3, 0.2, 0.5, 0.9, 1 - 1e-9, 1.0})
        sum += rgx_qtl_betainc(x, a, b);
    if (!(sum == sum)) { fprintf(stderr, "a special function returned NaN inside its domain\n"); return 1; }
    printf("ok\n");
    fflush(stdout);
    return 0;
}
