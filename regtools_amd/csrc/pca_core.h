// pca_core.h -- the arithmetic of the phenotype table's principal components (rgx_cohort_pheno_pcs; contract in include/regtools_amd.h), device +
// host compilable: pca_kernels.hip and the host twin in cohort_pcs.cpp run these same functions, so that Gram matrix and column sums agree bit for
// bit.  The one multiply-add of the contract is an explicit fma(); everything else that rounds switches contraction off for its own body, as
// pheno_core.h does.
#pragma once
#include "pheno_core.h"

namespace rgx {

constexpr uint32_t kPcaMaxSamples = 2048;    // S beyond this is RGX_ERR_ARG: 64 S^2 doubles of chunk partials, an O(S^3) host part
constexpr uint32_t kPcaMaxChunks = 64;       // the contract's chunks: n_chunks = min(64, ceil(K / 1024)), each of L = ceil(K / n_chunks) rows
constexpr uint32_t kPcaChunkRows = 1024;
constexpr uint32_t kPcaTile = 64;            // the device's output tile (samples x samples); no part of the contract

RGX_HD uint32_t pca_n_chunks(uint64_t n_rows) {
    const uint64_t c = (n_rows + kPcaChunkRows - 1) / kPcaChunkRows;
    return (uint32_t)(c < 1 ? 1 : c > kPcaMaxChunks ? kPcaMaxChunks : c);
}
// (no chunk is empty: (c - 1)^2 < 1024 (c - 1) < K for c <= 64)
RGX_HD uint64_t pca_chunk_rows(uint64_t n_rows, uint32_t n_chunks) { return (n_rows + n_chunks - 1) / n_chunks; }

// rank2 is an entry of a table of K rows
RGX_HD bool pca_rank_ok(uint32_t rank2, uint64_t n_rows) { return rank2 >= 2 && (uint64_t)rank2 <= 2 * n_rows; }

// the chain of a chunk partial: one rounding per step
RGX_HD double pca_fma(double a, double b, double acc) { return fma(a, b, acc); }
// the chain of a column sum, and of the chunk partials into their total
RGX_HD double pca_add(double a, double b) { RGX_FP_EXACT return a + b; }

// the sample covariance of columns s and t from the Gram entry and the two column sums
RGX_HD double pca_cov(double gram, double sum_s, double sum_t, uint64_t n_rows) {
    RGX_FP_EXACT
    return (gram - sum_s * sum_t / (double)n_rows) / (double)(n_rows - 1);
}

}  // namespace rgx
