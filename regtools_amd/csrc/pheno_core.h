// pheno_core.h -- per-entry arithmetic of the cohort's splicing phenotype table (rgx_cohort_phenotypes; contract in include/regtools_amd.h), device +
// host compilable: pheno_kernels.hip and the host twin in cohort_pheno.cpp run these same functions, so that the two agree bit for bit.
// Every function that rounds switches contraction off for its own body: hipcc fuses a * b + c into an FMA by default, and not alike for the device
// and the host.  A g++ build of this header (host emulation) needs -ffp-contract=off instead.
#pragma once
#include "common.h"

#if defined(__HIPCC__)
#include <math.h>
#else
#include <cmath>
#endif

#if defined(__clang__)
#define RGX_FP_EXACT _Pragma("clang fp contract(off)")
#else
#define RGX_FP_EXACT
#endif

namespace rgx {

constexpr uint32_t kPhenoPartials = 64;      // the contract's partial sums: sample s goes to partial s % 64 (a wave's strided loop)

// the value of `key` among the ascending keys[lo .. hi), or `hi` when it is not there
RGX_HD uint64_t pheno_find(const uint32_t *keys, uint64_t lo, uint64_t hi, uint32_t key) {
    const uint64_t end = hi;
    while (lo < hi) { const uint64_t mid = lo + (hi - lo) / 2; if (keys[mid] < key) lo = mid + 1; else hi = mid; }
    return lo < end && keys[lo] == key ? lo : end;
}

// One row's view of the matrix and of its cluster's denominators: the count and the denominator of sample s, 0 where the CSR has no entry
struct PhenoRow {
    const uint32_t *col_sample, *val_count, *cs_sample; const unsigned long long *cs_total;
    uint64_t e0, e1, d0, d1;
    RGX_HD uint32_t num(uint32_t s) const { const uint64_t q = pheno_find(col_sample, e0, e1, s); return q < e1 ? val_count[q] : 0u; }
    RGX_HD uint64_t den(uint32_t s) const { const uint64_t q = pheno_find(cs_sample, d0, d1, s); return q < d1 ? (uint64_t)cs_total[q] : 0ull; }
};

// the intron-excision ratio with LeafCutter's pseudocount; den > 0
RGX_HD double pheno_ratio(uint32_t num, uint64_t den) { RGX_FP_EXACT return ((double)num + 0.5) / ((double)den + 0.5); }

RGX_HD double pheno_add(double a, double b) { RGX_FP_EXACT return a + b; }
// (x - mean)^2 as a rounded difference and a rounded product: the add that takes it is a call of its own
RGX_HD double pheno_sq_dev(double x, double mean) { RGX_FP_EXACT const double d = x - mean; return d * d; }
RGX_HD double pheno_mean(double sum, uint32_t n_present) { RGX_FP_EXACT return sum / (double)n_present; }
RGX_HD double pheno_sd(double sum_sq, uint32_t n_samples) { RGX_FP_EXACT return sqrt(sum_sq / (double)n_samples); }
RGX_HD double pheno_z(double x, double mean, double sd) { RGX_FP_EXACT return (x - mean) / sd; }

// the row filters, in the contract's order: 1 = dropped as missing, 2 = dropped as flat, 0 = kept
RGX_HD uint32_t pheno_verdict(uint32_t n_na, uint32_t n_samples, uint32_t na_num, uint32_t na_den, double sd, double min_sd) {
    if (n_na == n_samples || (uint64_t)n_na * na_den > (uint64_t)n_samples * na_num) return 1u;
    if (!(sd > 0.0) || sd < min_sd) return 2u;
    return 0u;
}

// 64 bits that order as z does, -0.0 with +0.0 (no NaN comes here): the sort's key, low word first
RGX_HD uint64_t pheno_key(double z) {
    uint64_t b;
    memcpy(&b, &z, 8);
    if ((b << 1) == 0) b = 0;
    return (b >> 63) ? ~b : b | 0x8000000000000000ull;
}

}  // namespace rgx
