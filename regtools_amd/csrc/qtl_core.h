// qtl_core.h -- the arithmetic of the cohort's nominal cis-sQTL scan (rgx_cohort_qtl_nominal; contract in include/regtools_amd.h), device + host
// compilable: qtl_kernels.hip and the host twin in cohort_qtl.cpp run these same functions, so that residuals, yy, gg, r and slope agree bit for
// bit.  The multiply-adds of the contract are explicit fma()s; everything else that rounds switches contraction off for its own body, as
// pheno_core.h does.
#pragma once
#include "pca_core.h"

namespace rgx {

constexpr uint32_t kQtlMaxSamples = kPcaMaxSamples;
constexpr uint32_t kQtlTile = 64;            // the device's output tile (rows x usable variants); no part of the contract
constexpr uint64_t kQtlMaxPairs = (1ull << 32) - (1ull << 16);
constexpr uint64_t kQtlMaxTiles = 0x7fffffffull;
constexpr uint32_t kQtlMaxCond = 8;          // RGX_QTL_MAX_COND: the most variants a conditional series is conditioned on
constexpr uint32_t kQtlFlagDosage = 0, kQtlFlagRank = 1;     // the device's two flag words: a dosage outside the four values, a rank2 that is no rank

// a step of a dot64 partial and of a pair's chain: one rounding
RGX_HD double qtl_fma(double a, double b, double acc) { return fma(a, b, acc); }
// a halving add of dot64
RGX_HD double qtl_add(double a, double b) { RGX_FP_EXACT return a + b; }
// x[s] behind the projection on a unit vector q with d = dot64(x, q)
RGX_HD double qtl_project(double d, double q, double x) { return fma(-d, q, x); }

// an entry of a unit vector of the conditional pass: v[s] / |v| with nn = dot64(v, v)
RGX_HD double qtl_unit(double x, double nn) { RGX_FP_EXACT return x / sqrt(nn); }

RGX_HD bool qtl_dosage_ok(int8_t d) { return d >= -1 && d <= 2; }
RGX_HD double qtl_mean(uint32_t sum, uint32_t n_present) { RGX_FP_EXACT return (double)sum / (double)n_present; }
// ss of a residual is large enough to divide by: a row that is not flat, a variant the covariates do not explain
RGX_HD bool qtl_enough(double ss, uint32_t n_samples) { RGX_FP_EXACT return ss > 1e-12 * (double)n_samples; }

RGX_HD double qtl_r(double dot, double yy, double gg) { RGX_FP_EXACT const double p = yy * gg; return dot / sqrt(p); }
RGX_HD double qtl_slope(double dot, double gg) { RGX_FP_EXACT return dot / gg; }

// |r| as 64 bits that order as it does (no NaN comes here)
RGX_HD uint64_t qtl_abs_bits(double r) { uint64_t b; memcpy(&b, &r, 8); return b & 0x7fffffffffffffffull; }

// (tid, pos) as one ascending key
RGX_HD uint64_t qtl_key(uint32_t tid, uint32_t pos) { return (uint64_t)tid << 32 | pos; }
// the keys [first, last] a region reaches with its window
RGX_HD uint64_t qtl_key_first(uint32_t tid, uint32_t start, uint32_t window) { return qtl_key(tid, start - (start < window ? start : window)); }
RGX_HD uint64_t qtl_key_last(uint32_t tid, uint32_t end, uint32_t window) {
    const uint64_t e = (uint64_t)end + window;
    return qtl_key(tid, e > 0xffffffffull ? 0xffffffffu : (uint32_t)e);
}
// the same test for one variant's key: what the trans scan leaves out (a region whose last key lies in front of its first reaches nothing)
RGX_HD bool qtl_key_is_cis(uint64_t key, uint32_t tid, uint32_t start, uint32_t end, uint32_t window) {
    return key >= qtl_key_first(tid, start, window) && key <= qtl_key_last(tid, end, window);
}
// the first of the ascending keys[0 .. n) that is not below key (strict: above key)
RGX_HD uint32_t qtl_bound(const uint64_t *keys, uint32_t n, uint64_t key, bool strict) {
    uint32_t lo = 0, hi = n;
    while (lo < hi) { const uint32_t mid = lo + (hi - lo) / 2; if (keys[mid] < key || (strict && keys[mid] == key)) lo = mid + 1; else hi = mid; }
    return lo;
}

}  // namespace rgx
