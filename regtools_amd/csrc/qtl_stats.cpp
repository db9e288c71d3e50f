// qtl_stats.cpp -- the mathematics of the sQTL calls that runs on the host and touches neither the device nor a cohort (contract in
// include/regtools_amd.h): Student's t and its p (rgx_qtl_tstat, rgx_qtl_pvalue), the |r| a p asks for (rgx_qtl_r_threshold), the digamma, trigamma
// and incomplete beta functions and the beta fit with their exported faces, the finish of one series of permuted |r| (qtl_series_finish, declared
// in qtl_run.h) and the permutation generator (rgx_qtl_permutations).  Plain C++ in the widest type the host has: it compiles without HIP and
// without the library's internal headers; arithmetic shared with the device: qtl_core.h.
#include "../../include/regtools_amd.h"
#include "qtl_core.h"

#include <algorithm>
#include <cfloat>
#include <cmath>
#include <cstdio>

using namespace rgx;

// ---- t, p and the special functions --------------------------------------------------------------------------------------------------------------
extern "C" double rgx_qtl_tstat(double r, uint32_t dof) {
    RGX_FP_EXACT
    const double u = 1.0 - r * r;
    if (u <= 0.0) return copysign(INFINITY, r);
    return r * sqrt((double)dof / u);
}

namespace {

// the continued fraction of the incomplete beta function (Lentz's method, modified: Thompson and Barnett 1986), in the widest type the host has
long double qtl_beta_cf(long double a, long double b, long double x) {
    const long double tiny = 1e-300L, eps = 1e-19L;
    long double c = 1.0L, d = 1.0L - (a + b) * x / (a + 1.0L);
    if (fabsl(d) < tiny) d = tiny;
    d = 1.0L / d;
    long double h = d;
    for (int m = 1; m <= 10000; ++m) {
        const long double m2 = 2.0L * m;
        long double num = m * (b - m) * x / ((a + m2 - 1.0L) * (a + m2));
        d = 1.0L + num * d; if (fabsl(d) < tiny) d = tiny;
        c = 1.0L + num / c; if (fabsl(c) < tiny) c = tiny;
        d = 1.0L / d; h *= d * c;
        num = -(a + m) * (a + b + m) * x / ((a + m2) * (a + m2 + 1.0L));
        d = 1.0L + num * d; if (fabsl(d) < tiny) d = tiny;
        c = 1.0L + num / c; if (fabsl(c) < tiny) c = tiny;
        d = 1.0L / d;
        const long double del = d * c;
        h *= del;
        if (fabsl(del - 1.0L) < eps) break;
    }
    return h;
}
// Gamma(n / 2 + 1 / 2) / (Gamma(n / 2) Gamma(1 / 2)) = 1 / B(n / 2, 1 / 2), by the recurrence over n - 2 from n = 1 (1 / pi) or n = 2 (1 / 2)
long double inv_beta_half(uint32_t n) {
    long double v = n % 2 ? 1.0L / 3.14159265358979323846264338327950288L : 0.5L;
    for (uint32_t i = n % 2 ? 1 : 2; i < n; i += 2) v *= (long double)(i + 1) / (long double)i;       // (a -> a + 1 multiplies by (a + 1/2) / a, a = i / 2)
    return v;
}

long double digamma_l(long double x) {
    long double acc = 0.0L;
    for (; x < 32.0L; x += 1.0L) acc -= 1.0L / x;
    const long double i2 = 1.0L / (x * x);
    // sum B_2n / (2n x^2n), n = 1 .. 8
    const long double series = i2 * (1.0L / 12 - i2 * (1.0L / 120 - i2 * (1.0L / 252 - i2 * (1.0L / 240 - i2 * (1.0L / 132 - i2 * (691.0L / 32760 -
                               i2 * (1.0L / 12 - i2 * (3617.0L / 8160))))))));
    return acc + logl(x) - 0.5L / x - series;
}
long double trigamma_l(long double x) {
    long double acc = 0.0L;
    for (; x < 32.0L; x += 1.0L) acc += 1.0L / (x * x);
    const long double i2 = 1.0L / (x * x);
    // sum B_2n / x^(2n + 1), n = 1 .. 8
    const long double series = i2 * (1.0L / 6 - i2 * (1.0L / 30 - i2 * (1.0L / 42 - i2 * (1.0L / 30 - i2 * (5.0L / 66 - i2 * (691.0L / 2730 -
                               i2 * (7.0L / 6 - i2 * (3617.0L / 510))))))));
    return acc + 1.0L / x + 0.5L * i2 + series / x;
}
long double betainc_l(long double x, long double a, long double b) {
    if (x <= 0.0L) return 0.0L;
    if (x >= 1.0L) return 1.0L;
    const long double y = 1.0L - x;                                     // (exact: x is a double)
    const long double front = expl(a * logl(x) + b * log1pl(-x) - lgammal(a) - lgammal(b) + lgammal(a + b));
    long double p;
    if (x < (a + 1.0L) / (a + b + 2.0L)) p = front * qtl_beta_cf(a, b, x) / a;
    else p = 1.0L - front * qtl_beta_cf(b, a, y) / b;
    return p < 0.0L ? 0.0L : p > 1.0L ? 1.0L : p;
}

int beta_fit_l(const double *p, uint32_t n, long double &a, long double &b) {
    a = b = NAN;
    if (n < 2) return 2;
    long double sum = 0.0L, l1 = 0.0L, l2 = 0.0L;
    for (uint32_t i = 0; i < n; ++i) { sum += p[i]; l1 += logl((long double)p[i]); l2 += log1pl(-(long double)p[i]); }
    const long double m = sum / n;
    long double ss = 0.0L;
    for (uint32_t i = 0; i < n; ++i) { const long double d = (long double)p[i] - m; ss += d * d; }
    const long double v = ss / n;
    if (!(v > 0.0L)) return 2;
    const long double a0 = m * (m * (1.0L - m) / v - 1.0L), b0 = a0 * (1.0L / m - 1.0L);
    if (!(a0 > 0.0L) || !(b0 > 0.0L) || std::isinf(a0) || std::isinf(b0)) return 2;
    l1 /= n; l2 /= n;
    a = a0; b = b0;
    for (int step = 0; step < 100; ++step) {
        const long double pab = digamma_l(a + b), tab = trigamma_l(a + b);
        const long double g1 = digamma_l(a) - pab - l1, g2 = digamma_l(b) - pab - l2;
        const long double j11 = trigamma_l(a) - tab, j22 = trigamma_l(b) - tab, j12 = -tab;
        const long double det = j11 * j22 - j12 * j12;
        long double da = -(j22 * g1 - j12 * g2) / det, db = -(j11 * g2 - j12 * g1) / det;
        if (da != da || db != db || std::isinf(da) || std::isinf(db)) break;
        for (int h = 0; h < 200 && (!(a + da > 0.0L) || !(b + db > 0.0L)); ++h) { da *= 0.5L; db *= 0.5L; }
        if (!(a + da > 0.0L) || !(b + db > 0.0L)) break;
        const bool done = fabsl(da) < 1e-12L * a && fabsl(db) < 1e-12L * b;
        a += da; b += db;
        if (done) return 0;
    }
    a = a0; b = b0;
    return 1;
}

}  // namespace

extern "C" double rgx_qtl_pvalue(double t, uint32_t dof) {
    if (t != t || !dof) return NAN;
    if (std::isinf(t)) return 0.0;
    if (t == 0.0) return 1.0;
    const long double n = dof, a = 0.5L * n, b = 0.5L, t2 = (long double)t * (long double)t;
    const long double x = n / (n + t2), y = t2 / (n + t2);             // (y = 1 - x without the cancellation)
    // x^a y^b / B(a, b), with log x = -log1p(t^2 / n)
    const long double front = expl(-a * log1pl(t2 / n)) * sqrtl(y) * inv_beta_half(dof);
    long double p;
    if (x < (a + 1.0L) / (a + b + 2.0L)) p = front * qtl_beta_cf(a, b, x) / a;
    else p = 1.0L - front * qtl_beta_cf(b, a, y) / b;
    return (double)(p < 0.0L ? 0.0L : p > 1.0L ? 1.0L : p);
}

extern "C" double rgx_qtl_r_threshold(double p, uint32_t dof) {
    if (!(p >= 0.0) || !dof) return NAN;
    if (p >= 1.0) return 0.0;
    auto at = [](uint64_t bits) { double r; memcpy(&r, &bits, 8); return r; };
    const double one = 1.0;
    uint64_t lo = 0, hi;                                                // +0.0 fails (its p is 1), 1.0 passes (its p is 0)
    memcpy(&hi, &one, 8);
    while (hi - lo > 1) {
        const uint64_t mid = lo + (hi - lo) / 2;
        if (rgx_qtl_pvalue(rgx_qtl_tstat(at(mid), dof), dof) <= p) hi = mid; else lo = mid;
    }
    return at(hi);
}

extern "C" double rgx_qtl_digamma(double x) { return x > 0.0 ? (double)digamma_l(x) : NAN; }
extern "C" double rgx_qtl_trigamma(double x) { return x > 0.0 ? (double)trigamma_l(x) : NAN; }
extern "C" double rgx_qtl_betainc(double x, double a, double b) {
    if (!(a > 0.0) || !(b > 0.0) || !(x >= 0.0) || !(x <= 1.0) || std::isinf(a) || std::isinf(b)) return NAN;
    return (double)betainc_l(x, a, b);
}
extern "C" int rgx_qtl_beta_fit(const double *p, uint32_t n, double *shape1, double *shape2) {
    long double a = NAN, b = NAN;
    int status = 2;
    if (p) {
        bool inside = true;
        for (uint32_t i = 0; i < n; ++i) inside = inside && p[i] > 0.0 && p[i] < 1.0;
        if (inside) status = beta_fit_l(p, n, a, b);
    }
    if (shape1) *shape1 = (double)a;
    if (shape2) *shape2 = (double)b;
    return status;
}

// One series of B + 1 |r| values (a row's, a group's): n_ge and p_perm, then -- when the series has pairs -- the beta approximation of the p of
// b = 1 .. B and p_beta at best_r.  p: room for B doubles.  The sums are in ascending b, so the result does not depend on who runs it.
void qtl_series_finish(const double *row, uint32_t B, double best_r, uint32_t dof, bool has_pairs, double *p, uint32_t &n_ge_out, double &p_perm,
                       double &shape1, double &shape2, double &p_beta, uint8_t &status) {
    const uint64_t top = qtl_abs_bits(row[0]);
    uint32_t n_ge = 0;
    for (uint32_t b = 1; b <= B; ++b) n_ge += qtl_abs_bits(row[b]) >= top;
    n_ge_out = n_ge;
    p_perm = (double)(n_ge + 1) / (double)(B + 1);
    shape1 = shape2 = p_beta = NAN; status = 2;
    if (!has_pairs) return;
    for (uint32_t b = 1; b <= B; ++b) {
        const double pb = rgx_qtl_pvalue(rgx_qtl_tstat(row[b], dof), dof);
        p[b - 1] = pb < DBL_MIN ? DBL_MIN : pb > 1.0 - 0x1p-53 ? 1.0 - 0x1p-53 : pb;
    }
    long double a, b2;
    status = (uint8_t)beta_fit_l(p, B, a, b2);
    if (status == 2) return;
    shape1 = (double)a; shape2 = (double)b2;
    const double x = rgx_qtl_pvalue(rgx_qtl_tstat(best_r, dof), dof);
    p_beta = (double)betainc_l(x, shape1, shape2);
}

// ---- the permutations -----------------------------------------------------------------------------------------------------------------------------
extern "C" int rgx_qtl_permutations(uint32_t n_samples, uint32_t n_perm, uint64_t seed, uint16_t *out, char *err, size_t errlen) {
    const uint32_t S = n_samples;
    const bool bad = !S || S > 65536u || n_perm > 65535u || !out;
    if (bad && err && errlen) snprintf(err, errlen, "regtools_amd: rgx_qtl_permutations takes 1 to 65536 samples, at most 65535 permutations and room for them\n");
    if (bad) return RGX_ERR_ARG;
    uint64_t z = seed;
    auto next = [&]() {
        z += 0x9E3779B97F4A7C15ull;
        uint64_t x = z;
        x = (x ^ x >> 30) * 0xBF58476D1CE4E5B9ull;
        x = (x ^ x >> 27) * 0x94D049BB133111EBull;
        return x ^ x >> 31;
    };
    for (uint32_t b = 0; b <= n_perm; ++b) {
        uint16_t *p = out + (size_t)b * S;
        for (uint32_t s = 0; s < S; ++s) p[s] = (uint16_t)s;
        if (!b) continue;
        for (uint32_t i = S - 1; i >= 1; --i) {
            const uint32_t j = (uint32_t)(((unsigned __int128)next() * (i + 1)) >> 64);
            std::swap(p[i], p[j]);
        }
    }
    return RGX_OK;
}
