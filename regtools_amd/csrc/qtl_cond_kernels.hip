// qtl_cond_kernels.hip -- device half of the conditional cis-sQTL permutation pass (rgx_cohort_qtl_permute_conditional, cohort_qtl_cond.cpp;
// contract in include/regtools_amd.h; arithmetic in qtl_core.h, which the host twin runs too).  The residuals, the compaction, the G transpose and
// the plan are qtl_kernels.hip's; the slab loop and the wave's dot64 are qtl_tile.h's; the reference has no counterpart.  A SERIES c is table row
// series_row[c] with the m_c variants it is conditioned on; its PLACES are the row's usable cis variants in order, pb[c] .. pb[c + 1).
//   k_qtl_cond_counts  a thread per series: the row's number of usable cis variants, for the scan that gives pb
//   k_qtl_cond_basis   a wave per series: the conditioning residuals orthonormalised in order (each projected twice on those before it), z; then
//                 the row's residual projected on every z_j in order, y' with yy'; the status (1 collinear, 2 flat).  The vector sits in the
//                 wave's slice of LDS, where lane l alone touches the entries s % 64 == l -- of z in HBM too, so a lane reads back only what it
//                 wrote itself.  A conditioning variant that is not usable raises the flag word.
//   k_qtl_cond_beta    a wave per place: the variant's residual projected on every z_j in order; beta_j = the dot64 in front of projection j,
//                 gg' = dot64 of what is left.  beta lies in kQtlMaxCond planes of `cap` doubles, gg' in one.
//   k_qtl_perm_cond    one workgroup per (series, 64 consecutive permutations): y' in dynamic LDS; alpha[j][b] = the ONE chain fma(y'[perm[b][s]],
//                 z_j[s], acc) for its 64 permutations x m_c in 4 KB of static LDS, a wave per j; then k_qtl_perm's tile walk with QtlTilePerms and
//                 qtl_tile_product as they are.  The epilogue takes m_c fmas from a chain, dot = fma(-alpha[j][b], beta[j][u], dot) in order, and
//                 leaves out the places whose gg' is not enough; the largest |r| bits and the place stay in registers across tiles, the 16 lanes
//                 that share a permutation reduce by shuffles and one of them stores perm_r[c][b]: no atomics, no pair ever stored.
//   k_qtl_cond_best    a wave per series: its lanes count the places that take part (n_cis); lane 0 redoes the winning pair's chain, its alphas
//                 and the correction from row-major data: best_variant, best_r, best_slope.
// Every word has one writer (the flag word aside: its writers all store 1).  256 threads per workgroup, wave64, FP64 vector FMAs.
#include "qtl_tile.h"

namespace rgx {

namespace {
constexpr uint32_t kNoU = 0xffffffffu;
constexpr unsigned long long kNoPlace = ~0ull;
}  // namespace

// cnt has N + 1 words: the last is 0, and its place in the scan is the number of places
__global__ __launch_bounds__(256) void k_qtl_cond_counts(QtlCond q, uint32_t *__restrict__ cnt) {
    const uint64_t c = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (c > q.N) return;
    cnt[c] = c < q.N ? q.count[q.series_row[c]] : 0;
}

// dynamic LDS: 4 * S doubles
__global__ __launch_bounds__(256) void k_qtl_cond_basis(QtlCond q, const double *__restrict__ Y, const double *__restrict__ G,
                                                        const uint8_t *__restrict__ verdict, uint32_t *__restrict__ flag) {
    extern __shared__ __attribute__((aligned(16))) double qtl_lds[];
    const uint32_t l = threadIdx.x % 64, w = threadIdx.x / 64, S = q.S;
    const uint64_t c = (uint64_t)blockIdx.x * 4 + w;
    if (c >= q.N) return;                                    // (a wave leaves whole; no barrier follows)
    double *x = qtl_lds + (size_t)w * S;
    const uint32_t k = q.series_row[c], j0 = q.cond_begin[c], m = q.cond_begin[c + 1] - j0;
    double *zc = q.z + c * kQtlMaxCond * S;
    bool collinear = false;
    for (uint32_t j = 0; j < m && !collinear; ++j) {         // (j, v and every test are the same for the whole wave)
        const uint32_t v = q.cond_variant[j0 + j];
        if (verdict[v]) { if (!l) *flag = 1; collinear = true; break; }
        for (uint32_t s = l; s < S; s += 64) x[s] = G[(size_t)v * S + s];
        for (uint32_t pass = 0; pass < 2; ++pass) for (uint32_t i = 0; i < j; ++i) {
            const double *zi = zc + (size_t)i * S;
            const double d = qtl_dot64(x, zi, S, l);
            for (uint32_t s = l; s < S; s += 64) x[s] = qtl_project(d, zi[s], x[s]);
        }
        const double nn = qtl_dot64(x, x, S, l);
        if (!qtl_enough(nn, S)) { collinear = true; break; }
        for (uint32_t s = l; s < S; s += 64) zc[(size_t)j * S + s] = qtl_unit(x[s], nn);
    }
    if (collinear) {
        if (!l) { q.yyc[c] = 0.0; q.status[c] = 1; }
        return;
    }
    for (uint32_t s = l; s < S; s += 64) x[s] = Y[(size_t)k * S + s];
    for (uint32_t j = 0; j < m; ++j) {
        const double *zj = zc + (size_t)j * S;
        const double d = qtl_dot64(x, zj, S, l);
        for (uint32_t s = l; s < S; s += 64) x[s] = qtl_project(d, zj[s], x[s]);
    }
    const double ss = qtl_dot64(x, x, S, l);
    for (uint32_t s = l; s < S; s += 64) q.yc[c * S + s] = x[s];
    if (!l) { q.yyc[c] = ss; q.status[c] = qtl_enough(ss, S) ? 0 : 2; }
}

// the grid covers `cap` places, four a workgroup; the places there are: pb[N].  dynamic LDS: 4 * S doubles
__global__ __launch_bounds__(256) void k_qtl_cond_beta(QtlCond q, const double *__restrict__ G) {
    extern __shared__ __attribute__((aligned(16))) double qtl_lds[];
    const uint32_t l = threadIdx.x % 64, w = threadIdx.x / 64, S = q.S;
    const uint64_t p = (uint64_t)blockIdx.x * 4 + w;
    if (p >= q.pb[q.N] || p >= q.cap) return;
    // the last series whose places begin at or in front of p: it has places, since the next one's begin behind p
    uint32_t c_lo = 0, c_hi = q.N;
    while (c_lo + 1 < c_hi) { const uint32_t mid = c_lo + (c_hi - c_lo) / 2; if (q.pb[mid] <= p) c_lo = mid; else c_hi = mid; }
    const uint32_t c = c_lo;
    if (q.status[c]) return;
    const uint32_t k = q.series_row[c], m = q.cond_begin[c + 1] - q.cond_begin[c], v = q.u_var[q.lo[k] + ((uint32_t)p - q.pb[c])];
    double *x = qtl_lds + (size_t)w * S;
    for (uint32_t s = l; s < S; s += 64) x[s] = G[(size_t)v * S + s];
    for (uint32_t j = 0; j < m; ++j) {
        const double *zj = q.z + ((size_t)c * kQtlMaxCond + j) * S;
        const double d = qtl_dot64(x, zj, S, l);
        if (!l) q.beta[(size_t)j * q.cap + p] = d;
        for (uint32_t s = l; s < S; s += 64) x[s] = qtl_project(d, zj[s], x[s]);
    }
    const double ss = qtl_dot64(x, x, S, l);
    if (!l) q.ggc[p] = ss;
}

// permT: S rows of ldp uint16, ldp a multiple of 64 at or above B + 1, index 0 behind B; Gt: S rows of ldg doubles, ldg at or above U + 63, zero
// behind U.  n_ptiles = ldp / 64; the grid is N * n_ptiles.  Dynamic LDS: S doubles.
__global__ __launch_bounds__(256) void k_qtl_perm_cond(QtlCond q, const uint16_t *__restrict__ permT, size_t ldp, uint32_t n_ptiles, uint32_t n_perm1,
                                                       const double *__restrict__ Gt, size_t ldg, double *__restrict__ perm_r,
                                                       uint32_t *__restrict__ best_u) {
    extern __shared__ __attribute__((aligned(16))) double y_lds[];
    __shared__ double alpha[kQtlMaxCond][kQtlTile];
    const uint32_t tid = threadIdx.x, tx = tid % 16, ty = tid / 16, S = q.S;
    const uint32_t c = blockIdx.x / n_ptiles, b0 = (blockIdx.x % n_ptiles) * kQtlTile;
    const uint32_t k = q.series_row[c], first = q.lo[k], m = q.cond_begin[c + 1] - q.cond_begin[c];
    const uint32_t n = q.status[c] || q.pb[c + 1] > q.cap ? 0 : q.count[k];          // (cap is at or above every end: no place lies outside the planes)
    double *out = perm_r + (size_t)c * n_perm1;
    const QtlTilePerms a_src{permT + b0 + tid % kQtlTile, ldp, y_lds};

    unsigned long long top[4], top_at[4];
#pragma unroll
    for (uint32_t i = 0; i < 4; ++i) { top[i] = 0; top_at[i] = kNoPlace; }

    if (n) {                                                 // (c, k, first, n and m are the same for the whole workgroup)
        for (uint32_t s = tid; s < S; s += 256) y_lds[s] = q.yc[(size_t)c * S + s];
        __syncthreads();
        // wave w owns the chains of j = w and w + 4: lane b's index is contiguous with its neighbours', z_j[s] is one address for the wave
        for (uint32_t j = tid / kQtlTile; j < m; j += 4) {
            const double *zj = q.z + ((size_t)c * kQtlMaxCond + j) * S;
            double acc = 0.0;
            for (uint32_t s = 0; s < S; ++s) acc = qtl_fma(y_lds[a_src.load(s)], zj[s], acc);
            alpha[j][tid % kQtlTile] = acc;
        }
        __syncthreads();
        const double y2 = q.yyc[c];
        const size_t base = q.pb[c];

        for (uint32_t v0 = first; v0 - first < n; v0 += kQtlTile) {
            double acc[4][4];
            qtl_tile_product(a_src, Gt + v0 + tid % kQtlTile, ldg, S, acc);

            // the place ascends with j inside a thread and with v0: a strictly larger |r| alone replaces, so the earliest of equals stays
#pragma unroll
            for (uint32_t j = 0; j < 4; ++j) {
                const uint32_t u = v0 + qtl_tile_at(j, tx);
                if (u - first >= n) continue;
                const size_t p = base + (u - first);
                const double g2 = q.ggc[p];
                if (!qtl_enough(g2, S)) continue;
                double bt[kQtlMaxCond];
#pragma unroll
                for (uint32_t jj = 0; jj < kQtlMaxCond; ++jj) bt[jj] = jj < m ? q.beta[(size_t)jj * q.cap + p] : 0.0;
#pragma unroll
                for (uint32_t i = 0; i < 4; ++i) {
                    const uint32_t b = qtl_tile_at(i, ty);
                    double dot = acc[i][j];
#pragma unroll
                    for (uint32_t jj = 0; jj < kQtlMaxCond; ++jj) if (jj < m) dot = qtl_project(alpha[jj][b], bt[jj], dot);
                    const unsigned long long bits = qtl_abs_bits(qtl_r(dot, y2, g2));
                    if (top_at[i] == kNoPlace || bits > top[i]) { top[i] = bits; top_at[i] = u; }
                }
            }
        }
    }

    // the 16 lanes tx = 0 .. 15 of one ty share a permutation: they are neighbours inside a wave.  A series without pairs comes here with the
    // bits of +0.0 and no place in every lane.
#pragma unroll
    for (uint32_t i = 0; i < 4; ++i) {
#pragma unroll
        for (uint32_t off = 8; off; off >>= 1) {
            const unsigned long long ob = __shfl_xor(top[i], off, 64), oa = __shfl_xor(top_at[i], off, 64);
            if (oa != kNoPlace && (top_at[i] == kNoPlace || ob > top[i] || (ob == top[i] && oa < top_at[i]))) { top[i] = ob; top_at[i] = oa; }
        }
        const uint32_t b = b0 + qtl_tile_at(i, ty);
        if (tx || b >= n_perm1) continue;
        double v; const unsigned long long bits = top[i];
        memcpy(&v, &bits, 8);
        out[b] = v;
        if (!b) best_u[c] = (uint32_t)top_at[i];             // (no place: kNoU)
    }
}

__global__ __launch_bounds__(256) void k_qtl_cond_best(QtlCond q, const double *__restrict__ G, const uint32_t *__restrict__ best_u,
                                                       uint32_t *__restrict__ best_variant, double *__restrict__ best_r,
                                                       double *__restrict__ best_slope, uint32_t *__restrict__ n_cis, uint32_t *__restrict__ n_window) {
    const uint32_t l = threadIdx.x % 64, S = q.S;
    const uint64_t c = (uint64_t)blockIdx.x * 4 + threadIdx.x / 64;
    if (c >= q.N) return;
    const uint32_t k = q.series_row[c], first = q.lo[k], m = q.cond_begin[c + 1] - q.cond_begin[c];
    const uint32_t n = q.status[c] || q.pb[c + 1] > q.cap ? 0 : q.count[k];          // (cap is at or above every end: no place lies outside the planes)
    const size_t base = q.pb[c];
    uint32_t part = 0;
    for (uint32_t i = l; i < n; i += 64) part += qtl_enough(q.ggc[base + i], S);
#pragma unroll
    for (uint32_t off = 32; off; off >>= 1) part += __shfl_xor(part, off, 64);
    if (l) return;
    n_cis[c] = part; n_window[c] = q.count[k];
    const uint32_t u = best_u[c];
    if (u == kNoU) { best_variant[c] = 0xffffffffu; best_r[c] = 0.0; best_slope[c] = 0.0; return; }
    const uint32_t v = q.u_var[u];
    const size_t p = base + (u - first);
    const double *y = q.yc + (size_t)c * S, *x = G + (size_t)v * S;
    double dot = 0.0;
    for (uint32_t s = 0; s < S; ++s) dot = qtl_fma(y[s], x[s], dot);
    for (uint32_t j = 0; j < m; ++j) {
        const double *zj = q.z + ((size_t)c * kQtlMaxCond + j) * S;
        double a = 0.0;
        for (uint32_t s = 0; s < S; ++s) a = qtl_fma(y[s], zj[s], a);
        dot = qtl_project(a, q.beta[(size_t)j * q.cap + p], dot);
    }
    const double g2 = q.ggc[p];
    best_variant[c] = v; best_r[c] = qtl_r(dot, q.yyc[c], g2); best_slope[c] = qtl_slope(dot, g2);
}

void launch_qtl_cond_counts(const QtlCond &q, uint32_t *cnt, hipStream_t st) {
    hipLaunchKernelGGL(k_qtl_cond_counts, dim3(q.N / 256 + 1), dim3(256), 0, st, q, cnt);
}
void launch_qtl_cond_prepare(const QtlCond &q, const double *Y, const double *G, const uint8_t *verdict, uint32_t *flag, hipStream_t st) {
    hipLaunchKernelGGL(k_qtl_cond_basis, dim3((q.N + 3) / 4), dim3(256), (size_t)4 * q.S * 8, st, q, Y, G, verdict, flag);
    if (q.cap) hipLaunchKernelGGL(k_qtl_cond_beta, dim3((uint32_t)((q.cap + 3) / 4)), dim3(256), (size_t)4 * q.S * 8, st, q, G);
}
void launch_qtl_perm_cond(const QtlCond &q, const uint16_t *permT, size_t ldp, uint32_t n_perm1, const double *Gt, size_t ldg, double *perm_r,
                          uint32_t *best_u, hipStream_t st) {
    const uint32_t n_ptiles = (uint32_t)(ldp / kQtlTile);
    hipLaunchKernelGGL(k_qtl_perm_cond, dim3(q.N * n_ptiles), dim3(256), (size_t)q.S * 8, st, q, permT, ldp, n_ptiles, n_perm1, Gt, ldg, perm_r, best_u);
}
void launch_qtl_cond_best(const QtlCond &q, const double *G, const uint32_t *best_u, uint32_t *best_variant, double *best_r, double *best_slope,
                          uint32_t *n_cis, uint32_t *n_window, hipStream_t st) {
    hipLaunchKernelGGL(k_qtl_cond_best, dim3((q.N + 3) / 4), dim3(256), 0, st, q, G, best_u, best_variant, best_r, best_slope, n_cis, n_window);
}

}  // namespace rgx
