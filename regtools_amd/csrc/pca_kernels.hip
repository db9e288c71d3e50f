// pca_kernels.hip -- device half of the phenotype table's principal components (rgx_cohort_pheno_pcs, cohort_pcs.cpp; contract in
// include/regtools_amd.h; arithmetic in pca_core.h, which the host twin runs too): the S x S Gram matrix and the column sums of the K x S table
// q[k][s] = T[rank2[k][s]] of normal quantiles.  The reference has no counterpart.
//   k_pca_gram    one workgroup per (pair of 64-sample tiles with s-tile <= t-tile, chunk of rows): the chunk's partial of the 64 x 64 outputs,
//                 4 x 4 per thread in registers, each the contract's chain acc = fma(q[k][s], q[k][t], acc) in ascending k from +0.0 -- one
//                 thread owns a chain from its start to its end.  The diagonal pairs compute their whole tile, and wave 0 of each also the
//                 chunk's column sums of its 64 samples.
//   k_pca_reduce  per output element the chunk partials added in ascending chunk order from +0.0; both triangles and col_sum.
// No atomics, every word has one writer (the flag of a bad rank2 aside: its writers all store 1).  The rows come in slabs of 16: two 16 x 64
// panels gathered through T into LDS as doubles (consecutive lanes take consecutive samples of the row-major rank2), the next slab's gathers in
// flight under the current slab's FMAs.  A thread's four rows are 2 ty, 2 ty + 1, 32 + 2 ty, 33 + 2 ty and its columns likewise from tx, so that
// every 16-byte LDS load of a wave is conflict-free WITHOUT padding: the sixteen tx of a lane group read sixteen consecutive 16-byte slots -- one
// 256-byte bank row -- and the ty of a group read two addresses that the lanes share (a broadcast each).
// 256 threads per workgroup, wave64, FP64 vector FMAs (the f64 MFMA's order of adding its four products is not documented: not used).
#include "kernels.h"
#include "pca_core.h"

namespace rgx {

namespace {

constexpr uint32_t kSlab = 16;               // rows per trip through LDS
constexpr uint32_t kPerThread = kSlab * kPcaTile / 256;   // a thread's entries of one panel of one slab

// pair p of the tiles (ti <= tj) in row-major order of the upper triangle
__device__ __forceinline__ void pca_pair(uint32_t p, uint32_t n_tiles, uint32_t &ti, uint32_t &tj) {
    ti = 0;
    while (p >= n_tiles - ti) { p -= n_tiles - ti; ++ti; }
    tj = ti + p;
}

// a thread's entries of the slab at row k0 for the tile at sample s0: entry j is row k0 + tid / 64 + 4 j, sample s0 + tid % 64.  Outside the
// table, and for a rank2 that is no rank of a table of K rows (reported through *bad), the entry is +0.0 and T is not read.
__device__ __forceinline__ void pca_gather(const uint32_t *__restrict__ rank2, const double *__restrict__ T, uint64_t K, uint32_t S, uint64_t k0,
                                           uint64_t k_end, uint32_t s0, uint32_t *__restrict__ bad, double (&v)[kPerThread]) {
    const uint32_t s = s0 + threadIdx.x % kPcaTile;
#pragma unroll
    for (uint32_t j = 0; j < kPerThread; ++j) {
        const uint64_t k = k0 + threadIdx.x / kPcaTile + 4 * j;
        v[j] = 0.0;
        if (k < k_end && s < S) {
            const uint32_t r = rank2[k * S + s];
            if (pca_rank_ok(r, K)) v[j] = T[r - 2]; else *bad = 1;
        }
    }
}

}  // namespace

// part: per (pair, chunk) a 64 x 64 tile, row-major; col_part: per chunk S_pad = n_tiles * 64 column sums
__global__ __launch_bounds__(256) void k_pca_gram(const uint32_t *__restrict__ rank2, const double *__restrict__ T, uint64_t K, uint32_t S,
                                                  uint32_t n_tiles, uint32_t n_chunks, uint64_t chunk_rows, double *__restrict__ part,
                                                  double *__restrict__ col_part, uint32_t *__restrict__ bad) {
    __shared__ __attribute__((aligned(16))) double A[kSlab][kPcaTile];
    __shared__ __attribute__((aligned(16))) double B[kSlab][kPcaTile];
    uint32_t ti, tj;
    pca_pair(blockIdx.x, n_tiles, ti, tj);
    const uint32_t chunk = blockIdx.y, tid = threadIdx.x, tx = tid % 16, ty = tid / 16;
    const uint64_t k_begin = (uint64_t)chunk * chunk_rows, k_end = k_begin + chunk_rows < K ? k_begin + chunk_rows : K;
    const bool diag = ti == tj;

    double acc[4][4];
#pragma unroll
    for (uint32_t i = 0; i < 4; ++i)
#pragma unroll
        for (uint32_t j = 0; j < 4; ++j) acc[i][j] = 0.0;
    double col = 0.0;                                        // (wave 0 of a diagonal pair: the column sum of sample ti * 64 + tid)

    double va[kPerThread], vb[kPerThread];
    pca_gather(rank2, T, K, S, k_begin, k_end, ti * kPcaTile, bad, va);
    pca_gather(rank2, T, K, S, k_begin, k_end, tj * kPcaTile, bad, vb);
    for (uint64_t k0 = k_begin; k0 < k_end; k0 += kSlab) {
#pragma unroll
        for (uint32_t j = 0; j < kPerThread; ++j) { A[tid / kPcaTile + 4 * j][tid % kPcaTile] = va[j]; B[tid / kPcaTile + 4 * j][tid % kPcaTile] = vb[j]; }
        __syncthreads();
        if (k0 + kSlab < k_end) {                            // (the same for the whole workgroup)
            pca_gather(rank2, T, K, S, k0 + kSlab, k_end, ti * kPcaTile, bad, va);
            pca_gather(rank2, T, K, S, k0 + kSlab, k_end, tj * kPcaTile, bad, vb);
        }
        const uint32_t rows = k_end - k0 < kSlab ? (uint32_t)(k_end - k0) : kSlab;
        auto step = [&](uint32_t kk) {
            const double2 a0 = *(const double2 *)&A[kk][2 * ty], a1 = *(const double2 *)&A[kk][32 + 2 * ty];
            const double2 b0 = *(const double2 *)&B[kk][2 * tx], b1 = *(const double2 *)&B[kk][32 + 2 * tx];
            const double a[4] = {a0.x, a0.y, a1.x, a1.y}, b[4] = {b0.x, b0.y, b1.x, b1.y};
#pragma unroll
            for (uint32_t i = 0; i < 4; ++i)
#pragma unroll
                for (uint32_t j = 0; j < 4; ++j) acc[i][j] = pca_fma(a[i], b[j], acc[i][j]);
        };
        if (rows == kSlab) {
#pragma unroll
            for (uint32_t kk = 0; kk < kSlab; ++kk) step(kk);
        } else {
            for (uint32_t kk = 0; kk < rows; ++kk) step(kk);
        }
        if (diag && tid < kPcaTile) for (uint32_t kk = 0; kk < rows; ++kk) col = pca_add(col, A[kk][tid]);
        __syncthreads();
    }

    double *out = part + ((size_t)blockIdx.x * n_chunks + chunk) * (kPcaTile * kPcaTile);
#pragma unroll
    for (uint32_t i = 0; i < 4; ++i) {
        const uint32_t r = (i < 2 ? 0 : 32) + 2 * ty + (i & 1);
        *(double2 *)&out[r * kPcaTile + 2 * tx] = make_double2(acc[i][0], acc[i][1]);
        *(double2 *)&out[r * kPcaTile + 32 + 2 * tx] = make_double2(acc[i][2], acc[i][3]);
    }
    if (diag && tid < kPcaTile) col_part[(size_t)chunk * n_tiles * kPcaTile + ti * kPcaTile + tid] = col;
}

// gram[s][t] = gram[t][s] for s <= t, and col_sum[s] by the threads of the diagonal
__global__ __launch_bounds__(256) void k_pca_reduce(const double *__restrict__ part, const double *__restrict__ col_part, uint32_t S, uint32_t n_tiles,
                                                    uint32_t n_chunks, double *__restrict__ gram, double *__restrict__ col_sum) {
    const uint32_t t = blockIdx.x * 64 + threadIdx.x % 64, s = blockIdx.y * 4 + threadIdx.x / 64;
    if (s >= S || t >= S || s > t) return;
    const uint32_t ti = s / kPcaTile, tj = t / kPcaTile;
    const size_t pair = (size_t)ti * n_tiles - (size_t)ti * (ti - 1) / 2 + (tj - ti);       // (ti rows of n_tiles, n_tiles - 1, ... pairs lie in front)
    const double *p = part + pair * n_chunks * (kPcaTile * kPcaTile) + (s % kPcaTile) * kPcaTile + t % kPcaTile;
    double g = 0.0;
    for (uint32_t j = 0; j < n_chunks; ++j) g = pca_add(g, p[(size_t)j * (kPcaTile * kPcaTile)]);
    gram[(size_t)s * S + t] = g;
    gram[(size_t)t * S + s] = g;
    if (s == t) {
        double c = 0.0;
        for (uint32_t j = 0; j < n_chunks; ++j) c = pca_add(c, col_part[(size_t)j * n_tiles * kPcaTile + s]);
        col_sum[s] = c;
    }
}

void launch_pca_gram(const uint32_t *rank2, const double *T, uint64_t K, uint32_t S, double *part, double *col_part, uint32_t *bad, hipStream_t st) {
    const uint32_t n_tiles = (S + kPcaTile - 1) / kPcaTile, n_chunks = pca_n_chunks(K);
    hipLaunchKernelGGL(k_pca_gram, dim3(n_tiles * (n_tiles + 1) / 2, n_chunks), dim3(256), 0, st, rank2, T, K, S, n_tiles, n_chunks,
                       pca_chunk_rows(K, n_chunks), part, col_part, bad);
}
void launch_pca_reduce(const double *part, const double *col_part, uint64_t K, uint32_t S, double *gram, double *col_sum, hipStream_t st) {
    const uint32_t n_tiles = (S + kPcaTile - 1) / kPcaTile;
    hipLaunchKernelGGL(k_pca_reduce, dim3(n_tiles, (S + 3) / 4), dim3(256), 0, st, part, col_part, S, n_tiles, pca_n_chunks(K), gram, col_sum);
}

}  // namespace rgx
