// cohort_kernels.hip -- device half of the cohort junction-by-sample count matrix (rgx_cohort_add / rgx_cohort_finish, cohort.cpp).
// The reference has no counterpart: a cohort run there is one `regtools junctions extract` process per BAM (junctions_main.cc:45-59) and a
// script that merges the BED files.  Here every sample's rows are appended, in HBM, to an accumulator of 28-byte triples
//     (cohort tid, start, end | thick_start, thick_end, read_count, strand char << 24 | sample index)
// kept as seven columns per block of kCohortBlockRows triples (blocks are added, never re-copied); finish groups them by the reference's key
// (tid, start, end, strand class: junctions_extractor.cc:180-194) with ONE stable key-carrying radix sort (launch_radix_pass_keyed), so that the
// triples of a key end up side by side in sample order -- which is the CSR image's order -- and every output word has a single writer.
// Integer work bounded by HBM, wave64; no atomics per row anywhere (append: one atomicAdd per wave).
#include "kernels.h"

namespace rgx {

namespace {

__device__ __forceinline__ uint32_t cohort_word(uint32_t *const *__restrict__ blocks, uint32_t idx, uint32_t col) {
    return blocks[idx >> kCohortBlockLog2][(size_t)col * kCohortBlockRows + (idx & (kCohortBlockRows - 1))];
}
__device__ __forceinline__ uint32_t strand_class(uint32_t strand) { return strand == '+' ? 0u : strand == '-' ? 1u : 2u; }

}  // namespace

// One sample's rows -> triples.  src = u32 columns `stride` words apart: tid, start, end, thick_start, thick_end, read_count at columns 0..5 and the
// strand at column strand_col (the ten-column block launch_rows_out leaves in a context's HBM: 9; an uploaded table: 6).  A row takes part when it has
// both anchors (k_merge_table's rule, unsigned) or when every row does; the survivors of a wave take consecutive slots behind ONE atomicAdd on the
// accumulator's fill count (ballot + prefix of the lanes below), so a sample's triples lie behind those of every sample added before it.
__global__ __launch_bounds__(256) void k_cohort_append(const uint32_t *__restrict__ src, uint32_t n, size_t stride, uint32_t strand_col,
                                                       const uint32_t *__restrict__ tid_map, uint32_t n_map, uint32_t min_anchor, uint32_t only_anchored,
                                                       uint32_t sample, uint32_t *fill, uint32_t cap, uint32_t *const *__restrict__ blocks) {
    const uint32_t i = blockIdx.x * 256 + threadIdx.x;
    uint32_t tid = 0, start = 0, end = 0, ts = 0, te = 0, cnt = 0, strand = 0;
    bool keep = false;
    if (i < n) {
        tid = src[i]; start = src[stride + i]; end = src[2 * stride + i]; ts = src[3 * stride + i]; te = src[4 * stride + i]; cnt = src[5 * stride + i];
        strand = src[strand_col * stride + i] & 0xffu;
        keep = tid < n_map && (!only_anchored || ((uint32_t)(start - ts) >= min_anchor && (uint32_t)(te - end) >= min_anchor));
    }
    const uint64_t m = __ballot(keep);
    if (!m) return;
    const uint32_t lane = threadIdx.x & 63u;
    uint32_t base = 0;
    if (lane == (uint32_t)__ffsll((unsigned long long)m) - 1) base = atomicAdd(fill, (uint32_t)__popcll(m));
    base = __shfl(base, __ffsll((unsigned long long)m) - 1, 64);
    if (!keep) return;
    const uint32_t idx = base + (uint32_t)__popcll(m & ((1ull << lane) - 1ull));
    if (idx >= cap || idx < base) return;                 // (the host sized the blocks for every row of the sample: never taken, and never out of bounds)
    uint32_t *b = blocks[idx >> kCohortBlockLog2] + (idx & (kCohortBlockRows - 1));
    b[0] = tid_map[tid]; b[kCohortBlockRows] = start; b[2 * (size_t)kCohortBlockRows] = end; b[3 * (size_t)kCohortBlockRows] = ts;
    b[4 * (size_t)kCohortBlockRows] = te; b[5 * (size_t)kCohortBlockRows] = cnt; b[6 * (size_t)kCohortBlockRows] = strand << 24 | sample;
}

// the sort's key words: out[i] = word `which` (0 tid, 1 start, 2 end, 3 strand class) of triple perm[i] (perm null = i): one gather per word,
// the word's 8-bit passes then stream (key, permutation) pairs
__global__ __launch_bounds__(256) void k_cohort_key(uint32_t *const *__restrict__ blocks, const uint32_t *__restrict__ perm, uint32_t n, uint32_t which,
                                                    uint32_t *__restrict__ out) {
    const uint32_t i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const uint32_t e = perm ? perm[i] : i;
    out[i] = which < 3 ? cohort_word(blocks, e, which) : strand_class(cohort_word(blocks, e, 6) >> 24);
}

// the triples in sorted order, column by column: everything behind this streams
__global__ __launch_bounds__(256) void k_cohort_gather(uint32_t *const *__restrict__ blocks, const uint32_t *__restrict__ perm, uint32_t n, CohortSorted s) {
    const uint32_t i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const uint32_t e = perm[i];
    const uint32_t *b = blocks[e >> kCohortBlockLog2] + (e & (kCohortBlockRows - 1));
    s.tid[i] = b[0]; s.start[i] = b[kCohortBlockRows]; s.end[i] = b[2 * (size_t)kCohortBlockRows]; s.ts[i] = b[3 * (size_t)kCohortBlockRows];
    s.te[i] = b[4 * (size_t)kCohortBlockRows]; s.count[i] = b[5 * (size_t)kCohortBlockRows]; s.ss[i] = b[6 * (size_t)kCohortBlockRows];
}

__global__ __launch_bounds__(256) void k_cohort_heads(CohortSorted s, uint32_t n, uint32_t *__restrict__ head) {
    const uint32_t i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    head[i] = (i == 0 || s.tid[i] != s.tid[i - 1] || s.start[i] != s.start[i - 1] || s.end[i] != s.end[i - 1] ||
               strand_class(s.ss[i] >> 24) != strand_class(s.ss[i - 1] >> 24)) ? 1u : 0u;
}

// row_start[r] = sorted position of row r's first triple (single writer: the head itself); row_start[rows] = n
__global__ __launch_bounds__(256) void k_cohort_row_start(const uint32_t *__restrict__ head, const uint32_t *__restrict__ seg_excl, uint32_t n,
                                                          uint32_t *__restrict__ row_start) {
    const uint32_t i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    if (head[i]) row_start[seg_excl[i]] = i;
    if (i == n - 1) row_start[seg_excl[i] + head[i]] = n;
}

// One row per group of LANES lanes (1: the rows of a cohort whose keys are mostly private; 64: a wave per row when a key has hundreds of samples):
// the row's reductions over its run of sorted triples, in registers, written once.  The run is in sample order, so its last triple is the
// highest-numbered sample's: its character is the row's strand.
template <uint32_t LANES>
__global__ __launch_bounds__(256) void k_cohort_reduce(CohortSorted s, const uint32_t *__restrict__ row_start, uint32_t n_rows, uint32_t min_samples,
                                                       uint64_t min_total, CohortRows r) {
    const uint32_t row = (blockIdx.x * 256 + threadIdx.x) / LANES, l = threadIdx.x % LANES;
    if (row >= n_rows) return;                            // (LANES divides the wave: a row's lanes leave together)
    const uint32_t b = row_start[row], e = row_start[row + 1];
    unsigned long long total = 0; uint32_t ts = 0xffffffffu, te = 0;
    for (uint32_t k = b + l; k < e; k += LANES) { total += s.count[k]; ts = min(ts, s.ts[k]); te = max(te, s.te[k]); }
    if (LANES > 1) {
#pragma unroll
        for (uint32_t d = LANES / 2; d; d >>= 1) {
            total += __shfl_down(total, d, 64); ts = min(ts, (uint32_t)__shfl_down(ts, d, 64)); te = max(te, (uint32_t)__shfl_down(te, d, 64));
        }
    }
    if (l) return;
    const uint32_t n_with = e - b;
    const bool keep = n_with >= min_samples && total >= min_total;
    r.ts[row] = ts; r.te[row] = te; r.total[row] = total; r.keep[row] = keep; r.kept_nnz[row] = keep ? n_with : 0u;
}

// the rows that pass the filters, in order, straight into the result's image (cohort.cpp MatrixLayout): one writer per word
__global__ __launch_bounds__(256) void k_cohort_rows_out(CohortSorted s, const uint32_t *__restrict__ row_start, CohortRows r,
                                                         const uint32_t *__restrict__ out_row, const uint32_t *__restrict__ nnz_excl, uint32_t n_rows,
                                                         uint32_t n_nnz_kept, CohortImage o) {
    const uint32_t row = blockIdx.x * 256 + threadIdx.x;
    if (row >= n_rows) return;
    if (row == n_rows - 1) o.row_begin[out_row[row] + r.keep[row]] = n_nnz_kept;
    if (!r.keep[row]) return;
    const uint32_t q = out_row[row], b = row_start[row], e = row_start[row + 1];
    o.tid[q] = s.tid[b]; o.start[q] = s.start[b]; o.end[q] = s.end[b]; o.ts[q] = r.ts[row]; o.te[q] = r.te[row];
    o.n_with[q] = e - b; o.total[q] = r.total[row]; o.strand[q] = (uint8_t)(s.ss[e - 1] >> 24); o.row_begin[q] = nnz_excl[row];
}

// the CSR image: sorted position i belongs to row seg, whose kept triples start at nnz_excl[seg]
__global__ __launch_bounds__(256) void k_cohort_csr(CohortSorted s, const uint32_t *__restrict__ head, const uint32_t *__restrict__ seg_excl,
                                                    const uint32_t *__restrict__ row_start, CohortRows r, const uint32_t *__restrict__ nnz_excl, uint32_t n,
                                                    CohortImage o) {
    const uint32_t i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const uint32_t row = seg_excl[i] + head[i] - 1u;
    if (!r.keep[row]) return;
    const uint32_t d = nnz_excl[row] + (i - row_start[row]);
    o.col_sample[d] = s.ss[i] & 0xffffffu; o.val_count[d] = s.count[i];
}

static inline dim3 cohort_grid(uint64_t n) { return dim3((unsigned)((n + 255) / 256)); }

void launch_cohort_append(const uint32_t *src, uint32_t n, size_t stride, uint32_t strand_col, const uint32_t *tid_map, uint32_t n_map, uint32_t min_anchor,
                          bool only_anchored, uint32_t sample, uint32_t *fill, uint32_t cap, uint32_t *const *blocks, hipStream_t st) {
    if (n) hipLaunchKernelGGL(k_cohort_append, cohort_grid(n), dim3(256), 0, st, src, n, stride, strand_col, tid_map, n_map, min_anchor,
                              only_anchored ? 1u : 0u, sample, fill, cap, blocks);
}
void launch_cohort_key(uint32_t *const *blocks, const uint32_t *perm, uint32_t n, uint32_t which, uint32_t *out, hipStream_t st) {
    if (n) hipLaunchKernelGGL(k_cohort_key, cohort_grid(n), dim3(256), 0, st, blocks, perm, n, which, out);
}
void launch_cohort_gather(uint32_t *const *blocks, const uint32_t *perm, uint32_t n, CohortSorted s, uint32_t *head, hipStream_t st) {
    if (!n) return;
    hipLaunchKernelGGL(k_cohort_gather, cohort_grid(n), dim3(256), 0, st, blocks, perm, n, s);
    hipLaunchKernelGGL(k_cohort_heads, cohort_grid(n), dim3(256), 0, st, s, n, head);
}
void launch_cohort_row_start(const uint32_t *head, const uint32_t *seg_excl, uint32_t n, uint32_t *row_start, hipStream_t st) {
    if (n) hipLaunchKernelGGL(k_cohort_row_start, cohort_grid(n), dim3(256), 0, st, head, seg_excl, n, row_start);
}
void launch_cohort_reduce(CohortSorted s, const uint32_t *row_start, uint32_t n, uint32_t n_rows, uint32_t min_samples, uint64_t min_total, CohortRows r,
                          hipStream_t st) {
    if (!n_rows) return;
    // a wave per row from a mean of 32 samples per key on: below, most lanes of such a wave would find nothing to read
    if ((uint64_t)n_rows * 32 <= n) hipLaunchKernelGGL(k_cohort_reduce<64>, cohort_grid((uint64_t)n_rows * 64), dim3(256), 0, st, s, row_start, n_rows,
                                                        min_samples, min_total, r);
    else hipLaunchKernelGGL(k_cohort_reduce<1>, cohort_grid(n_rows), dim3(256), 0, st, s, row_start, n_rows, min_samples, min_total, r);
}
void launch_cohort_out(CohortSorted s, const uint32_t *head, const uint32_t *seg_excl, const uint32_t *row_start, CohortRows r, const uint32_t *out_row,
                       const uint32_t *nnz_excl, uint32_t n, uint32_t n_rows, uint32_t n_nnz_kept, CohortImage o, hipStream_t st) {
    if (!n_rows) return;
    hipLaunchKernelGGL(k_cohort_rows_out, cohort_grid(n_rows), dim3(256), 0, st, s, row_start, r, out_row, nnz_excl, n_rows, n_nnz_kept, o);
    hipLaunchKernelGGL(k_cohort_csr, cohort_grid(n), dim3(256), 0, st, s, head, seg_excl, row_start, r, nnz_excl, n, o);
}

}  // namespace rgx
