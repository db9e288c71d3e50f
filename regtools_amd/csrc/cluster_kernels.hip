// cluster_kernels.hip -- device half of the cohort's intron clusters (rgx_cohort_cluster, cohort_cluster.cpp; contract in include/regtools_amd.h).
// The reference has no counterpart.  Rows of the matrix are the vertices; two stable radix sorts of the row indices, by (tid, class, start) and by
// (tid, class, end), put the rows of a splice site side by side, and neighbours in such a group become an edge -- at most 2 n edges, no site ids.
// Components: hooking towards the smaller label with atomicMin, alternating with pointer jumping, one launch each, until a whole round changed
// nothing.  A label only ever falls and is always a row of the same component, so the fixed point -- every row carries the smallest row index of
// its component -- is unique and does not depend on the order the atomics arrive in; nothing rests on a lane seeing what another workgroup wrote
// in the same launch (a stale label is an older, larger label of the same component: the edge is looked at again next round).  The per-cluster
// sums are integer atomics (order-free); everything behind them has one writer per word, as in cohort_kernels.hip.
// 256 threads per workgroup, wave64, no LDS, integer work bounded by HBM.
#include "kernels.h"

namespace rgx {

namespace {
__device__ __forceinline__ void flag_round(bool changed, uint32_t *flag) {
    if (__ballot(changed) && (threadIdx.x & 63u) == 0) atomicOr(flag, 1u);          // one atomic per wave that changed something
}
}  // namespace

__global__ __launch_bounds__(256) void k_cluster_class(const uint8_t *__restrict__ strand, uint32_t n, uint32_t *__restrict__ cls) {
    const uint32_t i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const uint32_t c = strand[i];
    cls[i] = c == '+' ? 0u : c == '-' ? 1u : 2u;
}

// sorted position i and the one before it: an edge when both rows lie on the same site, a self loop otherwise (every slot has one writer)
__global__ __launch_bounds__(256) void k_cluster_edges(const uint32_t *__restrict__ perm, const uint32_t *__restrict__ tid, const uint32_t *__restrict__ cls,
                                                       const uint32_t *__restrict__ site, uint32_t n, uint32_t *__restrict__ ea, uint32_t *__restrict__ eb) {
    const uint32_t i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const uint32_t r1 = perm[i];
    uint32_t r0 = r1;
    if (i) { const uint32_t q = perm[i - 1]; if (tid[q] == tid[r1] && cls[q] == cls[r1] && site[q] == site[r1]) r0 = q; }
    ea[i] = r0; eb[i] = r1;
}

__global__ __launch_bounds__(256) void k_cc_init(uint32_t *__restrict__ parent, uint32_t n) {
    const uint32_t v = blockIdx.x * 256 + threadIdx.x;
    if (v < n) parent[v] = v;
}

// One edge per lane: the larger of the two ends' labels is hooked under the smaller.  After the jumps of the round before, a label is a root
// or close to one; when it is not, the atomicMin still only lowers a label to a row of the same component.
__global__ __launch_bounds__(256) void k_cc_hook(uint32_t *parent, const uint32_t *__restrict__ a, const uint32_t *__restrict__ b, uint32_t n_edges,
                                                 uint32_t n_vertices, uint32_t *flag) {
    const uint32_t e = blockIdx.x * 256 + threadIdx.x;
    bool changed = false;
    if (e < n_edges) {
        const uint32_t u = a[e], v = b[e];
        if (u != v && u < n_vertices && v < n_vertices) {
            const uint32_t pu = parent[u], pv = parent[v];
            if (pu != pv) { const uint32_t lo = min(pu, pv), hi = max(pu, pv); changed = atomicMin(&parent[hi], lo) > lo; }
        }
    }
    flag_round(changed, flag);
}

// Two jumps per lane and launch, never a walk to the root: parent[v] = parent[parent[parent[v]]].  Lane v is the only writer of parent[v] here.
__global__ __launch_bounds__(256) void k_cc_jump(uint32_t *parent, uint32_t n, uint32_t *flag) {
    const uint32_t v = blockIdx.x * 256 + threadIdx.x;
    bool changed = false;
    if (v < n) {
        const uint32_t p = parent[v], gp = parent[p];
        if (gp != p) { parent[v] = parent[gp]; changed = true; }
    }
    flag_round(changed, flag);
}

// rows and reads per component, in the slot of its root (cnt and tot zeroed by the caller); integer sums: the same whatever the order
__global__ __launch_bounds__(256) void k_cluster_tally(const uint32_t *__restrict__ label, const unsigned long long *__restrict__ total, uint32_t n,
                                                       uint32_t *cnt, unsigned long long *tot) {
    const uint32_t i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const uint32_t r = label[i];
    atomicAdd(&cnt[r], 1u); atomicAdd(&tot[r], total[i]);
}

__global__ __launch_bounds__(256) void k_cluster_roots(const uint32_t *__restrict__ label, const uint32_t *__restrict__ cnt,
                                                       const unsigned long long *__restrict__ tot, uint32_t n, uint32_t min_rows,
                                                       unsigned long long min_total, uint32_t *__restrict__ is_root, uint32_t *__restrict__ keep) {
    const uint32_t i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const bool root = label[i] == i;
    is_root[i] = root; keep[i] = root && cnt[i] >= min_rows && tot[i] >= min_total;
}

// cluster[i] from row i's root; a kept root also writes its cluster's row count and total.  sort_key = the cluster, dropped rows behind all of them.
__global__ __launch_bounds__(256) void k_cluster_assign(const uint32_t *__restrict__ label, const uint32_t *__restrict__ keep,
                                                        const uint32_t *__restrict__ cid_excl, const uint32_t *__restrict__ cnt,
                                                        const unsigned long long *__restrict__ tot, uint32_t n, uint32_t n_clusters,
                                                        uint32_t *__restrict__ cluster, uint32_t *__restrict__ sort_key, uint32_t *__restrict__ cl_count,
                                                        unsigned long long *__restrict__ cl_total) {
    const uint32_t i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const uint32_t r = label[i];
    const bool kept = keep[r] != 0;
    const uint32_t c = kept ? cid_excl[r] : 0xffffffffu;
    cluster[i] = c; sort_key[i] = kept ? c : n_clusters;
    if (kept && r == i) { cl_count[c] = cnt[i]; cl_total[c] = tot[i]; }
}

// out[k] = in[k] for k < n, out[n] = *last (the CSR offsets and their scan's total, widened)
__global__ __launch_bounds__(256) void k_cluster_widen(const uint32_t *__restrict__ in, uint32_t n, const uint32_t *__restrict__ last,
                                                       unsigned long long *__restrict__ out) {
    const uint32_t k = blockIdx.x * 256 + threadIdx.x;
    if (k <= n) out[k] = k < n ? in[k] : *last;
}

// One row per group of LANES lanes (as k_cohort_reduce): how many of a clustered row's count entries are not zero
template <uint32_t LANES>
__global__ __launch_bounds__(256) void k_cluster_row_len(const uint32_t *__restrict__ cluster, const unsigned long long *__restrict__ row_begin,
                                                         const uint32_t *__restrict__ val, uint32_t n, uint32_t *__restrict__ len) {
    const uint32_t row = (blockIdx.x * 256 + threadIdx.x) / LANES, l = threadIdx.x % LANES;
    if (row >= n) return;
    uint32_t k = 0;
    if (cluster[row] != 0xffffffffu) for (unsigned long long q = row_begin[row] + l, e = row_begin[row + 1]; q < e; q += LANES) k += val[q] != 0;
    if (LANES > 1) {
#pragma unroll
        for (uint32_t d = LANES / 2; d; d >>= 1) k += __shfl_down(k, d, 64);
    }
    if (!l) len[row] = k;
}

// (cluster of the row, sample, count) of every such entry, in the matrix's order, from ent_off[row] = exclusive scan of len on
template <uint32_t LANES>
__global__ __launch_bounds__(256) void k_cluster_expand(const uint32_t *__restrict__ cluster, const unsigned long long *__restrict__ row_begin,
                                                        const uint32_t *__restrict__ col, const uint32_t *__restrict__ val,
                                                        const uint32_t *__restrict__ ent_off, uint32_t n, uint32_t *__restrict__ e_cluster,
                                                        uint32_t *__restrict__ e_sample, uint32_t *__restrict__ e_count) {
    const uint32_t row = (blockIdx.x * 256 + threadIdx.x) / LANES, l = threadIdx.x % LANES;
    if (row >= n) return;                                 // (LANES is 1 or the wave: a row's lanes leave together)
    const uint32_t c = cluster[row];
    if (c == 0xffffffffu) return;
    uint32_t d = ent_off[row];
    const unsigned long long b = row_begin[row], e = row_begin[row + 1];
    if (LANES == 1) {
        for (unsigned long long q = b; q < e; ++q) { const uint32_t v = val[q]; if (v) { e_cluster[d] = c; e_sample[d] = col[q]; e_count[d] = v; ++d; } }
    } else {
        for (unsigned long long q0 = b; q0 < e; q0 += 64) {          // the wave's survivors take consecutive slots (ballot + prefix of the lanes below)
            const unsigned long long q = q0 + l;
            const uint32_t v = q < e ? val[q] : 0u;
            const uint64_t m = __ballot(v != 0);
            if (v) { const uint32_t at = d + (uint32_t)__popcll(m & ((1ull << l) - 1ull)); e_cluster[at] = c; e_sample[at] = col[q]; e_count[at] = v; }
            d += (uint32_t)__popcll(m);
        }
    }
}

// head[i] = 1 where sorted position i starts a new (cluster, sample)
__global__ __launch_bounds__(256) void k_cluster_cs_heads(const uint32_t *__restrict__ perm, const uint32_t *__restrict__ e_cluster,
                                                          const uint32_t *__restrict__ e_sample, uint32_t n, uint32_t *__restrict__ head) {
    const uint32_t i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    uint32_t h = 1;
    if (i) { const uint32_t a = perm[i], b = perm[i - 1]; h = (e_cluster[a] != e_cluster[b] || e_sample[a] != e_sample[b]) ? 1u : 0u; }
    head[i] = h;
}

// One (cluster, sample) run per group of LANES lanes: its 64-bit sum in registers, written once
template <uint32_t LANES>
__global__ __launch_bounds__(256) void k_cluster_cs_sum(const uint32_t *__restrict__ perm, const uint32_t *__restrict__ e_cluster,
                                                        const uint32_t *__restrict__ e_sample, const uint32_t *__restrict__ e_count,
                                                        const uint32_t *__restrict__ seg_start, uint32_t n_seg, uint32_t *__restrict__ seg_cluster,
                                                        uint32_t *__restrict__ cs_sample, unsigned long long *__restrict__ cs_total) {
    const uint32_t s = (blockIdx.x * 256 + threadIdx.x) / LANES, l = threadIdx.x % LANES;
    if (s >= n_seg) return;                               // (LANES divides the wave: a run's lanes leave together)
    const uint32_t b = seg_start[s], e = seg_start[s + 1];
    unsigned long long sum = 0;
    for (uint32_t k = b + l; k < e; k += LANES) sum += e_count[perm[k]];
#pragma unroll
    for (uint32_t d = LANES / 2; d; d >>= 1) sum += __shfl_down(sum, d, LANES);
    if (l) return;
    const uint32_t first = perm[b];
    seg_cluster[s] = e_cluster[first]; cs_sample[s] = e_sample[first]; cs_total[s] = sum;
}

// cs_begin[c] = the runs of clusters below c (a binary search per cluster: a cluster may have no run at all), c = 0 .. n_clusters
__global__ __launch_bounds__(256) void k_cluster_cs_begin(const uint32_t *__restrict__ seg_cluster, uint32_t n_seg, uint32_t n_clusters,
                                                          unsigned long long *__restrict__ cs_begin) {
    const uint32_t c = blockIdx.x * 256 + threadIdx.x;
    if (c > n_clusters) return;
    uint32_t lo = 0, hi = n_seg;
    while (lo < hi) { const uint32_t mid = lo + (hi - lo) / 2; if (seg_cluster[mid] < c) lo = mid + 1; else hi = mid; }
    cs_begin[c] = lo;
}

// ---- refinement (rgx_cohort_refine): rows leave the graph, the sorted orders are compacted to the rows that stay, the search runs again ----------
// alive[i] = the row takes part in clustering at all (max_intron 0: every row)
__global__ __launch_bounds__(256) void k_refine_eligible(const uint32_t *__restrict__ start, const uint32_t *__restrict__ end, uint32_t n,
                                                         uint32_t max_intron, uint32_t *__restrict__ alive) {
    const uint32_t i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    alive[i] = (max_intron == 0 || end[i] - start[i] <= max_intron) ? 1u : 0u;
}

// flag[j] = alive[order[j]]: the flag seen through the permutation, for the scan that gives every survivor its place
__global__ __launch_bounds__(256) void k_refine_flag(const uint32_t *__restrict__ order, const uint32_t *__restrict__ alive, uint32_t k,
                                                     uint32_t *__restrict__ flag) {
    const uint32_t j = blockIdx.x * 256 + threadIdx.x;
    if (j < k) flag[j] = alive[order[j]];
}

// out[pos[j]] = order[j] for the survivors (pos = exclusive scan of the flags: below the survivors' count, which is at most k).  Stable: a
// sorted order stays sorted.
__global__ __launch_bounds__(256) void k_refine_scatter(const uint32_t *__restrict__ order, const uint32_t *__restrict__ alive,
                                                        const uint32_t *__restrict__ pos, uint32_t k, uint32_t *__restrict__ out) {
    const uint32_t j = blockIdx.x * 256 + threadIdx.x;
    if (j >= k) return;
    const uint32_t r = order[j];
    if (alive[r]) out[pos[j]] = r;
}

// k_cluster_edges over a compacted order whose length only the device knows: *n_live (at most cap) positions hold rows, the slots behind them
// become self loops of row 0
__global__ __launch_bounds__(256) void k_refine_edges(const uint32_t *__restrict__ perm, const uint32_t *__restrict__ n_live,
                                                      const uint32_t *__restrict__ tid, const uint32_t *__restrict__ cls,
                                                      const uint32_t *__restrict__ site, uint32_t cap, uint32_t *__restrict__ ea,
                                                      uint32_t *__restrict__ eb) {
    const uint32_t i = blockIdx.x * 256 + threadIdx.x;
    if (i >= cap) return;
    uint32_t r0 = 0, r1 = 0;
    if (i < min(*n_live, cap)) {
        r0 = r1 = perm[i];
        if (i) { const uint32_t q = perm[i - 1]; if (tid[q] == tid[r1] && cls[q] == cls[r1] && site[q] == site[r1]) r0 = q; }
    }
    ea[i] = r0; eb[i] = r1;
}

// k_cluster_tally over the rows that are alive (cnt may be null: stage 1 needs the totals only)
__global__ __launch_bounds__(256) void k_refine_tally(const uint32_t *__restrict__ label, const unsigned long long *__restrict__ total,
                                                      const uint32_t *__restrict__ alive, uint32_t n, uint32_t *cnt, unsigned long long *tot) {
    const uint32_t i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n || !alive[i]) return;
    const uint32_t r = label[i];
    if (cnt) atomicAdd(&cnt[r], 1u);
    atomicAdd(&tot[r], total[i]);
}

// The weak test: an alive row leaves when total < min_reads or total * den < num * T, T = tot[its root].  Both products are taken whole (a 64-bit
// factor times a 32-bit one: 96 bits, as a high and a low 64-bit word) and compared exactly; equality stays.  Lane i is the only writer of alive[i].
__global__ __launch_bounds__(256) void k_refine_mark(const uint32_t *__restrict__ label, const unsigned long long *__restrict__ total,
                                                     const unsigned long long *__restrict__ tot, uint32_t n, unsigned long long min_reads,
                                                     uint32_t num, uint32_t den, uint32_t *__restrict__ alive) {
    const uint32_t i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n || !alive[i]) return;
    const unsigned long long t = total[i], T = tot[label[i]];
    const unsigned long long l_hi = __umul64hi(t, (unsigned long long)den), l_lo = t * den;
    const unsigned long long r_hi = __umul64hi(T, (unsigned long long)num), r_lo = T * num;
    const bool below = l_hi < r_hi || (l_hi == r_hi && l_lo < r_lo);
    if (t < min_reads || below) alive[i] = 0;
}

// k_cluster_roots where a row that is not alive is no root and is not kept
__global__ __launch_bounds__(256) void k_refine_roots(const uint32_t *__restrict__ label, const uint32_t *__restrict__ cnt,
                                                      const unsigned long long *__restrict__ tot, const uint32_t *__restrict__ alive, uint32_t n,
                                                      uint32_t min_rows, unsigned long long min_total, uint32_t *__restrict__ is_root,
                                                      uint32_t *__restrict__ keep) {
    const uint32_t i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const bool root = alive[i] != 0 && label[i] == i;
    is_root[i] = root; keep[i] = root && cnt[i] >= min_rows && tot[i] >= min_total;
}

static inline dim3 cluster_grid(uint64_t n) { return dim3((unsigned)((n + 255) / 256)); }

void launch_cluster_class(const uint8_t *strand, uint32_t n, uint32_t *cls, hipStream_t st) {
    if (n) hipLaunchKernelGGL(k_cluster_class, cluster_grid(n), dim3(256), 0, st, strand, n, cls);
}
void launch_cluster_edges(const uint32_t *perm, const uint32_t *tid, const uint32_t *cls, const uint32_t *site, uint32_t n, uint32_t *ea, uint32_t *eb,
                          hipStream_t st) {
    if (n) hipLaunchKernelGGL(k_cluster_edges, cluster_grid(n), dim3(256), 0, st, perm, tid, cls, site, n, ea, eb);
}
void launch_cc_init(uint32_t *parent, uint32_t n, hipStream_t st) {
    if (n) hipLaunchKernelGGL(k_cc_init, cluster_grid(n), dim3(256), 0, st, parent, n);
}
void launch_cc_hook(uint32_t *parent, const uint32_t *a, const uint32_t *b, uint32_t n_edges, uint32_t n_vertices, uint32_t *flag, hipStream_t st) {
    if (n_edges) hipLaunchKernelGGL(k_cc_hook, cluster_grid(n_edges), dim3(256), 0, st, parent, a, b, n_edges, n_vertices, flag);
}
void launch_cc_jump(uint32_t *parent, uint32_t n, uint32_t *flag, hipStream_t st) {
    if (n) hipLaunchKernelGGL(k_cc_jump, cluster_grid(n), dim3(256), 0, st, parent, n, flag);
}
void launch_cluster_tally(const uint32_t *label, const unsigned long long *total, uint32_t n, uint32_t *cnt, unsigned long long *tot, hipStream_t st) {
    if (n) hipLaunchKernelGGL(k_cluster_tally, cluster_grid(n), dim3(256), 0, st, label, total, n, cnt, tot);
}
void launch_cluster_roots(const uint32_t *label, const uint32_t *cnt, const unsigned long long *tot, uint32_t n, uint32_t min_rows, uint64_t min_total,
                          uint32_t *is_root, uint32_t *keep, hipStream_t st) {
    if (n) hipLaunchKernelGGL(k_cluster_roots, cluster_grid(n), dim3(256), 0, st, label, cnt, tot, n, min_rows, (unsigned long long)min_total, is_root, keep);
}
void launch_cluster_assign(const uint32_t *label, const uint32_t *keep, const uint32_t *cid_excl, const uint32_t *cnt, const unsigned long long *tot,
                           uint32_t n, uint32_t n_clusters, uint32_t *cluster, uint32_t *sort_key, uint32_t *cl_count, unsigned long long *cl_total,
                           hipStream_t st) {
    if (n) hipLaunchKernelGGL(k_cluster_assign, cluster_grid(n), dim3(256), 0, st, label, keep, cid_excl, cnt, tot, n, n_clusters, cluster, sort_key,
                              cl_count, cl_total);
}
void launch_cluster_widen(const uint32_t *in, uint32_t n, const uint32_t *last, unsigned long long *out, hipStream_t st) {
    hipLaunchKernelGGL(k_cluster_widen, cluster_grid((uint64_t)n + 1), dim3(256), 0, st, in, n, last, out);
}
void launch_cluster_row_len(const uint32_t *cluster, const unsigned long long *row_begin, const uint32_t *val, uint32_t n, bool wave_per_row, uint32_t *len,
                            hipStream_t st) {
    if (!n) return;
    if (wave_per_row) hipLaunchKernelGGL(k_cluster_row_len<64>, cluster_grid((uint64_t)n * 64), dim3(256), 0, st, cluster, row_begin, val, n, len);
    else hipLaunchKernelGGL(k_cluster_row_len<1>, cluster_grid(n), dim3(256), 0, st, cluster, row_begin, val, n, len);
}
void launch_cluster_expand(const uint32_t *cluster, const unsigned long long *row_begin, const uint32_t *col, const uint32_t *val, const uint32_t *ent_off,
                           uint32_t n, bool wave_per_row, uint32_t *e_cluster, uint32_t *e_sample, uint32_t *e_count, hipStream_t st) {
    if (!n) return;
    if (wave_per_row) hipLaunchKernelGGL(k_cluster_expand<64>, cluster_grid((uint64_t)n * 64), dim3(256), 0, st, cluster, row_begin, col, val, ent_off, n,
                                         e_cluster, e_sample, e_count);
    else hipLaunchKernelGGL(k_cluster_expand<1>, cluster_grid(n), dim3(256), 0, st, cluster, row_begin, col, val, ent_off, n, e_cluster, e_sample, e_count);
}
void launch_cluster_cs_heads(const uint32_t *perm, const uint32_t *e_cluster, const uint32_t *e_sample, uint32_t n, uint32_t *head, hipStream_t st) {
    if (n) hipLaunchKernelGGL(k_cluster_cs_heads, cluster_grid(n), dim3(256), 0, st, perm, e_cluster, e_sample, n, head);
}
void launch_cluster_cs_sum(const uint32_t *perm, const uint32_t *e_cluster, const uint32_t *e_sample, const uint32_t *e_count, const uint32_t *seg_start,
                           uint32_t n, uint32_t n_seg, uint32_t *seg_cluster, uint32_t *cs_sample, unsigned long long *cs_total, hipStream_t st) {
    if (!n_seg) return;
    // a wave per run from a mean of 32 entries on; eight lanes below, so that the few long runs of a giant cluster do not hold one lane each
    if ((uint64_t)n_seg * 32 <= n) hipLaunchKernelGGL(k_cluster_cs_sum<64>, cluster_grid((uint64_t)n_seg * 64), dim3(256), 0, st, perm, e_cluster, e_sample,
                                                       e_count, seg_start, n_seg, seg_cluster, cs_sample, cs_total);
    else hipLaunchKernelGGL(k_cluster_cs_sum<8>, cluster_grid((uint64_t)n_seg * 8), dim3(256), 0, st, perm, e_cluster, e_sample, e_count, seg_start, n_seg,
                            seg_cluster, cs_sample, cs_total);
}
void launch_cluster_cs_begin(const uint32_t *seg_cluster, uint32_t n_seg, uint32_t n_clusters, unsigned long long *cs_begin, hipStream_t st) {
    hipLaunchKernelGGL(k_cluster_cs_begin, cluster_grid((uint64_t)n_clusters + 1), dim3(256), 0, st, seg_cluster, n_seg, n_clusters, cs_begin);
}

void launch_refine_eligible(const uint32_t *start, const uint32_t *end, uint32_t n, uint32_t max_intron, uint32_t *alive, hipStream_t st) {
    if (n) hipLaunchKernelGGL(k_refine_eligible, cluster_grid(n), dim3(256), 0, st, start, end, n, max_intron, alive);
}
void launch_refine_compact(const uint32_t *order, uint32_t k, const uint32_t *alive, uint32_t *pos, uint32_t *out, uint32_t *n_live, uint32_t *tmp,
                           hipStream_t st) {
    if (!k) { launch_scan_u32(nullptr, nullptr, 0, n_live, tmp, st); return; }
    hipLaunchKernelGGL(k_refine_flag, cluster_grid(k), dim3(256), 0, st, order, alive, k, pos);
    launch_scan_u32(pos, pos, k, n_live, tmp, st);
    hipLaunchKernelGGL(k_refine_scatter, cluster_grid(k), dim3(256), 0, st, order, alive, pos, k, out);
}
void launch_refine_edges(const uint32_t *perm, const uint32_t *n_live, const uint32_t *tid, const uint32_t *cls, const uint32_t *site, uint32_t cap,
                         uint32_t *ea, uint32_t *eb, hipStream_t st) {
    if (cap) hipLaunchKernelGGL(k_refine_edges, cluster_grid(cap), dim3(256), 0, st, perm, n_live, tid, cls, site, cap, ea, eb);
}
void launch_refine_tally(const uint32_t *label, const unsigned long long *total, const uint32_t *alive, uint32_t n, uint32_t *cnt,
                         unsigned long long *tot, hipStream_t st) {
    if (n) hipLaunchKernelGGL(k_refine_tally, cluster_grid(n), dim3(256), 0, st, label, total, alive, n, cnt, tot);
}
void launch_refine_mark(const uint32_t *label, const unsigned long long *total, const unsigned long long *tot, uint32_t n, uint64_t min_reads,
                        uint32_t ratio_num, uint32_t ratio_den, uint32_t *alive, hipStream_t st) {
    if (n) hipLaunchKernelGGL(k_refine_mark, cluster_grid(n), dim3(256), 0, st, label, total, tot, n, (unsigned long long)min_reads, ratio_num, ratio_den,
                              alive);
}
void launch_refine_roots(const uint32_t *label, const uint32_t *cnt, const unsigned long long *tot, const uint32_t *alive, uint32_t n, uint32_t min_rows,
                         uint64_t min_total, uint32_t *is_root, uint32_t *keep, hipStream_t st) {
    if (n) hipLaunchKernelGGL(k_refine_roots, cluster_grid(n), dim3(256), 0, st, label, cnt, tot, alive, n, min_rows, (unsigned long long)min_total,
                              is_root, keep);
}

}  // namespace rgx
