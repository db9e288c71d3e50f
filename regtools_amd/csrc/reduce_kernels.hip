// reduce_kernels.hip -- the group-by behind the event sort and the writers of the result table.  Called by
// api_reduce.cpp (reduce_events); the small helpers (launch_fill_u32, launch_gather_u32) also by api_internal.h, api_entry.cpp and
// api_stage.cpp.
//   k_preagg                  <kAggTile> one workgroup per tile of consecutive events: one partial row per distinct key (LDS hash table)
//   k_heads                   head flag of every sorted position that starts a new key
//   k_reduce                  events -> unique rows: wave-segmented min / max, one atomic per run and wave
//   k_reduce_finish           count, newest read and strand per row; marks the first event of every row
//   k_reduce_partials, k_reduce_finish_partials   the same two over partial rows (sum / min / max of what k_preagg gathered)
//   k_name_rank               1-based rank of a row's first occurrence, from the scan of the marks
//   k_gather_u32, k_fill_u32  out[r] = table[idx[r]]; p[i] = v
//   k_fill_elems<T>           p[i] = v for elements of 1, 2, 4 or 8 bytes: the fill mode of the cohort runs (cohort_internal.h)
//   k_rows_out                the unique rows in final order as ten u32 columns (the shards' form, merge_kernels.hip reads it)
//   k_rows_table              the same rows in the host table block's layout (kernels.h table_block_rows)
// Constant owned here: kAggEmpty; the tile size of k_preagg is chosen at its launch.
#include "wave_prims.h"

namespace rgx {

__global__ void k_heads(EventSoA ev, const uint32_t *__restrict__ perm, uint32_t n, uint32_t *head) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    uint32_t h = 1;
    if (i > 0) {
        const uint32_t a = perm[i], b = perm[i - 1];
        h = (ev.tid[a] != ev.tid[b]) || (ev.start[a] != ev.start[b]) || (ev.ilen_cls[a] != ev.ilen_cls[b]);
    }
    head[i] = h;
}

// seg_excl = exclusive scan of head; the row of sorted position i is seg_excl[i] + head[i] - 1.
// ts_min must be pre-filled with 0xffffffff and te_max with 0.
__global__ void k_reduce(EventSoA ev, const uint32_t *__restrict__ perm, const uint32_t *__restrict__ head,
                         const uint32_t *__restrict__ seg_excl, uint32_t n, UniqueSoA u, uint32_t *head_pos) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    const bool valid = i < n;
    uint32_t row = 0, ts = 0xffffffffu, te = 0, hd = 0;
    if (valid) {
        const uint32_t e = perm[i];
        hd = head[i];
        row = seg_excl[i] + hd - 1;
        ts = ev.ts[e]; te = ev.te[e];
        if (hd) {
            head_pos[row] = i;
            u.tid[row] = ev.tid[e]; u.start[row] = ev.start[e]; u.end[row] = ev.start[e] + (ev.ilen_cls[e] >> 2);
            u.first_seen[row] = e;          // stable sort: the first event of the run is the earliest read
        }
    }
    // wave-segmented min/max: runs are contiguous in lane order (keys are sorted)
    const uint32_t lane = lane_id();
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const uint32_t r2 = __shfl_down(row, d, 64), ts2 = __shfl_down(ts, d, 64), te2 = __shfl_down(te, d, 64);
        const bool v2 = __shfl_down((uint32_t)valid, d, 64) != 0;
        if (lane + d < 64 && v2 && r2 == row) { ts = min(ts, ts2); te = max(te, te2); }
    }
    // the first lane of each run in this wave publishes
    const uint32_t prev_row = __shfl_up(row, 1, 64);
    const bool run_head = valid && (lane == 0 || prev_row != row);
    if (run_head) { atomicMin(&u.ts_min[row], ts); atomicMax(&u.te_max[row], te); }
}

// ---- round 4: pre-aggregation -------------------------------------------------------------------------------------------------------
// The events of one junction come close together in file order (the reads that support it start within a read length of each other), so
// most of the group-by can happen before anything is sorted: a workgroup takes kAggTile consecutive events, groups equal keys in an LDS hash
// table (open addressing; a slot holds the tile-local index of the event that claimed it, keys are compared in the staged key columns) and
// writes ONE partial row per distinct key of the tile -- key, number of events, min thick_start, max thick_end, first and last event index.
// The radix sort, the head flags and the reduce then run on the partial rows (bench file 7.5 M events -> ~0.4 M rows, long reads 125 M ->
// a few M) and combine them with sum / min / max, which do not care in which order the tiles appended their rows.  Exact for any input:
// events that do not repeat inside a tile simply stay rows of one.
constexpr uint32_t kAggEmpty = 0xffffffffu;
template <uint32_t kAggTile>
__global__ __launch_bounds__(256) void k_preagg(EventSoA ev, uint32_t n, PartialSoA p, uint32_t *p_total) {
    constexpr uint32_t kAggSlots = 2 * kAggTile;
    __shared__ uint32_t s_tid[kAggTile], s_start[kAggTile], s_ilen[kAggTile], s_slot[kAggSlots];
    __shared__ uint32_t s_cnt[kAggTile], s_ts[kAggTile], s_te[kAggTile], s_first[kAggTile], s_last[kAggTile];
    __shared__ uint32_t s_wave[4], s_base;
    const uint32_t base = blockIdx.x * kAggTile, t = threadIdx.x;
#pragma unroll
    for (uint32_t k = 0; k < kAggTile / 256; ++k) {
        const uint32_t i = t + 256 * k, e = base + i;
        if (e < n) { s_tid[i] = ev.tid[e]; s_start[i] = ev.start[e]; s_ilen[i] = ev.ilen_cls[e]; }
        s_cnt[i] = 0; s_ts[i] = 0xffffffffu; s_te[i] = 0; s_first[i] = 0xffffffffu; s_last[i] = 0;
        s_slot[i] = kAggEmpty; s_slot[i + kAggTile] = kAggEmpty;
    }
    __syncthreads();
    uint32_t mine = 0;                                        // bit k: my event k claimed a slot (it writes the key's row)
#pragma unroll
    for (uint32_t k = 0; k < kAggTile / 256; ++k) {
        const uint32_t i = t + 256 * k, e = base + i;
        if (e < n) {
            const uint32_t kt = s_tid[i], ks = s_start[i], kl = s_ilen[i];
            uint32_t h = ks * 0x9E3779B1u ^ kl * 0x85EBCA6Bu ^ kt * 0xC2B2AE35u;
            h = (h ^ h >> 15) & (kAggSlots - 1);
            uint32_t leader;
            for (;;) {
                const uint32_t prev = atomicCAS(&s_slot[h], kAggEmpty, i);
                if (prev == kAggEmpty) { leader = i; mine |= 1u << k; break; }
                if (s_tid[prev] == kt && s_start[prev] == ks && s_ilen[prev] == kl) { leader = prev; break; }
                h = (h + 1) & (kAggSlots - 1);
            }
            atomicAdd(&s_cnt[leader], 1u);
            atomicMin(&s_ts[leader], ev.ts[e]); atomicMax(&s_te[leader], ev.te[e]);
            atomicMin(&s_first[leader], i); atomicMax(&s_last[leader], i);
        }
    }
    __syncthreads();
    uint32_t tot;
    uint32_t at = block_excl_scan_256((uint32_t)__popc(mine), s_wave, tot);
    if (t == 0) s_base = tot ? atomicAdd(p_total, tot) : 0u;
    __syncthreads();
    at += s_base;
#pragma unroll
    for (uint32_t k = 0; k < kAggTile / 256; ++k) {
        if (mine >> k & 1u) {
            const uint32_t i = t + 256 * k;
            p.tid[at] = s_tid[i]; p.start[at] = s_start[i]; p.ilen_cls[at] = s_ilen[i];
            p.count[at] = s_cnt[i]; p.ts[at] = s_ts[i]; p.te[at] = s_te[i]; p.first[at] = base + s_first[i]; p.last[at] = base + s_last[i];
            ++at;
        }
    }
}

// k_reduce for partial rows: per key the sum of the counts, min / max of the thick bounds, the earliest first and the latest last event.
// u.count / te_max / last_seen must be pre-filled with 0, u.ts_min / first_seen with 0xffffffff.
__global__ void k_reduce_partials(PartialSoA p, const uint32_t *__restrict__ perm, const uint32_t *__restrict__ head,
                                  const uint32_t *__restrict__ seg_excl, uint32_t n, UniqueSoA u) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    const bool valid = i < n;
    uint32_t row = 0, ts = 0xffffffffu, te = 0, cnt = 0, first = 0xffffffffu, last = 0;
    if (valid) {
        const uint32_t e = perm[i];
        const uint32_t hd = head[i];
        row = seg_excl[i] + hd - 1;
        ts = p.ts[e]; te = p.te[e]; cnt = p.count[e]; first = p.first[e]; last = p.last[e];
        if (hd) { u.tid[row] = p.tid[e]; u.start[row] = p.start[e]; u.end[row] = p.start[e] + (p.ilen_cls[e] >> 2); }
    }
    const uint32_t lane = lane_id();
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const uint32_t r2 = __shfl_down(row, d, 64), ts2 = __shfl_down(ts, d, 64), te2 = __shfl_down(te, d, 64), c2 = __shfl_down(cnt, d, 64);
        const uint32_t f2 = __shfl_down(first, d, 64), l2 = __shfl_down(last, d, 64);
        const bool v2 = __shfl_down((uint32_t)valid, d, 64) != 0;
        if (lane + d < 64 && v2 && r2 == row) { ts = min(ts, ts2); te = max(te, te2); cnt += c2; first = min(first, f2); last = max(last, l2); }
    }
    const uint32_t prev_row = __shfl_up(row, 1, 64);
    const bool run_head = valid && (lane == 0 || prev_row != row);
    if (run_head) {
        atomicMin(&u.ts_min[row], ts); atomicMax(&u.te_max[row], te); atomicAdd(&u.count[row], cnt);
        atomicMin(&u.first_seen[row], first); atomicMax(&u.last_seen[row], last);
    }
}
__global__ void k_reduce_finish_partials(const uint8_t *__restrict__ ev_strand, uint32_t n_unique, UniqueSoA u, uint32_t *first_flag) {
    const uint32_t r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= n_unique) return;
    u.strand[r] = ev_strand[u.last_seen[r]];          // newest read's strand wins (junctions_extractor.cc:233)
    first_flag[u.first_seen[r]] = 1;
}

__global__ void k_reduce_finish(EventSoA ev, const uint32_t *__restrict__ perm, uint32_t n, uint32_t n_unique,
                                const uint32_t *__restrict__ head_pos, UniqueSoA u, uint32_t *first_flag) {
    const uint32_t r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= n_unique) return;
    const uint32_t hp = head_pos[r], nx = (r + 1 < n_unique) ? head_pos[r + 1] : n;
    u.count[r] = nx - hp;
    const uint32_t last = perm[nx - 1];
    u.last_seen[r] = last;
    u.strand[r] = ev.strand[last];          // newest read's strand wins (junctions_extractor.cc:233)
    first_flag[u.first_seen[r]] = 1;
}

__global__ void k_name_rank(uint32_t n_unique, const uint32_t *__restrict__ flag_scan, UniqueSoA u) {
    const uint32_t r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r < n_unique) u.name_rank[r] = flag_scan[u.first_seen[r]] + 1;   // 1-based rank of first occurrence
}

__global__ void k_gather_u32(uint32_t n, const uint32_t *__restrict__ table, const uint32_t *__restrict__ idx, uint32_t *out) {
    const uint32_t r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r < n) out[r] = table[idx[r]];
}

// the unique rows in final order as ten contiguous u32 columns (tid,start,end,ts,te,count,name_rank,first_seen,last_seen,strand):
// one block, one copy to the host
__global__ void k_rows_out(UniqueSoA u, const uint32_t *__restrict__ order, uint32_t n, uint32_t *out) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint32_t s = order[i];
    const size_t N = n;
    out[i] = u.tid[s]; out[N + i] = u.start[s]; out[2 * N + i] = u.end[s]; out[3 * N + i] = u.ts_min[s]; out[4 * N + i] = u.te_max[s];
    out[5 * N + i] = u.count[s]; out[6 * N + i] = u.name_rank[s]; out[7 * N + i] = u.first_seen[s]; out[8 * N + i] = u.last_seen[s];
    out[9 * N + i] = u.strand[s];
}

// one row of the host table block (layout: kernels.h table_block_rows)
__device__ __forceinline__ void table_row(uint8_t *out, size_t m, uint32_t i, uint32_t tid, uint32_t start, uint32_t end, uint32_t ts, uint32_t te, uint32_t count,
                                          uint64_t name_index, uint64_t first, uint64_t last, uint32_t strand, uint32_t min_anchor) {
    uint64_t *q8 = (uint64_t *)out;
    q8[i] = name_index; q8[m + i] = first; q8[2 * m + i] = last;
    uint32_t *q4 = (uint32_t *)(out + m * 24);
    q4[i] = tid; q4[m + i] = start; q4[2 * m + i] = end; q4[3 * m + i] = ts; q4[4 * m + i] = te; q4[5 * m + i] = count;
    uint8_t *q1 = out + m * 48;
    q1[i] = (uint8_t)strand;
    q1[m + i] = (uint32_t)(start - ts) >= min_anchor;       // OR over reads of (start - thick_start >= a) == the test on the minimum
    q1[2 * m + i] = (uint32_t)(te - end) >= min_anchor;
}
__global__ void k_rows_table(UniqueSoA u, const uint32_t *__restrict__ order, uint32_t n, uint32_t min_anchor, uint8_t *out) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint32_t s = order[i];
    table_row(out, table_block_rows(n), i, u.tid[s], u.start[s], u.end[s], u.ts_min[s], u.te_max[s], u.count[s], u.name_rank[s], u.first_seen[s], u.last_seen[s], u.strand[s], min_anchor);
}

__global__ void k_fill_u32(uint32_t *p, uint32_t v, size_t n) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) p[i] = v;
}
template <class T> __global__ void k_fill_elems(T *p, T v, size_t n) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) p[i] = v;
}

void launch_heads(EventSoA ev, const uint32_t *perm, uint32_t n, uint32_t *head, hipStream_t stream) {
    if (n) hipLaunchKernelGGL(k_heads, dim3((n + 255) / 256), dim3(256), 0, stream, ev, perm, n, head);
}
void launch_reduce(EventSoA ev, const uint32_t *perm, const uint32_t *head, const uint32_t *seg_excl, uint32_t n, UniqueSoA u,
                   uint32_t *head_pos, hipStream_t stream) {
    if (n) hipLaunchKernelGGL(k_reduce, dim3((n + 255) / 256), dim3(256), 0, stream, ev, perm, head, seg_excl, n, u, head_pos);
}
void launch_reduce_finish(EventSoA ev, const uint32_t *perm, uint32_t n, uint32_t n_unique, const uint32_t *head_pos, UniqueSoA u,
                          uint32_t *first_flag, hipStream_t stream) {
    if (n_unique) hipLaunchKernelGGL(k_reduce_finish, dim3((n_unique + 255) / 256), dim3(256), 0, stream, ev, perm, n, n_unique, head_pos, u, first_flag);
}
void launch_name_rank(uint32_t n_unique, const uint32_t *flag_scan, UniqueSoA u, hipStream_t stream) {
    if (n_unique) hipLaunchKernelGGL(k_name_rank, dim3((n_unique + 255) / 256), dim3(256), 0, stream, n_unique, flag_scan, u);
}
void launch_gather_u32(uint32_t n, const uint32_t *table, const uint32_t *idx, uint32_t *out, hipStream_t stream) {
    if (n) hipLaunchKernelGGL(k_gather_u32, dim3((n + 255) / 256), dim3(256), 0, stream, n, table, idx, out);
}
void launch_rows_out(UniqueSoA u, const uint32_t *order, uint32_t n, uint32_t *out, hipStream_t stream) {
    if (n) hipLaunchKernelGGL(k_rows_out, dim3((n + 255) / 256), dim3(256), 0, stream, u, order, n, out);
}
void launch_rows_table(UniqueSoA u, const uint32_t *order, uint32_t n, uint32_t min_anchor, uint8_t *out, hipStream_t stream) {
    if (n) hipLaunchKernelGGL(k_rows_table, dim3((n + 255) / 256), dim3(256), 0, stream, u, order, n, min_anchor, out);
}
void launch_preagg(EventSoA ev, uint32_t n, PartialSoA p, uint32_t *p_total, hipStream_t stream) {
    if (!n) return;
    // (measured, round 4: 2048 events per tile = 80 KB of LDS, two workgroups per CU: reduce 1.52 ms on the bench file against 1.40-1.42 with 1024)
    hipLaunchKernelGGL(k_preagg<1024>, dim3((n + 1023) / 1024), dim3(256), 0, stream, ev, n, p, p_total);
}
void launch_reduce_partials(PartialSoA p, const uint32_t *perm, const uint32_t *head, const uint32_t *seg_excl, uint32_t n, UniqueSoA u, hipStream_t stream) {
    if (n) hipLaunchKernelGGL(k_reduce_partials, dim3((n + 255) / 256), dim3(256), 0, stream, p, perm, head, seg_excl, n, u);
}
void launch_reduce_finish_partials(const uint8_t *ev_strand, uint32_t n_unique, UniqueSoA u, uint32_t *first_flag, hipStream_t stream) {
    if (n_unique) hipLaunchKernelGGL(k_reduce_finish_partials, dim3((n_unique + 255) / 256), dim3(256), 0, stream, ev_strand, n_unique, u, first_flag);
}
void launch_fill_u32(uint32_t *p, uint32_t v, size_t n, hipStream_t stream) {
    if (n) hipLaunchKernelGGL(k_fill_u32, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, p, v, n);
}
template <class T> static void fill_elems(void *p, uint64_t v, size_t n, hipStream_t stream) {
    hipLaunchKernelGGL(k_fill_elems<T>, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, (T *)p, (T)v, n);
}
void launch_fill_elems(void *p, uint32_t width, uint64_t v, size_t n, hipStream_t stream) {
    if (!n) return;
    if (width == 1) fill_elems<uint8_t>(p, v, n, stream);
    else if (width == 2) fill_elems<uint16_t>(p, v, n, stream);
    else if (width == 4) fill_elems<uint32_t>(p, v, n, stream);
    else fill_elems<uint64_t>(p, v, n, stream);
}

}  // namespace rgx
