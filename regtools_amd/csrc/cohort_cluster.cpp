// cohort_cluster.cpp -- the intron clusters of a cohort matrix: rgx_cohort_cluster (device), its host twin rgx_cohort_cluster_host and the
// perind.counts-style text (contract in include/regtools_amd.h; the reference has no counterpart).  Device side: cluster_kernels.hip.
//   rows -> two stable sorts by (tid, class, start) / (tid, class, end) -> edges between neighbours on a site -> components (hook + jump rounds,
//   components_run) -> rows and reads per root (integer atomics), filters, scan = cluster numbers -> stable sort by cluster = cl_row
//   -> the clustered rows' count entries as (cluster, sample, count) -> stable sort by sample, then cluster -> heads, scan, one sum per run = cs_*
#include "cohort_internal.h"

namespace {

rgx_cohort_clusters *clusters_alloc(uint64_t n, uint64_t n_clusters, uint64_t n_kept, uint64_t n_cs, bool pinned) {
    rgx_cohort_clusters *c = result_alloc<rgx_cohort_clusters>(pinned, [&](rgx_cohort_clusters &r, BlockTake &take) {
        take(r.cl_begin, n_clusters + 1); take(r.cl_total, n_clusters); take(r.cs_begin, n_clusters + 1); take(r.cs_total, n_cs);
        take(r.cluster, n); take(r.cl_row, n_kept); take(r.cs_sample, n_cs);
    });
    if (!c) return nullptr;
    c->n_rows = n; c->n_clusters = n_clusters;
    c->cl_begin[0] = 0; c->cs_begin[0] = 0;
    return c;
}

constexpr uint64_t kMaxClusterItems = (1ull << 32) - (1ull << 16);   // (rows, and count entries: the sort's tiles round the count up inside 32 bits)

int check_limits(const rgx_cohort_matrix *m, char *err, size_t errlen) {
    if (m->n > kMaxClusterItems || m->row_begin[m->n] > kMaxClusterItems) return fail(err, errlen, RGX_ERR_ARG,
        "regtools_amd: clustering takes at most %llu rows and %llu counts; the matrix has %llu and %llu\n", (unsigned long long)kMaxClusterItems,
        (unsigned long long)kMaxClusterItems, (unsigned long long)m->n, (unsigned long long)m->row_begin[m->n]);
    return RGX_OK;
}

// what the scans leave at the front of the row workspace (read back by one copy each time the host needs a size)
struct ClusterScalars { uint32_t flags[kCcBatch]; uint32_t n_components, n_clusters, n_kept, n_entries, n_cs, n_alive; };

}  // namespace

int components_run(uint32_t n_vertices, const EdgeList *lists, int n_lists, uint32_t *parent, uint32_t *d_flags, hipStream_t st, uint32_t *n_rounds,
                   char *err, size_t errlen) {
    uint32_t rounds = 0;
    launch_cc_init(parent, n_vertices, st);
    for (bool done = n_vertices == 0; !done;) {
        HIP_TRY(hipMemsetAsync(d_flags, 0, kCcBatch * 4, st));
        for (uint32_t k = 0; k < kCcBatch; ++k) {
            for (int l = 0; l < n_lists; ++l) launch_cc_hook(parent, lists[l].a, lists[l].b, lists[l].n, n_vertices, d_flags + k, st);
            launch_cc_jump(parent, n_vertices, d_flags + k, st);
        }
        uint32_t h[kCcBatch];
        HIP_TRY(read_back(st, h, d_flags, sizeof h));
        for (uint32_t k = 0; k < kCcBatch && !done; ++k) { ++rounds; done = h[k] == 0; }
        // (every round that changes something lowers a label: far fewer than one round per vertex, whatever the graph)
        if (!done && rounds > n_vertices + kCcBatch) return fail(err, errlen, RGX_ERR_DEVICE, "regtools_amd: the component search did not settle in %u rounds\n", rounds);
    }
    if (n_rounds) *n_rounds = rounds;
    return RGX_OK;
}

int cohort_matrix_image(rgx_cohort *co, const rgx_cohort_matrix *m, hipStream_t st, CohortImage *in, char *err, size_t errlen) {
    const uint32_t n = (uint32_t)m->n, nnz = (uint32_t)m->row_begin[m->n];
    const MatrixLayout L = matrix_layout(n, nnz);
    uint8_t *base = co->image.as<uint8_t>();
    if (matrix_serial(m) != co->image_serial) {
        // the columns needed, where the image has them: total, row_begin, tid, start, end in front of the thick bounds; col_sample, val_count, strand behind n_with
        if (co->cl_in.ensure(L.bytes + 256) != hipSuccess) { (void)hipGetLastError(); return fail(err, errlen, RGX_ERR_DEVICE,
            "regtools_amd: no device memory to upload the matrix (%u rows, %u counts)\n", n, nnz); }
        base = co->cl_in.as<uint8_t>();
        const uint8_t *h = (const uint8_t *)m->total - L.total;
        HIP_TRY(hipMemcpyAsync(base, h, L.ts, hipMemcpyHostToDevice, st));
        HIP_TRY(hipMemcpyAsync(base + L.col, h + L.col, L.strand + n - L.col, hipMemcpyHostToDevice, st));
    }
    *in = image_at(base, L);
    return RGX_OK;
}

extern "C" void rgx_cluster_params_default(rgx_cluster_params *p) { if (p) { p->min_rows = 1; p->min_total = 0; } }

extern "C" int rgx_cohort_cluster_path(rgx_cohort *co) { return co ? co->cluster_path : 0; }

extern "C" void rgx_cohort_clusters_free(rgx_cohort_clusters *cl) { result_free(cl); }

namespace {

// One device run over a matrix, as the stages rgx_cohort_cluster and rgx_cohort_refine are made of.  The caller holds the cohort's lock and has checked
// the limits; every stage enqueues on the cohort's stream and returns RGX_OK or the failed call's code.
struct ClusterRun : CohortRun {
    const rgx_cohort_matrix *m;
    uint32_t n = 0, nnz = 0, max_start = 0, max_end = 0, max_tid = 0, n_ineligible = 0, n_rounds = 0;
    CohortImage in{};
    // the row workspace: cluster's arrays, and refine's two further permutation buffers, alive flags and compaction scratch
    unsigned long long *tot = nullptr, *cl_total = nullptr, *o_cl_begin = nullptr, *o_cs_begin = nullptr;
    ClusterScalars *d_sc = nullptr;
    uint32_t *parent = nullptr, *ea0 = nullptr, *eb0 = nullptr, *ea1 = nullptr, *eb1 = nullptr, *perm0 = nullptr, *perm1 = nullptr, *key0 = nullptr,
             *key1 = nullptr, *cls = nullptr, *cluster = nullptr, *cl_count = nullptr, *tmp = nullptr, *perm2 = nullptr, *perm3 = nullptr,
             *alive = nullptr, *pos = nullptr;
    // refine: the rows still alive in stable order of (tid, class, start) and of (tid, class, end), and the buffer each may be compacted into
    const uint32_t *order[2] = {nullptr, nullptr}; uint32_t *order_spare[2] = {nullptr, nullptr};

    ClusterRun(rgx_cohort *co_, const rgx_cohort_matrix *m_, const char *name_, char *err_, size_t errlen_)
        : CohortRun(co_, name_, err_, errlen_), m(m_) {}
    uint32_t site_bits(int side) const { return std::max<uint32_t>(1, bitlen(side ? max_end : max_start)); }
    uint32_t tid_bits() const { return std::max<uint32_t>(1, bitlen(max_tid)); }

    // the matrix where the kernels read it (its image in HBM, or uploaded) and the row workspace; max_intron: what n_ineligible counts against
    int open(bool refine, uint32_t max_intron) {
        const bool in_hbm = matrix_serial(m) == co->image_serial;
        co->cluster_path = in_hbm ? 1 : 0;
        n = (uint32_t)m->n; nnz = (uint32_t)m->row_begin[m->n];
        if (!n) return RGX_OK;
        if (int rc = enter()) return rc;
        // the pass counts come from the data
        for (uint32_t i = 0; i < n; ++i) {
            max_start = std::max(max_start, m->start[i]); max_end = std::max(max_end, m->end[i]); max_tid = std::max(max_tid, m->tid[i]);
            if (max_intron && m->end[i] - m->start[i] > max_intron) ++n_ineligible;
        }
        if (int rc = cohort_matrix_image(co, m, st, &in, err, errlen)) return rc;
        mark("matrix in HBM");

        const size_t Nn = (size_t)n + 64;
        const size_t tmp_words = radix_tmp_words(n) + scan_tmp_words(n) + 64;
        if (int rc = grow(co->cl_rows, (Nn * (8 + 13 + (refine ? 4 : 0)) + 8 + 64 + tmp_words) * 4 + 256,
                          "regtools_amd: no device memory to cluster %u rows\n", n)) return rc;
        // first writers: the scalars' flags the memset of every search batch, their counts the scans (n_alive: launch_refine_compact, read only
        // behind a second search); cls k_cluster_class; perm0 .. perm3, key0, key1 the sorts' passes; alive k_refine_eligible; pos the compaction's
        // scan; ea*, eb* the edge kernels [0, n_edges); parent k_cc_init; tot and cnt (= ea0) the memsets of mark_weak and finish, then the tallies;
        // keep, is_root the root kernels; cid_excl and the counts' scans the scans; cluster, sort_key, cl_count, cl_total k_cluster_assign
        // (cl_count and cl_total [0, C)); o_cl_begin k_cluster_widen, o_cs_begin k_cluster_cs_begin, each [0, C]; len, ent_off k_cluster_row_len and
        // its scan; tmp: the passes' and scans' scratch.  All [0, n) unless said; the 64 pad elements of every array are never touched.
        Carve w = carve(co->cl_rows);
        tot = (unsigned long long *)w.u64(Nn); cl_total = (unsigned long long *)w.u64(Nn); o_cl_begin = (unsigned long long *)w.u64(Nn + 1);
        o_cs_begin = (unsigned long long *)w.u64(Nn + 1);
        d_sc = (ClusterScalars *)w.u32(64);
        parent = w.u32(Nn); ea0 = w.u32(Nn); eb0 = w.u32(Nn); ea1 = w.u32(Nn); eb1 = w.u32(Nn); perm0 = w.u32(Nn); perm1 = w.u32(Nn);
        key0 = w.u32(Nn); key1 = w.u32(Nn); cls = w.u32(Nn); cluster = w.u32(Nn); cl_count = w.u32(Nn); tmp = w.u32(tmp_words);
        if (refine) { perm2 = w.u32(Nn); perm3 = w.u32(Nn); alive = w.u32(Nn); pos = w.u32(Nn); }
        CARVE_TRY(w, "cluster rows");
        if (int rc = carved(w, "cluster rows")) return rc;
        return RGX_OK;
    }

    // 1. edges: neighbours in the stable order of (tid, class, start), then of (tid, class, end); the second sort takes the first one's buffers
    int site_edges() {
        launch_cluster_class(in.strand, n, cls, st);
        RadixSort by_site{{perm0, perm1}, tmp, n, st, {key0, key1}};
        by_site.by_keyed(in.start, site_bits(0)); by_site.by_keyed(cls, 2); by_site.by_keyed(in.tid, tid_bits());
        launch_cluster_edges(by_site.sorted(), in.tid, cls, in.start, n, ea0, eb0, st);
        by_site.reset();
        by_site.by_keyed(in.end, site_bits(1)); by_site.by_keyed(cls, 2); by_site.by_keyed(in.tid, tid_bits());
        launch_cluster_edges(by_site.sorted(), in.tid, cls, in.end, n, ea1, eb1, st);
        mark("site sorts + edges");
        return RGX_OK;
    }

    // 1 (refine). the same two sorts, each in buffers of its own: both orders stay, to be compacted as rows leave
    int site_orders(uint32_t max_intron) {
        launch_cluster_class(in.strand, n, cls, st);
        launch_refine_eligible(in.start, in.end, n, max_intron, alive, st);
        uint32_t *bufs[2][2] = {{perm0, perm1}, {perm2, perm3}};
        for (int side = 0; side < 2; ++side) {
            RadixSort by_site{{bufs[side][0], bufs[side][1]}, tmp, n, st, {key0, key1}};
            by_site.by_keyed(side ? in.end : in.start, site_bits(side)); by_site.by_keyed(cls, 2); by_site.by_keyed(in.tid, tid_bits());
            order[side] = by_site.sorted(); order_spare[side] = by_site.spare();
        }
        mark("site sorts");
        return RGX_OK;
    }

    // Both orders compacted to the rows alive now (k_in entries each; the survivors' count goes to d_sc->n_alive), then the edges between neighbours
    // on a site.  n_out: the survivors' count when the host knows it, else the edge kernels read it on the device and fill k_in slots.
    int compact_edges(uint32_t k_in, bool compact, const uint32_t *n_out) {
        for (int side = 0; side < 2; ++side) {
            if (compact) {
                launch_refine_compact(order[side], k_in, alive, pos, order_spare[side], &d_sc->n_alive, tmp, st);
                uint32_t *was = (uint32_t *)order[side]; order[side] = order_spare[side]; order_spare[side] = was;
            }
            uint32_t *ea = side ? ea1 : ea0, *eb = side ? eb1 : eb0;
            const uint32_t *site = side ? in.end : in.start;
            if (n_out) launch_cluster_edges(order[side], in.tid, cls, site, *n_out, ea, eb, st);
            else launch_refine_edges(order[side], &d_sc->n_alive, in.tid, cls, site, k_in, ea, eb, st);
        }
        mark("compaction + edges");
        return RGX_OK;
    }

    // 2. components: parent[i] = the smallest row of i's component, over n_edges entries of each edge list
    int components(uint32_t n_edges) {
        const EdgeList lists[2] = {{ea0, eb0, n_edges}, {ea1, eb1, n_edges}};
        uint32_t rounds = 0;
        const int rc = components_run(n, lists, 2, parent, d_sc->flags, st, &rounds, err, errlen);
        if (rc != RGX_OK) return rc;
        n_rounds += rounds;
        mark("components");
        return RGX_OK;
    }

    // refine, between the searches: T per stage-1 root, then the weak rows stop being alive (the edge arrays are free from the search on)
    int mark_weak(const rgx_refine_params &p) {
        HIP_TRY(hipMemsetAsync(tot, 0, (size_t)n * 8, st));
        launch_refine_tally(parent, in.total, alive, n, nullptr, tot, st);
        launch_refine_mark(parent, in.total, tot, n, p.min_reads, p.ratio_num, p.ratio_den, alive, st);
        mark("totals + weak rows");
        return RGX_OK;
    }

    // 3. clusters, 4. denominators, and the result in host memory.  with_alive: a row that is not alive is not tallied, no root and not kept.
    // n_alive_out: receives d_sc->n_alive, read back with the other scalars.
    int finish(bool with_alive, uint32_t min_rows, uint64_t min_total, uint32_t *n_alive_out, rgx_cohort_clusters **out) {
        // (the edge arrays are free from here on)
        uint32_t *cnt = ea0, *keep = eb0, *cid_excl = ea1, *sort_key = eb1, *is_root = cls;
        HIP_TRY(hipMemsetAsync(cnt, 0, (size_t)n * 4, st));
        HIP_TRY(hipMemsetAsync(tot, 0, (size_t)n * 8, st));
        if (with_alive) {
            launch_refine_tally(parent, in.total, alive, n, cnt, tot, st);
            launch_refine_roots(parent, cnt, tot, alive, n, min_rows, min_total, is_root, keep, st);
        } else {
            launch_cluster_tally(parent, in.total, n, cnt, tot, st);
            launch_cluster_roots(parent, cnt, tot, n, min_rows, min_total, is_root, keep, st);
        }
        launch_scan_u32(keep, cid_excl, n, &d_sc->n_clusters, tmp, st);
        launch_scan_u32(is_root, key0, n, &d_sc->n_components, tmp, st);
        ClusterScalars sc;
        HIP_TRY(read_back(st, &sc, d_sc, sizeof sc));
        const uint32_t C = sc.n_clusters, n_components = sc.n_components;
        if (n_alive_out) *n_alive_out = sc.n_alive;
        launch_cluster_assign(parent, keep, cid_excl, cnt, tot, n, C, cluster, sort_key, cl_count, cl_total, st);
        uint32_t *cl_begin32 = cnt;                                          // (assign was the last reader of cnt, keep and cid_excl)
        launch_scan_u32(cl_count, cl_begin32, C, &d_sc->n_kept, tmp, st);
        launch_cluster_widen(cl_begin32, C, &d_sc->n_kept, o_cl_begin, st);
        RadixSort by_cluster{{perm0, perm1}, tmp, n, st, {key0, key1}};
        by_cluster.by_keyed(sort_key, std::max<uint32_t>(1, bitlen(C)));    // (dropped rows carry C: behind every cluster)
        const uint32_t *cl_row = by_cluster.sorted();
        // 4. denominators: the entries of clustered rows that are not zero, as (cluster, sample, count)
        const bool wave_per_row = (uint64_t)n * 32 <= nnz;
        uint32_t *len = keep, *ent_off = cid_excl;
        launch_cluster_row_len(cluster, in.row_begin, in.val_count, n, wave_per_row, len, st);
        launch_scan_u32(len, ent_off, n, &d_sc->n_entries, tmp, st);
        HIP_TRY(read_back(st, &sc, d_sc, sizeof sc));
        const uint32_t n_kept = sc.n_kept, M = sc.n_entries;
        mark("clusters + cl_row");

        uint32_t n_cs = 0;
        const uint32_t *cs_sample = nullptr; const unsigned long long *cs_total = nullptr;
        if (M) {
            const size_t Mn = (size_t)M + 64;
            const size_t etmp_words = radix_tmp_words(M) + scan_tmp_words(M) + 64;
            if (int rc = grow(co->cl_entries, (Mn * (2 + 7) + etmp_words) * 4 + 256, "regtools_amd: no device memory for the clusters' %u counts\n", M)) return rc;
            // first writers: e_cluster, e_sample, e_count k_cluster_expand [0, M); eperm*, ekey* the sort's passes; then ekey0 (heads)
            // k_cluster_cs_heads, ekey1 (seg) the scan, the spare permutation k_cohort_row_start, each [0, M); then ekey0 (seg_cluster), ekey1
            // (samples) and sums k_cluster_cs_sum [0, n_cs); etmp: scratch.  The 64 pad elements of every array are never touched.
            Carve q = carve(co->cl_entries);
            unsigned long long *sums = (unsigned long long *)q.u64(Mn);
            uint32_t *e_cluster = q.u32(Mn), *e_sample = q.u32(Mn), *e_count = q.u32(Mn), *eperm0 = q.u32(Mn), *eperm1 = q.u32(Mn), *ekey0 = q.u32(Mn),
                     *ekey1 = q.u32(Mn), *etmp = q.u32(etmp_words);
            CARVE_TRY(q, "cluster entries");
            if (int rc = carved(q, "cluster entries")) return rc;
            launch_cluster_expand(cluster, in.row_begin, in.col_sample, in.val_count, ent_off, n, wave_per_row, e_cluster, e_sample, e_count, st);
            // stable LSD sort by (cluster, sample): the entries of one pair end up side by side
            RadixSort by_pair{{eperm0, eperm1}, etmp, M, st, {ekey0, ekey1}};
            by_pair.by_keyed(e_sample, std::max<uint32_t>(1, bitlen(std::max<uint32_t>(m->n_samples, 1) - 1)));
            by_pair.by_keyed(e_cluster, std::max<uint32_t>(1, bitlen(C - 1)));
            mark("entries + pair sort");
            uint32_t *head = ekey0, *seg = ekey1, *seg_start = by_pair.spare();
            launch_cluster_cs_heads(by_pair.sorted(), e_cluster, e_sample, M, head, st);
            launch_scan_u32(head, seg, M, &d_sc->n_cs, etmp, st);
            launch_cohort_row_start(head, seg, M, seg_start, st);
            HIP_TRY(read_back(st, &sc, d_sc, sizeof sc));
            n_cs = sc.n_cs;
            uint32_t *seg_cluster = head, *samples = seg;                   // (the heads and their scan are used up)
            launch_cluster_cs_sum(by_pair.sorted(), e_cluster, e_sample, e_count, seg_start, M, n_cs, seg_cluster, samples, sums, st);
            launch_cluster_cs_begin(seg_cluster, n_cs, C, o_cs_begin, st);
            cs_sample = samples; cs_total = sums;
        } else launch_cluster_cs_begin(nullptr, 0, C, o_cs_begin, st);
        mark("heads + sums");

        rgx_cohort_clusters *c = clusters_alloc(n, C, n_kept, n_cs, /*pinned=*/true);
        if (!c) { (void)hipStreamSynchronize(st); return fail(err, errlen, RGX_ERR_DEVICE, "regtools_amd: no memory for the clusters\n"); }
        CopyBack back{st};
        guards_back(back);
        back(c->cluster, cluster, (size_t)n * 4); back(c->cl_begin, o_cl_begin, ((size_t)C + 1) * 8); back(c->cs_begin, o_cs_begin, ((size_t)C + 1) * 8);
        back(c->cl_total, cl_total, (size_t)C * 8); back(c->cl_row, cl_row, (size_t)n_kept * 4); back(c->cs_sample, cs_sample, (size_t)n_cs * 4);
        back(c->cs_total, cs_total, (size_t)n_cs * 8);
        const hipError_t e_ = back.wait();
        if (e_ != hipSuccess) { rgx_cohort_clusters_free(c); return fail(err, errlen, RGX_ERR_DEVICE, "HIP error %s clustering the cohort\n", hipGetErrorString(e_)); }
        mark("copy");
        if (int rc = guards_check()) { rgx_cohort_clusters_free(c); return rc; }
        c->n_rounds = n_rounds; c->n_components = n_components; c->ms_cluster = now_ms() - t0;
        *out = c;
        return RGX_OK;
    }

    // the result of a matrix without rows: no launch
    int empty(rgx_cohort_clusters **out) {
        rgx_cohort_clusters *c = clusters_alloc(0, 0, 0, 0, false);
        if (!c) return fail(err, errlen, RGX_ERR_DEVICE, "regtools_amd: no memory for the clusters\n");
        c->n_rounds = 0; c->n_components = 0; c->ms_cluster = now_ms() - t0;
        *out = c;
        return RGX_OK;
    }
};

}  // namespace

extern "C" int rgx_cohort_cluster(rgx_cohort *co, const rgx_cohort_matrix *m, const rgx_cluster_params *p, rgx_cohort_clusters **out, char *err,
                                  size_t errlen) {
    if (!co || !m || !out) return fail(err, errlen, RGX_ERR_ARG, "regtools_amd: rgx_cohort_cluster needs a cohort and a matrix\n");
    *out = nullptr;
    std::lock_guard<std::mutex> lock(co->mu);
    ClusterRun run(co, m, "cluster", err, errlen);
    rgx_cluster_params prm; if (p) prm = *p; else rgx_cluster_params_default(&prm);
    int rc = check_limits(m, err, errlen);
    if (rc == RGX_OK) rc = run.open(/*refine=*/false, 0);
    if (rc != RGX_OK) return rc;
    if (!run.n) return run.empty(out);
    rc = run.site_edges();
    if (rc == RGX_OK) rc = run.components(run.n);
    if (rc == RGX_OK) rc = run.finish(/*with_alive=*/false, prm.min_rows, prm.min_total, nullptr, out);
    return rc;
}

extern "C" void rgx_refine_params_default(rgx_refine_params *p) {
    if (p) { p->max_intron = 0; p->min_reads = 0; p->ratio_num = 0; p->ratio_den = 1; p->min_rows = 1; p->min_total = 0; }
}

namespace {
int check_refine(const rgx_refine_params &p, char *err, size_t errlen) {
    if (p.ratio_den == 0 || p.ratio_num > p.ratio_den) return fail(err, errlen, RGX_ERR_ARG,
        "regtools_amd: the ratio %u/%u is not a share between 0 and 1\n", p.ratio_num, p.ratio_den);
    return RGX_OK;
}
}  // namespace

// Stages: the two site orders (kept, each in its own buffers) -> compacted to the eligible rows when some are not -> edges, search 1 -> T per root,
// weak rows marked -> both orders compacted again (their length now known to the device only: the edge kernel reads it, sized for stage 1's) ->
// edges, search 2 -> cluster's own numbering and denominators over the alive rows.  No host wait beyond the searches' own and finish's three; when
// no row can be weak (min_reads 0 and ratio_num 0) or none is eligible, stage 2 is stage 1 and the second search is not run.
extern "C" int rgx_cohort_refine(rgx_cohort *co, const rgx_cohort_matrix *m, const rgx_refine_params *p, rgx_cohort_clusters **out, char *err,
                                 size_t errlen) {
    if (!co || !m || !out) return fail(err, errlen, RGX_ERR_ARG, "regtools_amd: rgx_cohort_refine needs a cohort and a matrix\n");
    *out = nullptr;
    std::lock_guard<std::mutex> lock(co->mu);
    ClusterRun run(co, m, "refine", err, errlen);
    rgx_refine_params prm; if (p) prm = *p; else rgx_refine_params_default(&prm);
    int rc = check_refine(prm, err, errlen);
    if (rc == RGX_OK) rc = check_limits(m, err, errlen);
    if (rc == RGX_OK) rc = run.open(/*refine=*/true, prm.max_intron);
    if (rc != RGX_OK) return rc;
    if (!run.n) return run.empty(out);
    const uint32_t n_eligible = run.n - run.n_ineligible;
    const bool second = n_eligible && (prm.min_reads || prm.ratio_num);
    rc = run.site_orders(prm.max_intron);
    if (rc == RGX_OK) rc = run.compact_edges(run.n, /*compact=*/run.n_ineligible != 0, &n_eligible);
    if (rc == RGX_OK) rc = run.components(n_eligible);
    if (rc == RGX_OK && second) {
        rc = run.mark_weak(prm);
        if (rc == RGX_OK) rc = run.compact_edges(n_eligible, /*compact=*/true, nullptr);
        if (rc == RGX_OK) rc = run.components(n_eligible);
    }
    uint32_t n_alive = n_eligible;
    if (rc == RGX_OK) rc = run.finish(/*with_alive=*/true, prm.min_rows, prm.min_total, second ? &n_alive : nullptr, out);
    if (rc == RGX_OK) { (*out)->n_ineligible = run.n_ineligible; (*out)->n_weak = n_eligible - n_alive; }
    return rc;
}

// ---- the host twins: the same contracts in plain C++ (std::sort for the site groups, union-find, one pass per cluster) -----------------------
namespace {

struct UnionFind {
    std::vector<uint32_t> parent;
    explicit UnionFind(uint32_t n) : parent(n) { for (uint32_t i = 0; i < n; ++i) parent[i] = i; }
    uint32_t find(uint32_t v) { while (parent[v] != v) { parent[v] = parent[parent[v]]; v = parent[v]; } return v; }
    void unite(uint32_t a, uint32_t b) { a = find(a); b = find(b); if (a != b) parent[std::max(a, b)] = std::min(a, b); }   // (the root is the lowest row)
};

// the components of the rows that are alive (null: every row) under the link rule; a row that is not alive stays alone
UnionFind host_components(const rgx_cohort_matrix *m, const uint8_t *alive) {
    const uint32_t n = (uint32_t)m->n;
    UnionFind uf(n);
    std::vector<uint32_t> order;
    for (uint32_t i = 0; i < n; ++i) if (!alive || alive[i]) order.push_back(i);
    for (int side = 0; side < 2; ++side) {
        const uint32_t *site = side ? m->end : m->start;
        auto same = [&](uint32_t a, uint32_t b) { return m->tid[a] == m->tid[b] && rgx::strand_class(m->strand[a]) == rgx::strand_class(m->strand[b]) && site[a] == site[b]; };
        std::sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) {
            if (m->tid[a] != m->tid[b]) return m->tid[a] < m->tid[b];
            const uint32_t ca = rgx::strand_class(m->strand[a]), cb = rgx::strand_class(m->strand[b]);
            if (ca != cb) return ca < cb;
            if (site[a] != site[b]) return site[a] < site[b];
            return a < b;
        });
        for (size_t i = 1; i < order.size(); ++i) if (same(order[i - 1], order[i])) uf.unite(order[i - 1], order[i]);
    }
    return uf;
}

// filters, numbering, member rows and denominators of the components in uf, over the alive rows (null: every row)
int host_clusters(const rgx_cohort_matrix *m, UnionFind &uf, const uint8_t *alive, uint32_t min_rows, uint64_t min_total, double t0,
                  rgx_cohort_clusters **out, char *err, size_t errlen) {
    const uint32_t n = (uint32_t)m->n;
    auto live = [&](uint32_t i) { return !alive || alive[i]; };
    std::vector<uint32_t> rows_of(n, 0), cid(n, RGX_NO_CLUSTER);
    std::vector<uint64_t> total_of(n, 0);
    for (uint32_t i = 0; i < n; ++i) if (live(i)) { const uint32_t r = uf.find(i); ++rows_of[r]; total_of[r] += m->total[i]; }
    uint64_t n_components = 0, C = 0, n_kept = 0;
    for (uint32_t i = 0; i < n; ++i) if (live(i) && uf.parent[i] == i) {
        ++n_components;
        if (rows_of[i] >= min_rows && total_of[i] >= min_total) { cid[i] = (uint32_t)C++; n_kept += rows_of[i]; }
    }
    // the member rows, ascending within a cluster
    std::vector<uint64_t> begin(C + 1, 0);
    for (uint32_t i = 0; i < n; ++i) if (uf.parent[i] == i && cid[i] != RGX_NO_CLUSTER) begin[cid[i] + 1] = rows_of[i];
    for (uint64_t k = 0; k < C; ++k) begin[k + 1] += begin[k];
    std::vector<uint32_t> members(n_kept);
    { std::vector<uint64_t> at(begin.begin(), begin.end() - 1);
      for (uint32_t i = 0; i < n; ++i) { const uint32_t k = cid[uf.find(i)]; if (k != RGX_NO_CLUSTER) members[at[k]++] = i; } }
    // per cluster and sample: a dense accumulator and the list of the samples touched
    std::vector<uint64_t> acc(std::max<uint32_t>(m->n_samples, 1), 0), cs_begin(C + 1, 0), cs_total;
    std::vector<uint32_t> touched, cs_sample;
    for (uint64_t k = 0; k < C; ++k) {
        touched.clear();
        for (uint64_t q = begin[k]; q < begin[k + 1]; ++q) {
            const uint32_t r = members[q];
            for (uint64_t e = m->row_begin[r]; e < m->row_begin[r + 1]; ++e) {
                const uint32_t s = m->col_sample[e];
                if (!m->val_count[e] || s >= acc.size()) continue;
                if (!acc[s]) touched.push_back(s);
                acc[s] += m->val_count[e];
            }
        }
        std::sort(touched.begin(), touched.end());
        for (uint32_t s : touched) { cs_sample.push_back(s); cs_total.push_back(acc[s]); acc[s] = 0; }
        cs_begin[k + 1] = cs_sample.size();
    }
    rgx_cohort_clusters *c = clusters_alloc(n, C, n_kept, cs_sample.size(), false);
    if (!c) return fail(err, errlen, RGX_ERR_ARG, "regtools_amd: no memory for the clusters\n");
    for (uint32_t i = 0; i < n; ++i) {
        const uint32_t r = uf.find(i);
        c->cluster[i] = cid[r];
        if (r == i && cid[i] != RGX_NO_CLUSTER) c->cl_total[cid[i]] = total_of[i];
    }
    memcpy(c->cl_begin, begin.data(), (C + 1) * 8); memcpy(c->cs_begin, cs_begin.data(), (C + 1) * 8);
    if (n_kept) memcpy(c->cl_row, members.data(), n_kept * 4);
    if (!cs_sample.empty()) { memcpy(c->cs_sample, cs_sample.data(), cs_sample.size() * 4); memcpy(c->cs_total, cs_total.data(), cs_total.size() * 8); }
    c->n_rounds = 0; c->n_components = n_components; c->ms_cluster = now_ms() - t0;
    *out = c;
    return RGX_OK;
}

}  // namespace

extern "C" int rgx_cohort_cluster_host(const rgx_cohort_matrix *m, const rgx_cluster_params *p, rgx_cohort_clusters **out, char *err, size_t errlen) {
    if (!m || !out) return fail(err, errlen, RGX_ERR_ARG, "regtools_amd: rgx_cohort_cluster_host needs a matrix\n");
    *out = nullptr;
    const double t0 = now_ms();
    rgx_cluster_params prm; if (p) prm = *p; else rgx_cluster_params_default(&prm);
    const int rc_lim = check_limits(m, err, errlen);
    if (rc_lim != RGX_OK) return rc_lim;
    UnionFind uf = host_components(m, nullptr);
    return host_clusters(m, uf, nullptr, prm.min_rows, prm.min_total, t0, out, err, errlen);
}

extern "C" int rgx_cohort_refine_host(const rgx_cohort_matrix *m, const rgx_refine_params *p, rgx_cohort_clusters **out, char *err, size_t errlen) {
    if (!m || !out) return fail(err, errlen, RGX_ERR_ARG, "regtools_amd: rgx_cohort_refine_host needs a matrix\n");
    *out = nullptr;
    const double t0 = now_ms();
    rgx_refine_params prm; if (p) prm = *p; else rgx_refine_params_default(&prm);
    int rc = check_refine(prm, err, errlen);
    if (rc == RGX_OK) rc = check_limits(m, err, errlen);
    if (rc != RGX_OK) return rc;
    const uint32_t n = (uint32_t)m->n;
    std::vector<uint8_t> alive(n);
    uint64_t n_ineligible = 0, n_weak = 0;
    for (uint32_t i = 0; i < n; ++i) { alive[i] = prm.max_intron == 0 || m->end[i] - m->start[i] <= prm.max_intron; n_ineligible += !alive[i]; }
    UnionFind uf = host_components(m, alive.data());
    if (prm.min_reads || prm.ratio_num) {                    // (otherwise no row can be weak: stage 2 is stage 1)
        std::vector<uint64_t> T(n, 0);
        for (uint32_t i = 0; i < n; ++i) if (alive[i]) T[uf.find(i)] += m->total[i];
        for (uint32_t i = 0; i < n; ++i) if (alive[i]) {
            const unsigned __int128 lhs = (unsigned __int128)m->total[i] * prm.ratio_den, rhs = (unsigned __int128)T[uf.find(i)] * prm.ratio_num;
            if (m->total[i] < prm.min_reads || lhs < rhs) { alive[i] = 0; ++n_weak; }       // (T and the roots are stage 1's: the order does not matter)
        }
        if (n_weak) uf = host_components(m, alive.data());
    }
    rc = host_clusters(m, uf, alive.data(), prm.min_rows, prm.min_total, t0, out, err, errlen);
    if (rc == RGX_OK) { (*out)->n_ineligible = n_ineligible; (*out)->n_weak = n_weak; }
    return rc;
}

// ---- text ------------------------------------------------------------------------------------------------------------------------------
extern "C" size_t rgx_cohort_format_cluster_counts(const rgx_cohort_matrix *m, const rgx_cohort_clusters *cl, char *buf, size_t cap) {
    if (!m || !cl || cl->n_rows != m->n) return 0;
    return format_twice(buf, cap, [&](TextOut &o) {
        o.put("chrom");
        for (uint32_t g = 0; g < m->n_samples; ++g) { o.put(" ", 1); o.put(m->sample_name[g]); }
        o.put("\n", 1);
        for (uint64_t i = 0; i < m->n; ++i) {
            const uint32_t c = cl->cluster[i];
            if (c == RGX_NO_CLUSTER) continue;
            put_intron_id(o, m, cl, (uint32_t)i);
            uint64_t e = m->row_begin[i], d = cl->cs_begin[c];
            const uint64_t e_end = m->row_begin[i + 1], d_end = cl->cs_begin[c + 1];
            for (uint32_t g = 0; g < m->n_samples; ++g) {
                uint32_t a = 0; uint64_t b = 0;
                if (e < e_end && m->col_sample[e] == g) a = m->val_count[e++];
                if (d < d_end && cl->cs_sample[d] == g) b = cl->cs_total[d++];
                o.put(" ", 1); o.u(a); o.put("/", 1); o.u(b);
            }
            o.put("\n", 1);
        }
    });
}
