// cohort.cpp -- the cohort junction-by-sample count matrix: rgx_cohort_create / _add / _finish, their host twin rgx_cohort_merge_host and the two text
// formats (include/regtools_amd.h).
//
// Replaces the per-sample loop plus the merge a cohort run makes after src/junctions/junctions_main.cc:45-59 of the reference -- one BED file per BAM,
// joined by a script; the reference has no counterpart.  The semantics (rows that take part, contigs by name, key, reductions, order, filters) are
// stated once, in the header.  Device side: cohort_kernels.hip.  add is an enqueue: a sample's rows go from the block its extraction left in the source
// context's HBM (or from an uploaded copy of the host table) into the accumulator on the cohort's own stream; finish sorts, reduces and copies back.
#include "cohort_internal.h"

namespace {

inline bool anchored(const rgx_junction_table *t, uint64_t i, uint32_t min_anchor) {
    return (uint32_t)(t->start[i] - t->thick_start[i]) >= min_anchor && (uint32_t)(t->thick_end[i] - t->end[i]) >= min_anchor;
}

std::atomic<uint64_t> g_matrix_serial{0};

rgx_cohort_matrix *matrix_alloc(const CohortContigs &c, const std::vector<std::string> &samples, uint64_t n, uint64_t nnz, bool pinned) {
    // the block is the device's image (matrix_layout): ONE array, the members pointed into it from L
    const MatrixLayout L = matrix_layout(n, nnz);
    uint8_t *q = nullptr;
    rgx_cohort_matrix *m = result_alloc<rgx_cohort_matrix, uint64_t>(pinned, [&](rgx_cohort_matrix &, BlockTake &take) { take(q, L.bytes); });
    if (!m) return nullptr;
    result_extra<uint64_t>(m) = ++g_matrix_serial;
    m->n_ref = (int32_t)c.names.size();
    m->ref_name = (char **)calloc(c.names.size() + 1, sizeof(char *)); m->ref_len = (uint32_t *)calloc(c.names.size() + 1, 4);
    for (size_t i = 0; i < c.names.size(); ++i) { m->ref_name[i] = strdup(c.names[i].c_str()); m->ref_len[i] = c.lens[i]; }
    m->n_samples = (uint32_t)samples.size();
    m->sample_name = (char **)calloc(samples.size() + 1, sizeof(char *));
    for (size_t i = 0; i < samples.size(); ++i) m->sample_name[i] = strdup(samples[i].c_str());
    m->n = n;
    m->total = (uint64_t *)(q + L.total); m->row_begin = (uint64_t *)(q + L.row_begin); m->tid = (uint32_t *)(q + L.tid); m->start = (uint32_t *)(q + L.start);
    m->end = (uint32_t *)(q + L.end); m->thick_start = (uint32_t *)(q + L.ts); m->thick_end = (uint32_t *)(q + L.te); m->n_with = (uint32_t *)(q + L.n_with);
    m->col_sample = (uint32_t *)(q + L.col); m->val_count = (uint32_t *)(q + L.val); m->strand = (char *)(q + L.strand);
    m->row_begin[0] = 0;
    return m;
}

}  // namespace

// what rgx_cohort_finish's scans leave 16 words behind the append counter d_fill[0] (a block of 256 bytes): the distinct keys, and the rows and counts
// the filters keep (read back by one copy)
struct FinishTotals { uint32_t rows; struct Kept { uint32_t rows, nnz; } kept; };

extern "C" void rgx_cohort_params_default(rgx_cohort_params *p) { if (p) { p->only_anchored = 1; p->min_samples = 1; p->min_total = 1; } }

extern "C" int rgx_cohort_create(rgx_ctx *ctx, const rgx_cohort_params *p, rgx_cohort **out, char *err, size_t errlen) {
    if (!ctx || !out) return fail(err, errlen, RGX_ERR_ARG, "regtools_amd: a cohort needs a context\n");
    *out = nullptr;
    HIP_ENTER(ctx->device);
    std::unique_ptr<rgx_cohort> co(new rgx_cohort);
    co->device = ctx->device;
    if (p) co->p = *p; else rgx_cohort_params_default(&co->p);
    auto bail = [&](hipError_t e) { rgx_cohort *c = co.release(); rgx_cohort_destroy(c); return fail(err, errlen, RGX_ERR_DEVICE,
        "HIP error %s creating the cohort\n", hipGetErrorString(e)); };
    hipError_t e = hipStreamCreateWithFlags(&co->stream, hipStreamNonBlocking);
    if (e == hipSuccess) e = hipEventCreateWithFlags(&co->ev_src, hipEventDisableTiming);
    if (e == hipSuccess) e = hipEventCreateWithFlags(&co->ev_done, hipEventDisableTiming);
    if (e == hipSuccess) e = hipEventCreateWithFlags(&co->ev_up, hipEventDisableTiming);
    if (e == hipSuccess) e = hipMalloc((void **)&co->d_blocks, kMaxBlocks * sizeof(uint32_t *));
    if (e == hipSuccess) e = hipMalloc((void **)&co->d_fill, 256);
    if (e == hipSuccess) e = hipMemsetAsync(co->d_fill, 0, 256, co->stream);
    if (e != hipSuccess) return bail(e);
    *out = co.release();
    return RGX_OK;
}

extern "C" void rgx_cohort_destroy(rgx_cohort *co) {
    if (!co) return;
    (void)hipSetDevice(co->device);
    if (co->stream) (void)hipStreamSynchronize(co->stream);
    for (size_t k = 0; k < co->n_blocks; ++k) (void)hipFree(co->blocks[k]);
    for (auto &m : co->maps) if (m->dev) (void)hipFree(m->dev);
    if (co->d_blocks) (void)hipFree(co->d_blocks);
    if (co->d_fill) (void)hipFree(co->d_fill);
    co->up.release(); co->sort.release(); co->rows.release(); co->image.release();
    co->cl_in.release(); co->cl_rows.release(); co->cl_entries.release();
    co->ph_in.release(); co->ph_rows.release(); co->ph_entries.release();
    co->pc_in.release(); co->pc_part.release(); co->pc_out.release();
    co->qt_in.release(); co->qt_rows.release(); co->qt_t.release(); co->qt_out.release(); co->qp_in.release(); co->qp_out.release(); co->qx_tiles.release(); co->qc_in.release(); co->qc_ws.release();
    if (co->pinned_up) { if (co->pinned_up_locked) (void)hipHostFree(co->pinned_up); else free(co->pinned_up); }
    if (co->ev_src) (void)hipEventDestroy(co->ev_src);
    if (co->ev_done) (void)hipEventDestroy(co->ev_done);
    if (co->ev_up) (void)hipEventDestroy(co->ev_up);
    if (co->stream) (void)hipStreamDestroy(co->stream);
    (void)hipGetLastError();
    delete co;
}

extern "C" int rgx_cohort_add_path(rgx_cohort *co) { return co ? co->last_path : 0; }

extern "C" int rgx_cohort_add(rgx_cohort *co, rgx_ctx *src, const rgx_junction_table *t, uint32_t min_anchor, const char *sample_name,
                              uint32_t *sample_index, char *err, size_t errlen) {
    if (!co || !t || !sample_name) return fail(err, errlen, RGX_ERR_ARG, "regtools_amd: rgx_cohort_add needs a cohort, a table and a sample name\n");
    std::lock_guard<std::mutex> lock(co->mu);
    const double t0 = now_ms();
    if (co->sample_names.size() + 1 >= kMaxSamples) return fail(err, errlen, RGX_ERR_ARG, "regtools_amd: a cohort holds fewer than %u samples\n", kMaxSamples);
    if (t->n >= (1ull << 32)) return fail(err, errlen, RGX_ERR_ARG, "regtools_amd: sample %s has too many rows for a cohort\n", sample_name);
    const uint32_t n = (uint32_t)t->n, sample = (uint32_t)co->sample_names.size();
    // what the host needs to know of the rows: that every tid is the header's, how many take part, how wide the sort's words are (plain loops over
    // the columns, no branches: this runs between a file's wait and the submit that follows it)
    int32_t tid_lo = 0, tid_hi = -1;
    for (uint32_t i = 0; i < n; ++i) { tid_lo = std::min(tid_lo, t->tid[i]); tid_hi = std::max(tid_hi, t->tid[i]); }
    if (tid_lo < 0 || tid_hi >= t->n_ref) {
        uint32_t i = 0;
        while (t->tid[i] >= 0 && t->tid[i] < t->n_ref) ++i;
        return fail(err, errlen, RGX_ERR_ARG, "regtools_amd: row %u of sample %s is on contig %d of %d\n", i, sample_name, t->tid[i], t->n_ref);
    }
    uint64_t n_keep = 0; uint32_t mx_s = 0, mx_e = 0;
    const uint32_t every = co->p.only_anchored ? 0u : 1u;
    for (uint32_t i = 0; i < n; ++i) {
        const uint32_t k = every | (uint32_t)anchored(t, i, min_anchor);
        n_keep += k; mx_s = std::max(mx_s, k ? t->start[i] : 0u); mx_e = std::max(mx_e, k ? t->end[i] : 0u);
    }
    if (co->n_triples + n_keep > kMaxTriples) return fail(err, errlen, RGX_ERR_ARG,
        "regtools_amd: a cohort holds at most %llu (junction, sample) pairs; sample %s would make it %llu\n", (unsigned long long)kMaxTriples, sample_name,
        (unsigned long long)(co->n_triples + n_keep));
    std::vector<uint32_t> map;
    const int rc = co->contigs.map_sample(t, sample, sample_name, co->sample_names, map, err, errlen);
    if (rc != RGX_OK) return rc;
    // From here on the sample is part of the cohort (its contigs are): a device error below leaves the cohort unusable, and says so.
    co->sample_names.push_back(sample_name);
    if (sample_index) *sample_index = sample;
    co->last_path = 0;
    if (n_keep) {
        HIP_ENTER(co->device);
        const uint64_t need_rows = co->n_triples + n_keep;
        while ((uint64_t)co->n_blocks * kCohortBlockRows < need_rows) {
            uint32_t *b = nullptr;
            if (hipMalloc((void **)&b, (size_t)kCohortBlockRows * kCohortColumns * 4) != hipSuccess) { (void)hipGetLastError();
                return fail(err, errlen, RGX_ERR_DEVICE, "regtools_amd: no device memory for the cohort's block %zu (%llu triples so far)\n", co->n_blocks,
                            (unsigned long long)co->n_triples); }
            co->blocks[co->n_blocks] = b;
            HIP_TRY(hipMemcpyAsync(co->d_blocks + co->n_blocks, &co->blocks[co->n_blocks], sizeof(uint32_t *), hipMemcpyHostToDevice, co->stream));
            ++co->n_blocks;
        }
        if (co->maps.empty() || co->maps.back()->host != map) {
            std::unique_ptr<rgx_cohort::TidMap> m(new rgx_cohort::TidMap);
            m->host = map;
            HIP_TRY(hipMalloc((void **)&m->dev, std::max<size_t>(1, map.size()) * 4));
            co->maps.push_back(std::move(m));
            HIP_TRY(hipMemcpyAsync(co->maps.back()->dev, co->maps.back()->host.data(), map.size() * 4, hipMemcpyHostToDevice, co->stream));
        }
        const uint32_t *d_map = co->maps.back()->dev;
        const uint32_t cap = (uint32_t)std::min<uint64_t>((uint64_t)co->n_blocks * kCohortBlockRows, 0xffffffffu);
        const bool on_device = src && src->device == co->device && src->last_rows_valid && t->n == src->last_rows && t->n_records == src->last_records &&
                               t->n_events == src->last_events && t->inflated_bytes == src->last_bytes;
        if (on_device) {
            // behind the source context's last kernel, and in front of its next one: the next call there overwrites the rows
            HIP_TRY(hipEventRecord(co->ev_src, src->stream));
            HIP_TRY(hipStreamWaitEvent(co->stream, co->ev_src, 0));
            launch_cohort_append(src->buf(Buf::rows_out).as<uint32_t>(), n, n, 9, d_map, (uint32_t)map.size(), min_anchor, co->p.only_anchored != 0, sample,
                                 co->d_fill, cap, co->d_blocks, co->stream);
            HIP_TRY(hipEventRecord(co->ev_done, co->stream));
            HIP_TRY(hipStreamWaitEvent(src->stream, co->ev_done, 0));
            co->last_path = 1;
        } else {
            if (co->up_pending) { HIP_TRY(hipEventSynchronize(co->ev_up)); co->up_pending = false; }      // (the staging blocks are the last upload's)
            const size_t bytes = (size_t)n * kCohortColumns * 4;
            if (bytes > co->pinned_up_cap) {
                if (co->pinned_up) { if (co->pinned_up_locked) (void)hipHostFree(co->pinned_up); else free(co->pinned_up); }
                co->pinned_up = nullptr; co->pinned_up_cap = 0;
                const size_t want = bytes + bytes / 4;
                co->pinned_up_locked = hipHostMalloc(&co->pinned_up, want, hipHostMallocDefault) == hipSuccess;
                if (!co->pinned_up_locked) { (void)hipGetLastError(); co->pinned_up = malloc(want); }
                if (!co->pinned_up) return fail(err, errlen, RGX_ERR_DEVICE, "regtools_amd: no host memory to stage sample %s\n", sample_name);
                co->pinned_up_cap = want;
            }
            uint32_t *h = (uint32_t *)co->pinned_up;
            memcpy(h, t->tid, (size_t)n * 4); memcpy(h + n, t->start, (size_t)n * 4); memcpy(h + 2 * (size_t)n, t->end, (size_t)n * 4);
            memcpy(h + 3 * (size_t)n, t->thick_start, (size_t)n * 4); memcpy(h + 4 * (size_t)n, t->thick_end, (size_t)n * 4);
            memcpy(h + 5 * (size_t)n, t->read_count, (size_t)n * 4);
            for (uint32_t i = 0; i < n; ++i) h[6 * (size_t)n + i] = (uint8_t)t->strand[i];
            HIP_TRY(co->up.ensure(bytes));
            HIP_TRY(hipMemcpyAsync(co->up.p, h, bytes, hipMemcpyHostToDevice, co->stream));
            launch_cohort_append(co->up.as<uint32_t>(), n, n, 6, d_map, (uint32_t)map.size(), min_anchor, co->p.only_anchored != 0, sample, co->d_fill, cap,
                                 co->d_blocks, co->stream);
            HIP_TRY(hipEventRecord(co->ev_up, co->stream));
            co->up_pending = true;
        }
        co->n_triples += n_keep; co->max_start = std::max(co->max_start, mx_s); co->max_end = std::max(co->max_end, mx_e);
    } else if (src && src->device == co->device && src->last_rows_valid && t->n == src->last_rows && t->n_records == src->last_records &&
               t->n_events == src->last_events && t->inflated_bytes == src->last_bytes) co->last_path = 1;      // (nothing to move: where it would have come from)
    co->ms_add_total += now_ms() - t0;
    return RGX_OK;
}

extern "C" int rgx_cohort_finish(rgx_cohort *co, rgx_cohort_matrix **out, char *err, size_t errlen) {
    if (!co || !out) return fail(err, errlen, RGX_ERR_ARG, "regtools_amd: rgx_cohort_finish needs a cohort\n");
    *out = nullptr;
    std::lock_guard<std::mutex> lock(co->mu);
    const double t0 = now_ms();
    CohortRun run(co, "cohort", err, errlen);                           // (the device, the stream, and the fill mode of the two workspaces cut below)
    if (int rc = run.enter()) return rc;
    hipStream_t st = run.st;
    const bool trace = run.trace;
    double t_last = t0;
    auto mark = [&](const char *what) { if (trace) { (void)hipStreamSynchronize(st); const double t = now_ms(); fprintf(stderr,
        "[rgx trace] cohort: %-28s +%8.3f ms\n", what, t - t_last); t_last = t; } };
    uint32_t filled = 0;
    HIP_TRY(read_back(st, &filled, co->d_fill, 4));                      // (every append has run)
    co->up_pending = false;
    if (filled != co->n_triples) return fail(err, errlen, RGX_ERR_DEVICE,
        "regtools_amd: the cohort holds %u triples on the device and %llu by the host's count (a table changed between its extraction and its add?)\n",
        filled, (unsigned long long)co->n_triples);
    mark("appends drained");
    const uint32_t N = filled;
    uint32_t U = 0, Uk = 0, NNZ = 0;
    rgx_cohort_matrix *m = nullptr;
    if (N) {
        const size_t Nn = (size_t)N + 64;                                // (every array padded: row_start has one entry more than rows)
        const size_t tmp_words = radix_tmp_words(N) + scan_tmp_words(N) + 64;
        if (co->sort.ensure((Nn * (2 + 2 + 7) + tmp_words) * 4 + 256) != hipSuccess) { (void)hipGetLastError(); return fail(err, errlen, RGX_ERR_DEVICE,
            "regtools_amd: no device memory to sort %u triples\n", N); }
        // first writers: key0, key1, perm0, perm1 the sort's passes (launch_cohort_key gathers every key word); s.* k_cohort_gather; then, the sort
        // over, key0 (heads) k_cohort_gather, key1 (seg) the scan, the spare permutation k_cohort_row_start; tmp: scratch.  All [0, N); the 64 pad
        // elements of every array are never touched.  Not filled: the blocks of `add` with d_blocks, d_fill and the tid maps, which hold the
        // cohort's triples from add to finish, and `image` below, which holds the matrix for the calls that follow.
        Carve w = run.carve(co->sort);
        uint32_t *key0 = w.u32(Nn), *key1 = w.u32(Nn), *perm0 = w.u32(Nn), *perm1 = w.u32(Nn);
        CohortSorted s; s.tid = w.u32(Nn); s.start = w.u32(Nn); s.end = w.u32(Nn); s.ts = w.u32(Nn); s.te = w.u32(Nn); s.count = w.u32(Nn); s.ss = w.u32(Nn);
        uint32_t *tmp = w.u32(tmp_words); CARVE_TRY(w, "cohort sort");
        if (int rc = run.carved(w, "cohort sort")) return rc;
        FinishTotals *d_tot = (FinishTotals *)(co->d_fill + 16);
        // stable LSD radix sort by (tid, start, end, class): the triples of one key keep the order they were appended in, which is sample order.
        // Each key word is gathered through the permutation once; its 8-bit passes then stream (key, permutation) pairs.
        RadixSort by_key{{perm0, perm1}, tmp, N, st, {key0, key1}};
        auto sort_word = [&](uint32_t which, uint32_t nbits) {
            by_key.by_gathered([&](const uint32_t *perm_in, uint32_t *out) { launch_cohort_key(co->d_blocks, perm_in, N, which, out, st); }, nbits);
        };
        sort_word(3, 2);
        sort_word(2, std::max<uint32_t>(1, bitlen(co->max_end)));
        sort_word(1, std::max<uint32_t>(1, bitlen(co->max_start)));
        sort_word(0, std::max<uint32_t>(1, bitlen((uint32_t)std::max<size_t>(co->contigs.names.size(), 1) - 1)));
        mark("key sort");
        uint32_t *head = key0, *seg = key1, *row_start = by_key.spare();
        launch_cohort_gather(co->d_blocks, by_key.sorted(), N, s, head, st);
        launch_scan_u32(head, seg, N, &d_tot->rows, tmp, st);
        launch_cohort_row_start(head, seg, N, row_start, st);
        HIP_TRY(read_back(st, &U, &d_tot->rows, 4));
        mark("gather + heads");
        const size_t Un = (size_t)U + 64;
        if (co->rows.ensure(Un * (2 + 6) * 4 + 256) != hipSuccess) { (void)hipGetLastError(); return fail(err, errlen, RGX_ERR_DEVICE,
            "regtools_amd: no device memory for %u cohort rows\n", U); }
        // first writers: r.* k_cohort_reduce, out_row and nnz_excl the scans, all [0, U)
        Carve q = run.carve(co->rows);
        CohortRows r; r.total = (unsigned long long *)q.u64(Un); r.ts = q.u32(Un); r.te = q.u32(Un); r.keep = q.u32(Un); r.kept_nnz = q.u32(Un);
        uint32_t *out_row = q.u32(Un), *nnz_excl = q.u32(Un); CARVE_TRY(q, "cohort rows");
        if (int rc = run.carved(q, "cohort rows")) return rc;
        launch_cohort_reduce(s, row_start, N, U, co->p.min_samples, co->p.min_total, r, st);
        launch_scan_u32(r.keep, out_row, U, &d_tot->kept.rows, tmp, st);
        launch_scan_u32(r.kept_nnz, nnz_excl, U, &d_tot->kept.nnz, tmp, st);
        FinishTotals::Kept kept = {0, 0};
        HIP_TRY(read_back(st, &kept, &d_tot->kept, sizeof kept));
        Uk = kept.rows; NNZ = kept.nnz;
        mark("reduce + filters");
        const MatrixLayout L = matrix_layout(Uk, NNZ);
        co->image_serial = 0;                                            // (the image is about to be rewritten)
        if (co->image.ensure(L.bytes + 256) != hipSuccess) { (void)hipGetLastError(); return fail(err, errlen, RGX_ERR_DEVICE,
            "regtools_amd: no device memory for the cohort matrix (%u rows, %u counts)\n", Uk, NNZ); }
        uint8_t *b = co->image.as<uint8_t>();
        const CohortImage o = image_at(b, L);
        launch_cohort_out(s, head, seg, row_start, r, out_row, nnz_excl, N, U, NNZ, o, st);
        m = matrix_alloc(co->contigs, co->sample_names, Uk, NNZ, /*pinned=*/true);
        if (!m) { (void)hipStreamSynchronize(st); return fail(err, errlen, RGX_ERR_DEVICE, "regtools_amd: no memory for the cohort matrix\n"); }
        CopyBack back{st};
        run.guards_back(back);
        back((uint8_t *)m->total - L.total, b, L.bytes);                // (the whole image, where matrix_alloc pointed the members)
        const hipError_t e_ = back.wait();
        if (e_ != hipSuccess) { rgx_cohort_matrix_free(m); return fail(err, errlen, RGX_ERR_DEVICE, "HIP error %s finishing the cohort\n", hipGetErrorString(e_)); }
        if (int rc = run.guards_check()) { rgx_cohort_matrix_free(m); return rc; }
        co->image_serial = matrix_serial(m);
        mark("rows out + copy");
    } else {
        m = matrix_alloc(co->contigs, co->sample_names, 0, 0, false);
        if (!m) return fail(err, errlen, RGX_ERR_DEVICE, "regtools_amd: no memory for the cohort matrix\n");
        co->image_serial = matrix_serial(m);                             // (no rows: nothing of it needs to be in HBM)
    }
    m->n_triples = N; m->ms_add_total = co->ms_add_total; m->ms_finish = now_ms() - t0;
    *out = m;
    return RGX_OK;
}

extern "C" void rgx_cohort_matrix_free(rgx_cohort_matrix *m) {
    if (!m) return;
    for (int32_t i = 0; i < m->n_ref; ++i) free(m->ref_name[i]);
    for (uint32_t i = 0; i < m->n_samples; ++i) free(m->sample_name[i]);
    free(m->ref_name); free(m->ref_len); free(m->sample_name);
    result_free<rgx_cohort_matrix, uint64_t>(m);
}

// ---- the host twin: the same contract in plain C++ (records, std::sort, one pass over the runs) ----------------------------------------
extern "C" int rgx_cohort_merge_host(const rgx_junction_table *const *tables, const uint32_t *min_anchor, const char *const *names, int n,
                                     const rgx_cohort_params *p, rgx_cohort_matrix **out, char *err, size_t errlen) {
    if (!out || n < 0 || (n && (!tables || !min_anchor || !names))) return fail(err, errlen, RGX_ERR_ARG, "regtools_amd: bad arguments\n");
    *out = nullptr;
    if ((uint64_t)n >= kMaxSamples) return fail(err, errlen, RGX_ERR_ARG, "regtools_amd: a cohort holds fewer than %u samples\n", kMaxSamples);
    rgx_cohort_params prm; if (p) prm = *p; else rgx_cohort_params_default(&prm);
    const double t0 = now_ms();
    struct Rec { uint32_t tid, start, end, cls, sample, ts, te, count; char strand; };
    std::vector<Rec> recs;
    CohortContigs contigs; std::vector<std::string> samples;
    for (int g = 0; g < n; ++g) {
        const rgx_junction_table *t = tables[g];
        if (!t || !names[g]) return fail(err, errlen, RGX_ERR_ARG, "regtools_amd: sample %d has no table or no name\n", g);
        std::vector<uint32_t> map;
        const int rc = contigs.map_sample(t, (uint32_t)g, names[g], samples, map, err, errlen);
        if (rc != RGX_OK) return rc;
        samples.push_back(names[g]);
        for (uint64_t i = 0; i < t->n; ++i) {
            if (t->tid[i] < 0 || t->tid[i] >= t->n_ref) return fail(err, errlen, RGX_ERR_ARG, "regtools_amd: row %llu of sample %s is on contig %d of %d\n",
                (unsigned long long)i, names[g], t->tid[i], t->n_ref);
            if (prm.only_anchored && !anchored(t, i, min_anchor[g])) continue;
            const char c = t->strand[i];
            recs.push_back(Rec{map[(size_t)t->tid[i]], t->start[i], t->end[i], c == '+' ? 0u : c == '-' ? 1u : 2u, (uint32_t)g, t->thick_start[i],
                               t->thick_end[i], t->read_count[i], c});
        }
    }
    if (recs.size() > kMaxTriples) return fail(err, errlen, RGX_ERR_ARG, "regtools_amd: a cohort holds at most %llu (junction, sample) pairs\n",
        (unsigned long long)kMaxTriples);
    std::sort(recs.begin(), recs.end(), [](const Rec &a, const Rec &b) {
        if (a.tid != b.tid) return a.tid < b.tid;
        if (a.start != b.start) return a.start < b.start;
        if (a.end != b.end) return a.end < b.end;
        if (a.cls != b.cls) return a.cls < b.cls;
        return a.sample < b.sample;
    });
    auto same = [](const Rec &a, const Rec &b) { return a.tid == b.tid && a.start == b.start && a.end == b.end && a.cls == b.cls; };
    // first pass: how many rows and counts survive the filters
    uint64_t rows = 0, nnz = 0;
    for (size_t b = 0; b < recs.size();) {
        size_t e = b; uint64_t total = 0;
        while (e < recs.size() && same(recs[b], recs[e])) total += recs[e++].count;
        if (e - b >= prm.min_samples && total >= prm.min_total) { ++rows; nnz += e - b; }
        b = e;
    }
    rgx_cohort_matrix *m = matrix_alloc(contigs, samples, rows, nnz, false);
    if (!m) return fail(err, errlen, RGX_ERR_ARG, "regtools_amd: no memory for the cohort matrix\n");
    uint64_t q = 0, k = 0;
    for (size_t b = 0; b < recs.size();) {
        size_t e = b; uint64_t total = 0; uint32_t ts = 0xffffffffu, te = 0;
        while (e < recs.size() && same(recs[b], recs[e])) { total += recs[e].count; ts = std::min(ts, recs[e].ts); te = std::max(te, recs[e].te); ++e; }
        if (e - b >= prm.min_samples && total >= prm.min_total) {
            m->tid[q] = recs[b].tid; m->start[q] = recs[b].start; m->end[q] = recs[b].end; m->thick_start[q] = ts; m->thick_end[q] = te;
            m->strand[q] = recs[e - 1].strand; m->n_with[q] = (uint32_t)(e - b); m->total[q] = total; m->row_begin[q] = k;
            for (size_t i = b; i < e; ++i, ++k) { m->col_sample[k] = recs[i].sample; m->val_count[k] = recs[i].count; }
            ++q;
        }
        b = e;
    }
    m->row_begin[q] = k;
    m->n_triples = recs.size(); m->ms_finish = now_ms() - t0;
    *out = m;
    return RGX_OK;
}

// ---- text ------------------------------------------------------------------------------------------------------------------------------
extern "C" size_t rgx_cohort_format_bed12(const rgx_cohort_matrix *m, char *buf, size_t cap) {
    if (!m) return 0;
    return format_twice(buf, cap, [&](TextOut &o) {
        for (uint64_t i = 0; i < m->n; ++i) {
            const uint32_t ts = m->thick_start[i], te = m->thick_end[i];
            o.put(m->ref_name[m->tid[i]]);                       // everything behind the contig name: bounded numeric fields (format_bed12_rows)
            o.fmt("\t%u\t%u\tJUNC%08llu\t%llu\t%c\t%u\t%u\t255,0,0\t2\t%u,%u\t0,%u\n", ts, te, (unsigned long long)(i + 1),
                  (unsigned long long)m->total[i], m->strand[i], ts, te, (uint32_t)(m->start[i] - ts), (uint32_t)(te - m->end[i]),
                  (uint32_t)(m->end[i] - ts));
        }
    });
}

extern "C" size_t rgx_cohort_format_counts(const rgx_cohort_matrix *m, char *buf, size_t cap) {
    if (!m) return 0;
    return format_twice(buf, cap, [&](TextOut &o) {
        o.put("chrom\tstart\tend\tstrand");
        for (uint32_t g = 0; g < m->n_samples; ++g) { o.put("\t", 1); o.put(m->sample_name[g]); }
        o.put("\n", 1);
        for (uint64_t i = 0; i < m->n; ++i) {
            o.put(m->ref_name[m->tid[i]]);
            o.fmt("\t%u\t%u\t%c", m->start[i], m->end[i], m->strand[i]);
            uint64_t k = m->row_begin[i];
            const uint64_t e = m->row_begin[i + 1];
            for (uint32_t g = 0; g < m->n_samples; ++g) {
                if (k < e && m->col_sample[k] == g) { o.put("\t", 1); o.u(m->val_count[k]); ++k; }
                else o.put("\t0", 2);
            }
            o.put("\n", 1);
        }
    });
}
