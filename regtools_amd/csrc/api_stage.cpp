// api_stage.cpp -- stage entry points of the tail behind the DEFLATE launch: the exclusive scan, the radix sort and the group-by on the caller's
// own device arrays, so that tests can hand each of them inputs no BAM would (tests/test_gpu_stage_kernels.py).  Nothing here is a copy: the scan is
// launch_scan_u32, the sort is the RadixSort of api_internal.h driven the three ways the product drives it, the group-by is reduce_events.  Scratch
// is a buffer of the context carved the way reduce_events carves its "sort" buffer, with guard words behind the scan / radix scratch: a
// radix_tmp_words or scan_tmp_words that is too small for what a pass writes fails the call instead of going unseen in the buffer's growth slack.
#include "api_internal.h"

#include "cse_internal.h"

typedef StageGuard Guard;       // (api_internal.h: the interval stages' shared halves arm theirs where they carve)

extern "C" int rgx_k_scan_u32(rgx_ctx *c, const uint32_t *d_in, uint32_t *d_out, uint32_t n, uint32_t *d_total, char *err, size_t errlen) {
    if (!c || (n && (!d_in || !d_out))) return fail(err, errlen, RGX_ERR_ARG, "regtools_amd: bad arguments\n");
    HIP_ENTER(c->device);
    hipStream_t st = c->stream;
    DevBuf &b = c->buf(Buf::stage);
    const size_t tmp_words = scan_tmp_words(n);
    HIP_TRY(b.ensure((tmp_words + kGuardWords) * 4 + 256));
    Carve q(b);
    uint32_t *tmp = q.u32(tmp_words), *guard_at = q.u32(kGuardWords); CARVE_TRY(q, "stage");
    Guard g; g.arm(guard_at, st);
    launch_scan_u32(d_in, d_out, n, d_total, tmp, st);
    bool touched = false;
    HIP_TRY(g.check(st, &touched));
    if (touched) return fail(err, errlen, RGX_ERR_DEVICE, "regtools_amd: the scan wrote behind its scan_tmp_words(%u) words of scratch\n", n);
    return RGX_OK;
}

// BGZF member discovery (members_kernels.hip) on the caller's file in HBM (tests/test_gpu_member_discovery.py): MemberDiscovery is what stage_members runs, the
// scalar block is prepared the way stage_upload prepares it.  The candidate list and the member list have guard words behind them.
extern "C" int rgx_k_members(rgx_ctx *c, const void *d_bam, uint64_t bam_len, uint64_t root2, const uint32_t *d_true_sizes, const uint64_t *q_coff,
                             rgx_members_result **out, char *err, size_t errlen) {
    if (!c || !out || !q_coff || (bam_len && !d_bam)) return fail(err, errlen, RGX_ERR_ARG, "regtools_amd: bad arguments\n");
    *out = nullptr;
    rgx_members_result *r = (rgx_members_result *)calloc(1, sizeof *r);
    if (!r) return fail(err, errlen, RGX_ERR_ARG, "regtools_amd: out of memory\n");
    struct Holder { rgx_members_result *r; ~Holder() { rgx_members_result_free(r); } } hold{r};
    r->candidates = (uint64_t *)malloc(8); r->members = (rgx_member *)malloc(sizeof(rgx_member));
    for (int k = 0; k < 3; ++k) { r->q_index[k] = 0; r->q_upos[k] = ~0ull; }
    r->stop = 0xffffffffu;
    if (bam_len) {
        HIP_ENTER(c->device);
        hipStream_t st = c->stream;
        DevBuf &b_scalars = c->buf(Buf::scalars);
        HIP_TRY(b_scalars.ensure(sizeof(Scalars)));
        MemberDiscovery md;
        md.c = c; md.st = st; md.d_bam = (const uint8_t *)d_bam; md.bam_len = bam_len; md.d_true_sizes = d_true_sizes;
        md.d_sc = b_scalars.as<Scalars>(); md.h_sc = (Scalars *)c->pinned;
        HIP_TRY(hipMemsetAsync(md.d_sc, 0, sizeof(Scalars), st));
        { const int rc = md.candidates(/*guarded=*/true, err, errlen); if (rc != kGoOn) return rc; }
        if (md.n_cand) {
            md.chain(UINT64_MAX);
            if (root2 != UINT64_MAX) md.chain(root2);
            HIP_TRY(md.query(q_coff));
            const Scalars &h = *md.h_sc;
            if (h.n_members > md.n_cand) return fail(err, errlen, RGX_ERR_DEVICE, "regtools_amd: %u members of %u candidates\n", h.n_members, md.n_cand);
            r->n_candidates = md.n_cand; r->n_members = h.n_members; r->total_inflated = h.total_inflated; r->stop = h.stop;
            for (int k = 0; k < 3; ++k) { r->q_index[k] = h.q_index[k]; r->q_upos[k] = h.q_upos[k]; }
            free(r->candidates); free(r->members);
            r->candidates = (uint64_t *)malloc((size_t)md.n_cand * 8 + 8); r->members = (rgx_member *)malloc(((size_t)h.n_members + 1) * sizeof(rgx_member));
            if (!r->candidates || !r->members) return fail(err, errlen, RGX_ERR_ARG, "regtools_amd: out of memory\n");
            static_assert(sizeof(rgx_member) == sizeof(Member), "rgx_member is rgx::Member");
            HIP_TRY(hipMemcpyAsync(r->candidates, md.cand, (size_t)md.n_cand * 8, hipMemcpyDeviceToHost, st));
            if (r->n_members) HIP_TRY(hipMemcpyAsync(r->members, md.d_members, (size_t)r->n_members * sizeof(Member), hipMemcpyDeviceToHost, st));
            bool past_cand = false, past_members = false;
            HIP_TRY(md.g_cand.check(st, &past_cand));
            HIP_TRY(md.g_members.check(st, &past_members));
            if (past_cand) return fail(err, errlen, RGX_ERR_DEVICE, "regtools_amd: the candidate fill wrote behind its %u candidates\n", md.n_cand);
            if (past_members) return fail(err, errlen, RGX_ERR_DEVICE, "regtools_amd: the member fill wrote behind the room of %u members\n", md.n_cand);
        }
    }
    hold.r = nullptr;
    *out = r;
    return RGX_OK;
}
extern "C" void rgx_members_result_free(rgx_members_result *r) { if (!r) return; free(r->candidates); free(r->members); free(r); }

extern "C" int rgx_k_radix_sort(rgx_ctx *c, uint32_t n, uint32_t n_scratch, uint32_t n_words, const uint32_t *const *d_words, const uint32_t *nbits,
                                int mode, uint32_t *d_perm_out, char *err, size_t errlen) {
    if (!c || !n_words || !d_words || !nbits || mode < 0 || mode > 2 || (n && !d_perm_out)) return fail(err, errlen, RGX_ERR_ARG,
        "regtools_amd: bad arguments\n");
    for (uint32_t k = 0; k < n_words; ++k) if (!nbits[k] || nbits[k] > 32 || (n && !d_words[k])) return fail(err, errlen, RGX_ERR_ARG,
        "regtools_amd: word %u of the sort key has no column or not 1 to 32 bits\n", k);
    if (!n_scratch) n_scratch = n;
    if (n_scratch < n) return fail(err, errlen, RGX_ERR_ARG, "regtools_amd: scratch for %u keys does not hold a sort of %u\n", n_scratch, n);
    if (!n) return RGX_OK;
    HIP_ENTER(c->device);
    hipStream_t st = c->stream;
    // (reduce_events' "sort" buffer: two permutations, two key columns, the scratch of a pass and of a scan)
    DevBuf &b = c->buf(Buf::stage);
    const size_t E = n_scratch, rtmp = radix_tmp_words(n_scratch) + scan_tmp_words(n_scratch) + 64;
    HIP_TRY(b.ensure((E * 4 + rtmp + kGuardWords) * 4 + 256));
    Carve q(b);
    uint32_t *perm0 = q.u32(E), *perm1 = q.u32(E), *key0 = q.u32(E), *key1 = q.u32(E), *tmp = q.u32(rtmp), *guard_at = q.u32(kGuardWords);
    CARVE_TRY(q, "stage");
    Guard g; g.arm(guard_at, st);
    RadixSort rs{{perm0, perm1}, tmp, n, st, {key0, key1}};
    hipError_t copy_err = hipSuccess;
    for (uint32_t k = 0; k < n_words; ++k) {
        const uint32_t *w = d_words[k];
        if (mode == 0) rs.by(w, nbits[k]);
        else if (mode == 1) rs.by_keyed(w, nbits[k]);
        else rs.by_gathered([&](const uint32_t *perm_in, uint32_t *key_out) {
            if (perm_in) launch_gather_u32(n, w, perm_in, key_out, st);
            else if (copy_err == hipSuccess) copy_err = hipMemcpyAsync(key_out, w, (size_t)n * 4, hipMemcpyDeviceToDevice, st);
        }, nbits[k]);
    }
    HIP_TRY(copy_err);
    HIP_TRY(hipMemcpyAsync(d_perm_out, rs.sorted(), (size_t)n * 4, hipMemcpyDeviceToDevice, st));
    bool touched = false;
    HIP_TRY(g.check(st, &touched));
    if (touched) return fail(err, errlen, RGX_ERR_DEVICE, "regtools_amd: a radix pass over %u keys wrote behind the scratch sized for %u\n", n, n_scratch);
    return RGX_OK;
}

extern "C" int rgx_k_group_by(rgx_ctx *c, const uint32_t *d_tid, const uint32_t *d_start, const uint32_t *d_ilen_cls, const uint32_t *d_ts,
                              const uint32_t *d_te, const uint8_t *d_strand, uint32_t n_events, uint32_t group_bits, uint32_t ilen_bits,
                              const uint32_t *rank_of_group_host, uint32_t n_groups, int form, uint32_t *d_rows_out, uint64_t *n_rows_out,
                              uint32_t *d_ev_urow, uint32_t *d_urow_pos, char *err, size_t errlen) {
    if (!c || !n_rows_out || form < 0 || form > 2 || !rank_of_group_host || !n_groups || !group_bits || group_bits > 32 || !ilen_bits || ilen_bits > 32 ||
        (n_events && (!d_tid || !d_start || !d_ilen_cls || !d_ts || !d_te || !d_strand || !d_rows_out)) ||
        (form == 2 && n_events && (!d_ev_urow || !d_urow_pos))) return fail(err, errlen, RGX_ERR_ARG, "regtools_amd: bad arguments\n");
    *n_rows_out = 0;
    HIP_ENTER(c->device);
    hipStream_t st = c->stream;
    HIP_TRY(c->buf(Buf::scalars).ensure(sizeof(Scalars)));
    EventSoA ev; memset(&ev, 0, sizeof ev);
    ev.tid = (uint32_t *)d_tid; ev.start = (uint32_t *)d_start; ev.ilen_cls = (uint32_t *)d_ilen_cls; ev.ts = (uint32_t *)d_ts; ev.te = (uint32_t *)d_te;
    ev.strand = (uint8_t *)d_strand;
    HostRows R; RowMap rm;
    const int rc = reduce_events(c, ev, n_events, group_bits, ilen_bits, rank_of_group_host, n_groups, R, err, errlen, /*view_only=*/true,
                                 form == 2 ? &rm : nullptr, nullptr, /*allow_preagg=*/form == 0);
    c->last_rows_valid = false;            // these rows are no extraction's table (rgx_last_table_pack_device)
    if (rc != RGX_OK) return rc;
    if (R.n) HIP_TRY(hipMemcpyAsync(d_rows_out, c->buf(Buf::rows_out).p, R.n * 40, hipMemcpyDeviceToDevice, st));
    if (form == 2 && n_events) {
        HIP_TRY(hipMemcpyAsync(d_ev_urow, rm.ev_urow, (size_t)n_events * 4, hipMemcpyDeviceToDevice, st));
        if (R.n) HIP_TRY(hipMemcpyAsync(d_urow_pos, rm.urow_pos, R.n * 4, hipMemcpyDeviceToDevice, st));
    }
    HIP_TRY(hipStreamSynchronize(st));
    *n_rows_out = R.n;
    return RGX_OK;
}

extern "C" int rgx_k_components(rgx_ctx *c, uint32_t n_vertices, uint32_t n_edges, const uint32_t *d_a, const uint32_t *d_b, uint32_t *d_label_out,
                                uint32_t *n_rounds, char *err, size_t errlen) {
    if (!c || (n_edges && (!d_a || !d_b)) || (n_vertices && !d_label_out)) return fail(err, errlen, RGX_ERR_ARG, "regtools_amd: bad arguments\n");
    if (n_rounds) *n_rounds = 0;
    HIP_ENTER(c->device);
    hipStream_t st = c->stream;
    // (rgx_cohort_cluster's loop: the labels live in the caller's array, the scratch is the rounds' flag words)
    DevBuf &b = c->buf(Buf::stage);
    HIP_TRY(b.ensure((kCcBatch + kGuardWords) * 4 + 256));
    Carve q(b);
    uint32_t *flags = q.u32(kCcBatch), *guard_at = q.u32(kGuardWords); CARVE_TRY(q, "stage");
    Guard g; g.arm(guard_at, st);
    const EdgeList list = {d_a, d_b, n_edges};
    const int rc = components_run(n_vertices, &list, 1, d_label_out, flags, st, n_rounds, err, errlen);
    if (rc != RGX_OK) return rc;
    bool touched = false;
    HIP_TRY(g.check(st, &touched));
    if (touched) return fail(err, errlen, RGX_ERR_DEVICE, "regtools_amd: the component search wrote behind its %u flag words\n", kCcBatch);
    return RGX_OK;
}

// ---- the interval kernels of cis-splice-effects / annotate (cse_kernels.hip) on the caller's own junctions, events and windows ---------------------
// (tests/test_gpu_cse_edges.py).  Each runs the half its command runs: junction_scan_items is annotate_junctions' front, window_pair_batches is
// window_join's, assoc_join is `associate`'s join as it stands.  The variable-length outputs lie in Buf::stage with guard words behind them.
extern "C" int rgx_gtf_bin_index(const rgx_gtf *g) { return g && g->view.bin_start ? 1 : 0; }

extern "C" int rgx_k_junction_scan(rgx_ctx *c, const rgx_gtf *g, uint64_t n, const int32_t *contig, const uint32_t *start, const uint32_t *end1,
                                   const char *strand, int keep_single, int form, rgx_junction_items **out, char *err, size_t errlen) {
    if (!c || !g || !out || form < 0 || form > 1 || n >= (1ull << 31) || (n && (!contig || !start || !end1 || !strand)))
        return fail(err, errlen, RGX_ERR_ARG, "regtools_amd: bad arguments\n");
    *out = nullptr;
    const int64_t n_chroms = (int64_t)g->m.chroms.size();
    for (uint64_t i = 0; i < n; ++i) if (contig[i] >= n_chroms) return fail(err, errlen, RGX_ERR_ARG,
        "regtools_amd: junction %llu is on contig %d of an annotation with %lld\n", (unsigned long long)i, contig[i], (long long)n_chroms);
    std::vector<int32_t> ci(contig, contig + n); std::vector<uint32_t> js(start, start + n), je(end1, end1 + n);
    std::vector<uint8_t> sd((const uint8_t *)strand, (const uint8_t *)strand + n);
    GtfView view = g->view; view.keep_single = keep_single ? 1u : 0u;
    JunctionItemsHost R;
    const int rc = junction_scan_items(c, view, ci, js, je, sd, form, /*guarded=*/true, R, err, errlen);
    if (rc != RGX_OK) return rc;
    rgx_junction_items *r = (rgx_junction_items *)calloc(1, sizeof *r);
    r->n = n; r->visits_total = R.visits_total; r->flags = dup_u32(R.flags); r->visits = dup_u32(R.visits); r->item_off = dup_u32(R.off);
    r->item_kind = dup_u32(R.kind); r->item_a = dup_u32(R.a); r->item_b = dup_u32(R.b);
    *out = r;
    return RGX_OK;
}
extern "C" void rgx_junction_items_free(rgx_junction_items *r) {
    if (!r) return;
    free(r->flags); free(r->visits); free(r->item_off); free(r->item_kind); free(r->item_a); free(r->item_b); free(r);
}

static rgx_pair_list *pair_list(const std::vector<uint32_t> &first, const std::vector<uint32_t> &window, uint32_t n_batches) {
    rgx_pair_list *r = (rgx_pair_list *)calloc(1, sizeof *r);
    r->n = first.size(); r->n_batches = n_batches; r->first = dup_u32(first); r->window = dup_u32(window);
    return r;
}
extern "C" void rgx_pair_list_free(rgx_pair_list *r) { if (!r) return; free(r->first); free(r->window); free(r); }

extern "C" int rgx_k_window_pairs(rgx_ctx *c, const uint32_t *d_tid, const uint32_t *d_rpos, const uint32_t *d_rend, uint32_t n_events, uint32_t n_windows,
                                  const int32_t *w_tid, const int32_t *w_beg, const int32_t *w_end, uint64_t pair_batch, rgx_pair_list **out, char *err,
                                  size_t errlen) {
    if (!c || !out || (n_events && (!d_tid || !d_rpos || !d_rend)) || (n_windows && (!w_tid || !w_beg || !w_end)))
        return fail(err, errlen, RGX_ERR_ARG, "regtools_amd: bad arguments\n");
    *out = nullptr;
    HIP_ENTER(c->device);
    hipStream_t st = c->stream;
    HIP_TRY(c->buf(Buf::scalars).ensure(sizeof(Scalars)));
    EventSoA ev; memset(&ev, 0, sizeof ev);
    ev.tid = (uint32_t *)d_tid; ev.rpos = (uint32_t *)d_rpos; ev.rend = (uint32_t *)d_rend;
    const std::vector<int32_t> wt(w_tid, w_tid + n_windows), wb(w_beg, w_beg + n_windows), we(w_end, w_end + n_windows);
    std::vector<uint32_t> pe, pw;
    uint64_t n_pairs = 0; uint32_t n_batches = 0;
    const int rc = window_pair_batches(c, ev, n_events, wt, wb, we, pair_batch, /*guarded=*/true, [&](uint32_t w0, uint32_t, uint32_t total, const PairLayout &L) {
        const size_t at = pe.size();
        pe.resize(at + total); pw.resize(at + total);
        HIP_TRY(hipMemcpyAsync(pe.data() + at, L.pair_ev, (size_t)total * 4, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipMemcpyAsync(pw.data() + at, L.pair_win, (size_t)total * 4, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        for (size_t k = at; k < pw.size(); ++k) pw[k] += w0;                  // (a batch numbers its windows from 0)
        return (int)RGX_OK;
    }, n_pairs, n_batches, err, errlen);
    if (rc != RGX_OK) return rc;
    if (n_pairs != pe.size()) return fail(err, errlen, RGX_ERR_DEVICE, "regtools_amd: %llu pairs counted, %zu filled\n", (unsigned long long)n_pairs, pe.size());
    *out = pair_list(pe, pw, n_batches);
    return RGX_OK;
}

extern "C" int rgx_k_assoc_pairs(rgx_ctx *c, uint32_t n_windows, const int32_t *w_contig, const uint32_t *w_ces, const uint32_t *w_cee, uint32_t n_contigs,
                                 const uint32_t *contig_off, uint32_t n_junctions, const uint32_t *j_start, const uint32_t *j_end, rgx_pair_list **out,
                                 char *err, size_t errlen) {
    if (!c || !out || !contig_off || (n_windows && (!w_contig || !w_ces || !w_cee)) || (n_junctions && (!j_start || !j_end)))
        return fail(err, errlen, RGX_ERR_ARG, "regtools_amd: bad arguments\n");
    *out = nullptr;
    // the kernel trusts the buckets: they must tile [0, n_junctions), and every window's contig must have one
    bool ok = contig_off[0] == 0 && contig_off[n_contigs] == n_junctions;
    for (uint32_t k = 0; ok && k < n_contigs; ++k) ok = contig_off[k] <= contig_off[k + 1];
    for (uint32_t w = 0; ok && w < n_windows; ++w) ok = w_contig[w] < (int64_t)n_contigs;
    if (!ok) return fail(err, errlen, RGX_ERR_ARG, "regtools_amd: the contig buckets do not tile the junctions, or a window names a contig without one\n");
    const std::vector<int32_t> wch(w_contig, w_contig + n_windows);
    const std::vector<uint32_t> wces(w_ces, w_ces + n_windows), wcee(w_cee, w_cee + n_windows), off(contig_off, contig_off + n_contigs + 1),
        js(j_start, j_start + n_junctions), je(j_end, j_end + n_junctions);
    std::vector<uint32_t> pj, pw;
    uint64_t n_pairs = 0;
    const int rc = assoc_join(c, wch, wces, wcee, off, js, je, pj, pw, n_pairs, err, errlen);
    if (rc != RGX_OK) return rc;
    *out = pair_list(pj, pw, 1);
    return RGX_OK;
}
