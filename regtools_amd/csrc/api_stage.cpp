// api_stage.cpp -- stage entry points of the tail behind the DEFLATE launch: the exclusive scan, the radix sort and the group-by on the caller's
// own device arrays, so that tests can hand each of them inputs no BAM would (tests/test_gpu_stage_kernels.py).  Nothing here is a copy: the scan is
// launch_scan_u32, the sort is the RadixSort of api_internal.h driven the three ways the product drives it, the group-by is reduce_events.  Scratch
// is a buffer of the context carved the way reduce_events carves its "sort" buffer, with guard words behind the scan / radix scratch: a
// radix_tmp_words or scan_tmp_words that is too small for what a pass writes fails the call instead of going unseen in the buffer's growth slack.
#include "api_internal.h"

namespace {
constexpr uint32_t kGuardWords = 64, kGuardFill = 0xA5C3F00Du;

struct Guard {
    uint32_t *d = nullptr;
    void arm(uint32_t *at, hipStream_t st) { d = at; launch_fill_u32(d, kGuardFill, kGuardWords, st); }
    // behind the stream's work: hipSuccess and *touched says whether a word changed
    hipError_t check(hipStream_t st, bool *touched) const {
        uint32_t h[kGuardWords];
        hipError_t e = hipMemcpyAsync(h, d, sizeof h, hipMemcpyDeviceToHost, st);
        if (e == hipSuccess) e = hipStreamSynchronize(st);
        *touched = false;
        if (e == hipSuccess) for (uint32_t k = 0; k < kGuardWords; ++k) if (h[k] != kGuardFill) *touched = true;
        return e;
    }
};
}  // namespace

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
