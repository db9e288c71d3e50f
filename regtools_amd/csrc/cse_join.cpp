// cse_join.cpp -- which junctions belong to which variant: the window join of `identify` over one extraction, the same join window by
// window through the index for a damaged file, the pair join of `associate`, and the gather of a sharded extraction's events (8e).
#include "cse_internal.h"

// The pair workspace (Buf::cse_pairs, PairLayout of cse_internal.h): the two pair lists of the window join, then the pairs' events as an EventSoA of Pn
// rows.  A caller that brings the events itself leaves the lists' place empty.  The caller's CARVE_TRY(q, "cse_pairs") follows.
static PairLayout pair_layout(Carve &q, size_t Pn) {
    PairLayout L; memset(&L.pe, 0, sizeof L.pe);
    L.pair_ev = q.u32(Pn); L.pair_win = q.u32(Pn);
    L.pe.tid = q.u32(Pn); L.pe.start = q.u32(Pn); L.pe.ilen_cls = q.u32(Pn); L.pe.ts = q.u32(Pn); L.pe.te = q.u32(Pn); L.pe.strand = q.u8(Pn);
    return L;
}
// the group-by of one batch of nw windows' pairs (the window is the leading key), its rows behind R's
static int reduce_pair_batch(rgx_ctx *c, const EventSoA &pe, uint32_t total, uint32_t nw, uint32_t first_window, uint32_t ilen_bits, HostRows &R, char *err,
                             size_t errlen) {
    std::vector<uint32_t> ident(nw);
    for (uint32_t i = 0; i < nw; ++i) ident[i] = i;
    HostRows B;
    const int rc = reduce_events(c, pe, total, std::max<uint32_t>(1, bitlen(nw - 1)), ilen_bits, ident.data(), nw, B, err, errlen, false, nullptr, nullptr,
        /*allow_preagg=*/false);
    if (rc != RGX_OK) return rc;
    R.append(B, first_window);
    return RGX_OK;
}

// ---- a9: window join -------------------------------------------------------------------------------------------------------
int window_pair_batches(rgx_ctx *c, const EventSoA &ev, uint32_t n_events, const std::vector<int32_t> &w_tid, const std::vector<int32_t> &w_beg,
                        const std::vector<int32_t> &w_end, uint64_t pair_batch, bool guarded, const PairBatchFn &on_batch, uint64_t &n_pairs,
                        uint32_t &n_batches, char *err, size_t errlen) {
    n_pairs = 0; n_batches = 0;
    const uint32_t W = (uint32_t)w_tid.size();
    if (!W || !n_events) return RGX_OK;
    hipStream_t st = c->stream;
    DevBuf &b = c->buf(Buf::cse_windows), &sc = c->buf(Buf::scalars);
    const size_t Wn = W;
    const size_t Sn = Wn * kWinSlices;                               // count / base: one entry per (window, slice)
    HIP_TRY(b.ensure(Wn * 4 * 5 + Sn * 4 * 2 + scan_tmp_words((uint32_t)Sn) * 4 + 256));
    Carve w(b);
    int32_t *d_tid = w.take<int32_t>(Wn), *d_beg = w.take<int32_t>(Wn), *d_end = w.take<int32_t>(Wn);
    uint32_t *d_lo = w.u32(Wn), *d_hi = w.u32(Wn), *d_cnt = w.u32(Sn), *d_base = w.u32(Sn), *d_tmp = w.u32(scan_tmp_words((uint32_t)Sn));
    CARVE_TRY(w, "cse_windows");
    uint32_t *d_span = &sc.as<Scalars>()->max_span, *d_total = &sc.as<Scalars>()->window_pairs;
    HIP_TRY(upload(d_tid, w_tid, Wn, st));
    HIP_TRY(upload(d_beg, w_beg, Wn, st));
    HIP_TRY(upload(d_end, w_end, Wn, st));
    HIP_TRY(hipMemsetAsync(d_span, 0, 4, st));
    launch_max_span(ev, n_events, d_span, st);
    ktime_begin(c, 2);
    launch_window_pairs(false, ev, n_events, W, d_tid, d_beg, d_end, d_span, d_lo, d_hi, d_cnt, nullptr, nullptr, nullptr, st);
    ktime_end(c);
    // The (window, event) pairs are materialised in batches of whole windows: a VCF dense in splice-region variants of highly
    // expressed genes multiplies events by windows, and neither a 32-bit pair count nor HBM should be the limit of that.
    std::vector<uint32_t> h_cnt(Wn);
    {
        std::vector<uint32_t> h_slices(Sn);
        HIP_TRY(hipMemcpyAsync(h_slices.data(), d_cnt, Sn * 4, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        for (size_t k = 0; k < Wn; ++k) { uint64_t c = 0; for (uint32_t q = 0; q < kWinSlices; ++q) c += h_slices[k * kWinSlices + q];
            h_cnt[k] = c > 0xffffffffull ? 0xffffffffu : (uint32_t)c; }
    }
    static const uint64_t kPairBatch = getenv("REGTOOLS_AMD_PAIR_BATCH") ? strtoull(getenv("REGTOOLS_AMD_PAIR_BATCH"), nullptr, 10) : (1ull << 26);
    if (!pair_batch) pair_batch = kPairBatch;
    for (uint32_t w0 = 0; w0 < W;) {
        uint64_t total64 = h_cnt[w0];
        uint32_t w1 = w0 + 1;
        while (w1 < W && total64 + h_cnt[w1] <= pair_batch) total64 += h_cnt[w1++];
        if (total64 >= (1ull << 31)) return fail(err, errlen, RGX_ERR_ARG,
            "regtools_amd: one variant window holds %llu junction-supporting reads; more than the join handles\n", (unsigned long long)total64);
        const uint32_t nw = w1 - w0, total = (uint32_t)total64;
        n_pairs += total;
        ++n_batches;
        if (total) {
            launch_scan_u32(d_cnt + (size_t)w0 * kWinSlices, d_base + (size_t)w0 * kWinSlices, nw * kWinSlices, d_total, d_tmp, st);
            const size_t Pn = total;
            PairLayout L;
            StageGuard guard[2];
            if (guarded) {
                DevBuf &bp = c->buf(Buf::stage);
                HIP_TRY(bp.ensure((Pn + kGuardWords) * 4 * 2 + 256));
                Carve q(bp);
                memset(&L.pe, 0, sizeof L.pe);
                L.pair_ev = q.u32(Pn); uint32_t *g_ev = q.u32(kGuardWords); L.pair_win = q.u32(Pn); uint32_t *g_win = q.u32(kGuardWords); CARVE_TRY(q, "stage");
                guard[0].arm(g_ev, st); guard[1].arm(g_win, st);
            } else {
                DevBuf &bp = c->buf(Buf::cse_pairs);
                HIP_TRY(bp.ensure(Pn * 4 * 7 + Pn + 256));
                Carve q(bp);
                L = pair_layout(q, Pn); CARVE_TRY(q, "cse_pairs");
            }
            ktime_begin(c, 2);
            launch_window_pairs(true, ev, n_events, nw, d_tid + w0, d_beg + w0, d_end + w0, d_span, d_lo + w0, d_hi + w0,
                d_cnt + (size_t)w0 * kWinSlices, d_base + (size_t)w0 * kWinSlices, L.pair_ev, L.pair_win, st);
            ktime_end(c);
            if (guarded) for (const StageGuard &g : guard) {
                bool touched = false;
                HIP_TRY(g.check(st, &touched));
                if (touched) return fail(err, errlen, RGX_ERR_DEVICE, "regtools_amd: the window join's fill pass wrote behind the %u pairs its count pass counted\n", total);
            }
            const int rc = on_batch(w0, nw, total, L);
            if (rc != RGX_OK) return rc;
        }
        w0 = w1;
    }
    return RGX_OK;
}

// rows of every window in the order get_all_junctions would give for that window's extraction (thick_start, thick_end, name)
int window_join(rgx_ctx *c, const Prep &P, const std::vector<int32_t> &w_tid, const std::vector<int32_t> &w_beg, const std::vector<int32_t> &w_end,
                uint32_t ilen_bits, HostRows &R, uint64_t &n_pairs, char *err, size_t errlen) {
    R = HostRows();
    uint32_t n_batches = 0;
    return window_pair_batches(c, P.ev, P.n_events, w_tid, w_beg, w_end, 0, false, [&](uint32_t w0, uint32_t nw, uint32_t total, const PairLayout &L) {
        launch_pair_gather(P.ev, L.pair_ev, L.pair_win, total, L.pe, c->stream);
        return reduce_pair_batch(c, L.pe, total, nw, w0, ilen_bits, R, err, errlen);
    }, n_pairs, n_batches, err, errlen);
}

// `identify` on a file whose record stream ENDED somewhere (a member that does not inflate, an unreadable record): upstream reads every variant's window
// through
// the index on its own (identifier.cc:288-290) -- also the windows BEHIND the damage, which one pass over the file never reaches.  Here, for such a file only:
// one
// region extraction per window from the file's bytes in HBM (what `junctions extract -r` makes of a damaged file: the iterator's chunks are seeks of their
// own), the
// windows' events put together as window_join's pairs are, the same group-by behind them.  *w_abort (SIZE_MAX = none): the first window that reads a read
// bam_aux_get
// abort()s on (Prep::odd_aux); the windows behind it are not read.
int window_join_by_seeks(rgx_ctx *c, const uint8_t *d_file, size_t bam_len, const uint8_t *bai, size_t bai_len, const rgx_extract_params &ep0,
                         const std::vector<std::string> &w_region, uint32_t ilen_bits, HostRows &R, uint64_t &n_pairs, size_t &w_abort, char *err,
                         size_t errlen) {
    R = HostRows(); n_pairs = 0; w_abort = SIZE_MAX;
    const size_t W = w_region.size();
    hipStream_t st = c->stream;
    std::vector<uint32_t> h_col[6];                               // window (batch-local), start, ilen_cls, ts, te; [5] unused
    std::vector<uint8_t> h_strand;
    size_t w0 = 0;
    auto flush = [&](size_t w1) -> int {
        const size_t total = h_col[0].size(), nw = w1 - w0;
        if (total && nw) {
            if (total >= (1ull << 31)) return fail(err, errlen, RGX_ERR_ARG,
                "regtools_amd: %zu junction-supporting reads in one batch of windows; more than the join handles\n", total);
            DevBuf &bp = c->buf(Buf::cse_pairs);
            HIP_TRY(bp.ensure(total * 4 * 7 + total + 256));
            Carve q(bp);
            const EventSoA pe = pair_layout(q, total).pe; CARVE_TRY(q, "cse_pairs");          // (the pair lists' place stays empty)
            uint32_t *dst[5] = {pe.tid, pe.start, pe.ilen_cls, pe.ts, pe.te};
            for (int k = 0; k < 5; ++k) HIP_TRY(upload(dst[k], h_col[k], total, st));
            HIP_TRY(upload(pe.strand, h_strand, total, st));
            HIP_TRY(hipStreamSynchronize(st));
            const int rc = reduce_pair_batch(c, pe, (uint32_t)total, (uint32_t)nw, (uint32_t)w0, ilen_bits, R, err, errlen);
            if (rc != RGX_OK) return rc;
            n_pairs += total;
        }
        for (auto &v : h_col) v.clear();
        h_strand.clear();
        w0 = w1;
        return RGX_OK;
    };
    for (size_t w = 0; w < W; ++w) {
        rgx_extract_params q = ep0;
        q.region = w_region[w].c_str(); q.shard = 0; q.n_shards = 1;
        Prep Pw;
        EventsArgs a;
        a.c = c; a.p = &q; a.want_read_span = true;
        a.d_bam_in = d_file; a.bam_len = bam_len;
        a.index = bai; a.index_len = bai_len;
        const int rc = prepare_events(a, Pw, err, errlen);
        if (rc != RGX_OK) return rc;
        if (!Pw.odd_aux.empty()) { w_abort = w; break; }
        const size_t n = Pw.n_events;
        if (n) {
            const size_t at = h_col[0].size();
            for (int k = 0; k < 5; ++k) h_col[k].resize(at + n);
            h_strand.resize(at + n);
            const uint32_t *src[5] = {nullptr, Pw.ev.start, Pw.ev.ilen_cls, Pw.ev.ts, Pw.ev.te};
            for (int k = 1; k < 5; ++k) HIP_TRY(hipMemcpyAsync(h_col[k].data() + at, src[k], n * 4, hipMemcpyDeviceToHost, st));
            HIP_TRY(hipMemcpyAsync(h_strand.data() + at, Pw.ev.strand, n, hipMemcpyDeviceToHost, st));
            HIP_TRY(hipStreamSynchronize(st));
            std::fill(h_col[0].begin() + (ptrdiff_t)at, h_col[0].end(), (uint32_t)(w - w0));
        }
        if (h_col[0].size() >= (1u << 22)) { const int rc2 = flush(w + 1); if (rc2 != RGX_OK) return rc2; }
    }
    return flush(w_abort == SIZE_MAX ? W : w_abort);
}

extern "C" int rgx_window_join(rgx_ctx *c, const char *bam_path, const rgx_extract_params *p, uint64_t n_windows, const char *const *chrom, const int32_t *beg,
                               const int32_t *end, rgx_window_rows **out, char *err, size_t errlen) {
    if (!c || !bam_path || !p || !out || (n_windows && (!chrom || !beg || !end))) return fail(err, errlen, RGX_ERR_ARG, "regtools_amd: bad arguments\n");
    *out = nullptr;
    FileBytes bam; std::vector<uint8_t> bai;
    if (!bam.open(bam_path)) return fail(err, errlen, RGX_ERR_OPEN, "%s", kMsgOpen);
    std::string idx;
    if (find_index(bam_path, idx) != 0 || !read_index(idx, bai)) return fail(err, errlen, RGX_ERR_INDEX, "%s", kMsgIndex);
    rgx_extract_params ep = *p;
    ep.region = "."; ep.shard = 0; ep.n_shards = 1;
    Prep P;
    EventsArgs a;
    a.c = c; a.p = &ep; a.want_read_span = true;
    a.h_bam = bam.data(); a.bam_len = bam.size();
    a.index = bai.data(); a.index_len = bai.size();
    int rc = prepare_events(a, P, err, errlen);
    if (rc != RGX_OK) return rc;
    std::vector<int32_t> w_tid((size_t)n_windows), w_beg(beg, beg + n_windows), w_end(end, end + n_windows);
    for (uint64_t w = 0; w < n_windows; ++w) {
        int32_t tid = -1;
        for (size_t t = 0; t < P.hdr.names.size(); ++t) if (P.hdr.names[t] == chrom[w]) { tid = (int32_t)t; break; }
        if (tid < 0 || w_end[(size_t)w] < w_beg[(size_t)w]) return fail(err, errlen, RGX_ERR_REGION, "%s", kMsgRegion);
        w_tid[(size_t)w] = tid;
    }
    HostRows R; uint64_t n_pairs = 0;
    rc = window_join(c, P, w_tid, w_beg, w_end, std::min<uint32_t>(32, bitlen(ep.max_intron) + 2), R, n_pairs, err, errlen);
    if (rc != RGX_OK) return rc;
    rgx_window_rows *r = (rgx_window_rows *)calloc(1, sizeof *r);
    const size_t n = R.n;
    r->n = n;
    r->window = dup_u32(R.group); r->start = dup_u32(R.start); r->end = dup_u32(R.end); r->thick_start = dup_u32(R.ts); r->thick_end = dup_u32(R.te);
    r->read_count = dup_u32(R.count);
    r->name_index = (uint32_t *)malloc((n + 1) * 4); r->strand = (char *)malloc(n + 1);
    for (size_t i = 0; i < n; ++i) r->strand[i] = (char)R.strand[i];
    // names restart in every window: rank of the row's (global, window-major) first-seen rank among the rows of its window
    for (size_t lo = 0; lo < n;) {
        size_t hi = lo; while (hi < n && R.group[hi] == R.group[lo]) ++hi;
        std::vector<std::pair<uint32_t, size_t>> order;
        for (size_t i = lo; i < hi; ++i) order.push_back({R.name_rank[i], i});
        std::sort(order.begin(), order.end());
        for (size_t k = 0; k < order.size(); ++k) r->name_index[order[k].second] = (uint32_t)k + 1;
        lo = hi;
    }
    *out = r;
    return RGX_OK;
}
extern "C" void rgx_window_rows_free(rgx_window_rows *r) {
    if (!r) return;
    free(r->window); free(r->start); free(r->end); free(r->thick_start); free(r->thick_end); free(r->read_count); free(r->name_index); free(r->strand); free(r);
}

// ---- associate: the pair join ------------------------------------------------------------------------------------------------
// every (window, junction) pair of `associate` (associator.cc:258-265): the windows in file order (contig index into chrom_off, or -1; cis range), the
// BED's junctions bucketed by contig (chrom_off; js, je in bucket order).  pj / pw: the pairs' junction (bucket order) and window
int assoc_join(rgx_ctx *c, const std::vector<int32_t> &wch, const std::vector<uint32_t> &wces, const std::vector<uint32_t> &wcee,
               const std::vector<uint32_t> &chrom_off, const std::vector<uint32_t> &js, const std::vector<uint32_t> &je, std::vector<uint32_t> &pj,
               std::vector<uint32_t> &pw, uint64_t &n_pairs, char *err, size_t errlen) {
    pj.clear(); pw.clear(); n_pairs = 0;
    const uint32_t W = (uint32_t)wch.size(), J = (uint32_t)js.size();
    if (!W || !J) return RGX_OK;
    hipStream_t st = c->stream;
    HIP_ENTER(c->device);
    DevBuf &b = c->buf(Buf::cse_assoc), &sc = c->buf(Buf::scalars);
    HIP_TRY(sc.ensure(sizeof(Scalars)));
    const size_t Wn = W, Jn = J, Cn = chrom_off.size();
    HIP_TRY(b.ensure((Wn * 5 + Jn * 2 + Cn + scan_tmp_words(W)) * 4 + 512));
    Carve w(b);
    int32_t *d_wch = w.take<int32_t>(Wn); uint32_t *d_ces = w.u32(Wn), *d_cee = w.u32(Wn), *d_cnt = w.u32(Wn), *d_base = w.u32(Wn);
    uint32_t *d_js = w.u32(Jn), *d_je = w.u32(Jn), *d_off = w.u32(Cn), *d_tmp = w.u32(scan_tmp_words(W)); CARVE_TRY(w, "cse_assoc");
    uint32_t *d_total = &sc.as<Scalars>()->assoc_pairs;
    HIP_TRY(upload(d_wch, wch, Wn, st)); HIP_TRY(upload(d_ces, wces, Wn, st)); HIP_TRY(upload(d_cee, wcee, Wn, st));
    HIP_TRY(upload(d_js, js, Jn, st)); HIP_TRY(upload(d_je, je, Jn, st)); HIP_TRY(upload(d_off, chrom_off, Cn, st));
    launch_assoc_pairs(false, W, d_wch, d_ces, d_cee, d_off, d_js, d_je, d_cnt, nullptr, nullptr, nullptr, st);
    launch_scan_u32(d_cnt, d_base, W, d_total, d_tmp, st);
    uint32_t total = 0;
    std::vector<uint32_t> h_cnt(Wn);
    HIP_TRY(hipMemcpyAsync(h_cnt.data(), d_cnt, Wn * 4, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(&total, d_total, 4, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    { uint64_t t64 = 0; for (uint32_t x : h_cnt) t64 += x;                   // the device scan is 32 bits wide
      if (t64 >= (1ull << 31)) return fail(err, errlen, RGX_ERR_ARG, "regtools_amd: %llu (variant, junction) pairs; more than the join handles\n",
          (unsigned long long)t64); }
    if (total) {
        DevBuf &bp = c->buf(Buf::cse_pairs);
        HIP_TRY(bp.ensure((size_t)total * 8 + 256));
        Carve wp(bp);
        uint32_t *d_pj = wp.u32(total), *d_pw = wp.u32(total); CARVE_TRY(wp, "cse_pairs");
        launch_assoc_pairs(true, W, d_wch, d_ces, d_cee, d_off, d_js, d_je, d_cnt, d_base, d_pj, d_pw, st);
        pj.resize(total); pw.resize(total);
        HIP_TRY(hipMemcpyAsync(pj.data(), d_pj, (size_t)total * 4, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipMemcpyAsync(pw.data(), d_pw, (size_t)total * 4, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
    }
    n_pairs = total;
    return RGX_OK;
}

// SURVEY 8e for `identify`: the extraction is what is worth sharding (29 of config 4's 36 ms of device work) -- shard g of the BAM is inflated, framed
// and scanned on device g exactly as rgx_extract_multi's shards are (contiguous member ranges cut at record starts from the index, one host scan of
// the members for all), and the junction EVENTS (32 B each; config 4: 7.5 M = 230 MB) are gathered onto the first device in shard order = file order,
// where the windows are joined as on one device.  The gather is device-to-device copies (hipMemcpyPeerAsync: xGMI between two GPUs, a plain copy when
// a device is listed twice) -- no reduction is involved, so no collective.  A shard whose record stream ended for a reason that ends iteration upstream
// ends the event list (the shards behind it are dropped, as the table merge drops them).
int prepare_events_sharded(const std::vector<rgx_ctx *> &cs, const uint8_t *bam, size_t bam_len, const uint8_t *bai, size_t bai_len,
                           const rgx_extract_params *ep, Prep &P, char *err, size_t errlen) {
    const int n = (int)cs.size();
    EventsArgs a;
    a.c = cs[0]; a.p = ep; a.want_read_span = true;
    a.h_bam = bam; a.bam_len = bam_len;
    a.index = bai; a.index_len = bai_len;
    std::vector<Member> members; uint64_t total_inflated = 0;
    if (bam_len < ((size_t)8 << 20) || !scan_members_parallel(bam, bam_len, (int)usable_threads(24), members, total_inflated))
        // a file the host scan does not vouch for: one device, its own member discovery
        return prepare_events(a, P, err, errlen);
    SharedMembers sm{&members, total_inflated};
    std::vector<Prep> parts((size_t)n);
    std::vector<int> rcs((size_t)n, RGX_OK);
    std::vector<std::string> errs((size_t)n, std::string(512, '\0'));
    auto run = [&](int g) {
        rgx_extract_params q = *ep;
        q.shard = g; q.n_shards = n;
        EventsArgs ag = a; ag.c = cs[(size_t)g]; ag.p = &q; ag.shared = &sm;
        rcs[(size_t)g] = prepare_events(ag, parts[(size_t)g], &errs[(size_t)g][0], 512);
    };
    bool distinct = true;
    for (int a = 0; a < n; ++a) for (int b = a + 1; b < n; ++b) if (cs[(size_t)a]->device == cs[(size_t)b]->device) distinct = false;
    if (distinct) {
        std::vector<std::thread> pool;
        for (int g = 1; g < n; ++g) pool.emplace_back(run, g);
        run(0);
        for (auto &t : pool) t.join();
    } else for (int g = 0; g < n; ++g) run(g);                   // (shards that share a device take turns on it)
    for (int g = 0; g < n; ++g) if (rcs[(size_t)g] != RGX_OK) return fail(err, errlen, rcs[(size_t)g], "%s", errs[(size_t)g].c_str());
    int used = n;
    uint64_t N = 0, iterated = 0, rec = 0;
    for (int g = 0; g < n; ++g) {
        N += parts[(size_t)g].n_events; iterated += parts[(size_t)g].n_iterated; rec += parts[(size_t)g].n_rec;
        if (parts[(size_t)g].stream_ended) { used = g + 1; break; }
    }
    if (N >= 0xfffffff0ull) return fail(err, errlen, RGX_ERR_ARG, "regtools_amd: %llu junction events; more than the join handles\n", (unsigned long long)N);
    rgx_ctx *c0 = cs[0];
    HIP_TRY(hipSetDevice(c0->device));
    DevBuf &ball = c0->buf(Buf::cse_events_all);
    const size_t Nn = (size_t)N, stride = (Nn * 4 + 255) & ~(size_t)255;
    HIP_TRY(ball.ensure(stride * 8 + 256));
    Carve q(ball);
    auto column = [&] { return (uint32_t *)q.u8(stride); };          // (columns start 256 bytes apart at the least, whatever N is)
    EventSoA all; memset(&all, 0, sizeof all);
    all.tid = column(); all.start = column(); all.ilen_cls = column(); all.ts = column();
    all.te = column(); all.rpos = column(); all.rend = column(); all.strand = q.u8(stride); CARVE_TRY(q, "cse_events_all");
    size_t off = 0;
    for (int g = 0; g < used; ++g) {
        const Prep &pg = parts[(size_t)g];
        const size_t k = pg.n_events;
        if (!k) continue;
        const int dg = cs[(size_t)g]->device;
        HIP_TRY(hipSetDevice(dg));
        HIP_TRY(hipStreamSynchronize(cs[(size_t)g]->stream));      // (the shard's events are complete)
        (void)rgx_enable_peer(c0->device, dg);                       // (xGMI instead of a bounce through the host; a copy works either way)
        HIP_TRY(hipSetDevice(c0->device));
#define RGX_GATHER(F, BYTES) HIP_TRY(hipMemcpyPeerAsync((uint8_t *)all.F + off * (BYTES), c0->device, pg.ev.F, dg, k * (BYTES), c0->stream))
        RGX_GATHER(tid, 4); RGX_GATHER(start, 4); RGX_GATHER(ilen_cls, 4); RGX_GATHER(ts, 4); RGX_GATHER(te, 4); RGX_GATHER(rpos, 4); RGX_GATHER(rend, 4);
            RGX_GATHER(strand, 1);
#undef RGX_GATHER
        off += k;
    }
    HIP_TRY(hipStreamSynchronize(c0->stream));
    P = Prep();
    P.hdr = parts[0].hdr; P.ev = all; P.n_events = (uint32_t)N; P.n_iterated = iterated; P.n_rec = (uint32_t)std::min<uint64_t>(rec, 0xffffffffull);
    P.stream_ended = used < n || parts[(size_t)used - 1].stream_ended;
    for (int g = 0; g < used; ++g) P.odd_aux.insert(P.odd_aux.end(), parts[(size_t)g].odd_aux.begin(), parts[(size_t)g].odd_aux.end());
    return RGX_OK;
}
