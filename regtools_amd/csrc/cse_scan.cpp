// cse_scan.cpp -- the annotation on the device and what is scanned against it: every variant, every junction (row a11), and the
// library entry points of the two scans.
#include "cse_internal.h"

thread_local WorkerPool *tl_pool = nullptr;

// pooled = the tables go into a buffer of the CONTEXT (valid until its next call that loads an annotation: identify / associate / the annotate commands,
// which use the annotation inside the call) through one page-locked staging block and ONE copy -- eight synchronous copies out of pageable vectors into a
// fresh hipMalloc were 8 ms of config 4's `identify`, on its critical path behind the GTF thread.  rgx_gtf_load's annotation outlives the call: its own block.
int gtf_upload(rgx_ctx *c, rgx_gtf *g, char *err, size_t errlen, bool pooled) {
    const GtfModel &m = g->m;
    const size_t T = m.tx_id.size(), E = m.es.size(), B = m.bin_key.size(), S = m.bin_start.size();
    auto al = [](size_t x) { return (x + 255) & ~(size_t)255; };
    const size_t o_strand = 0, o_off = al(T), o_n = o_off + al(T * 4), o_es = o_n + al(T * 4), o_ee = o_es + al(E * 4), o_bk = o_ee + al(E * 4),
                 o_bt = o_bk + al(B * 8), o_bs = o_bt + al(B * 4), total = o_bs + al(S * 4) + 256;
    HIP_ENTER(c->device);
    uint8_t *d = nullptr;
    struct Piece { size_t off; const void *src; size_t bytes; };
    const Piece pieces[8] = {{o_strand, m.tx_strand.data(), T}, {o_off, m.tx_exon_off.data(), T * 4}, {o_n, m.tx_n_exons.data(), T * 4}, {o_es, m.es.data(),
        E * 4},
                             {o_ee, m.ee.data(), E * 4}, {o_bk, m.bin_key.data(), B * 8}, {o_bt, m.bin_tx.data(), B * 4}, {o_bs, m.bin_start.data(), S * 4}};
    if (pooled) {
        DevBuf &b = c->buf(Buf::gtf_tables);
        HIP_TRY(b.ensure(total));
        d = b.as<uint8_t>();
        g->dev = nullptr;                                          // (the context's: rgx_gtf_free leaves it alone)
        if (total > c->pinned_rows_cap) {
            if (c->pinned_rows) (void)hipHostFree(c->pinned_rows);
            c->pinned_rows = nullptr; c->pinned_rows_cap = 0;
            HIP_TRY(hipHostMalloc(&c->pinned_rows, total + total / 4, hipHostMallocDefault));
            c->pinned_rows_cap = total + total / 4;
        }
        uint8_t *stage = (uint8_t *)c->pinned_rows;
        // the pieces into the staging block, the large ones in slices on the stage's threads
        struct Slice { uint8_t *dst; const uint8_t *src; size_t n; };
        std::vector<Slice> sl;
        for (const Piece &q : pieces) for (size_t o = 0; o < q.bytes; o += (size_t)1 << 20) sl.push_back({stage + q.off + o, (const uint8_t *)q.src + o,
            std::min<size_t>((size_t)1 << 20, q.bytes - o)});
        if (tl_pool && sl.size() > 1) tl_pool->run(sl.size(), [&](size_t k) { memcpy(sl[k].dst, sl[k].src, sl[k].n); });
        else for (const Slice &x : sl) memcpy(x.dst, x.src, x.n);
        HIP_TRY(hipMemcpyAsync(d, stage, total - 256, hipMemcpyHostToDevice, c->stream));
        HIP_TRY(hipStreamSynchronize(c->stream));
    } else {
        HIP_TRY(hipMalloc(&g->dev, total));
        d = (uint8_t *)g->dev;
        for (const Piece &q : pieces) if (q.bytes) HIP_TRY(hipMemcpy(d + q.off, q.src, q.bytes, hipMemcpyHostToDevice));
    }
    g->view.tx_strand = d + o_strand; g->view.tx_exon_off = (const uint32_t *)(d + o_off); g->view.tx_n_exons = (const uint32_t *)(d + o_n);
    g->view.es = (const uint32_t *)(d + o_es); g->view.ee = (const uint32_t *)(d + o_ee);
    g->view.bin_key = (const uint64_t *)(d + o_bk); g->view.bin_tx = (const uint32_t *)(d + o_bt); g->view.n_bin = (uint32_t)B;
    if (S) { g->view.bin_start = (const uint32_t *)(d + o_bs); g->view.bin_stride = m.bin_stride; }
    else { g->view.bin_start = nullptr; g->view.bin_stride = 0; }
    g->view.keep_single = 0;
    return RGX_OK;
}

extern "C" int rgx_gtf_load(rgx_ctx *ctx, const char *gtf_path, rgx_gtf **out, char *err, size_t errlen) {
    *out = nullptr;
    if (!ctx || !gtf_path) return fail(err, errlen, RGX_ERR_ARG, "regtools_amd: bad arguments\n");
    rgx_gtf *g = new rgx_gtf();
    g->ctx = ctx;
    std::string e = g->m.load(gtf_path);
    if (!e.empty()) { delete g; return fail(err, errlen, RGX_ERR_FORMAT, "%s", e.c_str()); }
    g->m.release_load_scratch();                              // (this annotation lives as long as its caller keeps it)
    int rc = gtf_upload(ctx, g, err, errlen);
    if (rc != RGX_OK) { rgx_gtf_free(g); return rc; }
    *out = g;
    return RGX_OK;
}
extern "C" void rgx_gtf_free(rgx_gtf *g) { if (!g) return; if (g->dev) (void)hipFree(g->dev); delete g; }
extern "C" int rgx_gtf_info(const rgx_gtf *g, uint32_t *n_tx, uint32_t *n_exons, uint32_t *n_chroms) {
    if (n_tx) *n_tx = (uint32_t)g->m.tx_id.size();
    if (n_exons) *n_exons = (uint32_t)g->m.es.size();
    if (n_chroms) *n_chroms = (uint32_t)g->m.chroms.size();
    return RGX_OK;
}
extern "C" int rgx_gtf_transcript_bin(const rgx_gtf *g, const char *transcript_id, uint32_t *bin) {
    auto it = std::lower_bound(g->m.tx_id.begin(), g->m.tx_id.end(), std::string(transcript_id));
    if (it == g->m.tx_id.end() || *it != transcript_id) return RGX_ERR_ARG;
    *bin = g->m.tx_bin[(size_t)(it - g->m.tx_id.begin())];
    return RGX_OK;
}
extern "C" const char *rgx_gtf_transcript_id(const rgx_gtf *g, uint32_t t) { return t < g->m.tx_id.size() ? g->m.tx_id[t].c_str() : ""; }

void run_tasks(size_t T, const std::function<void(size_t)> &f) {
    if (T <= 1) { for (size_t t = 0; t < T; ++t) f(t); return; }
    if (tl_pool) { tl_pool->run(T, f); return; }
    std::vector<std::thread> th;
    for (size_t t = 1; t < T; ++t) th.emplace_back(f, t);
    f(0);
    for (auto &x : th) x.join();
}

// ---- a10 ----------------------------------------------------------------------------------------------------------------
static int variant_windows(rgx_ctx *c, const rgx_gtf *g, const std::vector<int32_t> &chrom, const std::vector<uint32_t> &pos0, const VariantOpts &o,
                           VariantHitsHost &H, char *err, size_t errlen, uint64_t *exon_visits = nullptr) {
    const uint32_t n = (uint32_t)chrom.size();
    H = VariantHitsHost();
    H.off.assign((size_t)n + 1, 0);
    if (!n) return RGX_OK;
    hipStream_t st = c->stream;
    HIP_ENTER(c->device);
    DevBuf &b = c->buf(Buf::cse_variants), &sc = c->buf(Buf::scalars);
    HIP_TRY(sc.ensure(sizeof(Scalars)));
    const size_t N = n;
    HIP_TRY(b.ensure(N * 4 * 7 + scan_tmp_words(n) * 4 + 256));
    Carve w(b);
    int32_t *d_chrom = w.take<int32_t>(N); uint32_t *d_pos = w.u32(N), *d_cnt = w.u32(N), *d_base = w.u32(N);
    uint32_t *d_ces = w.u32(N), *d_cee = w.u32(N), *d_last = w.u32(N), *d_tmp = w.u32(scan_tmp_words(n)); CARVE_TRY(w, "cse_variants");
    uint32_t *d_total = &sc.as<Scalars>()->variant_hits;
    HIP_TRY(upload(d_chrom, chrom, N, st));
    HIP_TRY(upload(d_pos, pos0, N, st));
    unsigned long long *d_visits = &sc.as<Scalars>()->variant_visits, h_visits = 0;
    HIP_TRY(hipMemsetAsync(d_visits, 0, 8, st));
    ktime_begin(c, 0);
    launch_variant_scan(false, g->view, n, d_chrom, d_pos, o, d_cnt, nullptr, d_ces, d_cee, nullptr, nullptr, d_visits, st, d_last);
    ktime_end(c);
    launch_scan_u32(d_cnt, d_base, n, d_total, d_tmp, st);
    uint32_t total = 0;
    HIP_TRY(hipMemcpyAsync(&total, d_total, 4, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(&h_visits, d_visits, 8, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    if (exon_visits) *exon_visits = h_visits;
    H.ces.resize(N); H.cee.resize(N); H.last.resize(N);
    HIP_TRY(hipMemcpy(H.last.data(), d_last, N * 4, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(H.ces.data(), d_ces, N * 4, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(H.cee.data(), d_cee, N * 4, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(H.off.data(), d_base, N * 4, hipMemcpyDeviceToHost));
    H.off[N] = total;
    if (total) {
        DevBuf &bh = c->buf(Buf::cse_variant_hits);
        HIP_TRY(bh.ensure((size_t)total * 12 + 256));
        Carve wh(bh);
        uint32_t *d_tx = wh.u32(total), *d_ad = wh.u32(2 * (size_t)total); CARVE_TRY(wh, "cse_variant_hits");
        ktime_begin(c, 0);
        launch_variant_scan(true, g->view, n, d_chrom, d_pos, o, d_cnt, d_base, d_ces, d_cee, d_tx, d_ad, nullptr, st);
        ktime_end(c);
        std::vector<uint32_t> ad((size_t)total * 2);
        H.tx.resize(total);
        HIP_TRY(hipMemcpyAsync(H.tx.data(), d_tx, (size_t)total * 4, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipMemcpyAsync(ad.data(), d_ad, (size_t)total * 8, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        H.ann.resize(total); H.dist.resize(total);
        for (size_t k = 0; k < total; ++k) { H.ann[k] = ad[2 * k]; H.dist[k] = ad[2 * k + 1]; }
    }
    return RGX_OK;
}

extern "C" int rgx_variant_windows(rgx_ctx *ctx, const rgx_gtf *g, uint64_t n, const char *const *chrom, const uint32_t *pos0, uint32_t intronic_min,
                                   uint32_t exonic_min, int all_intronic, int all_exonic, int skip_single, rgx_variant_hits **out, char *err, size_t errlen) {
    *out = nullptr;
    std::vector<int32_t> ci((size_t)n); std::vector<uint32_t> ps(pos0, pos0 + n);
    for (uint64_t i = 0; i < n; ++i) ci[(size_t)i] = g->m.chrom_of(chrom[i]);
    VariantOpts o{intronic_min, exonic_min, all_intronic, all_exonic, skip_single};
    VariantHitsHost H;
    int rc = variant_windows(ctx, g, ci, ps, o, H, err, errlen);
    if (rc != RGX_OK) return rc;
    rgx_variant_hits *r = (rgx_variant_hits *)calloc(1, sizeof *r);
    r->n = n; r->cis_start = dup_u32(H.ces); r->cis_end = dup_u32(H.cee); r->hit_off = dup_u32(H.off);
    r->hit_transcript = dup_u32(H.tx); r->hit_annotation = dup_u32(H.ann); r->hit_distance = dup_u32(H.dist);
    *out = r;
    return RGX_OK;
}
extern "C" void rgx_variant_hits_free(rgx_variant_hits *h) {
    if (!h) return;
    free(h->cis_start); free(h->cis_end); free(h->hit_off); free(h->hit_transcript); free(h->hit_annotation); free(h->hit_distance); free(h);
}

// ---- a11 ----------------------------------------------------------------------------------------------------------------
// The two launches of a11 and the scan between them: per junction the flags, the exon records of its candidates (wave form; the lane form adds into
// one counter: R.visits_total) and its items (kind, a, b) as the kernel wrote them, item_off[i] .. item_off[i + 1].  annotate_junctions makes the
// items unique behind this; the stage entry point rgx_k_junction_scan hands them out as they are.  guarded: the three item columns lie in Buf::stage
// with guard words behind each -- a fill pass that writes more than the count pass counted fails the call.
int junction_scan_items(rgx_ctx *c, const GtfView &view, const std::vector<int32_t> &chrom, const std::vector<uint32_t> &js, const std::vector<uint32_t> &je,
                        const std::vector<uint8_t> &strand, int form, bool guarded, JunctionItemsHost &R, char *err, size_t errlen) {
    const uint32_t n = (uint32_t)chrom.size();
    R = JunctionItemsHost();
    R.off.assign((size_t)n + 1, 0);
    if (!n) return RGX_OK;
    hipStream_t st = c->stream;
    HIP_ENTER(c->device);
    DevBuf &b = c->buf(Buf::cse_junctions), &sc = c->buf(Buf::scalars);
    HIP_TRY(sc.ensure(sizeof(Scalars)));
    const size_t N = n;
    HIP_TRY(b.ensure(N * 4 * 7 + N + scan_tmp_words(n) * 4 + 512));
    Carve w(b);
    int32_t *d_chrom = w.take<int32_t>(N); uint32_t *d_js = w.u32(N), *d_je = w.u32(N), *d_cnt = w.u32(N), *d_base = w.u32(N);
    uint32_t *d_flags = w.u32(N), *d_visit_each = w.u32(N), *d_tmp = w.u32(scan_tmp_words(n) + 8); uint8_t *d_strand = w.u8(N);
    CARVE_TRY(w, "cse_junctions");
    uint32_t *d_total = &sc.as<Scalars>()->junction_items;
    HIP_TRY(upload(d_chrom, chrom, N, st));
    HIP_TRY(upload(d_js, js, N, st));
    HIP_TRY(upload(d_je, je, N, st));
    HIP_TRY(upload(d_strand, strand, N, st));
    unsigned long long *d_visits = &sc.as<Scalars>()->junction_visits, h_visits = 0;
    HIP_TRY(hipMemsetAsync(d_visits, 0, 8, st));
    ktime_begin(c, 1);
    launch_junction_scan(false, view, n, d_chrom, d_js, d_je, d_strand, d_cnt, nullptr, d_flags, nullptr, nullptr, nullptr, d_visits, d_visit_each, st, form);
    ktime_end(c);
    launch_scan_u32(d_cnt, d_base, n, d_total, d_tmp, st);
    uint32_t total = 0;
    HIP_TRY(hipMemcpyAsync(&total, d_total, 4, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(&h_visits, d_visits, 8, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    R.flags.resize(N); R.visits.resize(N); R.kind.resize(total); R.a.resize(total); R.b.resize(total);
    HIP_TRY(hipMemcpy(R.flags.data(), d_flags, N * 4, hipMemcpyDeviceToHost));
    // SURVEY 8d's E_j: the lane form adds into one counter, the wave form writes one count per junction
    HIP_TRY(hipMemcpy(R.visits.data(), d_visit_each, N * 4, hipMemcpyDeviceToHost));
    for (size_t i = 0; i < N; ++i) h_visits += R.visits[i];
    R.visits_total = h_visits;
    HIP_TRY(hipMemcpy(R.off.data(), d_base, N * 4, hipMemcpyDeviceToHost));
    R.off[N] = total;
    if (total) {
        DevBuf &bi = c->buf(guarded ? Buf::stage : Buf::cse_junction_items);
        const size_t G = guarded ? kGuardWords : 0;
        HIP_TRY(bi.ensure(((size_t)total + G) * 12 + 256));
        Carve wi(bi);
        uint32_t *d_k = wi.u32(total), *g_k = wi.u32(G), *d_a = wi.u32(total), *g_a = wi.u32(G), *d_b = wi.u32(total), *g_b = wi.u32(G);
        CARVE_TRY(wi, guarded ? "stage" : "cse_junction_items");
        StageGuard guard[3];
        if (guarded) { guard[0].arm(g_k, st); guard[1].arm(g_a, st); guard[2].arm(g_b, st); }
        ktime_begin(c, 1);
        launch_junction_scan(true, view, n, d_chrom, d_js, d_je, d_strand, d_cnt, d_base, d_flags, d_k, d_a, d_b, nullptr, nullptr, st, form);
        ktime_end(c);
        HIP_TRY(hipMemcpyAsync(R.kind.data(), d_k, (size_t)total * 4, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipMemcpyAsync(R.a.data(), d_a, (size_t)total * 4, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipMemcpyAsync(R.b.data(), d_b, (size_t)total * 4, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        if (guarded) for (const StageGuard &g : guard) {
            bool touched = false;
            HIP_TRY(g.check(st, &touched));
            if (touched) return fail(err, errlen, RGX_ERR_DEVICE, "regtools_amd: the junction scan's fill pass wrote behind the %u items its count pass counted\n", total);
        }
    }
    return RGX_OK;
}

int annotate_junctions(rgx_ctx *c, const rgx_gtf *g, const std::vector<int32_t> &chrom, const std::vector<uint32_t> &js, const std::vector<uint32_t> &je,
                       const std::vector<uint8_t> &strand, JunctionAnnotHost &A, char *err, size_t errlen, uint64_t *exon_visits, bool keep_single) {
    const uint32_t n = (uint32_t)chrom.size();
    GtfView view = g->view; view.keep_single = keep_single ? 1u : 0u;          // (`junctions annotate -S` only)
    A = JunctionAnnotHost();
    A.tx_off.assign((size_t)n + 1, 0);
    if (!n) return RGX_OK;
    const size_t N = n;
    JunctionItemsHost R;
    const int rc = junction_scan_items(c, view, chrom, js, je, strand, /*form=*/-1, /*guarded=*/false, R, err, errlen);
    if (rc != RGX_OK) return rc;
    if (exon_visits) *exon_visits = R.visits_total;
    A.flags.swap(R.flags);
    const std::vector<uint32_t> &off = R.off, &kind = R.kind, &ia = R.a, &ib = R.b;
    // the reference keeps sets (junctions_annotator.h:41-45): unique skipped elements by coordinate, transcripts by id -- here small
    // vectors, sorted and made unique, ranges of junctions on the host's threads (std::set per junction: 20 of config 4's 280 ms)
    A.n_acc.resize(N); A.n_exo.resize(N); A.n_don.resize(N);
    const size_t T = N < 4096 ? 1 : usable_threads(16);
    std::vector<std::vector<uint32_t>> tx_part(T);
    std::vector<uint32_t> tx_cnt(N);
    auto work = [&](size_t t) {
        std::vector<uint32_t> acc, don, txs; std::vector<uint64_t> exo;
        auto uniq = [](auto &v) { std::sort(v.begin(), v.end()); v.erase(std::unique(v.begin(), v.end()), v.end()); return (uint32_t)v.size(); };
        for (size_t i = N * t / T; i < N * (t + 1) / T; ++i) {
            acc.clear(); don.clear(); txs.clear(); exo.clear();
            for (uint32_t k = off[i]; k < off[i + 1]; ++k) {
                if (kind[k] == ITEM_TX) txs.push_back(ia[k]);
                else if (kind[k] == ITEM_EXON) exo.push_back((uint64_t)ia[k] << 32 | ib[k]);
                else if (kind[k] == ITEM_DONOR) don.push_back(ia[k]);
                else acc.push_back(ia[k]);
            }
            A.n_acc[i] = uniq(acc); A.n_exo[i] = uniq(exo); A.n_don[i] = uniq(don);
            tx_cnt[i] = uniq(txs);                                    // transcript indices ascend with transcript ids
            tx_part[t].insert(tx_part[t].end(), txs.begin(), txs.end());
        }
    };
    run_tasks(T, work);
    for (size_t i = 0; i < N; ++i) A.tx_off[i + 1] = A.tx_off[i] + tx_cnt[i];
    A.tx.reserve(A.tx_off[N]);
    for (size_t t = 0; t < T; ++t) A.tx.insert(A.tx.end(), tx_part[t].begin(), tx_part[t].end());
    return RGX_OK;
}

extern "C" int rgx_annotate_junctions(rgx_ctx *ctx, const rgx_gtf *g, uint64_t n, const char *const *chrom, const uint32_t *start, const uint32_t *end1,
                                      const char *strand, rgx_junction_annot **out, char *err, size_t errlen) {
    *out = nullptr;
    std::vector<int32_t> ci((size_t)n); std::vector<uint32_t> js(start, start + n), je(end1, end1 + n); std::vector<uint8_t> sd((size_t)n);
    for (uint64_t i = 0; i < n; ++i) { ci[(size_t)i] = g->m.chrom_of(chrom[i]); sd[(size_t)i] = (uint8_t)strand[i]; }
    JunctionAnnotHost A;
    int rc = annotate_junctions(ctx, g, ci, js, je, sd, A, err, errlen);
    if (rc != RGX_OK) return rc;
    rgx_junction_annot *r = (rgx_junction_annot *)calloc(1, sizeof *r);
    r->n = n; r->flags = dup_u32(A.flags); r->n_acceptors_skipped = dup_u32(A.n_acc); r->n_exons_skipped = dup_u32(A.n_exo);
    r->n_donors_skipped = dup_u32(A.n_don); r->tx_off = dup_u32(A.tx_off); r->tx = dup_u32(A.tx);
    *out = r;
    return RGX_OK;
}
extern "C" void rgx_junction_annot_free(rgx_junction_annot *a) {
    if (!a) return;
    free(a->flags); free(a->n_acceptors_skipped); free(a->n_exons_skipped); free(a->n_donors_skipped); free(a->tx_off); free(a->tx); free(a);
}

// a10 for a whole VCF (V.vcf loaded by the caller, usually on a side thread): every record against the annotation on the device, strings on the host
int variant_scan_stage(rgx_ctx *c, const rgx_gtf *g, const VariantOpts &vo, VariantStage &V, uint64_t *exon_visits, char *err, size_t errlen) {
    const size_t n = V.vcf.recs.size();
    std::vector<int32_t> vchrom(n); std::vector<uint32_t> vpos(n);
    {   // (records of a VCF come contig by contig: one table lookup per run of equal names)
        const std::string *last = nullptr; int32_t last_c = -1;
        for (size_t i = 0; i < n; ++i) {
            const std::string &cn = V.vcf.recs[i].chrom;
            if (!last || *last != cn) { last = &cn; last_c = g->m.chrom_of(cn); }
            vchrom[i] = last_c; vpos[i] = V.vcf.recs[i].pos0;
        }
    }
    int rc = variant_windows(c, g, vchrom, vpos, vo, V.H, err, errlen, exon_visits);
    if (rc != RGX_OK) return rc;
    static const char *kAnn[] = {"non_splice_region", "exonic", "intronic", "splicing_exonic", "splicing_intronic"};
    // strings only for the splice relevant records (a few per cent of a VCF), built by threads over ranges of them
    V.relevant.clear();
    for (size_t i = 0; i < n; ++i) if (V.H.off[i + 1] != V.H.off[i]) V.relevant.push_back(i);
    const size_t R = V.relevant.size();
    V.vstr.assign(R, VStr());
    V.vstr_of.assign(n, UINT32_MAX);
    for (size_t r = 0; r < R; ++r) V.vstr_of[V.relevant[r]] = (uint32_t)r;
    auto build = [&](size_t r0, size_t r1) {
        std::vector<const std::string *> seen;
        for (size_t r = r0; r < r1; ++r) {
            const size_t i = V.relevant[r];
            VStr &s = V.vstr[r];
            seen.clear();
            for (uint32_t k = V.H.off[i]; k < V.H.off[i + 1]; ++k) {
                const uint32_t t = V.H.tx[k];
                const std::string &gn = g->m.tx_gene_name[t];
                bool dup = false; for (auto *x : seen) if (*x == gn) dup = true;
                if (!dup) { if (!seen.empty()) s.genes += ","; s.genes += gn; seen.push_back(&gn); }
                if (k != V.H.off[i]) { s.transcripts += ","; s.distances += ","; s.annotations += ","; }
                s.transcripts += g->m.tx_id[t]; s.distances += std::to_string(V.H.dist[k]); s.annotations += kAnn[V.H.ann[k]];
            }
        }
    };
    const size_t nt = R < 4096 ? 1 : std::min<size_t>(usable_threads(16), 16);
    run_tasks(nt, [&](size_t k) { build(R * k / nt, R * (k + 1) / nt); });
    return RGX_OK;
}
