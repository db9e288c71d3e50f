// cse_identify.cpp -- `cis-splice-effects identify` and `associate` as one staged run (IdentifyRun), their entry points, and `variants annotate`, which shares
// the run's first half.
#include "cse_internal.h"

extern "C" void rgx_identify_params_default(rgx_identify_params *p) {
    memset(p, 0, sizeof *p);
    p->intronic_min = 2; p->exonic_min = 3; p->skip_single = 1; p->strandness = -1; p->strand_tag[0] = 'X'; p->strand_tag[1] = 'S';
    p->min_anchor = 8; p->min_intron = 70; p->max_intron = 500000;
}

// One call of `identify` (p->bed_path == nullptr) or `associate`.  The stages run in the order of run(); each returns kGoOn, or the call's result.  What one
// stage leaves for the next are the members below.  Where the reference writes which stderr line is decided by where echo_variants() is called in front of
// each way out.
struct IdentifyRun {
    // -- the call's arguments --
    rgx_ctx *c; const std::vector<rgx_ctx *> *shards; const rgx_identify_params *p; rgx_identify_stats *stats; char *err; size_t errlen;
    // -- what the stages leave for one another --
    TraceTeardown teardown{"identify: locals released"};          // (in front of every other member: the last to go)
    rgx_identify_stats S;
    bool trace = false;
    double t0 = 0, tl = 0;
    void lap(double &slot) { const double t = now_ms(); slot += t - tl; tl = t; }
    // stage_inputs: the annotation and the VCF on their way in (two host threads: parsing only, no device calls), the BAM's events
    GtfGuard gtf;
    std::unique_ptr<VariantStage> V;                              // (on the heap: a finished call hands its teardown to the background thread)
    SideLoad gtf_load, vcf_load;
    FileBytes bam; std::vector<uint8_t> bai;
    // what htslib says when the BAM and its index are opened (no EOF member, an index older than the file): upstream opens both once per splice-relevant
    // variant, behind the variant's echo (identifier.cc:288-289)
    std::string bam_notes;
    Prep P;
    int rc_bam = RGX_OK;
    char err_bam[512];
    rgx_extract_params ep;
    EventsArgs whole_file_args() {                                // the BAM's events from the file's host bytes, unsharded, with `ep`
        EventsArgs a;
        a.c = c; a.p = &ep; a.want_read_span = true;
        a.h_bam = bam.data(); a.bam_len = bam.size();
        a.index = bai.data(); a.index_len = bai.size();
        return a;
    }
    // stage_annotation: the pool of the host stages from here on, the annotated VCF on its way out (a side thread that only reads V)
    PoolScope stage_pool;
    std::thread t_vcfout;
    int rc_vcf = RGX_OK;
    char err_vcf[512];
    double vcf_ms = 0;
    // stage_windows: every splice-relevant variant's window as the region parser reads it; the rows of a damaged file's windows, read one by one
    struct Windows { std::vector<int32_t> tid, beg, end; std::vector<std::string> region; bool by_seeks = false; HostRows R; } win;
    double jt = 0;
    void join_lap(const char *what) { if (trace) { const double t = now_ms(); fprintf(stderr, "[rgx trace] join: %-22s +%8.3f ms\n", what, t - jt); jt = t; } }
    // stage_join_bed / stage_join_bam: the junctions that go out, each with its variants
    JTable uj;

    // a variant's window (identifier.cc:270-274): -w around it, or the cis range the annotation walk left, in uint32 arithmetic
    struct Window { uint32_t rs, re; };
    Window window_of(size_t i) const {
        const uint32_t start = V->vcf.recs[i].pos0, end = start + 1;
        return Window{p->window ? (uint32_t)(start - p->window) : V->H.ces[i], p->window ? (uint32_t)(end + p->window) : V->H.cee[i]};
    }
    uint32_t ilen_bits() const { return std::min<uint32_t>(32, bitlen(p->max_intron) + 2); }
    void echo_variants(size_t upto);
    int died_reading_the_vcf();
    // the side threads read V, the annotation and p: joined before any member goes, on every way out
    ~IdentifyRun() { gtf_load.join(); vcf_load.join(); if (t_vcfout.joinable()) t_vcfout.join(); }
    int run();
    int stage_inputs();
    int stage_annotation();
    int stage_join_bed();
    int stage_windows();
    int windows_by_seeks(size_t w_bad);
    int stage_join_bam();
    int stage_outputs();
    void hand_to_reaper();
};

int IdentifyRun::run() {
    if (!c || !p) return fail(err, errlen, RGX_ERR_ARG, "regtools_amd: bad arguments\n");
    if (!p->vcf_path || !p->bam_path || !p->fasta_path || !p->gtf_path) return fail(err, errlen, RGX_ERR_ARG, "Error parsing inputs!(2)\n\n");
    if (p->strandness < 0 || p->strandness > 3) return fail(err, errlen, RGX_ERR_ARG, "Please supply strand specificity with '-s' option!\n\n");
    memset(&S, 0, sizeof S);
    ktime_collect(c); c->kms[0] = c->kms[1] = c->kms[2] = 0;
    trace = getenv("REGTOOLS_AMD_TRACE") != nullptr;
    t0 = tl = now_ms();
    { const int rc = stage_inputs(); if (rc != kGoOn) return rc; }
    { const int rc = stage_annotation(); if (rc != kGoOn) return rc; }
    if (p->bed_path) { const int rc = stage_join_bed(); if (rc != kGoOn) return rc; }
    else {
        { const int rc = stage_windows(); if (rc != kGoOn) return rc; }
        { const int rc = stage_join_bam(); if (rc != kGoOn) return rc; }
    }
    { const int rc = stage_outputs(); if (rc != kGoOn) return rc; }
    hand_to_reaper();
    return RGX_OK;
}

// The three inputs are independent until the variant scan, so they are read at the same time: the GTF and the VCF text on two host
// threads (parsing only, no device calls), the BAM on this one, which owns the device.  What the reference reports when several of them
// are unusable is decided afterwards, in its order: GtfParser::load (identifier.cc:258-259), the FASTA, the VCF, and the BAM only when a
// variant is splice relevant (it opens the BAM per such variant, :288-290) -- the extraction below is done ahead of knowing that.
int IdentifyRun::stage_inputs() {
    gtf.g = new rgx_gtf();
    gtf.g->ctx = c;
    V.reset(new VariantStage());
    gtf_load.start([this] { return gtf.g->m.load(p->gtf_path); });
    vcf_load.start([this] { return V->vcf.load(p->vcf_path, /*annotating=*/p->out_vcf != nullptr); });

    // ---- identify: the extraction, ONCE for all windows (the reference re-opens the BAM per variant: identifier.cc:288-290) ----
    err_bam[0] = 0; err_vcf[0] = 0;
    rgx_extract_params_default(&ep);
    if (p->bed_path) return kGoOn;
    ep.region = "."; ep.strandness = p->strandness; ep.strand_tag[0] = p->strand_tag[0]; ep.strand_tag[1] = p->strand_tag[1];
    ep.min_anchor = p->min_anchor; ep.min_intron = p->min_anchor /* ctor quirk junctions_extractor.h:200 */; ep.max_intron = p->max_intron;
    ep.fasta_path = (p->override_motif || p->strandness == 3) ? p->fasta_path : nullptr;   // ref_to_pass (identifier.cc:282-287)
    std::string idx;
    if (!bam.open(p->bam_path)) rc_bam = fail(err_bam, sizeof err_bam, RGX_ERR_OPEN, "%s", kMsgOpen);
    else if (find_index(p->bam_path, idx) != 0) { bam_notes = bam_open_notes(bam.data(), bam.size(), nullptr, nullptr);
        rc_bam = fail(err_bam, sizeof err_bam, RGX_ERR_INDEX, "%s", kMsgIndex); }
    else if (bam_notes = bam_open_notes(bam.data(), bam.size(), p->bam_path, idx.c_str()), !read_index(idx, bai)) rc_bam = fail(err_bam, sizeof err_bam,
        RGX_ERR_INDEX, "%s", kMsgIndex);
    else if (shards && shards->size() > 1) rc_bam = prepare_events_sharded(*shards, bam.data(), bam.size(), bai.data(), bai.size(), &ep, P, err_bam,
        sizeof err_bam);
    else rc_bam = prepare_events(whole_file_args(), P, err_bam, sizeof err_bam);
    lap(S.ms_extract);
    return kGoOn;
}

// a10: every variant against the annotation
int IdentifyRun::stage_annotation() {
    // (the host stages behind this point share one pool of threads; started here, where this thread would wait for the GTF otherwise)
    stage_pool.start(usable_threads(16));
    gtf_load.join();
    if (!gtf_load.err.empty()) return fail(err, errlen, RGX_ERR_FORMAT, "%s", gtf_load.err.c_str());
    // (the annotator's constructor prints the member before it assigns it: always the default, variants_annotator.h:141-152)
    if (p->echo) fputs("exonic_min_distance_ is 3\n", stderr);
    int rc = gtf_upload(c, gtf.g, err, errlen, /*pooled=*/true);
    if (rc != RGX_OK) return rc;
    lap(S.ms_gtf);                                              // (what of the GTF was still to do when the extraction was done)
    if (!host_fasta(c, p->fasta_path)) return fail(err, errlen, RGX_ERR_FASTA, "Unable to open FASTA file.\n\n");

    vcf_load.join();
    if (!vcf_load.err.empty()) return fail(err, errlen, vcf_load_code(V->vcf), "%s", vcf_load.err.c_str());
    if (p->echo) fputs("\n", stderr);                                // (identifier.cc:265, associator.cc:243)
    if (trace) fprintf(stderr, "[rgx trace] inputs: gtf thread %8.3f ms, vcf thread %8.3f ms, extraction %8.3f ms (side by side)\n",
        gtf_load.ms, vcf_load.ms, S.ms_extract);
    VariantOpts vo{p->intronic_min, p->exonic_min, p->all_intronic, p->all_exonic, p->skip_single};
    rc = variant_scan_stage(c, gtf.g, vo, *V, &S.exon_visits_variants, err, errlen);
    if (rc != RGX_OK) return rc;
    S.n_variants = V->vcf.recs.size(); S.n_relevant = V->relevant.size();
    lap(S.ms_variants);
    // the annotated VCF is written on a side thread while the windows are joined and the junctions annotated (it only reads V); it is complete, or
    // its error is the call's, before any junction output is opened
    if (p->out_vcf) t_vcfout = std::thread([this] { const double t = now_ms(); rc_vcf = write_annotated_vcf(p->out_vcf, *V, false, err_vcf, sizeof err_vcf,
        /*print_notes=*/false); vcf_ms = now_ms() - t; });
    return kGoOn;
}

// p->echo: what upstream writes to stderr for every splice-relevant variant, in file order, before it looks at the alignments of its window
// (identifier.cc:275-277, associator.cc:255-257): "Variant " + BED's operator<< (chrom, start, end, score, strand, each followed by a tab;
// bedFile.h:183-194; the score is what the annotation walk left there: H.last) and the window as the region string
// What reading the records says (vcf.notes: a name the header does not declare, ...) comes out here as well, a record's lines in front of its
// "Variant" lines: upstream reads, annotates and echoes one record after the other (identifier.cc:267-277).
void IdentifyRun::echo_variants(size_t upto) {
    const VcfText &vcf = V->vcf; const VariantHitsHost &H = V->H; const std::vector<size_t> &relevant = V->relevant;
    const bool all = upto >= relevant.size();
    if (!p->echo) {                                                    // (a library caller: the records' lines, and the BAM's once)
        vcf.flush_notes(all ? SIZE_MAX : relevant[upto - 1] + 1);
        if (upto && !relevant.empty()) fputs(bam_notes.c_str(), stderr);
        return;
    }
    std::string s;
    s.reserve(std::min(upto, relevant.size()) * 72);
    for (size_t w = 0; w < upto && w < relevant.size(); ++w) {
        const size_t i = relevant[w];
        if (vcf.notes_printed < vcf.notes.size() && vcf.notes[vcf.notes_printed].first <= i) {
            fwrite(s.data(), 1, s.size(), stderr); s.clear();
            vcf.flush_notes(i + 1);
        }
        const uint32_t start = vcf.recs[i].pos0, end = start + 1;
        const Window win_i = window_of(i);
        s += "Variant "; s += vcf.recs[i].chrom; s += '\t'; put_u(s, start); s += '\t'; put_u(s, end); s += '\t';
        if (H.last[i] == 0xffffffffu) s += "-1"; else put_u(s, H.last[i]);
        s += "\t\t\nVariant region is "; s += vcf.recs[i].chrom; s += ':'; put_u(s, win_i.rs); s += '-'; put_u(s, win_i.re); s += "\n\n";
        s += bam_notes;
    }
    fwrite(s.data(), 1, s.size(), stderr);
    if (all) vcf.flush_notes(SIZE_MAX);
}
// the record the reference's process ends in, once everything in front of it is echoed (its variants have had their windows read by then)
int IdentifyRun::died_reading_the_vcf() {
    if (V->vcf.fatal.empty()) return RGX_OK;
    return fail(err, errlen, V->vcf.fatal_aborts ? RGX_ERR_ABORT : RGX_ERR_EXIT, "%s\n", V->vcf.fatal.c_str());
}

// ---- associate: junctions from a BED12 (associator.cc:206-276) ----
int IdentifyRun::stage_join_bed() {
    const VcfText &vcf = V->vcf; const VariantHitsHost &H = V->H; const std::vector<size_t> &relevant = V->relevant;
    echo_variants(relevant.size());
    if (int rc_died = died_reading_the_vcf()) return rc_died;
    BedJunctions B;
    { std::string e = B.load(p->bed_path); if (!e.empty()) return fail(err, errlen, RGX_ERR_FORMAT, "%s", e.c_str()); }
    // bucket by contig, file order kept inside a bucket
    std::unordered_map<std::string, int32_t> cidx; std::vector<std::string> cname;
    std::vector<int32_t> jch(B.n());
    for (size_t i = 0; i < B.n(); ++i) { auto it = cidx.find(B.chrom[i]); if (it == cidx.end()) { it = cidx.emplace(B.chrom[i],
        (int32_t)cname.size()).first; cname.push_back(B.chrom[i]); } jch[i] = it->second; }
    std::vector<uint32_t> chrom_off(cname.size() + 1, 0), order(B.n()), js(B.n()), je(B.n());
    for (size_t i = 0; i < B.n(); ++i) chrom_off[(size_t)jch[i] + 1]++;
    for (size_t k = 0; k < cname.size(); ++k) chrom_off[k + 1] += chrom_off[k];
    { std::vector<uint32_t> fill(chrom_off.begin(), chrom_off.end() - 1);
      // Junction.end = line.end - 1 (:221)
      for (size_t i = 0; i < B.n(); ++i) { const uint32_t q = fill[(size_t)jch[i]]++; order[q] = (uint32_t)i; js[q] = B.start[i]; je[q] = B.end[i] - 1; } }
    const uint32_t W = (uint32_t)relevant.size(), J = (uint32_t)B.n();
    S.n_windows = W; S.n_events = J;
    std::vector<uint32_t> pj, pw;
    {
        std::vector<int32_t> wch(W); std::vector<uint32_t> wces(W), wcee(W);
        for (uint32_t w = 0; w < W; ++w) { const size_t vi = relevant[w]; auto it = cidx.find(vcf.recs[vi].chrom); wch[w] = it == cidx.end() ? -1 :
            it->second; wces[w] = H.ces[vi]; wcee[w] = H.cee[vi]; }
        const int rc = assoc_join(c, wch, wces, wcee, chrom_off, js, je, pj, pw, S.n_pairs, err, errlen);
        if (rc != RGX_OK) return rc;
    }
    S.n_window_rows = pj.size();
    {
        std::vector<uint32_t> crank_of, vrank_of;
        string_ranks(cname, crank_of, uj.chrom_name);
        run_string_ranks(relevant.size(), [&](size_t w) -> const std::string & { return vcf.recs[relevant[w]].chrom; }, vrank_of, uj.vchrom_name);
        uj.cand.reserve(pj.size());
        for (size_t r = 0; r < pj.size(); ++r) {
            const size_t vi = relevant[pw[r]], bi = order[pj[r]];
            uj.add(crank_of[(size_t)jch[bi]], B.start[bi], B.end[bi] - 1, vrank_of[pw[r]], vcf.recs[vi].pos0, (uint32_t)bi);
        }
        auto entry_of = [&](uint32_t bi) { return JEntry{B.ts[bi], B.te[bi], (uint32_t)atoi(B.score[bi].c_str()), B.strand[bi], B.color[bi], B.nblocks[bi]}; };
        uj.finish(entry_of, tl_pool);
    }
    S.n_junctions = uj.size();
    lap(S.ms_join);
    return kGoOn;
}

// windows (identifier.cc:270-274): "chrom:start-end" built with uint32 arithmetic, then parsed as sam_itr_querys would
int IdentifyRun::stage_windows() {
    const VcfText &vcf = V->vcf; const std::vector<size_t> &relevant = V->relevant;
    // (upstream opens the BAM for the first such variant)
    if (!relevant.empty() && rc_bam != RGX_OK) { echo_variants(1); return fail(err, errlen, rc_bam, "%s", err_bam); }
    if (relevant.empty()) P = Prep();                       // (no variant asks for the BAM: upstream never opens it)
    S.n_records = P.n_iterated; S.n_events = P.n_events;
    jt = now_ms();
    // a file whose record stream ended (damage): every window is read through the index on its own, as upstream reads it (window_join_by_seeks)
    win.by_seeks = P.stream_ended && !relevant.empty();
    BaiInfo bi; (void)parse_bai(bai.data(), bai.size(), bi, false);
    // (every window's region string goes through the region parser, as upstream; ranges of them on several threads, the first one that
    //  does not parse -- in file order -- aborts the run)
    const size_t W = relevant.size();
    win.tid.resize(W); win.beg.resize(W); win.end.resize(W);
    if (win.by_seeks) win.region.resize(W);
    const size_t nt = W < 4096 ? 1 : stage_pool.pool->threads();
    std::vector<size_t> bad(nt, SIZE_MAX);
    stage_pool.pool->run(nt, [&](size_t t) {
        for (size_t w = W * t / nt; w < W * (t + 1) / nt; ++w) {
            const size_t i = relevant[w];
            const Window win_i = window_of(i);
            const std::string region = vcf.recs[i].chrom + ":" + std::to_string(win_i.rs) + "-" + std::to_string(win_i.re);
            int32_t tid, beg, en;
            if (!parse_region(P.hdr, region.c_str(), tid, beg, en) || tid >= bi.n_ref || en < beg) { bad[t] = w; return; }
            win.tid[w] = tid; win.beg[w] = beg; win.end[w] = en;
            if (win.by_seeks) win.region[w] = region;
        }
    });
    size_t w_bad = SIZE_MAX;
    // (a thread stops at its first: the first thread's is the file's first)
    for (size_t t = 0; t < nt && w_bad == SIZE_MAX; ++t) w_bad = bad[t];
    // -s XS: a read with an N operation whose strand tag lies behind an aux field of unknown type ends the process in the first window that READS it
    // (tid, pos < end, bam_endpos > beg: hts.c:1946-1957) -- bam_aux_get abort()s, sam.c:1233-1252, nothing printed -- behind that variant's echo
    if (win.by_seeks) { const int rc = windows_by_seeks(w_bad); if (rc != kGoOn) return rc; }
    else if (!P.odd_aux.empty())
        for (size_t w = 0; w < std::min(W, w_bad); ++w)
            for (const Prep::OddAux &o : P.odd_aux)
                if (o.tid == win.tid[w] && o.pos < win.end[w] && o.end > win.beg[w]) {
                    echo_variants(w + 1);
                    return fail(err, errlen, RGX_ERR_ABORT,
                        "regtools_amd: a read at %s:%d has an auxiliary field of unknown type in front of its strand tag: the reference "
                        "abort()s in this variant's window\n", vcf.recs[relevant[w]].chrom.c_str(), o.pos + 1);
                }
    // aborts the run
    if (w_bad != SIZE_MAX) { echo_variants(w_bad + 1); return fail(err, errlen, RGX_ERR_REGION, "%s", kMsgRegion); }
    echo_variants(relevant.size());
    if (int rc_died = died_reading_the_vcf()) return rc_died;
    S.n_windows = win.tid.size();
    join_lap("window regions");
    return kGoOn;
}

// the windows in front of the first that does not parse, each read through the index on its own; the rows are win.R
int IdentifyRun::windows_by_seeks(size_t w_bad) {
    const VcfText &vcf = V->vcf; const std::vector<size_t> &relevant = V->relevant;
    const uint8_t *d_file = P.d_file;
    // (a sharded extraction left no whole copy of the file in HBM: once more, unsharded)
    Prep P0;
    if (!d_file) {
        const int rc0 = prepare_events(whole_file_args(), P0, err, errlen);
        if (rc0 != RGX_OK) { echo_variants(1); return rc0; }
        d_file = P0.d_file;
    }
    win.region.resize(std::min(relevant.size(), w_bad));
    size_t w_abort = SIZE_MAX;
    const int rcj = window_join_by_seeks(c, d_file, bam.size(), bai.data(), bai.size(), ep, win.region, ilen_bits(), win.R, S.n_pairs, w_abort, err, errlen);
    if (rcj != RGX_OK) { echo_variants(1); return rcj; }
    if (w_abort != SIZE_MAX) {
        echo_variants(w_abort + 1);
        return fail(err, errlen, RGX_ERR_ABORT,
            "regtools_amd: a read in the window of the variant at %s:%u has an auxiliary field of unknown type in front of its strand "
            "tag: the reference abort()s there\n", vcf.recs[relevant[w_abort]].chrom.c_str(), vcf.recs[relevant[w_abort]].pos0 + 1);
    }
    return kGoOn;
}

// a9 for `identify`: the rows of every window, those that lie in their variant's cis range (identifier.cc:292-294), the table
int IdentifyRun::stage_join_bam() {
    const VcfText &vcf = V->vcf; const VariantHitsHost &H = V->H; const std::vector<size_t> &relevant = V->relevant;
    HostRows &R = win.R;
    if (!win.by_seeks) { const int rc = window_join(c, P, win.tid, win.beg, win.end, ilen_bits(), R, S.n_pairs, err, errlen); if (rc != RGX_OK) return rc; }
    S.n_window_rows = R.n;
    join_lap("window_join");
    std::vector<uint32_t> crank_of, vrank_of;
    string_ranks(P.hdr.names, crank_of, uj.chrom_name);
    // (a window's contig is its variant's: the variant's name ranks like the window's contig)
    run_string_ranks(relevant.size(), [&](size_t w) -> const std::string & { return vcf.recs[relevant[w]].chrom; }, vrank_of, uj.vchrom_name);
    join_lap("keep: name ranks");
    uj.cand.reserve(R.n);
    for (size_t r = 0; r < R.n; ++r) {
        const size_t vi = relevant[R.group[r]];
        const uint32_t ces = H.ces[vi], cee = H.cee[vi];
        const uint32_t js = R.start[r], je = R.end[r];
        if (!((js >= ces && js <= cee) || (je <= cee && je >= ces))) continue;           // identifier.cc:292-294
        uj.add(crank_of[(size_t)win.tid[R.group[r]]], js, je, vrank_of[R.group[r]], vcf.recs[vi].pos0, (uint32_t)r);
    }
    join_lap("keep: filter");
    uj.finish([&](uint32_t r) { return JEntry{R.ts[r], R.te[r], R.count[r], std::string(1, (char)R.strand[r]), "255,0,0", 2}; }, tl_pool);
    S.n_junctions = uj.size();
    join_lap("keep: first-insert map");
    lap(S.ms_join);
    win = Windows();                                            // (the windows' rows go here, in front of the outputs, not with the call's teardown)
    return kGoOn;
}

// a11 + the output files, then the call's figures
int IdentifyRun::stage_outputs() {
    if (t_vcfout.joinable()) t_vcfout.join();
    if (rc_vcf != RGX_OK) return fail(err, errlen, rc_vcf, "%s", err_vcf);
    if (trace) fprintf(stderr, "[rgx trace] outputs: annotated VCF (side thread) %8.3f ms\n", vcf_ms);
    lap(S.ms_output);                                           // (what of the VCF was still being written when the join was done)
    const int rc = write_junction_outputs(c, gtf.g, p->fasta_path, uj, p->out_tsv, p->out_bed, &S.exon_visits_junctions, &S.ms_annotate, err, errlen,
        p->echo != 0);
    if (rc != RGX_OK) return rc;
    { const double t = now_ms(); S.ms_output += t - tl - S.ms_annotate; tl = t; }
    ktime_collect(c); S.ms_k_variant_scan = c->kms[0]; S.ms_k_junction_scan = c->kms[1]; S.ms_k_window_pairs = c->kms[2];
    S.ms_total = now_ms() - t0;
    if (stats) *stats = S;
    if (trace) { fprintf(stderr, "[rgx trace] identify: total %8.3f ms\n", S.ms_total); teardown.t = now_ms(); }
    return kGoOn;
}

// The outputs are written.  What is left is teardown -- unmapping the BAM (8.5 ms for 533 MB: page tables), the annotation's tables and its
// block of HBM (4 ms), the VCF's lines and strings (3 ms): 15 of config 4's 75 ms.  Round 4: the process's background thread does it
// (worker_pool.h Reaper; rgx_ctx_destroy and the process's exit wait for it), the call returns.
void IdentifyRun::hand_to_reaper() {
    VariantStage *vs = V.release();
    rgx_gtf *gg = gtf.release();
    // (the junction table and the index image go the same way, and FIRST: freed by this thread, their blocks' munmap waited for the address-space
    //  lock behind the background thread's unmapping of the 533 MB BAM -- 5-7 ms of the caller's time between "total" and the return, round 6)
    JTable *ujh = new JTable(std::move(uj));
    std::vector<uint8_t> *baih = new std::vector<uint8_t>(std::move(bai));
    Reaper::get().later([ujh, baih] { delete ujh; delete baih; });
    bam.release_later();
    // (host memory only: the annotation's device tables are the context's, gtf_upload(pooled) -- no HIP call on that thread)
    Reaper::get().later([vs, gg] { delete vs; rgx_gtf_free(gg); });
}

extern "C" int rgx_identify(rgx_ctx *c, const rgx_identify_params *p, rgx_identify_stats *stats, char *err, size_t errlen) {
    return IdentifyRun{c, nullptr, p, stats, err, errlen}.run();
}

// `identify` with the extraction sharded over the listed devices (prepare_events_sharded); everything behind it on the first one.  A device may be
// listed more than once (its shards take turns on it).  The outputs do not depend on the list.
extern "C" int rgx_identify_multi(const int *devices, int n_devices, const rgx_identify_params *p, rgx_identify_stats *stats, char *err, size_t errlen) {
    if (!devices || n_devices <= 0 || n_devices > 255 || !p) return fail(err, errlen, RGX_ERR_ARG, "regtools_amd: bad arguments\n");
    static std::mutex call_mu;                                    // the cached contexts are shared by every call of the process: calls take turns
    std::lock_guard<std::mutex> lock(call_mu);
    std::vector<rgx_ctx *> cs((size_t)n_devices);
    std::map<int, int> seen;
    for (int g = 0; g < n_devices; ++g) {
        int rc = RGX_OK;
        cs[(size_t)g] = rgx_multi_context(devices[g], seen[devices[g]]++, err, errlen, &rc);
        if (rc != RGX_OK) return rc;
    }
    return IdentifyRun{cs[0], &cs, p, stats, err, errlen}.run();
}

// ---- `cis-splice-effects associate` (cis_splice_effects_associator.cc:234-276): identify with p->bed_path set -------------------
extern "C" int rgx_associate(rgx_ctx *c, const rgx_identify_params *p, rgx_identify_stats *stats, char *err, size_t errlen) {
    if (!c || !p || !p->bed_path) return fail(err, errlen, RGX_ERR_ARG, "Error parsing inputs!(2)\n\n");
    rgx_identify_params q = *p;
    q.bam_path = p->bed_path;          // only checked for presence on this branch
    q.strandness = 0;
    return rgx_identify(c, &q, stats, err, errlen);
}

// ---- `variants annotate` (variants_annotator.cc:541-550) ---------------------------------------------------------------------------
extern "C" int rgx_variants_annotate(rgx_ctx *c, const rgx_identify_params *p, rgx_identify_stats *stats, char *err, size_t errlen) {
    if (!c || !p || !p->vcf_path || !p->gtf_path) return fail(err, errlen, RGX_ERR_ARG, "Error parsing inputs!(2)\n\n");
    rgx_identify_stats S; memset(&S, 0, sizeof S);
    ktime_collect(c); c->kms[0] = c->kms[1] = c->kms[2] = 0;
    const double t0 = now_ms();
    // the VCF is read on a side thread while this one parses the GTF (as `identify` reads its inputs side by side); the GTF's error comes first
    GtfGuard gtf(new rgx_gtf());
    rgx_gtf *g = gtf.g;
    g->ctx = c;
    VariantStage V;
    SideLoad vcf_load;
    vcf_load.start([&] { return V.vcf.load(p->vcf_path); });
    {
        const std::string e = load_text([&] { return g->m.load(p->gtf_path); });
        if (!e.empty()) return fail(err, errlen, RGX_ERR_FORMAT, "%s", e.c_str());
    }
    int rc = gtf_upload(c, g, err, errlen, /*pooled=*/true);
    if (rc != RGX_OK) return rc;
    S.ms_gtf = now_ms() - t0;
    VariantOpts vo{p->intronic_min, p->exonic_min, p->all_intronic, p->all_exonic, p->skip_single};
    vcf_load.join();
    if (!vcf_load.err.empty()) return fail(err, errlen, vcf_load_code(V.vcf), "%s", vcf_load.err.c_str());
    rc = variant_scan_stage(c, g, vo, V, &S.exon_visits_variants, err, errlen);
    if (rc != RGX_OK) return rc;
    S.n_variants = V.vcf.recs.size(); S.n_relevant = V.relevant.size();
    S.ms_variants = now_ms() - t0 - S.ms_gtf;
    rc = write_annotated_vcf(p->out_vcf, V, true, err, errlen);
    if (rc != RGX_OK) return rc;
    ktime_collect(c); S.ms_k_variant_scan = c->kms[0]; S.ms_k_junction_scan = c->kms[1]; S.ms_k_window_pairs = c->kms[2];
    S.ms_total = now_ms() - t0; S.ms_output = S.ms_total - S.ms_gtf - S.ms_variants;
    if (stats) *stats = S;
    return RGX_OK;
}
