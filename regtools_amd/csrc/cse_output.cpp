// cse_output.cpp -- what the commands write: the annotated VCF, the annotated junction rows of `identify` / `associate` (formatted on the call's threads, put
// out in order by a writer thread), and `junctions annotate`.
#include "cse_internal.h"

// -v / `variants annotate -o`: what htslib writes for bcf_hdr_append x4 + bcf_hdr_write, then per record bcf_update_info_string x4 +
// bcf_write (variants_annotator.cc:130-154, 521-533) -- every record goes through BCF's typed form and back (vcf_rewrite.h).
// all_records = false writes only the splice relevant ones (identifier.cc:278-280), true every one (annotator.cc:545-548).
int write_annotated_vcf(const char *path, const VariantStage &V, bool all_records, char *err, size_t errlen, bool print_notes) {
    FILE *fv = path ? fopen(path, "w") : stdout;
    if (!fv) return fail(err, errlen, RGX_ERR_OPEN, "Unable to open output VCF file.\n\n");
    if (fv != stdout) setvbuf(fv, nullptr, _IOFBF, 1 << 22);
    const VcfText &vcf = V.vcf;
    std::vector<size_t> todo;
    const size_t R = vcf.recs.size();
    for (size_t ri = 0; ri < R; ++ri) if (all_records || V.H.off[ri + 1] != V.H.off[ri]) todo.push_back(ri);
    const std::string e = write_annotated_vcf_records(fv, vcf, todo, [&](size_t ri) -> VcfAnnot {
        if (V.H.off[ri + 1] == V.H.off[ri]) return VcfAnnot{nullptr, nullptr, nullptr, nullptr};
        const VStr &s = V.vstr[V.vstr_of[ri]];
        return VcfAnnot{&s.genes, &s.transcripts, &s.distances, &s.annotations};
    }, print_notes);
    if (fv != stdout) fclose(fv);
    // (the record the reference's process ends in -- exit(1), or abort() -- is the one behind the last one written)
    if (!e.empty()) return fail(err, errlen, e != vcf.fatal ? RGX_ERR_OPEN : vcf.fatal_aborts ? RGX_ERR_ABORT : RGX_ERR_EXIT, "%s\n", e.c_str());
    return RGX_OK;
}

static const char *kJunctionHeader = "chrom\tstart\tend\tname\tscore\tstrand\tsplice_site\tacceptors_skipped\texons_skipped\tdonors_skipped\t"
                                     "anchor\tknown_donor\tknown_acceptor\tknown_junction\tgene_names\tgene_ids\ttranscripts";

// get_splice_site (junctions_annotator.cc:94-114); je = AnnotatedJunction.end
static int splice_site(const Fasta &fa, const std::string &chrom, uint32_t js, uint32_t je, const std::string &strand, std::string &site, char *err,
    size_t errlen) {
    std::string s1, s2;
    if (!fa.fetch(chrom, (int64_t)js + 1, (int64_t)js + 2, s1)) return fail(err, errlen, RGX_ERR_FASTA,
        "Unable to extract FASTA sequence for position %s:%u-%u\n\n", chrom.c_str(), js + 1, js + 2);
    if (!fa.fetch(chrom, (int64_t)je - 2, (int64_t)je - 1, s2)) return fail(err, errlen, RGX_ERR_FASTA,
        "Unable to extract FASTA sequence for position %s:%u-%u\n\n", chrom.c_str(), je - 2, je - 1);
    site = strand == "-" ? rev_comp(s2) + "-" + rev_comp(s1) : s1 + "-" + s2;
    return RGX_OK;
}

// what get_reference_sequence writes to stderr for a junction's two look-ups (junctions_annotator.cc:366-370), the second only if the first one was read
static void append_positions(std::string &o, const std::string &chrom, uint32_t js, uint32_t je, bool both = true) {
    o += "position = "; o += chrom; o += ':'; o += std::to_string(js + 1); o += '-'; o += std::to_string(js + 2); o += '\n';
    if (both) { o += "position = "; o += chrom; o += ':'; o += std::to_string(je - 2); o += '-'; o += std::to_string(je - 1); o += '\n'; }
}

// AnnotatedJunction::print (junctions_annotator.h:84-126) up to the transcripts column, row i of an annotate_junctions() result
static void append_junction_row(std::string &o, const rgx_gtf *g, const JunctionAnnotHost &A, size_t i, const std::string &chrom, uint32_t js, uint32_t je,
    const std::string &name,
                                const std::string &score, const std::string &strand, const std::string &site) {
    const uint32_t f = A.flags[i];
    const bool kd = f & 1, ka = f & 2, kj = f & 4;
    const char *anchor = kj ? "DA" : kd ? (ka ? "NDA" : "D") : ka ? "A" : "N";          // annotate_anchor :295-308
    o += chrom; o += '\t'; put_u(o, js); o += '\t'; put_u(o, je); o += '\t'; o += name; o += '\t'; o += score; o += '\t'; o += strand; o += '\t'; o += site;
        o += '\t';
    put_u(o, A.n_acc[i]); o += '\t'; put_u(o, A.n_exo[i]); o += '\t'; put_u(o, A.n_don[i]); o += '\t'; o += anchor;
    o += kd ? "\t1" : "\t0"; o += ka ? "\t1" : "\t0"; o += kj ? "\t1" : "\t0";
    if (A.tx_off[i + 1] > A.tx_off[i]) {
        // set< vector<string> > of (gene name, gene id): lexicographic, unique
        std::vector<std::pair<const std::string *, const std::string *>> genes;
        for (uint32_t k = A.tx_off[i]; k < A.tx_off[i + 1]; ++k) genes.push_back({&g->m.tx_gene_name[A.tx[k]], &g->m.tx_gene_id[A.tx[k]]});
        auto less = [](const std::pair<const std::string *, const std::string *> &x, const std::pair<const std::string *, const std::string *> &y) {
            const int c = x.first->compare(*y.first); return c < 0 || (c == 0 && *x.second < *y.second); };
        std::sort(genes.begin(), genes.end(), less);
        genes.erase(std::unique(genes.begin(), genes.end(), [](const auto &x, const auto &y) { return *x.first == *y.first && *x.second == *y.second; }),
            genes.end());
        o += '\t'; for (size_t k = 0; k < genes.size(); ++k) { if (k) o += ','; o += *genes[k].first; }
        o += '\t'; for (size_t k = 0; k < genes.size(); ++k) { if (k) o += ','; o += *genes[k].second; }
        o += '\t';
        for (uint32_t k = A.tx_off[i]; k < A.tx_off[i + 1]; ++k) { if (k != A.tx_off[i]) o += ','; o += g->m.tx_id[A.tx[k]]; }
    } else o += "\tNA\tNA\tNA";
}
static void print_junction_row(FILE *fo, const rgx_gtf *g, const JunctionAnnotHost &A, size_t i, const std::string &chrom, uint32_t js, uint32_t je,
    const std::string &name,
                               const std::string &score, const std::string &strand, const std::string &site) {
    std::string o;
    append_junction_row(o, g, A, i, chrom, js, je, name, score, strand, site);
    fwrite(o.data(), 1, o.size(), fo);
}

// a11 + outputs (annotate_junctions identifier.cc:222-246 / associator.cc:182-203)
int write_junction_outputs(rgx_ctx *c, const rgx_gtf *g, const char *fasta_path, const JTable &uj, const char *out_tsv, const char *out_bed,
                           uint64_t *exon_visits, double *ms_annotate, char *err, size_t errlen, bool echo) {
    const double t0 = now_ms();
    TraceTeardown teardown{"outputs: locals released"};
    Fasta *fap = host_fasta(c, fasta_path);
    if (!fap) return fail(err, errlen, RGX_ERR_FASTA, "Unable to open FASTA file.\n\n");
    const Fasta &fa = *fap;
    std::vector<int32_t> jc; std::vector<uint32_t> jjs, jje; std::vector<uint8_t> jst;
    jc.reserve(uj.size()); jjs.reserve(uj.size()); jje.reserve(uj.size()); jst.reserve(uj.size());
    {
        std::vector<int32_t> gtf_chrom(uj.chrom_name.size());
        for (size_t k = 0; k < gtf_chrom.size(); ++k) gtf_chrom[k] = g->m.chrom_of(uj.chrom_name[k]);
        for (const JTable::Row &r : uj.rows) {
            jc.push_back(gtf_chrom[r.crank]); jjs.push_back(r.js); jje.push_back(r.jend + 1);
            jst.push_back(r.e.strand.size() == 1 ? (uint8_t)r.e.strand[0] : (uint8_t)'?');
        }
    }
    JunctionAnnotHost A;
    int rc = annotate_junctions(c, g, jc, jjs, jje, jst, A, err, errlen, exon_visits);
    if (rc != RGX_OK) return rc;
    if (ms_annotate) *ms_annotate += now_ms() - t0;
    const bool trace = getenv("REGTOOLS_AMD_TRACE") != nullptr;
    double t_last = now_ms();
    auto lap = [&](const char *what) { if (trace) { const double t = now_ms(); fprintf(stderr, "[rgx trace] outputs: %-18s +%8.3f ms\n", what, t - t_last);
        t_last = t; } };
    // get_splice_site for every junction up front, on several host threads: two 2-base reads at random places of a multi-GB FASTA mapping are
    // two page faults per junction (0.13 s of config 4's 0.47 s when done row by row in the print loop).  The FIRST junction that fails, in
    // output order, ends the run with its message after the rows before it were written -- as the row-by-row loop did.
    std::vector<std::string> sites(uj.size());
    size_t first_bad = SIZE_MAX; char bad_msg[512] = {0};
    const std::vector<JTable::Row> &rows = uj.rows;
    {
        const size_t n = rows.size();
        const size_t T = n < 2048 ? 1 : usable_threads(16);
        std::vector<size_t> bad(T, SIZE_MAX); std::vector<std::string> msg(T);
        auto work = [&](size_t t) {
            for (size_t k = n * t / T; k < n * (t + 1) / T; ++k) {
                const JTable::Row &r = rows[k];
                char e2[512] = {0};
                if (splice_site(fa, uj.chrom_name[r.crank], r.js, r.jend + 1, r.e.strand, sites[k], e2, sizeof e2) != RGX_OK) { bad[t] = k; msg[t] = e2;
                    return; }
            }
        };
        run_tasks(T, work);
        for (size_t t = 0; t < T; ++t) if (bad[t] < first_bad) { first_bad = bad[t]; snprintf(bad_msg, sizeof bad_msg, "%s", msg[t].c_str()); }
    }
    lap("splice sites");
    if (echo) {                                                    // (in output order; the junction whose look-up fails is the last one heard of)
        std::string s;
        const size_t upto = std::min(rows.size(), first_bad);
        s.reserve(upto * 64);
        for (size_t k = 0; k < upto; ++k) append_positions(s, uj.chrom_name[rows[k].crank], rows[k].js, rows[k].jend + 1);
        if (first_bad != SIZE_MAX) {
            const JTable::Row &r = rows[first_bad];
            std::string tmp;
            append_positions(s, uj.chrom_name[r.crank], r.js, r.jend + 1, fa.fetch(uj.chrom_name[r.crank], (int64_t)r.js + 1, (int64_t)r.js + 2, tmp));
        }
        fwrite(s.data(), 1, s.size(), stderr);
    }
    FILE *fo = out_tsv ? fopen(out_tsv, "w") : stdout;
    if (!fo) return fail(err, errlen, RGX_ERR_OPEN, "Unable to open %s", out_tsv);
    FILE *fj = out_bed ? fopen(out_bed, "w") : nullptr;
    if (fo != stdout) setvbuf(fo, nullptr, _IOFBF, 1 << 22);
    if (fj) setvbuf(fj, nullptr, _IOFBF, 1 << 22);
    fprintf(fo, "%s\tvariant_info\n", kJunctionHeader);
    // the rows are formatted by several threads, each into its own memory stream, and written out in order (66 k rows: 80 ms in one thread)
    // (round 6: four chunks per thread, handed out as threads come free -- rows that name many transcripts made equal shares take 1.6 to 5.4 ms -- and
    //  a writer thread that puts the chunks out in order while the later ones are still being formatted)
    const size_t n_rows = std::min(rows.size(), first_bad);
    const size_t T = n_rows < 4096 ? 1 : 4 * usable_threads(16);
    struct Chunk { std::string tsv, bed; bool ok = true; std::atomic<int> ready{0}; };
    std::vector<Chunk> chunks(T);
    const bool want_bed = fj != nullptr;
    std::vector<double> task_ms(T, 0);
    auto format = [&](size_t t) {
        Chunk &ck = chunks[t];
        const double t_task = trace ? now_ms() : 0;
        struct Stamp { double &slot; double t0; bool on; ~Stamp() { if (on) slot = now_ms() - t0; } } stamp{task_ms[t], t_task, trace};
        // (whatever the task ends in: the writer waits for every chunk in turn)
        struct Ready { Chunk &ck; ~Ready() { ck.ready.store(1, std::memory_order_release); } } ready{ck};
        try {
            const size_t i0 = n_rows * t / T, i1 = n_rows * (t + 1) / T;
            ck.tsv.reserve((i1 - i0) * 224);
            if (want_bed) ck.bed.reserve((i1 - i0) * 96);
            std::string name, score;
            for (size_t i = i0; i < i1; ++i) {
                // (a row names a handful of transcripts anywhere in three 8 MB string tables: their lines are asked for a few rows ahead --
                //  the formatting was bound by those misses, not by the text)
                if (i + 6 < i1) for (uint32_t k = A.tx_off[i + 6]; k < A.tx_off[i + 7]; ++k) {
                    const uint32_t t2 = A.tx[k];
                    __builtin_prefetch(&g->m.tx_gene_name[t2]); __builtin_prefetch(&g->m.tx_gene_id[t2]); __builtin_prefetch(&g->m.tx_id[t2]);
                }
                const JTable::Row &r = rows[i];
                const std::string &chrom = uj.chrom_name[r.crank];
                const uint32_t js = r.js, jend = r.jend, je = jend + 1;
                const JEntry &e = r.e;
                { char nb[32]; snprintf(nb, sizeof nb, "JUNC%08zu", i + 1); name = nb; }
                if (want_bed) {
                    std::string &b = ck.bed;
                    b += chrom; b += '\t'; put_u(b, e.ts); b += '\t'; put_u(b, e.te); b += '\t'; b += name; b += '\t'; put_u(b, e.count); b += '\t';
                        b += e.strand; b += '\t';
                    put_u(b, e.ts); b += '\t'; put_u(b, e.te); b += '\t'; b += e.color; b += '\t'; put_i(b, e.nblocks); b += '\t';
                    put_u(b, (uint32_t)(js - e.ts)); b += ','; put_u(b, (uint32_t)(e.te - jend)); b += "\t0,"; put_u(b, (uint32_t)(jend - e.ts)); b += '\n';
                }
                score.clear(); put_u(score, e.count);
                append_junction_row(ck.tsv, g, A, i, chrom, js, je, name, score, e.strand, sites[i]);
                ck.tsv += '\t';
                for (uint32_t k = r.v0; k < r.v1; ++k) {                                // variant_set_to_string
                    if (k != r.v0) ck.tsv += ',';
                    ck.tsv += uj.vchrom_name[uj.vars[k].first]; ck.tsv += ':'; put_i(ck.tsv, (int)uj.vars[k].second); ck.tsv += '-'; put_i(ck.tsv,
                        (int)(uj.vars[k].second + 1));
                }
                ck.tsv += '\n';
            }
        } catch (...) { ck.ok = false; }
    };
    std::atomic<bool> mem_bad{false};
    std::thread writer;
    if (T > 1) writer = std::thread([&] {
        for (Chunk &ck : chunks) {
            while (!ck.ready.load(std::memory_order_acquire)) std::this_thread::sleep_for(std::chrono::microseconds(50));
            if (!ck.ok) { mem_bad.store(true); return; }            // (what was written stays; the call fails)
            if (!ck.tsv.empty()) fwrite(ck.tsv.data(), 1, ck.tsv.size(), fo);
            if (fj && !ck.bed.empty()) fwrite(ck.bed.data(), 1, ck.bed.size(), fj);
            std::string().swap(ck.tsv); std::string().swap(ck.bed);
        }
    });
    JoinThread join_writer{writer};
    run_tasks(T, format);
    if (trace) { double lo = 1e9, hi = 0, sum = 0; for (double v : task_ms) { lo = std::min(lo, v); hi = std::max(hi, v); sum += v; } fprintf(stderr,
        "[rgx trace] outputs: %zu format tasks: min %.3f avg %.3f max %.3f ms\n", T, lo, sum / (double)T, hi); }
    lap("rows formatted");
    bool mem_ok = true;
    if (writer.joinable()) { writer.join(); mem_ok = !mem_bad.load(); }
    else {
        for (const Chunk &ck : chunks) if (!ck.ok) mem_ok = false;
        if (mem_ok) for (Chunk &ck : chunks) { if (!ck.tsv.empty()) fwrite(ck.tsv.data(), 1, ck.tsv.size(), fo); if (fj &&
            !ck.bed.empty()) fwrite(ck.bed.data(), 1, ck.bed.size(), fj); }
    }
    if (!mem_ok) { if (fo != stdout) fclose(fo); if (fj) fclose(fj); return fail(err, errlen, RGX_ERR_OPEN, "regtools_amd: no memory for the output rows\n"); }
    if (first_bad != SIZE_MAX) { if (fo != stdout) fclose(fo); if (fj) fclose(fj); return fail(err, errlen, RGX_ERR_FASTA, "%s", bad_msg); }
    if (fo != stdout) fclose(fo);
    if (fj) fclose(fj);
    lap("rows");
    if (trace) teardown.t = now_ms();
    return RGX_OK;
}

// ---- `junctions annotate` (junctions_main.cc:62-93) --------------------------------------------------------------------------------
extern "C" int rgx_junctions_annotate(rgx_ctx *c, const char *bed_path, const char *fasta_path, const char *gtf_path, const char *out_path, uint64_t *n_rows,
                                      char *err, size_t errlen) {
    return rgx_junctions_annotate_opts(c, bed_path, fasta_path, gtf_path, out_path, 0, n_rows, err, errlen);
}
// include_single_exon: -S (junctions_annotator.cc:392-393: skip_single_exon_genes_ = false)
extern "C" int rgx_junctions_annotate_opts(rgx_ctx *c, const char *bed_path, const char *fasta_path, const char *gtf_path, const char *out_path,
                                           int options, uint64_t *n_rows, char *err, size_t errlen) {
    const int include_single_exon = options & RGX_ANNOTATE_SINGLE_EXON;
    const bool echo = (options & RGX_ANNOTATE_ECHO) != 0;
    if (!c || !bed_path || !fasta_path || !gtf_path) return fail(err, errlen, RGX_ERR_ARG, "Error parsing inputs!(2)\n\n");
    rgx_gtf *g = nullptr;
    int rc = rgx_gtf_load(c, gtf_path, &g, err, errlen);
    if (rc != RGX_OK) return rc;
    GtfGuard guard(g);
    FILE *fo = out_path ? fopen(out_path, "w") : stdout;
    if (!fo) return fail(err, errlen, RGX_ERR_OPEN, "Unable to open %s", out_path);
    fprintf(fo, "%s\n", kJunctionHeader);
    BedJunctions B;
    const std::string bed_err = B.load(bed_path);                 // rows before a bad line are still annotated and printed, as upstream
    const Fasta *fap = host_fasta(c, fasta_path);
    const bool have_fa = fap != nullptr;
    const size_t n = B.n();
    std::vector<int32_t> jc(n); std::vector<uint8_t> jst(n);
    for (size_t i = 0; i < n; ++i) { jc[i] = g->m.chrom_of(B.chrom[i]); jst[i] = B.strand[i].size() == 1 ? (uint8_t)B.strand[i][0] : (uint8_t)'?'; }
    JunctionAnnotHost A;
    rc = annotate_junctions(c, g, jc, B.start, B.end, jst, A, err, errlen, nullptr, include_single_exon != 0);
    size_t done = 0;
    for (size_t i = 0; i < n && rc == RGX_OK; ++i) {
        std::string site;
        std::string said;
        if (!have_fa) { rc = fail(err, errlen, RGX_ERR_FASTA, "Unable to extract FASTA sequence for position %s:%u-%u\n\n", B.chrom[i].c_str(),
            B.start[i] + 1, B.start[i] + 2); if (echo) { append_positions(said, B.chrom[i], B.start[i], B.end[i], false); fputs(said.c_str(), stderr);
                } break; }
        rc = splice_site(*fap, B.chrom[i], B.start[i], B.end[i], B.strand[i], site, err, errlen);
        if (echo) {
            std::string tmp;
            append_positions(said, B.chrom[i], B.start[i], B.end[i], rc == RGX_OK || fap->fetch(B.chrom[i], (int64_t)B.start[i] + 1, (int64_t)B.start[i] + 2,
                tmp));
            fputs(said.c_str(), stderr);
        }
        if (rc != RGX_OK) break;
        print_junction_row(fo, g, A, i, B.chrom[i], B.start[i], B.end[i], B.name[i], B.score[i], B.strand[i], site);
        fputc('\n', fo);
        ++done;
    }
    if (fo != stdout) fclose(fo);
    if (n_rows) *n_rows = done;
    if (rc == RGX_OK && !bed_err.empty()) return fail(err, errlen, RGX_ERR_FORMAT, "%s", bed_err.c_str());
    return rc;
}
