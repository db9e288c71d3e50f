// regtools_main.cpp -- host CLI in front of libregtools_amd.so: `regtools-amd junctions extract ...`.
//
// Keeps the reference's sub-command surface for the accelerated path: same flags, defaults, stderr echo and exit
// codes as /root/reference/src/junctions/junctions_extractor.cc:42-143 (parse_options/usage),
// src/junctions/junctions_main.cc:45-107 (dispatch, exception -> exit code) and src/regtools.cc:36-74
// (banner, top-level usage).  Everything data-parallel happens behind the C ABI (include/regtools_amd.h).
#include <errno.h>
#include <getopt.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <time.h>
#include <unistd.h>

#include <algorithm>
#include <iostream>
#include <sstream>
#include <stdexcept>
#include <string>
#include <memory>
#include <vector>

#include "regtools_amd.h"

namespace {

// An empty line in a GTF: upstream's loader calls line.at(0) on it outside any try block (gtf_parser.cc:230), the std::out_of_range is nobody's to catch,
// the process prints libstdc++'s terminate message and aborts (status 134).  The library reports the line as an error; the tool then does what upstream
// does -- the same call, uncaught (the handlers around it take std::runtime_error only) -- so the message and the status are the reference's.
// (`cis-splice-effects identify / associate` catch std::exception around everything, cis_splice_effects_main.cc:35-51, :55-71 (std::logic_error): there the
// same exception's
// what() is the message and the status is 1 -- caught = true)
void die_as_upstream_on_empty_gtf_line(const char *err, bool caught = false) {
    if (strcmp(err, "basic_string::at")) return;
    if (!caught) { std::cerr.flush(); fflush(nullptr); (void)std::string().at(0); }
    try { (void)std::string().at(0); } catch (const std::out_of_range &e) { throw std::runtime_error(e.what()); }
}

// htslib ends the process itself on two kinds of VCF record (vcf.c:1610-1614 exit(1); :1638-1639 abort()), past every handler of the tool: the
// library reports them (RGX_ERR_EXIT / RGX_ERR_ABORT with what htslib printed) and the tool goes the same way.
void die_where_upstreams_library_does(int rc, const char *err) {
    if (rc != RGX_ERR_EXIT && rc != RGX_ERR_ABORT) return;
    // (what htslib printed; the library's own words -- a read whose aux fields bam_aux_get abort()s on, sam.c:1233-1252 -- are not upstream's: nothing is
    // printed there)
    std::cerr.flush(); if (strncmp(err, "regtools_amd:", 13)) fputs(err, stderr); fflush(nullptr);
    if (rc == RGX_ERR_ABORT) abort();
    exit(1);
}

struct HelpRequested { std::string text; };

struct ExtractOptions {
    std::string bam = "NA", ref = "NA", output = "NA", barcodes = "NA", region = ".", tag = "XS";
    uint32_t min_anchor = 8, min_intron = 70, max_intron = 500000;
    int strandness = -1;
    int device = 0;
};

void extract_usage(std::ostream &out) {
    out << "Usage:\t\tregtools junctions extract [options] indexed_alignments.bam\n"
        << "Options:\n"
        << "\t\t-a INT\tMinimum anchor length. Junctions which satisfy a minimum \n\t\t\t anchor length on both sides are reported. [8]\n"
        << "\t\t-m INT\tMinimum intron length. [70]\n"
        << "\t\t-M INT\tMaximum intron length. [500000]\n"
        << "\t\t-o FILE\tThe file to write output to. [STDOUT]\n"
        << "\t\t-r STR\tThe region to identify junctions \n\t\t\t in \"chr:start-end\" format. Entire BAM by default.\n"
        << "\t\t-s INT\tStrandness mode \n\t\t\t XS, use XS tags provided by aligner; RF, first-strand; FR, second-strand. REQUIRED\n"
        << "\t\t-t STR\tTag used in bam to label strand. [XS]\n"
        << "\t\t-b STR\tThe file containing the barcodes of interest for single cell data.\n\n";
}

// junctions_extractor.cc:42-122
ExtractOptions parse_extract(int argc, char **argv) {
    ExtractOptions o;
    optind = 1;
    int c;
    while ((c = getopt(argc, argv, "ha:m:M:o:r:t:s:b:")) != -1) {
        switch (c) {
            case 'h': { std::ostringstream ss; extract_usage(ss); throw HelpRequested{ss.str()}; }
            case 'a': o.min_anchor = (uint32_t)atoi(optarg); break;
            case 'm': o.min_intron = (uint32_t)atoi(optarg); break;
            case 'M': o.max_intron = (uint32_t)atoi(optarg); break;
            case 'o': o.output = optarg; break;
            case 'r': o.region = optarg; break;
            case 't': o.tag = optarg; break;
            case 's': {
                std::string s = optarg;
                if (s == "XS") o.strandness = 0; else if (s == "RF") o.strandness = 1; else if (s == "FR") o.strandness = 2;
                else if (s == "intron-motif") o.strandness = 3;
                else throw std::runtime_error("Unrecognized strandness argument!\n\n");
                break;
            }
            case 'b': o.barcodes = optarg; break;
            default: extract_usage(std::cerr); throw std::runtime_error("Error parsing inputs!(1)\n\n");
        }
    }
    if (argc - optind >= 1) o.bam = argv[optind++];
    if (argc - optind >= 1) o.ref = argv[optind++];
    if (optind < argc || o.bam == "NA") { extract_usage(std::cerr); throw std::runtime_error("Error parsing inputs!(2)\n\n"); }
    if (o.strandness == -1) { extract_usage(std::cerr); throw std::runtime_error("Please supply strandness mode with '-s' option!\n\n"); }
    if (o.strandness == 3 && o.ref == "NA") { extract_usage(std::cerr); throw std::runtime_error("Strandness mode 'intron-motif' requires a fasta file!\n\n"); }
    std::cerr << "Minimum junction anchor length: " << o.min_anchor << "\nMinimum intron length: " << o.min_intron
              << "\nMaximum intron length: " << o.max_intron << "\nAlignment: " << o.bam << "\nOutput file: " << o.output << "\n";
    if (o.barcodes != "NA") std::cerr << "Barcode file: " << o.barcodes << "\n";
    std::cerr << std::endl;
    return o;
}

// junctions_main.cc:45-59
double wall_ms() { struct timespec ts; clock_gettime(CLOCK_MONOTONIC, &ts); return ts.tv_sec * 1e3 + ts.tv_nsec * 1e-6; }

int junctions_extract(int argc, char **argv) {
    try {
        const double t_start = wall_ms();
        ExtractOptions o = parse_extract(argc, argv);
        char err[512] = {0};
        rgx_ctx *ctx = nullptr;
        if (const char *d = getenv("REGTOOLS_AMD_DEVICE")) o.device = atoi(d);
        // REGTOOLS_AMD_DEVICES=0,1,2,...: the file is sharded over these GPUs (rgx_extract_multi: a host thread per device, one RCCL
        // all-gather of the shards' rows, merge on the first); the output does not depend on the list
        std::vector<int> devices;
        if (const char *d = getenv("REGTOOLS_AMD_DEVICES")) {
            for (const char *q = d; *q;) { char *e; long v = strtol(q, &e, 10); if (e == q) break; devices.push_back((int)v); q = *e == ',' ? e + 1 : e;
                if (*e && *e != ',') break; }
        }
        if (devices.size() == 1) o.device = devices[0];
        if (devices.size() <= 1 && rgx_ctx_create(o.device, &ctx, err, sizeof err) != RGX_OK) throw std::runtime_error(err);
        const double t_ctx = wall_ms();
        rgx_extract_params p;
        rgx_extract_params_default(&p);
        p.region = o.region.c_str(); p.strandness = o.strandness;
        p.strand_tag[0] = o.tag.size() > 0 ? o.tag[0] : 0; p.strand_tag[1] = o.tag.size() > 1 ? o.tag[1] : 0;
        p.min_anchor = o.min_anchor; p.min_intron = o.min_intron; p.max_intron = o.max_intron;
        p.fasta_path = o.ref == "NA" ? nullptr : o.ref.c_str();
        p.barcodes = o.barcodes != "NA";                                   // -b (junctions_extractor.cc:82-84, :393-395)
        rgx_junction_table *t = nullptr;
        int rc = devices.size() > 1 ? rgx_extract_multi(devices.data(), (int)devices.size(), o.bam.c_str(), &p, &t, err, sizeof err)
                                    : rgx_extract(ctx, o.bam.c_str(), &p, &t, err, sizeof err);
        // (an aux field of unknown type in front of a spliced read's strand tag: upstream's bam_aux_get abort()s, sam.c:1248 -- nothing printed, SIGABRT)
        if (rc == RGX_ERR_ABORT) { std::cerr.flush(); fflush(nullptr); abort(); }
        if (rc != RGX_OK) { if (ctx) rgx_ctx_destroy(ctx); throw std::runtime_error(err); }
        const double t_extract = wall_ms();
        // one formatting pass: a row is a contig name + at most 160 bytes of numbers (Junction::print, junctions_extractor.h:90-98)
        size_t max_name = 0;
        for (int32_t i = 0; i < t->n_ref; ++i) max_name = std::max(max_name, strlen(t->ref_name[i]));
        // (uninitialised on purpose: a zero-filled vector of that size -- 51 MB for 300 k rows, of which 30 are written -- was 10 of the process's 250 ms)
        size_t text_cap = (size_t)t->n * (max_name + 160) + 1;
        std::unique_ptr<char[]> text(new char[text_cap]);
        size_t n = rgx_table_format_bed12(t, 1, text.get(), text_cap);
        if (n > text_cap) { text_cap = n + 1; text.reset(new char[text_cap]); n = rgx_table_format_bed12(t, 1, text.get(), text_cap); }
        const double t_format = wall_ms();
        FILE *f = o.output == "NA" ? stdout : fopen(o.output.c_str(), "w");
        // (an output file that cannot be opened is skipped as upstream's ofstream would; a write that comes up SHORT -- full disk, closed pipe --
        //  is an error here: the process ends with _exit below, nothing later could report it)
        bool short_write = false;
        if (f) { short_write = fwrite(text.get(), 1, n, f) != n; if (f != stdout) short_write |= fclose(f) != 0; else short_write |= fflush(f) != 0; }
        const double t_write = wall_ms();
        if (p.barcodes) {                                                  // print_all_junctions: an unopenable file is skipped silently (cc:255-256, :272)
            if (FILE *b = fopen(o.barcodes.c_str(), "w")) {
                const size_t nb = rgx_table_format_barcodes(t, 1, nullptr, 0);
                std::vector<char> bt(nb + 1);
                rgx_table_format_barcodes(t, 1, bt.data(), nb);
                short_write |= fwrite(bt.data(), 1, nb, b) != nb; short_write |= fclose(b) != 0;
            }
        }
        if (short_write) { fprintf(stderr, "regtools-amd: writing the output failed (%s)\n", strerror(errno)); fflush(stderr); _exit(1); }
        if (getenv("REGTOOLS_AMD_STATS"))
            fprintf(stderr, "[regtools_amd] records=%llu events=%llu junctions=%llu inflate=%.3fms records=%.3fms scan=%.3fms reduce=%.3fms total=%.3fms\n",
                    (unsigned long long)t->n_records, (unsigned long long)t->n_events, (unsigned long long)t->n, t->ms_inflate, t->ms_records,
                    t->ms_scan, t->ms_reduce, t->ms_total),
            fprintf(stderr, "[regtools_amd] process: options %.1f ms, context %.1f ms, extract %.1f ms (pipeline %.1f), format %.1f ms, write %.1f ms\n",
                    0.0, t_ctx - t_start, t_extract - t_ctx, t->ms_total, t_format - t_extract, t_write - t_format);
        // the outputs are on disk: leave without handing gigabytes of device memory back one buffer at a time and without the runtime's
        // orderly shutdown (both happen anyway when the process ends; ~0.1 s of a 0.3 s run)
        fflush(stdout); fflush(stderr);
        _exit(0);
    } catch (const HelpRequested &h) {
        std::cerr << h.text << std::endl;
        return 0;
    } catch (const std::runtime_error &e) {
        std::cerr << e.what() << std::endl;
        return 1;
    }
    return 0;
}

// ---- junctions annotate (junctions_annotator.cc:385-437, junctions_main.cc:62-93) ------------------------------------------------
void annotate_usage(std::ostream &out) {
    out << "Usage:\t\tregtools junctions annotate [options] junctions.bed ref.fa annotations.gtf\n"
        << "Options:\t-S include single exon genes\n"
        << "\t\t-o FILE\tThe file to write output to. [STDOUT]\n\n";
}

rgx_ctx *open_ctx() {
    char err[512] = {0};
    rgx_ctx *ctx = nullptr;
    int dev = 0; if (const char *d = getenv("REGTOOLS_AMD_DEVICE")) dev = atoi(d);
    if (rgx_ctx_create(dev, &ctx, err, sizeof err) != RGX_OK) throw std::runtime_error(err);
    return ctx;
}

int junctions_annotate(int argc, char **argv) {
    try {
        std::string out = "NA";
        bool skip_single = true;
        optind = 1;
        int c;
        while ((c = getopt(argc, argv, "So:h")) != -1) {
            switch (c) {
                case 'S': skip_single = false; break;
                case 'o': out = optarg; break;
                case 'h': { std::ostringstream ss; annotate_usage(ss); throw HelpRequested{ss.str()}; }
                default: annotate_usage(std::cerr); throw std::runtime_error("Error parsing inputs!(1)\n\n");
            }
        }
        std::string bed, ref = "NA", gtf;
        if (argc - optind >= 3) { bed = argv[optind++]; ref = argv[optind++]; gtf = argv[optind++]; }
        if (optind < argc || ref == "NA" || bed.empty() || gtf.empty()) { annotate_usage(std::cerr); throw std::runtime_error("Error parsing inputs!(2)\n\n"); }
        std::cerr << "Reference: " << ref << "\nGTF: " << gtf << "\nJunctions: " << bed << "\n" << (skip_single ? "Skipping single exon genes.\n" : "");
        if (out != "NA") std::cerr << "Output file: " << out << "\n";
        std::cerr << "\n";
        rgx_ctx *ctx = open_ctx();
        char err[512] = {0};
        uint64_t n = 0;
        int rc = rgx_junctions_annotate_opts(ctx, bed.c_str(), ref.c_str(), gtf.c_str(), out == "NA" ? nullptr : out.c_str(), (skip_single ? 0 :
            RGX_ANNOTATE_SINGLE_EXON) | RGX_ANNOTATE_ECHO, &n, err, sizeof err);
        rgx_ctx_destroy(ctx);
        if (rc != RGX_OK) { die_as_upstream_on_empty_gtf_line(err); throw std::runtime_error(err); }
        std::cerr << "\nAnnotated " << n << " lines.\n";
    } catch (const HelpRequested &h) {
        std::cerr << h.text << std::endl;
        return 0;
    } catch (const std::runtime_error &e) {
        std::cerr << e.what() << std::endl;
        return 1;
    }
    return 0;
}

// ---- junctions cohort: many BAMs -> one junction-by-sample table.  The reference has no such command (a cohort run there is the loop around
// `junctions extract`, junctions_main.cc:45-59, and a script); it is not listed in the usage texts the reference pins. --------------------------------
void cohort_usage(std::ostream &out) {
    out << "Usage:\t\tregtools-amd junctions cohort [options] -s STRANDNESS [-L list.txt] [a.bam b.bam ...]\n"
        << "\t\tThe union of the samples' junctions (the lines of each sample's `junctions extract`) with one read-count column per sample.\n"
        << "Options:\n"
        << "\t\t-a INT\tMinimum anchor length, as in extract. [8]\n"
        << "\t\t-m INT\tMinimum intron length. [70]\n"
        << "\t\t-M INT\tMaximum intron length. [500000]\n"
        << "\t\t-r STR\tThe region to identify junctions in, as in extract. Entire BAM by default.\n"
        << "\t\t-s INT\tStrandness mode: XS, RF, FR. REQUIRED\n"
        << "\t\t-t STR\tTag used in bam to label strand. [XS]\n"
        << "\t\t-o FILE\tThe cohort's junctions as BED12; the score is the summed read count. [STDOUT]\n"
        << "\t\t-c FILE\tThe counts table: chrom, start, end, strand and one column per sample.\n"
        << "\t\t-k FILE\tThe cluster counts: junctions linked through a shared start or end, <reads on the junction>/<reads on its cluster>\n"
        << "\t\t\t per sample, laid out as LeafCutter's perind.counts.\n"
        << "\t\t-K INT\tKeep clusters of at least INT junctions. [1]\n"
        << "\t\t-T INT\tKeep clusters with at least INT reads over all samples. [0]\n"
        << "\t\t-l INT\tThe longest intron that takes part in clustering. [0: no limit]\n"
        << "\t\t-J INT\tJunctions with fewer than INT reads over all samples are removed from their cluster. [0]\n"
        << "\t\t-p DEC\tJunctions that carry less than this share of their cluster's reads are removed; a decimal in [0, 1] with at most\n"
        << "\t\t\t nine digits behind the point, read exactly. [0]\n"
        << "\t\t\t With -l, -J or -p the clusters are refined: those junctions leave and the rest is clustered again, as LeafCutter does\n"
        << "\t\t\t (its customary settings: -l 100000 -J 5 -p 0.001 -K 2 -T 30).\n"
        << "\t\t-q FILE\tThe phenotype table for sQTL mapping: per clustered junction and sample the intron-excision ratio, standardised\n"
        << "\t\t\t across samples and rank-normalised across junctions, modelled on LeafCutter's prepare_phenotype_table.py.\n"
        << "\t\t\t The clusters are those -k writes with the same -K, -T, -l, -J and -p, whether or not -k is given.\n"
        << "\t\t-x DEC\tJunctions whose cluster has no reads in more than this share of the samples are left out of -q; a decimal as -p. [0.4]\n"
        << "\t\t-d DEC\tJunctions whose ratio varies by less than this standard deviation are left out of -q. [0.005]\n"
        << "\t\t-P FILE\tThe principal components of the -q table, the covariates of an sQTL run, laid out as LeafCutter's .PCs file: one line\n"
        << "\t\t\t per component, one column per sample. The table is computed as for -q, whether or not -q is given.\n"
        << "\t\t-C INT\tThe number of components -P writes, at most the table's rows and the samples. [10]\n"
        << "\t\t-g FILE\tThe samples' genotypes for -Q: a VCF (plain, gzip, bgzip) or a BCF whose sample names are the cohort's. The dosage is the\n"
        << "\t\t\t number of non-reference alleles of a diploid GT call of a biallelic record.\n"
        << "\t\t-Q FILE\tThe nominal cis-sQTL scan: every row of the -q table against every variant of -g within the window around its intron,\n"
        << "\t\t\t with an intercept and the first -C components (at most the samples less three) in the model: one line per pair with\n"
        << "\t\t\t r, slope, its standard error, t and the two-sided p. The table and the components are computed as for -q and -P.\n"
        << "\t\t-w INT\tThe cis window of -Q, -R, -G and -I on either side of the intron. [100000]\n"
        << "\t\t-R FILE\tThe permutation pass of the cis-sQTL scan: one line per row of the -q table that has variants of -g in its window, with its\n"
        << "\t\t\t best variant, the empirical p of that variant's |r| among -B permutations of the samples and its beta approximation.\n"
        << "\t\t\t Needs -g; the table, the components and the window are those of -Q, beside which it may stand.\n"
        << "\t\t-G FILE\tThe grouped permutation pass: one line per cluster of the -q table whose introns have variants of -g in their windows, with\n"
        << "\t\t\t the cluster's best (intron, variant) and the empirical p and beta approximation of the largest |r| over ALL its introns.\n"
        << "\t\t\t Needs -g; everything else as for -R, beside which (and beside -Q) it may stand.\n"
        << "\t\t-I FILE\tThe conditionally independent signals: every row of the -q table whose corrected p of -R is at most -F is searched for\n"
        << "\t\t\t further variants of its window that act beside those already found, forward and then backward: one line per signal, -R's\n"
        << "\t\t\t columns, then its rank and the number of variants it is conditioned on. Needs -g; everything else as for -R.\n"
        << "\t\t-F FLOAT\tThe threshold of -I on the beta-approximated p, above 0 and at most 1. [0.05]\n"
        << "\t\t-B INT\tThe permutations of -R, -G and -I, 1 to 65535. [1000]\n"
        << "\t\t-e INT\tThe seed of -R's, -G's and -I's permutations. [0]\n"
        << "\t\t-X FILE\tThe trans-sQTL scan: every row of the -q table against EVERY variant of -g, with the model of -Q: one line per pair whose\n"
        << "\t\t\t two-sided p is at most -u, with r, slope, its standard error, t and p. Needs -g; the table and the components are those of -Q.\n"
        << "\t\t-u FLOAT\tThe p-value threshold of -X, above 0 and at most 1. [1e-5]\n"
        << "\t\t-W INT\tLeave out of -X the variants within this distance of the row's intron; 'off' keeps them. [5000000]\n"
        << "\t\t-A\tTake every junction of a sample, not only those anchored on both sides.\n"
        << "\t\t-n INT\tKeep junctions seen in at least INT samples. [1]\n"
        << "\t\t-N INT\tKeep junctions with at least INT reads over all samples. [1]\n"
        << "\t\t-L FILE\tOne BAM path per line, optionally a tab and the sample's name.\n"
        << "\t\t\t A sample's name is its file's base name without .bam unless the list gives one; names must differ.\n\n";
}

struct CohortInput { std::string path, name; };

// -p: "digits[.digits]" read exactly as num / 10^k, k <= 9, value in [0, 1]
bool cohort_parse_ratio(const char *arg, uint32_t *num, uint32_t *den) {
    const std::string s = arg;
    const size_t dot = s.find('.');
    const std::string whole = s.substr(0, dot), frac = dot == std::string::npos ? "" : s.substr(dot + 1);
    if (whole.empty() && frac.empty()) return false;
    if (whole.size() > 9 || frac.size() > 9) return false;
    for (char ch : whole + frac) if (ch < '0' || ch > '9') return false;
    uint64_t d = 1, v = 0;
    for (char ch : whole) v = v * 10 + (uint64_t)(ch - '0');
    for (char ch : frac) { v = v * 10 + (uint64_t)(ch - '0'); d *= 10; }
    if (v > d) return false;
    *num = (uint32_t)v; *den = (uint32_t)d;
    return true;
}

std::string cohort_default_name(const std::string &path) {
    std::string b = path.substr(path.find_last_of('/') == std::string::npos ? 0 : path.find_last_of('/') + 1);
    if (b.size() > 4 && b.compare(b.size() - 4, 4, ".bam") == 0) b.resize(b.size() - 4);
    return b;
}

// a whole file into page-locked memory (rgx_host_alloc): the form under which a pipeline's upload overlaps the inflate
bool cohort_read_pinned(const std::string &path, void **out, size_t *len) {
    FILE *f = fopen(path.c_str(), "rb");
    if (!f) return false;
    bool ok = fseek(f, 0, SEEK_END) == 0;
    const long n = ok ? ftell(f) : -1;
    ok = ok && n >= 0 && fseek(f, 0, SEEK_SET) == 0;
    void *p = ok ? rgx_host_alloc((size_t)n + 64) : nullptr;
    ok = ok && p && (n == 0 || fread(p, 1, (size_t)n, f) == (size_t)n);
    fclose(f);
    if (!ok) { if (p) rgx_host_free(p); return false; }
    *out = p; *len = (size_t)n;
    return true;
}

// hts_idx_load's order (hts.c:2031-2042): <fn>.csi, <stem>.csi, <fn>.bai, <stem>.bai
bool cohort_read_index(const std::string &bam, std::vector<char> &out) {
    const size_t dot = bam.find_last_of('.');
    const std::string stem = dot == std::string::npos || dot == 0 ? bam : bam.substr(0, dot);
    for (const std::string &cand : {bam + ".csi", stem + ".csi", bam + ".bai", stem + ".bai"}) {
        FILE *f = fopen(cand.c_str(), "rb");
        if (!f) continue;
        out.clear();
        char chunk[1 << 16]; size_t k;
        while ((k = fread(chunk, 1, sizeof chunk, f)) > 0) out.insert(out.end(), chunk, chunk + k);
        fclose(f);
        return true;
    }
    return false;
}

int junctions_cohort(int argc, char **argv) {
    try {
        ExtractOptions o;
        std::string counts = "NA", clusters = "NA", phenotypes = "NA", components = "NA", genotypes = "NA", qtl = "NA", perm = "NA", grouped = "NA";
        uint32_t n_components = 10, window = 100000, n_perm = 1000;
        uint64_t seed = 0;
        std::string trans = "NA", indep = "NA";
        double trans_pval = 1e-5, indep_pval = 0.05;
        bool trans_exclude = true;
        uint32_t trans_window = 5000000;
        rgx_pheno_params qp;
        rgx_pheno_params_default(&qp);
        rgx_cohort_params cp;
        rgx_cohort_params_default(&cp);
        rgx_cluster_params kp;
        rgx_cluster_params_default(&kp);
        rgx_refine_params rp;
        rgx_refine_params_default(&rp);
        bool refine = false;
        std::vector<CohortInput> in;
        optind = 1;
        int c;
        while ((c = getopt(argc, argv, "ha:m:M:r:s:t:o:c:An:N:L:k:K:T:l:J:p:q:x:d:P:C:g:Q:w:R:B:e:G:X:u:W:I:F:")) != -1) {
            switch (c) {
                case 'h': cohort_usage(std::cout); return 0;
                case 'a': o.min_anchor = (uint32_t)atoi(optarg); break;
                case 'm': o.min_intron = (uint32_t)atoi(optarg); break;
                case 'M': o.max_intron = (uint32_t)atoi(optarg); break;
                case 'r': o.region = optarg; break;
                case 't': o.tag = optarg; break;
                case 'o': o.output = optarg; break;
                case 'c': counts = optarg; break;
                case 'A': cp.only_anchored = 0; break;
                case 'n': cp.min_samples = (uint32_t)atoi(optarg); break;
                case 'N': cp.min_total = (uint64_t)atoll(optarg); break;
                case 'k': clusters = optarg; break;
                case 'K': kp.min_rows = (uint32_t)atoi(optarg); break;
                case 'T': kp.min_total = (uint64_t)atoll(optarg); break;
                case 'l': rp.max_intron = (uint32_t)atoi(optarg); refine = true; break;
                case 'J': rp.min_reads = (uint64_t)atoll(optarg); refine = true; break;
                case 'p':
                    if (!cohort_parse_ratio(optarg, &rp.ratio_num, &rp.ratio_den)) throw std::runtime_error("Unrecognized ratio argument!\n\n");
                    refine = true; break;
                case 'q': phenotypes = optarg; break;
                case 'P': components = optarg; break;
                case 'g': genotypes = optarg; break;
                case 'Q': qtl = optarg; break;
                case 'w': {
                    char *end = nullptr;
                    errno = 0;
                    const long long v = strtoll(optarg, &end, 10);
                    if (end == optarg || *end || errno || v < 0 || v > 0xffffffffll || optarg[0] == ' ' || optarg[0] == '+' || optarg[0] == '-')
                        throw std::runtime_error("Unrecognized window argument!\n\n");
                    window = (uint32_t)v;
                    break;
                }
                case 'R': perm = optarg; break;
                case 'G': grouped = optarg; break;
                case 'X': trans = optarg; break;
                case 'I': indep = optarg; break;
                case 'u': case 'F': {
                    char *end = nullptr;
                    double &pval = c == 'u' ? trans_pval : indep_pval;
                    pval = strtod(optarg, &end);
                    if (end == optarg || *end || !(pval > 0 && pval <= 1)) throw std::runtime_error("Unrecognized threshold argument!\n\n");
                    break;
                }
                case 'W': {
                    if (std::string(optarg) == "off") { trans_exclude = false; break; }
                    char *end = nullptr;
                    errno = 0;
                    const long long v = strtoll(optarg, &end, 10);
                    if (end == optarg || *end || errno || v < 0 || v > 0xffffffffll || optarg[0] == ' ' || optarg[0] == '+' || optarg[0] == '-')
                        throw std::runtime_error("Unrecognized exclusion argument!\n\n");
                    trans_exclude = true; trans_window = (uint32_t)v;
                    break;
                }
                case 'B': {
                    char *end = nullptr;
                    errno = 0;
                    const long long v = strtoll(optarg, &end, 10);
                    if (end == optarg || *end || errno || v < 1 || v > 65535 || optarg[0] == ' ' || optarg[0] == '+')
                        throw std::runtime_error("Unrecognized permutations argument!\n\n");
                    n_perm = (uint32_t)v;
                    break;
                }
                case 'e': {
                    char *end = nullptr;
                    errno = 0;
                    const unsigned long long v = strtoull(optarg, &end, 10);
                    if (end == optarg || *end || errno || optarg[0] == ' ' || optarg[0] == '+' || optarg[0] == '-')
                        throw std::runtime_error("Unrecognized seed argument!\n\n");
                    seed = v;
                    break;
                }
                case 'C': {
                    char *end = nullptr;
                    errno = 0;
                    const long long v = strtoll(optarg, &end, 10);
                    if (end == optarg || *end || errno || v < 1 || v > 0xffffffffll || optarg[0] == ' ' || optarg[0] == '+')
                        throw std::runtime_error("Unrecognized component count argument!\n\n");
                    n_components = (uint32_t)v;
                    break;
                }
                case 'x':
                    if (!cohort_parse_ratio(optarg, &qp.na_num, &qp.na_den)) throw std::runtime_error("Unrecognized ratio argument!\n\n");
                    break;
                case 'd': {
                    char *end = nullptr;
                    qp.min_sd = strtod(optarg, &end);
                    if (end == optarg || *end || !(qp.min_sd >= 0)) throw std::runtime_error("Unrecognized deviation argument!\n\n");
                    break;
                }
                case 's': {
                    std::string s = optarg;
                    if (s == "XS") o.strandness = 0; else if (s == "RF") o.strandness = 1; else if (s == "FR") o.strandness = 2;
                    else throw std::runtime_error("Unrecognized strandness argument!\n\n");
                    break;
                }
                case 'L': {
                    FILE *f = fopen(optarg, "r");
                    if (!f) { cohort_usage(std::cerr); throw std::runtime_error(std::string("Unable to read the list of BAM files ") + optarg + "\n\n"); }
                    char *line = nullptr; size_t cap = 0; ssize_t k;
                    while ((k = getline(&line, &cap, f)) >= 0) {
                        std::string s(line, (size_t)k);
                        while (!s.empty() && (s.back() == '\n' || s.back() == '\r')) s.pop_back();
                        if (s.empty()) continue;
                        const size_t tab = s.find('\t');
                        CohortInput ci; ci.path = s.substr(0, tab);
                        if (tab != std::string::npos) ci.name = s.substr(tab + 1);
                        in.push_back(ci);
                    }
                    free(line); fclose(f);
                    break;
                }
                default: cohort_usage(std::cerr); throw std::runtime_error("Error parsing inputs!(1)\n\n");
            }
        }
        for (; optind < argc; ++optind) { CohortInput ci; ci.path = argv[optind]; in.push_back(ci); }
        if (in.empty()) { cohort_usage(std::cerr); throw std::runtime_error("Error parsing inputs!(2)\n\n"); }
        if (o.strandness == -1) { cohort_usage(std::cerr); throw std::runtime_error("Please supply strandness mode with '-s' option!\n\n"); }
        if ((qtl != "NA" || perm != "NA" || grouped != "NA" || trans != "NA" || indep != "NA") && genotypes == "NA") { cohort_usage(std::cerr); throw std::runtime_error("Please supply the genotypes with '-g' option!\n\n"); }
        for (CohortInput &ci : in) if (ci.name.empty()) ci.name = cohort_default_name(ci.path);
        for (size_t a = 0; a < in.size(); ++a) for (size_t b = 0; b < a; ++b) if (in[a].name == in[b].name)
            throw std::runtime_error("Two samples are named " + in[a].name + " (" + in[b].path + ", " + in[a].path + "); name them in a list (-L)\n\n");

        char err[512] = {0};
        int device = 0; if (const char *d = getenv("REGTOOLS_AMD_DEVICE")) device = atoi(d);
        // two files in flight: file k + 1 goes up and inflates under file k's tail, on the runtime's default hardware queues
        rgx_pipeline *pl = nullptr;
        if (rgx_pipeline_create(device, 2, &pl, err, sizeof err) != RGX_OK) throw std::runtime_error(err);
        rgx_cohort *co = nullptr;
        if (rgx_cohort_create(rgx_pipeline_ctx(pl, 1), &cp, &co, err, sizeof err) != RGX_OK) { rgx_pipeline_destroy(pl); throw std::runtime_error(err); }
        rgx_extract_params p;
        rgx_extract_params_default(&p);
        p.region = o.region.c_str(); p.strandness = o.strandness;
        p.strand_tag[0] = o.tag.size() > 0 ? o.tag[0] : 0; p.strand_tag[1] = o.tag.size() > 1 ? o.tag[1] : 0;
        p.min_anchor = o.min_anchor; p.min_intron = o.min_intron; p.max_intron = o.max_intron;

        struct Flight { void *bam = nullptr; size_t bam_len = 0; std::vector<char> index; uint64_t ticket = 0; };
        std::vector<Flight> fl(in.size());
        std::string failure;
        auto submit = [&](size_t k) {
            if (!cohort_read_pinned(in[k].path, &fl[k].bam, &fl[k].bam_len)) {
                failure = "[E::hts_open_format] fail to open file '" + in[k].path + "'\nUnable to open BAM/SAM file.\n\n"; return false; }
            if (!cohort_read_index(in[k].path, fl[k].index)) { failure = "Unable to open BAM/SAM index. Make sure alignments are indexed\n\n"; return false; }
            if (rgx_extract_submit(pl, fl[k].bam, fl[k].bam_len, fl[k].index.data(), fl[k].index.size(), &p, &fl[k].ticket, err, sizeof err) != RGX_OK) {
                failure = err; return false; }
            return true;
        };
        size_t submitted = 0;
        bool ok = true;
        while (ok && submitted < std::min<size_t>(2, in.size())) ok = submit(submitted++);
        int rc_abort = RGX_OK;
        for (size_t k = 0; ok && k < in.size(); ++k) {
            rgx_junction_table *t = nullptr;
            int rc = rgx_extract_wait(pl, fl[k].ticket, &t, err, sizeof err);
            rgx_host_free(fl[k].bam); fl[k].bam = nullptr;       // (the wait is over: the pipeline no longer reads the file)
            if (rc == RGX_OK) rc = rgx_cohort_add(co, rgx_pipeline_ctx(pl, fl[k].ticket), t, o.min_anchor, in[k].name.c_str(), nullptr, err, sizeof err);
            if (t) rgx_table_free(t);
            if (rc != RGX_OK) { failure = err; rc_abort = rc; ok = false; break; }
            // file k is added: the context it ran on may take the next file (whose rows overwrite file k's in HBM)
            if (submitted < in.size()) ok = submit(submitted++);
        }
        rgx_cohort_matrix *m = nullptr;
        if (ok && rgx_cohort_finish(co, &m, err, sizeof err) != RGX_OK) { failure = err; ok = false; }
        rgx_cohort_clusters *cl = nullptr;                  // (straight behind the finish: the matrix is still in HBM)
        rp.min_rows = kp.min_rows; rp.min_total = kp.min_total;
        const bool want_qtl = qtl != "NA", want_perm = perm != "NA", want_group = grouped != "NA", want_trans = trans != "NA",
                   want_indep = indep != "NA", want_scan = want_qtl || want_perm || want_group || want_trans || want_indep;
        const bool want_pheno = phenotypes != "NA" || components != "NA" || want_scan;
        if (ok && (clusters != "NA" || want_pheno) && (refine ? rgx_cohort_refine(co, m, &rp, &cl, err, sizeof err) : rgx_cohort_cluster(co, m, &kp, &cl, err, sizeof err)) != RGX_OK) {
            failure = err; ok = false; }
        rgx_pheno_table *ph = nullptr;
        if (ok && want_pheno && rgx_cohort_phenotypes(co, m, cl, &qp, &ph, err, sizeof err) != RGX_OK) { failure = err; ok = false; }
        // -C clipped to the table; a table of fewer than two rows (or of no samples) has no components: the file is its header line
        rgx_pheno_pcs *pcs = nullptr;
        const uint32_t n_clip = ph && ph->n_rows >= 2 ? (uint32_t)std::min<uint64_t>({n_components, ph->n_rows, ph->n_samples}) : 0;
        const uint32_t n_pcs = components != "NA" ? n_clip : 0;
        // -Q and -R: the first n_cov components are the covariates -- those of -C further clipped to the samples less three -- of the same decomposition
        const uint32_t n_cov = want_scan && ph && ph->n_samples >= 3 ? std::min<uint32_t>(n_clip, ph->n_samples - 3) : 0;
        if (ok && std::max(n_pcs, n_cov) && rgx_cohort_pheno_pcs(co, ph, std::max(n_pcs, n_cov), &pcs, err, sizeof err) != RGX_OK) { failure = err; ok = false; }
        rgx_genotypes *gt = nullptr;
        if (ok && want_scan && rgx_genotypes_load(genotypes.c_str(), m, &gt, err, sizeof err) != RGX_OK) { failure = err; ok = false; }
        // a table without rows has no pairs: the file is its header line
        rgx_qtl_result *qr = nullptr;
        rgx_qtl_perm_result *pr = nullptr;
        rgx_qtl_group_result *gr = nullptr;
        rgx_qtl_trans_result *tr = nullptr;
        rgx_qtl_indep_result *ir = nullptr;
        if (ok && want_scan && ph->n_rows) {
            std::vector<rgx_qtl_region> regions((size_t)ph->n_rows);
            int rc = rgx_cohort_pheno_regions(m, ph, regions.data(), err, sizeof err);
            if (rc == RGX_OK && want_qtl) rc = rgx_cohort_qtl_nominal(co, ph, regions.data(), gt->n_variants, gt->tid, gt->pos, gt->dosage, n_cov,
                                                                      pcs ? pcs->component : nullptr, window, &qr, err, sizeof err);
            if (rc == RGX_OK && (want_perm || want_group || want_indep)) {
                std::vector<uint16_t> perms(((size_t)n_perm + 1) * ph->n_samples);
                rc = rgx_qtl_permutations(ph->n_samples, n_perm, seed, perms.data(), err, sizeof err);
                if (rc == RGX_OK && want_perm) rc = rgx_cohort_qtl_permute(co, ph, regions.data(), gt->n_variants, gt->tid, gt->pos, gt->dosage, n_cov,
                                                              pcs ? pcs->component : nullptr, window, n_perm, perms.data(), &pr, err, sizeof err);
                if (rc == RGX_OK && want_group) {
                    std::vector<uint32_t> group((size_t)ph->n_rows);
                    uint32_t n_groups = 0;
                    rc = rgx_cohort_pheno_groups(cl, ph, group.data(), &n_groups, err, sizeof err);
                    if (rc == RGX_OK) rc = rgx_cohort_qtl_permute_grouped(co, ph, regions.data(), gt->n_variants, gt->tid, gt->pos, gt->dosage, n_cov,
                                                                          pcs ? pcs->component : nullptr, window, n_perm, perms.data(), n_groups,
                                                                          group.data(), &gr, err, sizeof err);
                }
                if (rc == RGX_OK && want_indep) rc = rgx_cohort_qtl_independent(co, ph, regions.data(), gt->n_variants, gt->tid, gt->pos, gt->dosage,
                    n_cov, pcs ? pcs->component : nullptr, window, n_perm, perms.data(), indep_pval, RGX_QTL_MAX_COND, &ir, err, sizeof err);
            }
            // -X: the p-value threshold becomes the smallest |r| kept (too few samples for a degree of freedom: the call says so)
            if (rc == RGX_OK && want_trans) rc = rgx_cohort_qtl_trans(co, ph, regions.data(), gt->n_variants, gt->tid, gt->pos, gt->dosage, n_cov,
                pcs ? pcs->component : nullptr, ph->n_samples >= n_cov + 3 ? rgx_qtl_r_threshold(trans_pval, ph->n_samples - n_cov - 2) : 0.0,
                trans_exclude ? 1 : 0, trans_window, 0, &tr, err, sizeof err);
            if (rc != RGX_OK) { failure = err; ok = false; }
        }
        if (!ok) {
            rgx_cohort_qtl_indep_free(ir);
            rgx_cohort_qtl_trans_free(tr);
            rgx_cohort_qtl_group_free(gr);
            rgx_cohort_qtl_perm_free(pr);
            rgx_cohort_qtl_free(qr);
            rgx_genotypes_free(gt);
            rgx_cohort_pheno_pcs_free(pcs);
            if (ph) rgx_cohort_phenotypes_free(ph);
            if (cl) rgx_cohort_clusters_free(cl);
            if (m) rgx_cohort_matrix_free(m);
            rgx_pipeline_destroy(pl);                       // (runs what is still queued to its end: the buffers below were promised to it)
            for (Flight &f : fl) if (f.bam) rgx_host_free(f.bam);
            rgx_cohort_destroy(co);
            if (rc_abort == RGX_ERR_ABORT) { std::cerr.flush(); fflush(nullptr); abort(); }
            throw std::runtime_error(failure);
        }
        // the texts first, the files after: a failure above leaves no output behind
        const size_t nb = rgx_cohort_format_bed12(m, nullptr, 0);
        std::unique_ptr<char[]> bed(new char[nb + 1]);
        rgx_cohort_format_bed12(m, bed.get(), nb);
        size_t nc = 0; std::unique_ptr<char[]> tsv;
        if (counts != "NA") { nc = rgx_cohort_format_counts(m, nullptr, 0); tsv.reset(new char[nc + 1]); rgx_cohort_format_counts(m, tsv.get(), nc); }
        size_t nk = 0; std::unique_ptr<char[]> ktx;
        if (cl && clusters != "NA") { nk = rgx_cohort_format_cluster_counts(m, cl, nullptr, 0); ktx.reset(new char[nk + 1]); rgx_cohort_format_cluster_counts(m, cl, ktx.get(), nk); }
        size_t nq = 0; std::unique_ptr<char[]> qtx;
        if (ph && phenotypes != "NA") { nq = rgx_cohort_format_phenotypes(m, cl, ph, nullptr, 0); qtx.reset(new char[nq + 1]); rgx_cohort_format_phenotypes(m, cl, ph, qtx.get(), nq); }
        size_t np = 0; std::unique_ptr<char[]> ptx;
        if (components != "NA") {
            // (beside -Q with more covariates than -P has components this cannot be: n_cov <= n_clip = n_pcs)
            np = rgx_cohort_format_pheno_pcs(m, pcs, nullptr, 0); ptx.reset(new char[np + 1]); rgx_cohort_format_pheno_pcs(m, pcs, ptx.get(), np); }
        size_t nt = 0; std::unique_ptr<char[]> ttx;
        if (want_qtl) {
            nt = rgx_cohort_format_qtl(m, cl, ph, qr, gt->pos, gt->id, nullptr, 0); ttx.reset(new char[nt + 1]);
            rgx_cohort_format_qtl(m, cl, ph, qr, gt->pos, gt->id, ttx.get(), nt); }
        size_t nr = 0; std::unique_ptr<char[]> rtx;
        if (want_perm) {
            nr = rgx_cohort_format_qtl_perm(m, cl, ph, pr, gt->pos, gt->id, nullptr, 0); rtx.reset(new char[nr + 1]);
            rgx_cohort_format_qtl_perm(m, cl, ph, pr, gt->pos, gt->id, rtx.get(), nr); }
        size_t ng = 0; std::unique_ptr<char[]> gtx;
        if (want_group) {
            ng = rgx_cohort_format_qtl_group(m, cl, ph, gr, gt->pos, gt->id, nullptr, 0); gtx.reset(new char[ng + 1]);
            rgx_cohort_format_qtl_group(m, cl, ph, gr, gt->pos, gt->id, gtx.get(), ng); }
        size_t nx = 0; std::unique_ptr<char[]> xtx;
        if (want_trans) {
            nx = rgx_cohort_format_qtl_trans(m, cl, ph, tr, gt->pos, gt->id, nullptr, 0); xtx.reset(new char[nx + 1]);
            rgx_cohort_format_qtl_trans(m, cl, ph, tr, gt->pos, gt->id, xtx.get(), nx); }
        size_t ni = 0; std::unique_ptr<char[]> itx;
        if (want_indep) {
            ni = rgx_cohort_format_qtl_indep(m, cl, ph, ir, gt->pos, gt->id, nullptr, 0); itx.reset(new char[ni + 1]);
            rgx_cohort_format_qtl_indep(m, cl, ph, ir, gt->pos, gt->id, itx.get(), ni); }
        bool short_write = false;
        FILE *f = o.output == "NA" ? stdout : fopen(o.output.c_str(), "w");
        if (!f) throw std::runtime_error("Unable to write " + o.output + "\n\n");
        short_write = fwrite(bed.get(), 1, nb, f) != nb; if (f != stdout) short_write |= fclose(f) != 0; else short_write |= fflush(f) != 0;
        if (counts != "NA") {
            FILE *g = fopen(counts.c_str(), "w");
            if (!g) throw std::runtime_error("Unable to write " + counts + "\n\n");
            short_write |= fwrite(tsv.get(), 1, nc, g) != nc; short_write |= fclose(g) != 0;
        }
        if (cl && clusters != "NA") {
            FILE *g = fopen(clusters.c_str(), "w");
            if (!g) throw std::runtime_error("Unable to write " + clusters + "\n\n");
            short_write |= fwrite(ktx.get(), 1, nk, g) != nk; short_write |= fclose(g) != 0;
        }
        if (ph && phenotypes != "NA") {
            FILE *g = fopen(phenotypes.c_str(), "w");
            if (!g) throw std::runtime_error("Unable to write " + phenotypes + "\n\n");
            short_write |= fwrite(qtx.get(), 1, nq, g) != nq; short_write |= fclose(g) != 0;
        }
        if (components != "NA") {
            FILE *g = fopen(components.c_str(), "w");
            if (!g) throw std::runtime_error("Unable to write " + components + "\n\n");
            short_write |= fwrite(ptx.get(), 1, np, g) != np; short_write |= fclose(g) != 0;
        }
        if (want_qtl) {
            FILE *g = fopen(qtl.c_str(), "w");
            if (!g) throw std::runtime_error("Unable to write " + qtl + "\n\n");
            short_write |= fwrite(ttx.get(), 1, nt, g) != nt; short_write |= fclose(g) != 0;
        }
        if (want_perm) {
            FILE *g = fopen(perm.c_str(), "w");
            if (!g) throw std::runtime_error("Unable to write " + perm + "\n\n");
            short_write |= fwrite(rtx.get(), 1, nr, g) != nr; short_write |= fclose(g) != 0;
        }
        if (want_group) {
            FILE *g = fopen(grouped.c_str(), "w");
            if (!g) throw std::runtime_error("Unable to write " + grouped + "\n\n");
            short_write |= fwrite(gtx.get(), 1, ng, g) != ng; short_write |= fclose(g) != 0;
        }
        if (want_trans) {
            FILE *g = fopen(trans.c_str(), "w");
            if (!g) throw std::runtime_error("Unable to write " + trans + "\n\n");
            short_write |= fwrite(xtx.get(), 1, nx, g) != nx; short_write |= fclose(g) != 0;
        }
        if (want_indep) {
            FILE *g = fopen(indep.c_str(), "w");
            if (!g) throw std::runtime_error("Unable to write " + indep + "\n\n");
            short_write |= fwrite(itx.get(), 1, ni, g) != ni; short_write |= fclose(g) != 0;
        }
        if (short_write) { fprintf(stderr, "regtools-amd: writing the output failed (%s)\n", strerror(errno)); fflush(stderr); _exit(1); }
        if (getenv("REGTOOLS_AMD_STATS"))
            fprintf(stderr, "[regtools_amd] cohort: %u samples, %llu triples, %llu rows, adds %.3f ms, finish %.3f ms\n", m->n_samples,
                    (unsigned long long)m->n_triples, (unsigned long long)m->n, m->ms_add_total, m->ms_finish);
        if (cl && getenv("REGTOOLS_AMD_STATS"))
            fprintf(stderr, "[regtools_amd] clusters: %llu of %llu components kept, %u rounds, %.3f ms, %llu rows over the intron limit, %llu weak\n",
                    (unsigned long long)cl->n_clusters, (unsigned long long)cl->n_components, cl->n_rounds, cl->ms_cluster,
                    (unsigned long long)cl->n_ineligible, (unsigned long long)cl->n_weak);
        if (ph && getenv("REGTOOLS_AMD_STATS"))
            fprintf(stderr, "[regtools_amd] phenotypes: %llu rows kept of %llu clustered, %llu dropped as missing, %llu as flat, %.3f ms\n",
                    (unsigned long long)ph->n_rows, (unsigned long long)ph->n_clustered, (unsigned long long)ph->n_drop_na,
                    (unsigned long long)ph->n_drop_sd, ph->ms_pheno);
        if (components != "NA" && ph && getenv("REGTOOLS_AMD_STATS"))
            fprintf(stderr, "[regtools_amd] pcs: %llu rows, %u samples, %u components written, %.3f ms (gram %.3f ms, eigen %.3f ms)\n",
                    (unsigned long long)ph->n_rows, ph->n_samples, n_pcs, pcs ? pcs->ms_pcs : 0.0, pcs ? pcs->ms_gram : 0.0, pcs ? pcs->ms_eigen : 0.0);
        if (want_qtl && getenv("REGTOOLS_AMD_STATS"))
            fprintf(stderr, "[regtools_amd] qtl: %u variants of %llu records (%llu multi-allelic, %llu without GT, %llu on contigs the cohort does not know), "
                    "%u covariates, %llu pairs written, %llu constant variants, %llu explained, %llu flat rows, %.3f ms (residuals %.3f ms, pairs %.3f ms)\n",
                    gt->n_variants, (unsigned long long)gt->n_records, (unsigned long long)gt->n_multiallelic, (unsigned long long)gt->n_no_gt,
                    (unsigned long long)gt->n_unknown_contig, n_cov, (unsigned long long)(qr ? qr->n_pairs : 0), (unsigned long long)(qr ? qr->n_constant : 0),
                    (unsigned long long)(qr ? qr->n_explained : 0), (unsigned long long)(qr ? qr->n_flat_rows : 0), qr ? qr->ms_qtl : 0.0,
                    qr ? qr->ms_residual : 0.0, qr ? qr->ms_pairs : 0.0);
        if (want_perm && getenv("REGTOOLS_AMD_STATS")) {
            uint64_t n_lines = 0;
            for (uint64_t k = 0; pr && k < pr->n_rows; ++k) n_lines += pr->n_cis[k] != 0;
            fprintf(stderr, "[regtools_amd] perm: %u permutations from seed %llu, %u variants, %u covariates, %llu pairs, %llu rows written, %llu tiles, "
                    "%.3f ms (residuals %.3f ms, products %.3f ms, beta %.3f ms)\n", n_perm, (unsigned long long)seed, gt->n_variants, n_cov,
                    (unsigned long long)(pr ? pr->n_pairs : 0), (unsigned long long)n_lines, (unsigned long long)(pr ? pr->n_tiles : 0),
                    pr ? pr->ms_perm : 0.0, pr ? pr->ms_residual : 0.0, pr ? pr->ms_products : 0.0, pr ? pr->ms_beta : 0.0);
        }
        if (want_group && getenv("REGTOOLS_AMD_STATS")) {
            uint64_t n_lines = 0;
            for (uint64_t g = 0; gr && g < gr->n_groups; ++g) n_lines += gr->group_n_cis[g] != 0;
            fprintf(stderr, "[regtools_amd] group: %u permutations from seed %llu, %u variants, %u covariates, %u groups, %llu pairs, %llu groups written, "
                    "%llu tiles, %.3f ms (residuals %.3f ms, products %.3f ms, beta %.3f ms)\n", n_perm, (unsigned long long)seed, gt->n_variants, n_cov,
                    gr ? gr->n_groups : 0u, (unsigned long long)(gr ? gr->n_pairs : 0), (unsigned long long)n_lines,
                    (unsigned long long)(gr ? gr->n_tiles : 0), gr ? gr->ms_perm : 0.0, gr ? gr->ms_residual : 0.0, gr ? gr->ms_products : 0.0,
                    gr ? gr->ms_beta : 0.0);
        }
        if (want_trans && getenv("REGTOOLS_AMD_STATS"))
            fprintf(stderr, "[regtools_amd] trans: p <= %g, exclusion %s, %u variants, %u covariates, %llu pairs tested, %llu hits written, %llu tiles, "
                    "%llu with hits, %.3f ms (residuals %.3f ms, count %.3f ms, emit %.3f ms)\n", trans_pval,
                    trans_exclude ? std::to_string(trans_window).c_str() : "off", gt->n_variants, n_cov, (unsigned long long)(tr ? tr->n_tested : 0),
                    (unsigned long long)(tr ? tr->n_hits : 0), (unsigned long long)(tr ? tr->n_tiles : 0), (unsigned long long)(tr ? tr->n_hit_tiles : 0),
                    tr ? tr->ms_trans : 0.0, tr ? tr->ms_residual : 0.0, tr ? tr->ms_count : 0.0, tr ? tr->ms_emit : 0.0);
        if (want_indep && getenv("REGTOOLS_AMD_STATS"))
            fprintf(stderr, "[regtools_amd] indep: %llu rows entered, %u forward rounds, %llu conditional series, %llu signals written\n",
                    (unsigned long long)(ir ? ir->n_entered : 0), ir ? ir->n_forward_rounds : 0u, (unsigned long long)(ir ? ir->n_series_total : 0),
                    (unsigned long long)(ir ? ir->n_signals : 0));
        rgx_cohort_qtl_indep_free(ir);
        rgx_cohort_qtl_trans_free(tr);
        rgx_cohort_qtl_group_free(gr);
        rgx_cohort_qtl_perm_free(pr);
        rgx_cohort_qtl_free(qr);
        rgx_genotypes_free(gt);
        rgx_cohort_pheno_pcs_free(pcs);
        rgx_cohort_phenotypes_free(ph);
        rgx_cohort_clusters_free(cl);
        rgx_cohort_matrix_free(m);
        rgx_cohort_destroy(co);
        rgx_pipeline_destroy(pl);
        for (Flight &fb : fl) if (fb.bam) rgx_host_free(fb.bam);
    } catch (const std::runtime_error &e) {
        std::cerr << e.what() << std::endl;
        return 1;
    }
    return 0;
}

int junctions_usage(std::ostream &out) {
    out << "Usage:\t\tregtools junctions <command> [options]\n"
        << "Command:\textract\t\tIdentify exon-exon junctions from alignments.\n"
        << "\t\tannotate\tAnnotate the junctions.\n\n";
    return 0;
}

// junctions_main.cc:96-107
int junctions_main(int argc, char **argv) {
    if (argc > 1) {
        std::string sub = argv[1];
        if (sub == "extract") return junctions_extract(argc - 1, argv + 1);
        if (sub == "annotate") return junctions_annotate(argc - 1, argv + 1);
        if (sub == "cohort") return junctions_cohort(argc - 1, argv + 1);
    }
    return junctions_usage(std::cout);
}

// ---- cis-splice-effects identify (cis_splice_effects_identifier.cc:112-219, cis_splice_effects_main.cc:35-93) -------------
void space_options(std::ostream &out);

void window_options(std::ostream &out) {
    out << "\t\t-a INT\tMinimum anchor length. Junctions which satisfy a minimum \n\t\t\t anchor length on both sides are reported. [8]\n"
        << "\t\t-m INT\tMinimum intron length. [70]\n\t\t-M INT\tMaximum intron length. [500000]\n"
        << "\t\t-w INT\tWindow size in b.p to identify splicing events in.\n\t\t\t The tool identifies events in variant.start +/- w basepairs.\n"
        << "\t\t\t Default behaviour is to look at the window between previous and next exons.\n";
}

void identify_usage(std::ostream &out, bool associate = false) {
    out << "Usage:\t\tregtools cis-splice-effects " << (associate ? "associate [options] variants.vcf junctions.bed" :
        "identify [options] variants.vcf alignments.bam") << " ref.fa annotations.gtf\n"
        << "Options:\n"
        << "\t\t-o STR\tOutput file containing the aberrant splice junctions with annotations. [STDOUT]\n"
        << "\t\t-v STR\tOutput file containing variants annotated as splice relevant (VCF format).\n"
        << "\t\t-j STR\tOutput file containing the aberrant junctions in BED12 format.\n";
    if (!associate)
        out << "\t\t-s INT\tStrandness mode \n\t\t\t XS, use XS tags provided by aligner; RF, first-strand; FR, second-strand. intron-motif, infer strand using canonical intron motifs. REQUIRED\n"
            << "\t\t-C\tOverride strand assignments by inferring based on canonical motifs. Does not need to be specified if passing '-s intron-motif'.\n"
            << "\t\t-t STR\tTag used in bam to label strand. [XS]\n";
    window_options(out);
    space_options(out);
    if (!associate)
        out << "\t\t-b STR\tThe file containing the barcodes of interest for single cell data.\n"
            << "\t\t-C\tTells cis-splice-effects identify that you want intron-motif method to take priority when assigning strand. i.e. decide strandedness based on the fasta rather than what is encoded in the alignment file.\n";
    out << "\n";
}

bool file_exists(const std::string &p) { FILE *f = fopen(p.c_str(), "rb"); if (!f) return false; fclose(f); return true; }

// associate = true: `cis-splice-effects associate` (cis_splice_effects_associator.cc:104-180): no -s/-t/-b/-C, the second positional is a BED12
int cse_identify(int argc, char **argv, bool associate = false) {
    try {
        rgx_identify_params p;
        rgx_identify_params_default(&p);
        std::string out_tsv = "NA", out_vcf = "NA", out_bed = "NA", tag = "XS", barcodes = "NA";
        optind = 1;
        int c;
        while ((c = getopt(argc, argv, associate ? "o:w:v:j:e:Ei:ISha:m:M:" : "o:w:v:j:e:Ei:ISht:s:a:m:M:b:C")) != -1) {
            switch (c) {
                case 'o': out_tsv = optarg; break;
                case 'w': p.window = (uint32_t)atoi(optarg); break;
                case 'v': out_vcf = optarg; break;
                case 'j': out_bed = optarg; break;
                case 'i': p.intronic_min = (uint32_t)atoi(optarg); break;
                case 'e': p.exonic_min = (uint32_t)atoi(optarg); break;
                case 'I': p.all_intronic = 1; break;
                case 'E': p.all_exonic = 1; break;
                case 'S': p.skip_single = 0; break;
                case 'h': { std::ostringstream ss; identify_usage(ss, associate); throw HelpRequested{ss.str()}; }
                case 's': {
                    std::string s = optarg;
                    if (s == "XS") p.strandness = 0; else if (s == "RF") p.strandness = 1; else if (s == "FR") p.strandness = 2;
                    else if (s == "intron-motif") p.strandness = 3;
                    else throw std::runtime_error("Unrecognized strandness argument!\n\n");
                    break;
                }
                case 't': tag = optarg; break;
                case 'a': p.min_anchor = (uint32_t)atoi(optarg); break;
                case 'm': p.min_intron = (uint32_t)atoi(optarg); break;
                case 'M': p.max_intron = (uint32_t)atoi(optarg); break;
                case 'b': barcodes = optarg; break;
                case 'C': p.override_motif = 1; break;
                default: identify_usage(std::cerr, associate); throw std::runtime_error("Error parsing inputs!(1)\n\n");
            }
        }
        std::string vcf = "NA", bam = "NA", ref = "NA", gtf = "NA";
        if (argc - optind >= 4) { vcf = argv[optind++]; bam = argv[optind++]; ref = argv[optind++]; gtf = argv[optind++]; }
        if (optind < argc || vcf == "NA" || bam == "NA" || ref == "NA" || gtf == "NA") { identify_usage(std::cerr, associate);
            throw std::runtime_error("Error parsing inputs!(2)\n\n"); }
        if (associate) p.strandness = 0;
        if (p.strandness == -1) { identify_usage(std::cerr); throw std::runtime_error("Please supply strand specificity with '-s' option!\n\n"); }
        if (!file_exists(vcf) || !file_exists(bam) || !file_exists(ref) ||
            !file_exists(gtf)) throw std::runtime_error("Please make sure input files exist.\n\n");
        // the echo of parse_options (identifier.cc:203-218, associator.cc:156-171), then what identify() / associate() write while they work (p.echo)
        std::cerr << "Variant file: " << vcf << (associate ? "\nJunctions BED file: " :
            "\nAlignment file: ") << bam << "\nReference fasta file: " << ref << "\nAnnotation file: " << gtf << "\n";
        if (p.window != 0) std::cerr << "Window size: " << p.window << "\n";
        if (out_tsv != "NA") std::cerr << "Output file: " << out_tsv << "\n";
        if (out_bed != "NA") std::cerr << "Output junctions BED file: " << out_bed << "\n";
        if (out_vcf != "NA") std::cerr << "Annotated variants file: " << out_vcf << "\n";
        std::cerr << "\n";
        p.echo = 1;
        if (associate) p.bed_path = bam.c_str();
        p.vcf_path = vcf.c_str(); p.bam_path = bam.c_str(); p.fasta_path = ref.c_str(); p.gtf_path = gtf.c_str();
        p.out_tsv = out_tsv == "NA" ? nullptr : out_tsv.c_str(); p.out_vcf = out_vcf == "NA" ? nullptr : out_vcf.c_str(); p.out_bed = out_bed == "NA" ?
            nullptr : out_bed.c_str();
        p.strand_tag[0] = tag.size() > 0 ? tag[0] : 0; p.strand_tag[1] = tag.size() > 1 ? tag[1] : 0;
        char err[512] = {0};
        rgx_ctx *ctx = nullptr;
        int dev = 0; if (const char *d = getenv("REGTOOLS_AMD_DEVICE")) dev = atoi(d);
        // REGTOOLS_AMD_DEVICES=0,1,...: identify's extraction is sharded over these GPUs (rgx_identify_multi); the outputs do not depend on the list
        std::vector<int> devices;
        if (const char *d = getenv("REGTOOLS_AMD_DEVICES")) {
            for (const char *q = d; *q;) { char *e; long v = strtol(q, &e, 10); if (e == q) break; devices.push_back((int)v); q = *e == ',' ? e + 1 : e;
                if (*e && *e != ',') break; }
        }
        if (devices.size() == 1) dev = devices[0];
        const bool multi = !associate && devices.size() > 1;
        if (!multi && rgx_ctx_create(dev, &ctx, err, sizeof err) != RGX_OK) throw std::runtime_error(err);
        rgx_identify_stats st;
        int rc = associate ? rgx_associate(ctx, &p, &st, err, sizeof err)
                           : multi ? rgx_identify_multi(devices.data(), (int)devices.size(), &p, &st, err, sizeof err) : rgx_identify(ctx, &p, &st, err,
                               sizeof err);
        if (ctx) rgx_ctx_destroy(ctx);
        die_where_upstreams_library_does(rc, err);
        if (rc != RGX_OK) { die_as_upstream_on_empty_gtf_line(err, /*caught=*/true); throw std::runtime_error(err); }
        if (barcodes != "NA") {
            // identify's extractor is built without a barcode file (identifier.cc:288 -> junctions_extractor.h:197-205), so every junction's map
            // is empty and print_barcodes (identifier.cc:239-241) writes "0\t" per junction; an unopenable file ends the run (set_ostream :90-95)
            FILE *b = fopen(barcodes.c_str(), "w");
            if (!b) throw std::runtime_error("Unable to open " + barcodes);
            for (uint64_t i = 0; i < st.n_junctions; ++i) fputs("0\t\n", b);
            fclose(b);
        }
        if (getenv("REGTOOLS_AMD_STATS"))
            fprintf(stderr,
                "[regtools_amd] variants=%llu relevant=%llu windows=%llu pairs=%llu junctions=%llu total=%.3fms (gtf %.3f variants %.3f extract %.3f join %.3f annotate %.3f output %.3f)\n",
                    (unsigned long long)st.n_variants, (unsigned long long)st.n_relevant, (unsigned long long)st.n_windows, (unsigned long long)st.n_pairs,
                    (unsigned long long)st.n_junctions, st.ms_total, st.ms_gtf, st.ms_variants, st.ms_extract, st.ms_join, st.ms_annotate, st.ms_output);
    } catch (const HelpRequested &h) {
        std::cerr << h.text << std::endl;
        return 0;
    } catch (const std::runtime_error &e) {
        std::cerr << e.what() << std::endl;
        return 1;
    }
    return 0;
}

// ---- variants annotate (variants_annotator.cc:48-110, variants_main.cc) -------------------------------------------------------------
void space_options(std::ostream &out) {
    out << "\t\t-e INT\tMaximum distance from the start/end of an exon \n\t\t\t to annotate a variant as relevant to splicing, the variant \n\t\t\t is in exonic space, i.e a coding variant. [3]\n"
        << "\t\t-i INT\tMaximum distance from the start/end of an exon \n\t\t\t to annotate a variant as relevant to splicing, the variant \n\t\t\t is in intronic space. [2]\n"
        << "\t\t-I\tAnnotate variants in intronic space within a transcript(not to be used with -i).\n"
        << "\t\t-E\tAnnotate variants in exonic space within a transcript(not to be used with -e).\n"
        << "\t\t-S\tDon't skip single exon transcripts.\n";
}

void variants_usage(std::ostream &out) {
    out << "Usage:\t\tregtools variants annotate [options] variants.vcf annotations.gtf\n"
        << "Options:\n"
        << "\t\t-o FILE\tThe file to write output to. [STDOUT]\n";
    space_options(out);
    out << "\n";
}

int variants_annotate(int argc, char **argv) {
    try {
        rgx_identify_params p;
        rgx_identify_params_default(&p);
        std::string out = "NA";
        optind = 1;
        int c;
        while ((c = getopt(argc, argv, "e:Ei:ISho:")) != -1) {
            switch (c) {
                case 'i': p.intronic_min = (uint32_t)atoi(optarg); break;
                case 'e': p.exonic_min = (uint32_t)atoi(optarg); break;
                case 'I': p.all_intronic = 1; break;
                case 'E': p.all_exonic = 1; break;
                case 'S': p.skip_single = 0; break;
                case 'o': out = optarg; break;
                case 'h': { std::ostringstream ss; variants_usage(ss); throw HelpRequested{ss.str()}; }
                default: variants_usage(std::cout); throw std::runtime_error("Error parsing inputs!(1)\n\n");
            }
        }
        std::string vcf = "NA", gtf = "NA";
        if (argc - optind >= 2) { vcf = argv[optind++]; gtf = argv[optind++]; }
        if (optind < argc || vcf == "NA" || gtf == "NA") { variants_usage(std::cout); throw std::runtime_error("Error parsing inputs!(2)\n\n"); }
        p.vcf_path = vcf.c_str(); p.gtf_path = gtf.c_str(); p.out_vcf = out == "NA" ? nullptr : out.c_str();
        // variants_annotator.cc:93-108
        std::cerr << "Variant file: " << vcf << "\nGTF file: " << gtf << "\nOutput vcf file: " << out << "\n";
        if (!p.all_intronic) std::cerr << "Intronic min distance: " << p.intronic_min << "\n";
        if (!p.all_exonic) std::cerr << "Exonic min distance: " << p.exonic_min << "\n";
        if (!p.skip_single) std::cerr << "Not skipping single exon genes.\n";
        if (out != "NA") std::cerr << "Output file: " << out << "\n";
        std::cerr << "\n";
        rgx_ctx *ctx = open_ctx();
        char err[512] = {0};
        int rc = rgx_variants_annotate(ctx, &p, nullptr, err, sizeof err);
        rgx_ctx_destroy(ctx);
        die_where_upstreams_library_does(rc, err);
        if (rc != RGX_OK) { die_as_upstream_on_empty_gtf_line(err); throw std::runtime_error(err); }
    } catch (const HelpRequested &h) {
        std::cerr << h.text << std::endl;
        return 0;
    } catch (const std::runtime_error &e) {
        std::cerr << e.what() << std::endl;
        return 1;
    }
    return 0;
}

int variants_main(int argc, char **argv) {
    if (argc > 1 && std::string(argv[1]) == "annotate") return variants_annotate(argc - 1, argv + 1);
    std::cout << "Usage:\t\tregtools variants <command> [options]\nCommand:\tannotate\t\tAnnotate variants with splicing information.\n\n";
    return 0;
}

int cse_main(int argc, char **argv) {
    if (argc > 1) {
        std::string sub = argv[1];
        if (sub == "identify") return cse_identify(argc - 1, argv + 1);
        if (sub == "associate") return cse_identify(argc - 1, argv + 1, true);
    }
    std::cout << "Usage:\t\tregtools cis-splice-effects <command> [options]\nCommand:\tidentify\t\tIdentify cis splicing effects.\n\t\tassociate\tAssociate extracted junctions with variants\n\n";
    return 0;
}

}  // namespace

// regtools.cc:36-74: the banner and the top-level usage are the reference's bytes (pinned against the reference's own main() in tests/test_cli_contract.py);
// the library's own version string is rgx_version() (REGTOOLS_AMD_TRACE prints it)
int main(int argc, char **argv) {
    // this process makes one library call: the context does without streams of its own (api.cpp ensure_upload_streams)
    setenv("REGTOOLS_AMD_ONE_SHOT", "1", 0);
    std::cerr << "\nProgram:\tregtools\nVersion:\t1.0.0" << std::endl;
    if (getenv("REGTOOLS_AMD_TRACE")) std::cerr << "[rgx trace] " << rgx_version() << std::endl;
    if (argc > 1) {
        std::string sub = argv[1];
        if (sub == "junctions") return junctions_main(argc - 1, argv + 1);
        if (sub == "cis-splice-effects") return cse_main(argc - 1, argv + 1);
        if (sub == "variants") return variants_main(argc - 1, argv + 1);
        // listed by the usage text below, as upstream's; not part of this build (out of scope)
        if (sub == "cis-ase") {
            std::cerr << "regtools-amd: the cis-ase commands are not part of the MI355X build; use the reference binary for them\n";
            return 1;
        }
    }
    std::cerr << "Usage:\t\tregtools <command> [options]\n"
              << "Command:\tjunctions\t\tTools that operate on feature junctions (e.g. exon-exon junctions from RNA-seq).\n"
              << "\t\tcis-ase\t\t\tTools related to allele specific expression in cis.\n"
              << "\t\tcis-splice-effects\tTools related to splicing effects of variants.\n"
              << "\t\tvariants\t\tTools that operate on variants.\n\n";
    return 0;
}
