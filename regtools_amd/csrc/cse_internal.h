// cse_internal.h -- what the translation units of `cis-splice-effects identify / associate`, `variants annotate` and `junctions annotate` share (SURVEY 8a
// rows a9-a12, 8f rows f2, f3): the annotation handle, the results of the two annotation scans, the small RAII helpers of a call with side threads, and
// the functions one unit calls in another.  cse_api.cpp (1,400 lines) split by command, as api.cpp was along its stages (api_internal.h) --
//   cse_scan.cpp      rows a10, a11: the annotation's upload, variants and junctions against it
//   cse_join.cpp      row a9: the window join (one pass, or by seeks), the associate pair join, the sharded extraction's gather
//   cse_output.cpp    the annotated VCF, the junction rows and their writer thread, `junctions annotate`
//   cse_identify.cpp  IdentifyRun: `identify` / `associate` as stages; `variants annotate`
// Host code here parses text and assembles strings; every interval computation is a kernel.
#pragma once
#include "api_internal.h"
#include "cse_table.h"

struct rgx_gtf {
    rgx_ctx *ctx = nullptr;
    GtfModel m;
    void *dev = nullptr;     // one allocation holding all flat arrays
    GtfView view{};
};

// the host stages of a call share one pool of threads (set by the call: IdentifyRun::stage_annotation)
extern thread_local WorkerPool *tl_pool;                     // (cse_scan.cpp)
// the pool of one call and its time as tl_pool: from start() to the end of the scope, whichever way that is left
struct PoolScope {
    std::unique_ptr<WorkerPool> pool; WorkerPool *prev = nullptr;
    void start(size_t threads) { pool.reset(new WorkerPool(threads)); prev = tl_pool; tl_pool = pool.get(); }
    ~PoolScope() { if (pool) tl_pool = prev; }
};
// f(t) for t in [0, T): on the pool the running `identify` call keeps for all its host stages (six of them start a dozen threads each otherwise:
// 2-3 ms of a 70 ms call), or on threads of its own where no such call is running
void run_tasks(size_t T, const std::function<void(size_t)> &f);

// ---- what a call with side threads is made of -----------------------------------------------------------------------------------------
struct GtfGuard {
    rgx_gtf *g;
    GtfGuard(rgx_gtf *g_ = nullptr) : g(g_) {}
    GtfGuard(const GtfGuard &) = delete;
    GtfGuard &operator=(const GtfGuard &) = delete;
    rgx_gtf *release() { rgx_gtf *r = g; g = nullptr; return r; }
    ~GtfGuard() { rgx_gtf_free(g); }
};
struct JoinThread { std::thread &t; ~JoinThread() { if (t.joinable()) t.join(); } };
// REGTOOLS_AMD_TRACE: how long the scope's locals took to go (t set at the scope's last line; declared in front of them)
struct TraceTeardown { const char *what; double t = 0; ~TraceTeardown() { if (t > 0) fprintf(stderr, "[rgx trace] %s +%8.3f ms\n", what, now_ms() - t); } };
// A text loader's verdict ("" = loaded); what it throws (bad_alloc from its vectors) becomes one.  start(): on a thread of its own (parsing only, no device
// calls), joined by join() or by the end of the scope -- declare it BEHIND what the loader writes into.
template <class Load> std::string load_text(Load load) {
    try { return load(); } catch (const std::exception &e) { return std::string("regtools_amd: ") + e.what() + "\n"; }
}
struct SideLoad {
    std::thread th; std::string err; double ms = 0;
    template <class Load> void start(Load load) { th = std::thread([this, load] { const double t = now_ms(); err = load_text(load); ms = now_ms() - t; }); }
    void join() { if (th.joinable()) th.join(); }
    ~SideLoad() { join(); }
};

// ---- results of the stages -------------------------------------------------------------------------------------------------------------
struct VariantHitsHost { std::vector<uint32_t> ces, cee, off, tx, ann, dist, last; };      // last: upstream's variant.score behind the walk (0xffffffff = "-1")
struct JunctionAnnotHost { std::vector<uint32_t> flags, n_acc, n_exo, n_don, tx_off, tx; };
// a11 as the kernel leaves it: junction i's items (kind, a, b) are off[i] .. off[i + 1], in visiting order, duplicates included
struct JunctionItemsHost { std::vector<uint32_t> flags, visits, off, kind, a, b; uint64_t visits_total = 0; };
struct VStr { std::string genes, transcripts, distances, annotations; };
struct VariantStage {
    VcfText vcf;
    VariantHitsHost H;
    // comma strings in visitation order (variants_annotator.cc:479-506), one entry per splice relevant record (the others are written as "NA" x4)
    std::vector<VStr> vstr;
    std::vector<uint32_t> vstr_of;     // record -> its entry of vstr, UINT32_MAX when not splice relevant
    std::vector<size_t> relevant;      // indices into vcf.recs
};
inline int vcf_load_code(const VcfText &vcf) { return vcf.death == 2 ? RGX_ERR_ABORT : vcf.death == 1 ? RGX_ERR_EXIT : RGX_ERR_OPEN; }

// ---- small things every unit uses --------------------------------------------------------------------------------------------------------
// a column of a C result struct: the vector's words in a malloc block of its own (one word more, so that an empty column is a pointer too)
inline uint32_t *dup_u32(const std::vector<uint32_t> &v) {
    uint32_t *p = (uint32_t *)malloc((v.size() + 1) * 4);
    if (!v.empty()) memcpy(p, v.data(), v.size() * 4);
    return p;
}
// the first n elements of a host vector into a device array, on the stream (under HIP_TRY)
template <class T> hipError_t upload(T *dst, const std::vector<T> &v, size_t n, hipStream_t st) {
    return hipMemcpyAsync(dst, v.data(), n * sizeof(T), hipMemcpyHostToDevice, st);
}
// (text is appended to strings with to_chars: 66 k rows through fprintf into memory streams were 8.5 ms on 16 threads, a std::set of string pairs per row
// among them)
inline void put_u(std::string &o, uint64_t v) { char b[24]; auto r = std::to_chars(b, b + sizeof b, v); o.append(b, (size_t)(r.ptr - b)); }
inline void put_i(std::string &o, int64_t v) { char b[24]; auto r = std::to_chars(b, b + sizeof b, v); o.append(b, (size_t)(r.ptr - b)); }

// ---- functions one unit calls in another -------------------------------------------------------------------------------------------------
// multi.cpp: the process-wide context of the nth listing of a device (rgx_extract_multi's cache)
rgx_ctx *rgx_multi_context(int device, int nth, char *err, size_t errlen, int *rc);
// cse_scan.cpp
int gtf_upload(rgx_ctx *c, rgx_gtf *g, char *err, size_t errlen, bool pooled = false);
int annotate_junctions(rgx_ctx *c, const rgx_gtf *g, const std::vector<int32_t> &chrom, const std::vector<uint32_t> &js, const std::vector<uint32_t> &je,
                       const std::vector<uint8_t> &strand, JunctionAnnotHost &A, char *err, size_t errlen, uint64_t *exon_visits = nullptr,
                       bool keep_single = false);
int junction_scan_items(rgx_ctx *c, const GtfView &view, const std::vector<int32_t> &chrom, const std::vector<uint32_t> &js, const std::vector<uint32_t> &je,
                        const std::vector<uint8_t> &strand, int form, bool guarded, JunctionItemsHost &R, char *err, size_t errlen);
int variant_scan_stage(rgx_ctx *c, const rgx_gtf *g, const VariantOpts &vo, VariantStage &V, uint64_t *exon_visits, char *err, size_t errlen);
// cse_join.cpp
// The pair workspace of one batch of windows: the two pair lists of the window join (window numbers batch-local), then -- in the product's
// Buf::cse_pairs -- room for the pairs' events as an EventSoA of as many rows.
struct PairLayout { uint32_t *pair_ev, *pair_win; EventSoA pe; };
// on_batch(first window, windows, pairs, the batch's lists): called for every batch that holds a pair, behind its fill pass on the stream
typedef std::function<int(uint32_t w0, uint32_t nw, uint32_t total, const PairLayout &L)> PairBatchFn;
// The planning and counting half of the window join and its per-batch fill.  pair_batch: pairs per batch of whole windows (a window above it is a
// batch of its own), 0 = the product's (2^26, or REGTOOLS_AMD_PAIR_BATCH).  guarded: the lists lie in Buf::stage with guard words behind each.
int window_pair_batches(rgx_ctx *c, const EventSoA &ev, uint32_t n_events, const std::vector<int32_t> &w_tid, const std::vector<int32_t> &w_beg,
                        const std::vector<int32_t> &w_end, uint64_t pair_batch, bool guarded, const PairBatchFn &on_batch, uint64_t &n_pairs,
                        uint32_t &n_batches, char *err, size_t errlen);
int window_join(rgx_ctx *c, const Prep &P, const std::vector<int32_t> &w_tid, const std::vector<int32_t> &w_beg, const std::vector<int32_t> &w_end,
                uint32_t ilen_bits, HostRows &R, uint64_t &n_pairs, char *err, size_t errlen);
int window_join_by_seeks(rgx_ctx *c, const uint8_t *d_file, size_t bam_len, const uint8_t *bai, size_t bai_len, const rgx_extract_params &ep0,
                         const std::vector<std::string> &w_region, uint32_t ilen_bits, HostRows &R, uint64_t &n_pairs, size_t &w_abort, char *err,
                         size_t errlen);
int assoc_join(rgx_ctx *c, const std::vector<int32_t> &wch, const std::vector<uint32_t> &wces, const std::vector<uint32_t> &wcee,
               const std::vector<uint32_t> &chrom_off, const std::vector<uint32_t> &js, const std::vector<uint32_t> &je, std::vector<uint32_t> &pj,
               std::vector<uint32_t> &pw, uint64_t &n_pairs, char *err, size_t errlen);
int prepare_events_sharded(const std::vector<rgx_ctx *> &cs, const uint8_t *bam, size_t bam_len, const uint8_t *bai, size_t bai_len,
                           const rgx_extract_params *ep, Prep &P, char *err, size_t errlen);
// cse_output.cpp
int write_annotated_vcf(const char *path, const VariantStage &V, bool all_records, char *err, size_t errlen, bool print_notes = true);
int write_junction_outputs(rgx_ctx *c, const rgx_gtf *g, const char *fasta_path, const JTable &uj, const char *out_tsv, const char *out_bed,
                           uint64_t *exon_visits, double *ms_annotate, char *err, size_t errlen, bool echo = false);
