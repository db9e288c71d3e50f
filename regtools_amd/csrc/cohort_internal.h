// cohort_internal.h -- what the cohort's translation units (cohort*.cpp) share: the cohort itself with its contig table, the layout of a matrix's
// block and the serial kept beside a matrix, CopyBack (the one way results come back from the device), CohortRun (the base of every device run) with
// Events, and the ids the text formats print.  A result's block: result_block.h; the two-pass text writer: text_out.h; what the sQTL calls share
// beyond this: qtl_run.h.
#pragma once
#include "api_internal.h"
#include "result_block.h"
#include "text_out.h"

// The cohort's contig table: the samples' header names in order of first appearance.
struct CohortContigs {
    std::vector<std::string> names; std::vector<uint32_t> lens, first_sample;
    std::unordered_map<std::string, uint32_t> index;
    // map[tid of t] = cohort tid.  A name that is already there with another length changes nothing and is an error.
    int map_sample(const rgx_junction_table *t, uint32_t sample, const char *sample_name, const std::vector<std::string> &sample_names,
                   std::vector<uint32_t> &map, char *err, size_t errlen) {
        std::unordered_map<std::string, uint32_t> own;                       // (a header may list a name twice)
        for (int32_t i = 0; i < t->n_ref; ++i) {
            const std::string nm = t->ref_name[i];
            auto it = index.find(nm);
            if (it != index.end() && lens[it->second] != t->ref_len[i]) return fail(err, errlen, RGX_ERR_ARG,
                "regtools_amd: contig %s is %u long in sample %s and %u in sample %s\n", nm.c_str(), lens[it->second],
                sample_names[first_sample[it->second]].c_str(), t->ref_len[i], sample_name);
            auto o = own.find(nm);
            if (o != own.end() && o->second != t->ref_len[i]) return fail(err, errlen, RGX_ERR_ARG,
                "regtools_amd: contig %s is %u long in sample %s and %u in sample %s\n", nm.c_str(), o->second, sample_name, t->ref_len[i], sample_name);
            own[nm] = t->ref_len[i];
        }
        map.resize((size_t)std::max<int32_t>(t->n_ref, 0));
        for (int32_t i = 0; i < t->n_ref; ++i) {
            const std::string nm = t->ref_name[i];
            auto it = index.find(nm);
            if (it == index.end()) {
                it = index.emplace(nm, (uint32_t)names.size()).first;
                names.push_back(nm); lens.push_back(t->ref_len[i]); first_sample.push_back(sample);
            }
            map[(size_t)i] = it->second;
        }
        return RGX_OK;
    }
};

// The matrix's row and CSR arrays live in ONE block in this order, every array 16-byte aligned: finish writes the same image on the device and
// copies it once.
struct MatrixLayout { size_t total, row_begin, tid, start, end, ts, te, n_with, col, val, strand, bytes; };
inline MatrixLayout matrix_layout(uint64_t n, uint64_t nnz) {
    MatrixLayout L; size_t o = 0;
    auto take = [&](size_t bytes) { const size_t at = o; o += (bytes + 15) & ~(size_t)15; return at; };
    L.total = take((size_t)n * 8); L.row_begin = take((size_t)(n + 1) * 8);
    L.tid = take((size_t)n * 4); L.start = take((size_t)n * 4); L.end = take((size_t)n * 4); L.ts = take((size_t)n * 4); L.te = take((size_t)n * 4);
    L.n_with = take((size_t)n * 4); L.col = take((size_t)nnz * 4); L.val = take((size_t)nnz * 4); L.strand = take((size_t)n + 1);
    L.bytes = o;
    return L;
}
inline CohortImage image_at(uint8_t *b, const MatrixLayout &L) {
    CohortImage o; o.total = (unsigned long long *)(b + L.total); o.row_begin = (unsigned long long *)(b + L.row_begin); o.tid = (uint32_t *)(b + L.tid);
    o.start = (uint32_t *)(b + L.start); o.end = (uint32_t *)(b + L.end); o.ts = (uint32_t *)(b + L.ts); o.te = (uint32_t *)(b + L.te);
    o.n_with = (uint32_t *)(b + L.n_with); o.col_sample = (uint32_t *)(b + L.col); o.val_count = (uint32_t *)(b + L.val); o.strand = b + L.strand;
    return o;
}
// serial: every matrix the library hands out has its own (never 0), kept beside it in its box; a cohort remembers that of the matrix whose image
// its last finish left in HBM
inline uint64_t matrix_serial(const rgx_cohort_matrix *m) { return result_extra<uint64_t>(const_cast<rgx_cohort_matrix *>(m)); }

// The one way results come back: device-to-host copies enqueued on the stream, none of no bytes and none behind a failed one, then the call's
// one wait, which also answers for the kernel launches queued before it.
struct CopyBack {
    hipStream_t st; hipError_t e = hipSuccess;
    void operator()(void *dst, const void *src, size_t bytes) { if (e == hipSuccess && bytes) e = hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, st); }
    hipError_t wait() {
        if (e == hipSuccess) e = hipStreamSynchronize(st);
        if (e == hipSuccess) e = rgx::pending_launch_error();
        return e;
    }
};
// a few scalars the host needs now: one copy, one wait
inline hipError_t read_back(hipStream_t st, void *dst, const void *src, size_t bytes) { CopyBack back{st}; back(dst, src, bytes); return back.wait(); }

// The ids of the text formats: "clu_N_strand" of row i's cluster (the strand by rgx::strand_class: +, -, NA), and the intron id
// "contig:start:end:clu_N_strand".
inline void put_clu(TextOut &o, const rgx_cohort_matrix *m, const rgx_cohort_clusters *cl, uint32_t i) {
    const uint32_t cls = rgx::strand_class(m->strand[i]);
    o.fmt("clu_%llu_%s", (unsigned long long)cl->cluster[i] + 1, cls == 0 ? "+" : cls == 1 ? "-" : "NA");
}
inline void put_intron_id(TextOut &o, const rgx_cohort_matrix *m, const rgx_cohort_clusters *cl, uint32_t i) {
    o.put(m->ref_name[m->tid[i]]); o.fmt(":%u:%u:", m->start[i], m->end[i]); put_clu(o, m, cl, i);
}

constexpr uint64_t kMaxTriples = (1ull << 32) - (1ull << 16);        // (the sort's tiles round the count up inside 32 bits)
constexpr uint32_t kMaxSamples = 1u << 24;                           // (a triple keeps its sample in 24 bits, beside the strand character)
constexpr size_t kMaxBlocks = (size_t)1 << (32 - kCohortBlockLog2);

struct rgx_cohort {
    int device = 0;
    rgx_cohort_params p{};
    std::mutex mu;
    hipStream_t stream = nullptr;
    hipEvent_t ev_src = nullptr, ev_done = nullptr, ev_up = nullptr; bool up_pending = false;
    CohortContigs contigs; std::vector<std::string> sample_names;
    std::vector<uint32_t *> blocks = std::vector<uint32_t *>(kMaxBlocks, nullptr);   // (fixed size: copies to the device table read its elements in place)
    size_t n_blocks = 0;
    uint32_t **d_blocks = nullptr; uint32_t *d_fill = nullptr;
    // a sample's tid map must outlive its append, which is only enqueued: maps stay until the cohort goes (most samples share the one before)
    struct TidMap { std::vector<uint32_t> host; uint32_t *dev = nullptr; };
    std::vector<std::unique_ptr<TidMap>> maps;
    uint64_t n_triples = 0; uint32_t max_start = 0, max_end = 0;
    int last_path = 0; double ms_add_total = 0;
    void *pinned_up = nullptr; size_t pinned_up_cap = 0; bool pinned_up_locked = false;
    DevBuf up, sort, rows, image;
    // rgx_cohort_cluster (cohort_cluster.cpp): the matrix whose image `image` holds (0: none), an uploaded matrix, the row and the entry workspace
    uint64_t image_serial = 0;
    int cluster_path = 0;
    DevBuf cl_in, cl_rows, cl_entries;
    // rgx_cohort_phenotypes (cohort_pheno.cpp): the uploaded cluster result, the row and the entry workspace
    DevBuf ph_in, ph_rows, ph_entries;
    // rgx_cohort_pheno_pcs (cohort_pcs.cpp): rank2 and the quantile table, the chunk partials, the Gram matrix with the column sums
    DevBuf pc_in, pc_part, pc_out;
    // the sQTL calls' shared stages (QtlPrep, qtl_prep.cpp): the uploaded inputs, the row-major residuals with the per-row and per-variant arrays
    // (and the words the run asks for), the sample-major panels
    DevBuf qt_in, qt_rows, qt_t;
    // rgx_cohort_qtl_nominal (cohort_qtl.cpp): the pairs; rgx_cohort_qtl_trans (cohort_qtl_trans.cpp): the hits
    DevBuf qt_out;
    // rgx_cohort_qtl_permute and _grouped (cohort_qtl_perm.cpp): the sample-major permutations with the member lists, perm_r with the best pairs
    DevBuf qp_in, qp_out;
    // rgx_cohort_qtl_trans (cohort_qtl_trans.cpp): the per-tile words
    DevBuf qx_tiles;
    // rgx_cohort_qtl_permute_conditional (cohort_qtl_cond.cpp): the series' lists; the bases, rows, betas and the result's arrays
    DevBuf qc_in, qc_ws;
};

// What every device run of a cohort call (ClusterRun, PhenoRun, PcsRun, the sQTL runs behind QtlPrep: qtl_run.h) is made of.  The caller holds the
// cohort's lock; `err` and `errlen` are named as HIP_TRY and CARVE_TRY want them.
struct CohortRun {
    rgx_cohort *co; char *err; size_t errlen; const char *name;
    double t0, t_last; bool trace = false; hipStream_t st = nullptr;
    CohortRun(rgx_cohort *co_, const char *name_, char *err_, size_t errlen_)
        : co(co_), err(err_), errlen(errlen_), name(name_), t0(now_ms()), t_last(t0) {}
    // with REGTOOLS_AMD_TRACE set: waits for the stream and prints what the stage took
    void mark(const char *what) {
        if (!trace) return;
        (void)hipStreamSynchronize(st);
        const double t = now_ms();
        fprintf(stderr, "[rgx trace] %s: %-28s +%8.3f ms\n", name, what, t - t_last); t_last = t;
    }
    // the cohort's device and stream, in front of the run's first device call
    int enter() {
        HIP_ENTER(co->device); st = co->stream; trace = getenv("REGTOOLS_AMD_TRACE") != nullptr;
        const char *f = getenv("REGTOOLS_AMD_FILL"); fill = f && *f && strcmp(f, "0") != 0;
        return RGX_OK;
    }
    // The fill mode (REGTOOLS_AMD_FILL, read per call, off by default; DESIGN.md "Workspace words").  A workspace word is written in the call that
    // reads it or never read; with the mode on a word that breaks the rule shows in the result instead of reading as the zero of fresh memory or
    // as what the call before left.  Every workspace is cut with carve() and handed to carved() behind its CARVE_TRY, in front of the first upload
    // or launch into it: carved() enqueues the fills -- a quiet NaN over every floating-point array, the value 1 in every element of an integer
    // array, the guard byte from the end of the last array to the buffer's capacity -- and notes the guard's first bytes, which guards_back()
    // puts in front of the call's one wait and guards_check() reads behind it: a changed byte fails the call.
    // Exempt, because their contents live from one call to the next: `image` (the matrix in HBM), the blocks of `add` with d_blocks and d_fill,
    // and the tid maps.  `up`, `cl_in` and the other upload buffers that are not cut with Carve are written whole by their copies.
    bool fill = false; CarveLog carve_log;
    struct Guard { const char *what; const uint8_t *base, *at; size_t n; };
    static constexpr uint32_t kMaxGuards = 12;
    Guard guard[kMaxGuards]; uint32_t n_guards = 0; uint8_t guard_host[kMaxGuards][kCarveGuardWindow];
    Carve carve(const DevBuf &b) { return Carve(b.p, b.cap, fill ? &carve_log : nullptr); }
    int carved(const Carve &w, const char *what) {
        if (!fill) return RGX_OK;
        const CarveLog &lg = carve_log;
        const size_t cap = (size_t)(w.at - w.base) + w.left;
        if (w.log != &lg || lg.full || lg.end > cap) return fail(err, errlen, RGX_ERR_DEVICE, "regtools_amd: the %s buffer has more arrays than the fill mode's log\n", what);
        for (uint32_t i = 0; i < lg.n; ++i) {
            const CarveLog::Array &a = lg.a[i];
            if (a.kind == CarveKind::fp) launch_fill_elems(w.base + a.off, 4, 0x7ff80000u, a.bytes / 4, st);
            else launch_fill_elems(w.base + a.off, (uint32_t)a.kind, 1, a.bytes / (size_t)a.kind, st);
        }
        if (cap > lg.end) HIP_TRY(hipMemsetAsync(w.base + lg.end, kCarveGuardByte, cap - lg.end, st));
        uint32_t g = 0;
        while (g < n_guards && strcmp(guard[g].what, what) != 0) ++g;       // (a workspace cut again in the same call, grown or not: its newest guard counts)
        if (g == kMaxGuards) return fail(err, errlen, RGX_ERR_DEVICE, "regtools_amd: more workspaces in one call than the fill mode's guards (%s)\n", what);
        guard[g] = Guard{what, w.base, w.base + lg.end, std::min(kCarveGuardWindow, cap - lg.end)};
        if (g == n_guards) ++n_guards;
        return RGX_OK;
    }
    void guards_back(CopyBack &back) { for (uint32_t g = 0; g < n_guards; ++g) back(guard_host[g], guard[g].at, guard[g].n); }
    // behind the wait of the CopyBack that guards_back() went into
    int guards_check() {
        for (uint32_t g = 0; g < n_guards; ++g)
            if (!carve_guard_check(guard_host[g], guard[g].n, guard[g].what, err, errlen)) return RGX_ERR_DEVICE;
        return RGX_OK;
    }
    // b holds `bytes` or the call fails with this message
    int grow(DevBuf &b, size_t bytes, const char *fmt, ...) {
        if (b.ensure(bytes) == hipSuccess) return RGX_OK;
        (void)hipGetLastError();
        if (err && errlen) { va_list ap; va_start(ap, fmt); vsnprintf(err, errlen, fmt, ap); va_end(ap); }
        return RGX_ERR_DEVICE;
    }
};
// a run's events: all created in front of their first record, all destroyed with the run
template <size_t N> struct Events {
    hipEvent_t e[N] = {};
    ~Events() { for (hipEvent_t x : e) if (x) (void)hipEventDestroy(x); }
    hipError_t create() { hipError_t rc = hipSuccess; for (hipEvent_t &x : e) if (rc == hipSuccess) rc = hipEventCreate(&x); return rc; }
    hipEvent_t operator[](size_t i) const { return e[i]; }
};

// cohort_cluster.cpp: where the kernels read matrix m of n > 0 rows -- its image in HBM when m is the matrix of co's last finish, else the
// columns the cluster and phenotype kernels need, uploaded on st into co->cl_in
int cohort_matrix_image(rgx_cohort *co, const rgx_cohort_matrix *m, hipStream_t st, CohortImage *in, char *err, size_t errlen);

// cohort_pcs.cpp: T[r - 2] = rgx_pheno_quantile(r, K) for r = 2 .. 2 K, the table the principal components and the sQTL scan look rank2 up in
void pheno_quantile_table(uint64_t K, std::vector<double> &T);
