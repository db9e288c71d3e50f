// qtl_run.h -- what the nominal cis-sQTL scan (cohort_qtl.cpp) and its permutation pass (cohort_qtl_perm.cpp) share: the arguments and their checks,
// the host half of the contract (basis, dot64, residual, the twin's steps (1)-(6)) and QtlRun, the device stages both calls are made of, defined
// in cohort_qtl.cpp; then what the permutation pass shares with the grouped pass (cohort_qtl_group.cpp), PermRun among it, defined in
// cohort_qtl_perm.cpp.  The results' blocks are result_block.h's, their copies back CopyBack's and their text text_out.h's (cohort_internal.h).
#pragma once
#include "cohort_internal.h"
#include "qtl_core.h"

struct QtlArgs {
    const rgx_pheno_table *ph; const rgx_qtl_region *regions; uint32_t V; const uint32_t *var_tid, *var_pos; const int8_t *dosage;
    uint32_t n_cov; const double *cov; uint32_t window;
};

// the arguments the host can judge, the same for the device and the twin
int check_qtl(const QtlArgs &a, char *err, size_t errlen);
// RGX_ERR_ARG for a raised flag word of the device (qtl_core.h), RGX_OK for none
int bad_flags(const uint32_t *flag, uint64_t K, char *err, size_t errlen);
// Q (C x S) = the orthonormal basis of the intercept and the covariates
int qtl_basis(uint32_t S, uint32_t n_cov, const double *cov, std::vector<double> &Q, char *err, size_t errlen);

// Steps (1)-(6) of the contract in plain C++, as both host twins run them: the residuals row-major, yy, gg, the verdicts, the usable variants and
// per row its range [lo, lo + cnt) among them; P = the sum of cnt.  t_res and t_pairs: now_ms() in front of and behind the residual loops.
struct QtlHost {
    std::vector<double> T, Q, Y, G, yy, gg; std::vector<uint8_t> verdict; std::vector<uint32_t> u_var, lo, cnt; std::vector<uint64_t> u_key;
    uint64_t P = 0; double t_res = 0, t_pairs = 0;
};
int qtl_host_prepare(const QtlArgs &a, QtlHost &h, char *err, size_t errlen);
// the continued fraction of the incomplete beta function at (a, b, x), for rgx_qtl_pvalue and rgx_qtl_betainc
long double qtl_beta_cf(long double a, long double b, long double x);


// What the permutation pass (cohort_qtl_perm.cpp, where they are defined) shares with the grouped pass (cohort_qtl_group.cpp).  A SERIES of B + 1
// values is a table row's, or a group's with its member lists.
// the permutations as the host can judge them; n_series of `series` ("rows", "groups") get B + 1 values each
int check_perm(uint64_t n_series, const char *series, uint32_t S, uint32_t B, const uint16_t *perm, char *err, size_t errlen);
size_t qtl_host_threads();
// one series of B + 1 |r| values: n_ge, p_perm and, when the series has pairs, the beta approximation with p_beta at best_r; p: room for B doubles
void qtl_series_finish(const double *row, uint32_t B, double best_r, uint32_t dof, bool has_pairs, double *p, uint32_t &n_ge, double &p_perm,
                       double &shape1, double &shape2, double &p_beta, uint8_t &status);
// The twin's products of one series, its members rows[0 .. n) in ascending table row: series[b] = the largest |r| of permutation b over all members'
// cis variants (+0.0 without pairs), and permutation 0's best pair, RGX_NO_PAIR and +0.0 without one.  best_row may be null.
void qtl_series_products(const QtlHost &h, uint32_t S, uint32_t B, const uint16_t *perm, const uint32_t *rows, uint32_t n, double *series,
                         uint32_t *best_row, uint32_t &best_variant, double &best_r, double &best_slope);

// The members of every group in ascending table row.
struct Members { std::vector<uint32_t> begin, row; };
// What a series is in each of the two results.  Without lists (begin null) series k is table row k alone and its pairs are n_cis[k].
struct Series { uint64_t n; const uint32_t *begin, *row; uint64_t *pairs; uint32_t *best_row; };
inline Series series_of(rgx_qtl_perm_result *q) { return {q->n_rows, nullptr, nullptr, nullptr, nullptr}; }
inline Series series_of(rgx_qtl_group_result *q) { return {q->n_groups, q->grp_begin, q->grp_row, q->group_n_cis, q->best_row}; }
// the pair counts of the series (and the grouped result's n_pairs), the verdict counts, the tile count, then qtl_series_finish for every series,
// sixteen a task among the host's threads; q's arrays from steps (1)-(6), its lists and perm_r, best_* are in place
template <class R> int perm_finish(R *q, bool device, char *err, size_t errlen);

// the verdict counts of any of the three results: constant and explained variants, rows without enough variance
template <class R> void count_verdicts(R *q) {
    for (uint32_t v = 0; v < q->n_variants; ++v) { q->n_constant += q->variant_verdict[v] == 1; q->n_explained += q->variant_verdict[v] == 2; }
    for (uint64_t k = 0; k < q->n_rows; ++k) q->n_flat_rows += !qtl_enough(q->yy[k], q->n_samples);
}

// what the three sQTL texts ask of their arguments: the clusters are the matrix's, every table row is a clustered matrix row, and the result
// q (null: the header line alone) is the table's and comes with its variants' positions and ids
template <class Q> bool qtl_text_args_ok(const rgx_cohort_matrix *m, const rgx_cohort_clusters *cl, const rgx_pheno_table *ph, const Q *q,
                                         const uint32_t *var_pos, const char *const *variant_id) {
    if (!m || !cl || !ph || cl->n_rows != m->n || (q && (q->n_rows != ph->n_rows || (q->n_variants && (!var_pos || !variant_id))))) return false;
    for (uint64_t k = 0; k < ph->n_rows; ++k) if (ph->row[k] >= m->n || cl->cluster[ph->row[k]] == RGX_NO_CLUSTER) return false;
    return true;
}

// One device run, as the stages rgx_cohort_qtl_nominal is made of.  The caller holds the cohort's lock and has checked the arguments; every stage
// enqueues on the cohort's stream and returns RGX_OK or the failed call's code.
struct QtlRun {
    rgx_cohort *co; QtlArgs a; char *err; size_t errlen;
    double t0, t_last; bool trace = false; hipStream_t st = nullptr;
    bool best_only = false;                                       // the permutation pass: no Yt, no pair arrays (set in front of open())
    hipEvent_t ev[4] = {nullptr, nullptr, nullptr, nullptr};     // uploads begin, residuals done, products begin, best done
    uint32_t K, S, V, C, n_blocks; size_t ldy, ldg;
    uint64_t P = 0, n_tiles = 0;
    std::vector<double> T, Q;
    // uploads
    const double *d_T = nullptr, *d_Q = nullptr; const uint32_t *rank2 = nullptr, *regions = nullptr, *var_tid = nullptr, *var_pos = nullptr;
    const int8_t *dosage = nullptr;
    // per row and per variant
    double *Y = nullptr, *G = nullptr, *yy = nullptr, *gg = nullptr, *u_gg = nullptr; uint64_t *u_key = nullptr, *head = nullptr;
    uint32_t *usable = nullptr, *place = nullptr, *u_var = nullptr, *lo = nullptr, *count = nullptr, *pair_begin = nullptr, *blk_lo = nullptr,
             *tile_count = nullptr, *tile_begin = nullptr, *tmp = nullptr; uint8_t *verdict = nullptr;
    double *Yt = nullptr, *Gt = nullptr;
    double *r = nullptr, *slope = nullptr; uint32_t *pair_variant = nullptr, *best = nullptr;

    QtlRun(rgx_cohort *co_, const QtlArgs &a_, char *err_, size_t errlen_)
        : co(co_), a(a_), err(err_), errlen(errlen_), t0(now_ms()), t_last(t0), K((uint32_t)a_.ph->n_rows), S(a_.ph->n_samples), V(a_.V),
          C(a_.n_cov + 1), n_blocks((K + kQtlTile - 1) / kQtlTile), ldy((size_t)n_blocks * kQtlTile),
          ldg(((size_t)a_.V + kQtlTile - 1) / kQtlTile * kQtlTile + kQtlTile) {}
    ~QtlRun() { for (hipEvent_t e : ev) if (e) (void)hipEventDestroy(e); }
    void mark(const char *what) {
        if (!trace) return;
        (void)hipStreamSynchronize(st);
        const double t = now_ms();
        fprintf(stderr, "[rgx trace] qtl %s: %-28s +%8.3f ms\n", best_only ? "permute" : "nominal", what, t - t_last); t_last = t;
    }
    uint32_t *flag() const { return (uint32_t *)(head + 2); }                 // head: P, the tile count, the two flag words, the usable variants
    uint32_t *n_usable() const { return (uint32_t *)(head + 3); }

    // 1. the quantile table and the basis (host), then the inputs in HBM and the workspaces
    int open() {
        HIP_ENTER(co->device);
        st = co->stream;
        trace = getenv("REGTOOLS_AMD_TRACE") != nullptr;
        try { pheno_quantile_table(K, T); }
        catch (const std::bad_alloc &) { return fail(err, errlen, RGX_ERR_ARG, "regtools_amd: no memory for the %llu quantiles\n", (unsigned long long)(2ull * K - 1)); }
        int rc = qtl_basis(S, a.n_cov, a.cov, Q, err, errlen);
        if (rc != RGX_OK) return rc;
        mark("quantile table + basis");
        for (hipEvent_t &e : ev) HIP_TRY(hipEventCreate(&e));
        const size_t n_T = 2 * (size_t)K - 1, n_Q = (size_t)C * S, n_ks = (size_t)K * S, n_vs = (size_t)V * S;
        if (co->qt_in.ensure((n_T + n_Q) * 8 + (n_ks + 3 * (size_t)K + 2 * (size_t)V) * 4 + n_vs + 256) != hipSuccess) { (void)hipGetLastError();
            return fail(err, errlen, RGX_ERR_DEVICE, "regtools_amd: no device memory for a table of %u rows, %u variants and %u samples\n", K, V, S); }
        Carve u(co->qt_in);
        double *t_up = u.take<double>(n_T), *q_up = u.take<double>(n_Q);
        uint32_t *r_up = u.u32(n_ks), *g_up = u.u32(3 * (size_t)K), *vt_up = u.u32(V), *vp_up = u.u32(V); int8_t *d_up = u.take<int8_t>(n_vs);
        CARVE_TRY(u, "sQTL input");
        const size_t n_scan = std::max<size_t>(std::max<size_t>((size_t)K + 1, V), (size_t)n_blocks + 1);
        if (co->qt_rows.ensure((n_ks + n_vs + K + 2 * (size_t)V) * 8 + (size_t)V * 8 + 32 +
                               (3 * (size_t)V + 3 * (size_t)K + 2 + 3 * (size_t)n_blocks + 2 + scan_tmp_words((uint32_t)n_scan)) * 4 + V + 256) != hipSuccess) {
            (void)hipGetLastError();
            return fail(err, errlen, RGX_ERR_DEVICE, "regtools_amd: no device memory for the residuals of %u rows and %u variants\n", K, V); }
        Carve w(co->qt_rows);
        Y = w.take<double>(n_ks); G = w.take<double>(n_vs); yy = w.take<double>(K); gg = w.take<double>(V); u_gg = w.take<double>(V);
        u_key = w.u64(V); head = w.u64(4);
        usable = w.u32(V); place = w.u32(V); u_var = w.u32(V); lo = w.u32(K); count = w.u32((size_t)K + 1); pair_begin = w.u32((size_t)K + 1);
        blk_lo = w.u32(n_blocks); tile_count = w.u32((size_t)n_blocks + 1); tile_begin = w.u32((size_t)n_blocks + 1);
        tmp = w.u32(scan_tmp_words((uint32_t)n_scan)); verdict = w.u8(V);
        CARVE_TRY(w, "sQTL row");
        const size_t ldy_used = best_only ? 0 : ldy;
        if (co->qt_t.ensure((size_t)S * (ldy_used + ldg) * 8 + 256) != hipSuccess) { (void)hipGetLastError();
            return fail(err, errlen, RGX_ERR_DEVICE, "regtools_amd: no device memory for the sample-major residuals of %u rows and %u variants\n", K, V); }
        Carve t(co->qt_t);
        Yt = t.take<double>((size_t)S * ldy_used); Gt = t.take<double>((size_t)S * ldg);
        CARVE_TRY(t, "sQTL panel");
        HIP_TRY(hipEventRecord(ev[0], st));
        HIP_TRY(hipMemcpyAsync(r_up, a.ph->rank2, n_ks * 4, hipMemcpyHostToDevice, st));
        HIP_TRY(hipMemcpyAsync(t_up, T.data(), n_T * 8, hipMemcpyHostToDevice, st));
        HIP_TRY(hipMemcpyAsync(q_up, Q.data(), n_Q * 8, hipMemcpyHostToDevice, st));
        HIP_TRY(hipMemcpyAsync(g_up, a.regions, (size_t)K * 12, hipMemcpyHostToDevice, st));
        if (V) {
            HIP_TRY(hipMemcpyAsync(vt_up, a.var_tid, (size_t)V * 4, hipMemcpyHostToDevice, st));
            HIP_TRY(hipMemcpyAsync(vp_up, a.var_pos, (size_t)V * 4, hipMemcpyHostToDevice, st));
            HIP_TRY(hipMemcpyAsync(d_up, a.dosage, n_vs, hipMemcpyHostToDevice, st));
        }
        HIP_TRY(hipMemsetAsync(head, 0, 32, st));
        d_T = t_up; d_Q = q_up; rank2 = r_up; regions = g_up; var_tid = vt_up; var_pos = vp_up; dosage = d_up;
        mark("inputs in HBM");
        return RGX_OK;
    }
    // 2. a wave per row and per variant
    int residuals() {
        launch_qtl_residual_pheno(rank2, d_T, K, S, d_Q, C, Y, yy, flag(), st);
        launch_qtl_residual_geno(dosage, V, S, d_Q, C, G, gg, verdict, usable, flag(), st);
        mark("residuals");
        return RGX_OK;
    }
    // 3. the usable variants side by side; both sides sample-major
    int compact() {
        launch_scan_u32(usable, place, V, n_usable(), tmp, st);
        launch_qtl_compact(usable, place, V, var_tid, var_pos, gg, u_var, u_key, u_gg, st);
        if (!best_only) launch_qtl_transpose(Y, nullptr, nullptr, K, S, ldy, Yt, st);
        launch_qtl_transpose(G, u_var, n_usable(), 0, S, ldg, Gt, st);
        HIP_TRY(hipEventRecord(ev[1], st));
        mark("compaction + transposes");
        return RGX_OK;
    }
    // 4. the rows' ranges [lo, lo + count), the tiles, and P and the tile count in head: enqueued, no wait
    int plan_launch() {
        launch_qtl_plan(regions, K, S, yy, u_key, n_usable(), a.window, lo, count, blk_lo, tile_count, (unsigned long long *)head, st);
        return RGX_OK;
    }
    // the nominal scan's own stages (cohort_qtl.cpp): the wait for P and the pair arrays, the products, the copies back
    int plan();
    int pairs();
    int finish(rgx_qtl_result **out);
};

// The device run of the permutation pass, ungrouped (mem null: series k is table row k) or grouped: QtlRun's shared stages with the permutation
// stage behind them.  `series` ("rows", "groups") is the word the messages use.
struct PermRun {
    QtlRun run; uint32_t B; const uint16_t *perm; size_t ldp; uint32_t n_series; const char *series; const Members *mem;
    std::vector<uint16_t> permT;
    uint16_t *d_permT = nullptr; uint32_t *d_begin = nullptr, *d_row = nullptr;
    double *perm_r = nullptr, *best_r = nullptr, *best_slope = nullptr; uint32_t *best_row = nullptr, *best_u = nullptr, *best_variant = nullptr;

    PermRun(rgx_cohort *co, const QtlArgs &a, uint32_t B_, const uint16_t *perm_, uint32_t n_series_, const char *series_, const Members *mem_,
            char *err, size_t errlen)
        : run(co, a, err, errlen), B(B_), perm(perm_), ldp(((size_t)B_ + 1 + kQtlTile - 1) / kQtlTile * kQtlTile), n_series(n_series_),
          series(series_), mem(mem_) { run.best_only = true; }
    // 1.-5. every stage up to the products and the best pairs, enqueued: no wait
    int launch();
    // 5. the member lists and the permutations sample-major in HBM, the products, the best pairs
    int products();
    // 6. the copies back into q behind the call's one wait, then the host's part (perm_finish); q stays the caller's
    template <class R> int finish(R *q);
    // RGX_ERR_DEVICE: q could not be had
    int no_result();
};
