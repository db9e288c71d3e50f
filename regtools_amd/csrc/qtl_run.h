// qtl_run.h -- what the four sQTL calls share: the nominal scan (cohort_qtl.cpp), the permutation pass (cohort_qtl_perm.cpp), the grouped pass
// (cohort_qtl_group.cpp), the trans scan (cohort_qtl_trans.cpp) and the conditional pass with its forward-backward search (cohort_qtl_cond.cpp).  The arguments and their checks, the host half of the contract (the basis and
// the twins' steps (1)-(6)) and QtlPrep, the device stages every call begins with, are defined in qtl_prep.cpp; the host's mathematics in
// qtl_stats.cpp; what the permutation pass shares with the grouped pass, PermRun among it, in cohort_qtl_perm.cpp.  A run's base is CohortRun, the
// results' blocks are result_block.h's, their copies back CopyBack's and their text text_out.h's (cohort_internal.h).
#pragma once
#include "cohort_internal.h"
#include "qtl_core.h"

struct QtlArgs {
    const rgx_pheno_table *ph; const rgx_qtl_region *regions; uint32_t V; const uint32_t *var_tid, *var_pos; const int8_t *dosage;
    uint32_t n_cov; const double *cov; uint32_t window;
};

// a = the entry point's arguments, checked as far as the host can judge them, the same for the device and the twin
int qtl_args(QtlArgs &a, const rgx_pheno_table *ph, const rgx_qtl_region *regions, uint32_t V, const uint32_t *var_tid, const uint32_t *var_pos,
             const int8_t *dosage, uint32_t n_cov, const double *cov, uint32_t window, char *err, size_t errlen);
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

// What the permutation pass (cohort_qtl_perm.cpp, where they are defined but for qtl_host_threads: qtl_prep.cpp, and qtl_series_finish:
// qtl_stats.cpp) shares with the grouped pass (cohort_qtl_group.cpp).  A SERIES of B + 1 values is a table row's, or a group's with its member lists.
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

// the permutation pass's result with its head filled in (cohort_qtl_perm.cpp); null: no memory
rgx_qtl_perm_result *perm_alloc(uint64_t K, uint32_t S, uint32_t V, uint32_t n_cov, uint32_t B, bool pinned);

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

// What every sQTL result carries in front of its own fields
template <class R> void qtl_result_head(R *q, uint64_t K, uint32_t S, uint32_t V, uint32_t n_cov) {
    q->n_rows = K; q->n_samples = S; q->n_variants = V; q->n_cov = n_cov; q->dof = S - n_cov - 2;
}
// the twins: yy, gg and the verdicts out of steps (1)-(6)
template <class R> void qtl_result_fill(R *q, const QtlHost &h) {
    memcpy(q->yy, h.yy.data(), q->n_rows * 8);
    if (q->n_variants) { memcpy(q->gg, h.gg.data(), (size_t)q->n_variants * 8); memcpy(q->variant_verdict, h.verdict.data(), q->n_variants); }
}

// The shared device stages of the four sQTL calls: the inputs in HBM, the residuals, the usable variants side by side, the panels sample-major and
// the rows' ranges (qtl_prep.cpp).  Each scan's run derives from it and puts its own stages behind these.  The caller holds the cohort's lock and
// has checked the arguments; every stage enqueues on the cohort's stream and returns RGX_OK or the failed call's code.
struct QtlPrep : CohortRun {
    QtlArgs a; bool want_Yt; size_t own_words;                  // own_words: 32-bit words of the row workspace the deriving run asks for (`own`)
    Events<2> ev;                                               // uploads begin, residuals done
    uint32_t K, S, V, C, n_blocks; size_t ldy, ldg;
    std::vector<double> T, Q;
    // uploads
    const double *d_T = nullptr, *d_Q = nullptr; const uint32_t *rank2 = nullptr, *regions = nullptr, *var_tid = nullptr, *var_pos = nullptr;
    const int8_t *dosage = nullptr;
    // per row and per variant
    double *Y = nullptr, *G = nullptr, *yy = nullptr, *gg = nullptr, *u_gg = nullptr; uint64_t *u_key = nullptr, *head = nullptr;
    uint32_t *usable = nullptr, *place = nullptr, *u_var = nullptr, *lo = nullptr, *count = nullptr, *blk_lo = nullptr, *tile_count = nullptr,
             *own = nullptr, *tmp = nullptr; uint8_t *verdict = nullptr;
    double *Yt = nullptr, *Gt = nullptr;

    // name: the label of the trace lines ("qtl nominal", ...); want_Yt: the rows sample-major too (the scans with tiles of rows)
    QtlPrep(rgx_cohort *co, const char *name, const QtlArgs &a, bool want_Yt, size_t own_words, char *err, size_t errlen);
    uint32_t *flag() const { return (uint32_t *)(head + 2); }                 // head: P, the tile count, the two flag words, the usable variants
    uint32_t *n_usable() const { return (uint32_t *)(head + 3); }

    // 1. the quantile table and the basis (host), then the inputs in HBM and the workspaces
    int open();
    // 2. a wave per row and per variant
    int residuals();
    // 3. the usable variants side by side; both sides sample-major
    int compact();
    // 4. the rows' ranges [lo, lo + count), the tiles, and P and the tile count in head: enqueued, no wait
    int plan_launch();
    // 1.-3. in order
    int prepare() { int rc = open(); if (rc == RGX_OK) rc = residuals(); if (rc == RGX_OK) rc = compact(); return rc; }
    // the end of a device entry point: a failed call waits for the stream, which reads the caller's arrays and this run's, and may write the result
    int done(int rc) { if (rc != RGX_OK && st) (void)hipStreamSynchronize(st); return rc; }
    // the three arrays every result has, enqueued with its others
    template <class R> void copy_back(CopyBack &back, R *q) const {
        back(q->yy, yy, (size_t)K * 8); back(q->gg, gg, (size_t)V * 8); back(q->variant_verdict, verdict, V);
    }
    // the call's one wait in front of its result, then the milliseconds between the events; `where` ends the message of a failure
    struct Interval { hipEvent_t from, to; float *ms; };
    int wait(CopyBack &back, std::initializer_list<Interval> intervals, const char *where);
};

// The device run of the permutation pass, ungrouped (mem null: series k is table row k) or grouped: QtlPrep's shared stages with the permutation
// stage behind them.  `series` ("rows", "groups") is the word the messages use.
struct PermRun : QtlPrep {
    uint32_t B; const uint16_t *perm; size_t ldp; uint32_t n_series; const char *series; const Members *mem;
    Events<2> ev_products;                                      // products begin, best done
    std::vector<uint16_t> permT;
    uint16_t *d_permT = nullptr; uint32_t *d_begin = nullptr, *d_row = nullptr;
    double *perm_r = nullptr, *best_r = nullptr, *best_slope = nullptr; uint32_t *best_row = nullptr, *best_u = nullptr, *best_variant = nullptr;

    PermRun(rgx_cohort *co, const QtlArgs &a, uint32_t B_, const uint16_t *perm_, uint32_t n_series_, const char *series_, const Members *mem_,
            char *err, size_t errlen)
        : QtlPrep(co, "qtl permute", a, /*want_Yt=*/false, 0, err, errlen), B(B_), perm(perm_),
          ldp(((size_t)B_ + 1 + kQtlTile - 1) / kQtlTile * kQtlTile), n_series(n_series_), series(series_), mem(mem_) {}
    // 1.-5. every stage up to the products and the best pairs, enqueued: no wait
    int launch() { int rc = prepare(); if (rc == RGX_OK) rc = plan_launch(); if (rc == RGX_OK) rc = products(); return rc; }
    // 5a. the member lists and the permutations sample-major in HBM (the conditional pass, cohort_qtl_cond.cpp, puts its own products behind them)
    int stage_perms();
    // 5b. the products and the best pairs
    int series_products();
    // 5. 5a, then 5b
    int products() { int rc = stage_perms(); if (rc == RGX_OK) rc = series_products(); return rc; }
    // 6. the copies back into q behind the call's one wait, then the host's part (perm_finish); q stays the caller's
    template <class R> int finish(R *q);
    // RGX_ERR_DEVICE: q could not be had
    int no_result() { return fail(err, errlen, RGX_ERR_DEVICE, "regtools_amd: no memory for the result of %u %s and %u permutations\n", n_series, series, B); }
};
