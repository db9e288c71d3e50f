// cohort_qtl_perm.cpp -- the permutation pass of the cohort's cis-sQTL scan: rgx_cohort_qtl_permute (device), its host twin
// rgx_cohort_qtl_permute_host and the text (contract in include/regtools_amd.h; FastQTL's --permute and tensorQTL's map_cis, which the reference
// does not contain).  Device side: qtl_perm_kernels.hip behind QtlPrep's shared stages (qtl_run.h, qtl_prep.cpp); arithmetic: qtl_core.h; the beta
// approximation of one series and the permutation generator: qtl_stats.cpp.  What is defined here over SERIES -- PermRun, check_perm, perm_finish,
// the twin's qtl_series_products -- is the grouped pass's too (cohort_qtl_group.cpp), where a series is a group; here it is table row k alone.
//   QtlPrep: inputs in HBM -> residuals Y, G with yy, gg and the verdicts -> the usable variants compacted -> Gt sample-major -> per row its range
//   -> the permutations sample-major in HBM -> one workgroup per (row, 64 permutations): perm_r -> a thread per row: the best pair of permutation 0
//   -> ONE wait, the copies back -> on the host: n_ge, p_perm, the beta approximation
#include "qtl_run.h"

#include <cmath>

rgx_qtl_perm_result *perm_alloc(uint64_t K, uint32_t S, uint32_t V, uint32_t n_cov, uint32_t B, bool pinned) {
    rgx_qtl_perm_result *q = result_alloc<rgx_qtl_perm_result>(pinned, [&](rgx_qtl_perm_result &r, BlockTake &take) {
        take(r.yy, K); take(r.gg, V); take(r.perm_r, K * ((size_t)B + 1)); take(r.best_r, K); take(r.best_slope, K); take(r.p_perm, K);
        take(r.beta_shape1, K); take(r.beta_shape2, K); take(r.p_beta, K); take(r.n_cis, K); take(r.best_variant, K); take(r.n_ge, K);
        take(r.variant_verdict, V); take(r.beta_status, K);
    });
    if (q) { qtl_result_head(q, K, S, V, n_cov); q->n_perm = B; }
    return q;
}

// what the host can judge of the permutations, the same for the device and the twin; n_series of `series` (rows, groups) get B + 1 values each
int check_perm(uint64_t n_series, const char *series, uint32_t S, uint32_t B, const uint16_t *perm, char *err, size_t errlen) {
    if (!B || B > 65535u) return fail(err, errlen, RGX_ERR_ARG, "regtools_amd: the permutation pass takes 1 to 65535 permutations; %u were asked for\n", B);
    if (!perm) return fail(err, errlen, RGX_ERR_ARG, "regtools_amd: the permutation pass needs its permutations\n");
    if (n_series * ((uint64_t)B + 1) > kQtlMaxPairs) return fail(err, errlen, RGX_ERR_ARG,
        "regtools_amd: %llu %s x %u permutations and the identity; the permutation pass takes at most 2^32 - 2^16 of them\n",
        (unsigned long long)n_series, series, B);
    for (uint32_t s = 0; s < S; ++s) if (perm[s] != s) return fail(err, errlen, RGX_ERR_ARG,
        "regtools_amd: row 0 of the permutations is not the identity (sample %u stands at %u)\n", (uint32_t)perm[s], s);
    std::vector<uint8_t> seen(S);
    for (uint32_t b = 1; b <= B; ++b) {
        std::fill(seen.begin(), seen.end(), 0);
        const uint16_t *row = perm + (size_t)b * S;
        for (uint32_t s = 0; s < S; ++s) {
            if (row[s] >= S || seen[row[s]]) return fail(err, errlen, RGX_ERR_ARG,
                "regtools_amd: row %u of the permutations is no permutation of 0 .. %u (index %u at %u)\n", b, S - 1, (uint32_t)row[s], s);
            seen[row[s]] = 1;
        }
    }
    return RGX_OK;
}

// The twin's products of one series (qtl_run.h)
void qtl_series_products(const QtlHost &h, uint32_t S, uint32_t B, const uint16_t *perm, const uint32_t *rows, uint32_t n, double *series,
                         uint32_t *best_row, uint32_t &best_variant, double &best_r, double &best_slope) {
    std::vector<double> yp(S);
    std::vector<uint64_t> top((size_t)B + 1, 0);
    if (best_row) *best_row = RGX_NO_PAIR;
    best_variant = RGX_NO_PAIR; best_r = 0.0; best_slope = 0.0;
    // members in ascending row, variants in ascending order: a strictly larger |r| alone replaces, so the earliest of equals stays
    for (uint32_t i = 0; i < n; ++i) {
        const uint32_t k = rows[i];
        const double *y = h.Y.data() + (size_t)k * S;
        for (uint32_t b = 0; b <= B && h.cnt[k]; ++b) {
            const uint16_t *pb = perm + (size_t)b * S;
            for (uint32_t s = 0; s < S; ++s) yp[s] = y[pb[s]];
            for (uint32_t j = 0; j < h.cnt[k]; ++j) {
                const uint32_t v = h.u_var[h.lo[k] + j]; const double *x = h.G.data() + (size_t)v * S;
                double acc = 0.0;
                for (uint32_t s = 0; s < S; ++s) acc = qtl_fma(yp[s], x[s], acc);
                const double r = qtl_r(acc, h.yy[k], h.gg[v]);
                const uint64_t bits = qtl_abs_bits(r);
                if (!b && (best_variant == RGX_NO_PAIR || bits > top[0])) {
                    if (best_row) *best_row = k;
                    best_variant = v; best_r = r; best_slope = qtl_slope(acc, h.gg[v]);
                }
                if (bits > top[b]) top[b] = bits;
            }
        }
    }
    memcpy(series, top.data(), ((size_t)B + 1) * 8);
}

static const char *const kNoPermMemory = "regtools_amd: no device memory for %u permutations of %u %s\n";

template <class R> int perm_finish(R *q, bool device, char *err, size_t errlen) {
    const Series sr = series_of(q);
    const uint64_t N = sr.n; const uint32_t B = q->n_perm, dof = q->dof;
    count_verdicts(q);
    const uint64_t p_tiles = ((uint64_t)B + 1 + kQtlTile - 1) / kQtlTile;
    for (uint64_t g = 0; g < N; ++g) {
        const uint32_t m_end = sr.begin ? sr.begin[g + 1] : (uint32_t)g + 1;
        uint64_t n = 0;
        for (uint32_t m = sr.begin ? sr.begin[g] : (uint32_t)g; m < m_end; ++m) {
            const uint32_t c = q->n_cis[sr.row ? sr.row[m] : m];
            n += c;
            if (device) q->n_tiles += p_tiles * (((uint64_t)c + kQtlTile - 1) / kQtlTile);
        }
        if (sr.pairs) { sr.pairs[g] = n; q->n_pairs += n; }
    }
    const double t0 = now_ms();
    try {
        WorkerPool pool(N * B < 4096 ? 1 : qtl_host_threads());
        const uint64_t chunk = 16, n_tasks = (N + chunk - 1) / chunk;
        pool.run((size_t)n_tasks, [&](size_t task) {
            std::vector<double> p(B);
            for (uint64_t g = task * chunk; g < N && g < (task + 1) * chunk; ++g)
                qtl_series_finish(q->perm_r + g * ((size_t)B + 1), B, q->best_r[g], dof, (sr.pairs ? sr.pairs[g] : q->n_cis[g]) != 0, p.data(),
                                  q->n_ge[g], q->p_perm[g], q->beta_shape1[g], q->beta_shape2[g], q->p_beta[g], q->beta_status[g]);
        });
    } catch (const std::exception &) { return fail(err, errlen, RGX_ERR_ARG, "regtools_amd: no memory or threads for the beta approximation\n"); }
    q->ms_beta = now_ms() - t0;
    return RGX_OK;
}
template int perm_finish(rgx_qtl_perm_result *, bool, char *, size_t);
template int perm_finish(rgx_qtl_group_result *, bool, char *, size_t);

int PermRun::stage_perms() {
    const uint32_t N = n_series;
    if ((uint64_t)N * (ldp / kQtlTile) > 0x7fffffffull) return fail(err, errlen, RGX_ERR_ARG,
        "regtools_amd: %u %s x %zu blocks of 64 permutations are more than 2^31 - 1 workgroups\n", N, series, ldp / kQtlTile);
    try { permT.assign((size_t)S * ldp, 0); }
    catch (const std::bad_alloc &) { return fail(err, errlen, RGX_ERR_ARG, "regtools_amd: no memory for %u permutations of %u samples\n", B, S); }
    for (uint32_t b = 0; b <= B; ++b) for (uint32_t s = 0; s < S; ++s) permT[(size_t)s * ldp + b] = perm[(size_t)b * S + s];
    const size_t n_begin = mem ? (size_t)N + 1 : 0, n_mem = mem ? mem->row.size() : 0;
    if (int rc = grow(co->qp_in, permT.size() * 2 + (n_begin + n_mem) * 4 + 256, kNoPermMemory, B, N, series)) return rc;
    Carve in = carve(co->qp_in);                              // (every array written whole by its upload)
    d_permT = in.take<uint16_t>(permT.size());
    if (mem) { d_begin = in.u32(n_begin); d_row = in.u32(n_mem); }
    CARVE_TRY(in, mem ? "grouped sQTL permutation" : "sQTL permutation");
    if (int rc = carved(in, mem ? "grouped sQTL permutation" : "sQTL permutation")) return rc;
    HIP_TRY(hipMemcpyAsync(d_permT, permT.data(), permT.size() * 2, hipMemcpyHostToDevice, st));
    if (mem) { HIP_TRY(hipMemcpyAsync(d_begin, mem->begin.data(), n_begin * 4, hipMemcpyHostToDevice, st)); }
    if (n_mem) { HIP_TRY(hipMemcpyAsync(d_row, mem->row.data(), n_mem * 4, hipMemcpyHostToDevice, st)); }
    mark(mem ? "members + permutations in HBM" : "permutations in HBM");
    return RGX_OK;
}

int PermRun::series_products() {
    const uint32_t N = n_series;
    const size_t n_out = (size_t)N * ((size_t)B + 1);
    if (int rc = grow(co->qp_out, n_out * 8 + (size_t)N * (mem ? 28 : 24) + 256, kNoPermMemory, B, N, series)) return rc;
    // first writers: perm_r, best_row, best_u k_qtl_perm (every series, +0.0 and RGX_NO_PAIR without pairs); best_variant, best_r, best_slope
    // k_qtl_perm_best (every series)
    Carve o = carve(co->qp_out);
    perm_r = o.take<double>(n_out); best_r = o.take<double>(N); best_slope = o.take<double>(N); best_u = o.u32(N); best_variant = o.u32(N);
    if (mem) best_row = o.u32(N);
    CARVE_TRY(o, mem ? "grouped sQTL permutation result" : "sQTL permutation result");
    if (int rc = carved(o, mem ? "grouped sQTL permutation result" : "sQTL permutation result")) return rc;
    HIP_TRY(ev_products.create());
    HIP_TRY(hipEventRecord(ev_products[0], st));
    // (without lists all three of d_begin, d_row and best_row are null: series g is table row g alone)
    launch_qtl_perm(Y, N, S, d_permT, ldp, B + 1, Gt, ldg, lo, count, yy, u_gg, d_begin, d_row, perm_r, best_row, best_u, st);
    mark(mem ? "grouped permuted products" : "permuted products");
    launch_qtl_perm_best(Y, G, N, S, best_row, best_u, u_var, yy, gg, best_variant, best_r, best_slope, st);
    HIP_TRY(hipEventRecord(ev_products[1], st));
    mark("best pairs");
    return RGX_OK;
}

template <class R> int PermRun::finish(R *q) {
    const size_t N = n_series;
    uint64_t h[4] = {0, 0, 0, 0};
    CopyBack back{st};
    copy_back(back, q);
    back(q->n_cis, count, (size_t)K * 4); back(q->perm_r, perm_r, N * ((size_t)B + 1) * 8); back(q->best_r, best_r, N * 8);
    back(q->best_slope, best_slope, N * 8);
    if (mem) back(series_of(q).best_row, best_row, N * 4);
    back(q->best_variant, best_variant, N * 4); back(h, head, 32);
    float ms_res = 0, ms_pr = 0;
    int rc = wait(back, {{ev[0], ev[1], &ms_res}, {ev_products[0], ev_products[1], &ms_pr}},
                  mem ? "grouped sQTL permutation pass" : "sQTL permutation pass");
    if (rc != RGX_OK) return rc;
    rc = bad_flags((const uint32_t *)(h + 2), K, err, errlen);
    if (rc != RGX_OK) return rc;
    if (!mem) q->n_pairs = h[0];                                      // (the grouped result's is the sum over its groups: perm_finish)
    rc = perm_finish(q, /*device=*/true, err, errlen);
    if (rc != RGX_OK) return rc;
    q->ms_residual = ms_res; q->ms_products = ms_pr; q->ms_perm = now_ms() - t0;
    return RGX_OK;
}
template int PermRun::finish(rgx_qtl_perm_result *);
template int PermRun::finish(rgx_qtl_group_result *);

extern "C" void rgx_cohort_qtl_perm_free(rgx_qtl_perm_result *q) { result_free(q); }

extern "C" int rgx_cohort_qtl_permute(rgx_cohort *co, const rgx_pheno_table *ph, const rgx_qtl_region *regions, uint32_t n_variants,
                                      const uint32_t *var_tid, const uint32_t *var_pos, const int8_t *dosage, uint32_t n_cov, const double *covariates,
                                      uint32_t window, uint32_t n_perm, const uint16_t *perm, rgx_qtl_perm_result **out, char *err, size_t errlen) {
    if (!co || !ph || !out) return fail(err, errlen, RGX_ERR_ARG, "regtools_amd: rgx_cohort_qtl_permute needs a cohort and a phenotype table\n");
    *out = nullptr;
    std::lock_guard<std::mutex> lock(co->mu);
    QtlArgs a; int rc = qtl_args(a, ph, regions, n_variants, var_tid, var_pos, dosage, n_cov, covariates, window, err, errlen);
    if (rc == RGX_OK) rc = check_perm(ph->n_rows, "rows", ph->n_samples, n_perm, perm, err, errlen);
    if (rc != RGX_OK) return rc;
    PermRun p(co, a, n_perm, perm, (uint32_t)ph->n_rows, "rows", nullptr, err, errlen);
    rc = p.launch();
    rgx_qtl_perm_result *q = nullptr;
    if (rc == RGX_OK && !(q = perm_alloc(ph->n_rows, ph->n_samples, n_variants, n_cov, n_perm, /*pinned=*/true))) rc = p.no_result();
    if (rc == RGX_OK) rc = p.finish(q);
    if (p.done(rc) != RGX_OK) { rgx_cohort_qtl_perm_free(q); return rc; }
    *out = q;
    return RGX_OK;
}

extern "C" int rgx_cohort_qtl_permute_host(const rgx_pheno_table *ph, const rgx_qtl_region *regions, uint32_t n_variants, const uint32_t *var_tid,
                                           const uint32_t *var_pos, const int8_t *dosage, uint32_t n_cov, const double *covariates, uint32_t window,
                                           uint32_t n_perm, const uint16_t *perm, rgx_qtl_perm_result **out, char *err, size_t errlen) {
    if (!ph || !out) return fail(err, errlen, RGX_ERR_ARG, "regtools_amd: rgx_cohort_qtl_permute_host needs a phenotype table\n");
    *out = nullptr;
    const double t0 = now_ms();
    QtlArgs a; int rc = qtl_args(a, ph, regions, n_variants, var_tid, var_pos, dosage, n_cov, covariates, window, err, errlen);
    if (rc == RGX_OK) rc = check_perm(ph->n_rows, "rows", ph->n_samples, n_perm, perm, err, errlen);
    if (rc != RGX_OK) return rc;
    QtlHost h;
    rc = qtl_host_prepare(a, h, err, errlen);
    if (rc != RGX_OK) return rc;
    const uint64_t K = ph->n_rows; const uint32_t S = ph->n_samples, V = n_variants, B = n_perm;
    rgx_qtl_perm_result *q = perm_alloc(K, S, V, n_cov, B, false);
    if (!q) return fail(err, errlen, RGX_ERR_ARG, "regtools_amd: no memory for the result of %llu rows and %u permutations\n", (unsigned long long)K, B);
    qtl_result_fill(q, h);
    memcpy(q->n_cis, h.cnt.data(), K * 4);
    q->n_pairs = h.P;
    try {
        WorkerPool pool(h.P * ((uint64_t)B + 1) * S < (1u << 20) ? 1 : qtl_host_threads());
        pool.run((size_t)K, [&](size_t k) {
            const uint32_t row = (uint32_t)k;
            qtl_series_products(h, S, B, perm, &row, 1, q->perm_r + k * ((size_t)B + 1), nullptr, q->best_variant[k], q->best_r[k], q->best_slope[k]);
        });
    } catch (const std::exception &) { rgx_cohort_qtl_perm_free(q); return fail(err, errlen, RGX_ERR_ARG, "regtools_amd: no memory or threads for the permutation pass\n"); }
    const double t1 = now_ms();
    rc = perm_finish(q, /*device=*/false, err, errlen);
    if (rc != RGX_OK) { rgx_cohort_qtl_perm_free(q); return rc; }
    q->ms_residual = h.t_pairs - h.t_res; q->ms_products = t1 - h.t_pairs; q->ms_perm = now_ms() - t0;
    *out = q;
    return RGX_OK;
}

// ---- text ---------------------------------------------------------------------------------------------------------------------------------------------
extern "C" size_t rgx_cohort_format_qtl_perm(const rgx_cohort_matrix *m, const rgx_cohort_clusters *cl, const rgx_pheno_table *ph,
                                             const rgx_qtl_perm_result *q, const uint32_t *var_pos, const char *const *variant_id, char *buf, size_t cap) {
    if (!qtl_text_args_ok(m, cl, ph, q, var_pos, variant_id)) return 0;
    return format_twice(buf, cap, [&](TextOut &o) {
        o.put("phenotype_id\tnum_var\tbeta_shape1\tbeta_shape2\tdof\tvariant_id\tdistance\tr\tslope\tslope_se\ttstat\tpval_nominal\t"
              "pval_perm\tpval_beta\n");
        for (uint64_t k = 0; q && k < q->n_rows; ++k) {
            if (!q->n_cis[k]) continue;
            const uint32_t i = ph->row[k], v = q->best_variant[k];
            const double t = rgx_qtl_tstat(q->best_r[k], q->dof);
            put_intron_id(o, m, cl, i);
            o.fmt("\t%u\t", q->n_cis[k]);
            o.g17(q->beta_shape1[k], '\t'); o.g17(q->beta_shape2[k], '\t');
            o.fmt("%u\t", q->dof);
            o.put(variant_id[v]);
            o.fmt("\t%lld\t", (long long)var_pos[v] - (long long)m->start[i]);
            o.g17(q->best_r[k], '\t'); o.g17(q->best_slope[k], '\t'); o.g17(q->best_slope[k] / t, '\t'); o.g17(t, '\t');
            o.g17(rgx_qtl_pvalue(t, q->dof), '\t'); o.g17(q->p_perm[k], '\t'); o.g17(q->p_beta[k], '\n');
        }
    });
}
