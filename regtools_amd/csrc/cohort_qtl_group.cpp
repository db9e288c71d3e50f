// cohort_qtl_group.cpp -- the grouped permutation pass of the cohort's cis-sQTL scan: rgx_cohort_qtl_permute_grouped (device), its host twin
// rgx_cohort_qtl_permute_grouped_host, rgx_cohort_pheno_groups and the text (contract in include/regtools_amd.h; FastQTL's --grp and tensorQTL's
// group_s, which the reference does not contain).  What is about groups is here: their checks, the member lists, the result and the text.  The
// device run (PermRun over qtl_perm_kernels.hip, behind QtlPrep's shared stages: qtl_run.h), the twin's products of one series, the permutation
// checks and the finish over series are cohort_qtl_perm.cpp's, where a series without lists is a table row; arithmetic: qtl_core.h.
//   QtlPrep: inputs in HBM -> residuals -> the usable variants compacted -> Gt sample-major -> per row its range
//   -> the groups' member lists (host, counting sort) and the permutations sample-major in HBM -> one workgroup per (group, 64 permutations): perm_r
//   -> a thread per group: the best pair of permutation 0 -> ONE wait, the copies back -> on the host: n_ge, p_perm, the beta approximation
#include "qtl_run.h"

#include <cmath>

namespace {

// the result with its member lists in place
rgx_qtl_group_result *group_alloc(uint64_t K, uint32_t S, uint32_t V, uint32_t n_cov, uint32_t B, uint32_t G, const Members &mem, bool pinned) {
    rgx_qtl_group_result *q = result_alloc<rgx_qtl_group_result>(pinned, [&](rgx_qtl_group_result &r, BlockTake &take) {
        take(r.yy, K); take(r.gg, V); take(r.perm_r, G * ((size_t)B + 1)); take(r.best_r, G); take(r.best_slope, G); take(r.p_perm, G);
        take(r.beta_shape1, G); take(r.beta_shape2, G); take(r.p_beta, G); take(r.group_n_cis, G); take(r.n_cis, K); take(r.grp_begin, (size_t)G + 1);
        take(r.grp_row, mem.row.size()); take(r.best_row, G); take(r.best_variant, G); take(r.n_ge, G); take(r.variant_verdict, V);
        take(r.beta_status, G);
    });
    if (!q) return nullptr;
    qtl_result_head(q, K, S, V, n_cov); q->n_perm = B; q->n_groups = G;
    memcpy(q->grp_begin, mem.begin.data(), ((size_t)G + 1) * 4);
    if (!mem.row.empty()) memcpy(q->grp_row, mem.row.data(), mem.row.size() * 4);
    return q;
}

// what the host can judge of the groups, the same for the device and the twin
int check_groups(uint64_t K, uint32_t G, const uint32_t *group, char *err, size_t errlen) {
    if (!G || G > 0x7fffffffu) return fail(err, errlen, RGX_ERR_ARG, "regtools_amd: the grouped permutation pass takes 1 to 2^31 - 1 groups; %u were given\n", G);
    if (!group) return fail(err, errlen, RGX_ERR_ARG, "regtools_amd: the grouped permutation pass needs the rows' groups\n");
    for (uint64_t k = 0; k < K; ++k) if (group[k] >= G && group[k] != RGX_NO_GROUP) return fail(err, errlen, RGX_ERR_ARG,
        "regtools_amd: row %llu is of group %u; there are %u groups\n", (unsigned long long)k, group[k], G);
    return RGX_OK;
}

// The members of every group in ascending table row: a stable counting sort of group[].
int group_members(uint64_t K, uint32_t G, const uint32_t *group, Members &m, char *err, size_t errlen) {
    try {
        m.begin.assign((size_t)G + 1, 0);
        for (uint64_t k = 0; k < K; ++k) if (group[k] != RGX_NO_GROUP) ++m.begin[group[k] + 1];
        for (uint32_t g = 0; g < G; ++g) m.begin[g + 1] += m.begin[g];
        m.row.resize(m.begin[G]);
        std::vector<uint32_t> at(m.begin.begin(), m.begin.end() - 1);
        for (uint64_t k = 0; k < K; ++k) if (group[k] != RGX_NO_GROUP) m.row[at[group[k]]++] = (uint32_t)k;
    } catch (const std::bad_alloc &) { return fail(err, errlen, RGX_ERR_ARG, "regtools_amd: no memory for the member lists of %u groups\n", G); }
    return RGX_OK;
}

}  // namespace

extern "C" void rgx_cohort_qtl_group_free(rgx_qtl_group_result *q) { result_free(q); }

extern "C" int rgx_cohort_pheno_groups(const rgx_cohort_clusters *cl, const rgx_pheno_table *ph, uint32_t *group_out, uint32_t *n_groups, char *err,
                                       size_t errlen) {
    if (!cl || !ph || !n_groups || (ph->n_rows && !group_out)) return fail(err, errlen, RGX_ERR_ARG,
        "regtools_amd: rgx_cohort_pheno_groups needs the clusters, a phenotype table and room for the groups\n");
    *n_groups = 0;
    for (uint64_t k = 0; k < ph->n_rows; ++k) if (ph->row[k] >= cl->n_rows || cl->cluster[ph->row[k]] == RGX_NO_CLUSTER) return fail(err, errlen,
        RGX_ERR_ARG, "regtools_amd: row %llu of the phenotype table (matrix row %u) is not clustered\n", (unsigned long long)k, ph->row[k]);
    try {
        std::vector<uint32_t> number((size_t)cl->n_clusters, RGX_NO_GROUP);
        uint32_t G = 0;
        for (uint64_t k = 0; k < ph->n_rows; ++k) {
            uint32_t &g = number[cl->cluster[ph->row[k]]];
            if (g == RGX_NO_GROUP) g = G++;
            group_out[k] = g;
        }
        *n_groups = G;
    } catch (const std::bad_alloc &) { return fail(err, errlen, RGX_ERR_ARG, "regtools_amd: no memory for %llu cluster numbers\n",
                                                   (unsigned long long)cl->n_clusters); }
    return RGX_OK;
}

extern "C" int rgx_cohort_qtl_permute_grouped(rgx_cohort *co, const rgx_pheno_table *ph, const rgx_qtl_region *regions, uint32_t n_variants,
                                              const uint32_t *var_tid, const uint32_t *var_pos, const int8_t *dosage, uint32_t n_cov,
                                              const double *covariates, uint32_t window, uint32_t n_perm, const uint16_t *perm, uint32_t n_groups,
                                              const uint32_t *group, rgx_qtl_group_result **out, char *err, size_t errlen) {
    if (!co || !ph || !out) return fail(err, errlen, RGX_ERR_ARG, "regtools_amd: rgx_cohort_qtl_permute_grouped needs a cohort and a phenotype table\n");
    *out = nullptr;
    std::lock_guard<std::mutex> lock(co->mu);
    QtlArgs a; int rc = qtl_args(a, ph, regions, n_variants, var_tid, var_pos, dosage, n_cov, covariates, window, err, errlen);
    if (rc == RGX_OK) rc = check_groups(ph->n_rows, n_groups, group, err, errlen);
    if (rc == RGX_OK) rc = check_perm(n_groups, "groups", ph->n_samples, n_perm, perm, err, errlen);
    Members mem;
    if (rc == RGX_OK) rc = group_members(ph->n_rows, n_groups, group, mem, err, errlen);
    if (rc != RGX_OK) return rc;
    PermRun p(co, a, n_perm, perm, n_groups, "groups", &mem, err, errlen);
    rc = p.launch();
    rgx_qtl_group_result *q = nullptr;
    if (rc == RGX_OK && !(q = group_alloc(ph->n_rows, ph->n_samples, n_variants, n_cov, n_perm, n_groups, mem, /*pinned=*/true))) rc = p.no_result();
    if (rc == RGX_OK) rc = p.finish(q);
    if (p.done(rc) != RGX_OK) { rgx_cohort_qtl_group_free(q); return rc; }
    *out = q;
    return RGX_OK;
}

extern "C" int rgx_cohort_qtl_permute_grouped_host(const rgx_pheno_table *ph, const rgx_qtl_region *regions, uint32_t n_variants,
                                                   const uint32_t *var_tid, const uint32_t *var_pos, const int8_t *dosage, uint32_t n_cov,
                                                   const double *covariates, uint32_t window, uint32_t n_perm, const uint16_t *perm,
                                                   uint32_t n_groups, const uint32_t *group, rgx_qtl_group_result **out, char *err, size_t errlen) {
    if (!ph || !out) return fail(err, errlen, RGX_ERR_ARG, "regtools_amd: rgx_cohort_qtl_permute_grouped_host needs a phenotype table\n");
    *out = nullptr;
    const double t0 = now_ms();
    QtlArgs a; int rc = qtl_args(a, ph, regions, n_variants, var_tid, var_pos, dosage, n_cov, covariates, window, err, errlen);
    if (rc == RGX_OK) rc = check_groups(ph->n_rows, n_groups, group, err, errlen);
    if (rc == RGX_OK) rc = check_perm(n_groups, "groups", ph->n_samples, n_perm, perm, err, errlen);
    Members mem;
    if (rc == RGX_OK) rc = group_members(ph->n_rows, n_groups, group, mem, err, errlen);
    if (rc != RGX_OK) return rc;
    QtlHost h;
    rc = qtl_host_prepare(a, h, err, errlen);
    if (rc != RGX_OK) return rc;
    const uint64_t K = ph->n_rows; const uint32_t S = ph->n_samples, V = n_variants, B = n_perm, G = n_groups;
    rgx_qtl_group_result *q = group_alloc(K, S, V, n_cov, B, G, mem, false);
    if (!q) return fail(err, errlen, RGX_ERR_ARG, "regtools_amd: no memory for the result of %u groups and %u permutations\n", G, B);
    qtl_result_fill(q, h);
    memcpy(q->n_cis, h.cnt.data(), K * 4);
    try {
        uint64_t P = 0;
        for (uint32_t k : mem.row) P += h.cnt[k];
        WorkerPool pool(P * ((uint64_t)B + 1) * S < (1u << 20) ? 1 : qtl_host_threads());
        pool.run((size_t)G, [&](size_t g) {
            qtl_series_products(h, S, B, perm, mem.row.data() + mem.begin[g], mem.begin[g + 1] - mem.begin[g], q->perm_r + g * ((size_t)B + 1),
                                &q->best_row[g], q->best_variant[g], q->best_r[g], q->best_slope[g]);
        });
    } catch (const std::exception &) { rgx_cohort_qtl_group_free(q); return fail(err, errlen, RGX_ERR_ARG,
                                           "regtools_amd: no memory or threads for the grouped permutation pass\n"); }
    const double t1 = now_ms();
    rc = perm_finish(q, /*device=*/false, err, errlen);
    if (rc != RGX_OK) { rgx_cohort_qtl_group_free(q); return rc; }
    q->ms_residual = h.t_pairs - h.t_res; q->ms_products = t1 - h.t_pairs; q->ms_perm = now_ms() - t0;
    *out = q;
    return RGX_OK;
}

// ---- text ---------------------------------------------------------------------------------------------------------------------------------------------
extern "C" size_t rgx_cohort_format_qtl_group(const rgx_cohort_matrix *m, const rgx_cohort_clusters *cl, const rgx_pheno_table *ph,
                                              const rgx_qtl_group_result *q, const uint32_t *var_pos, const char *const *variant_id, char *buf,
                                              size_t cap) {
    if (!qtl_text_args_ok(m, cl, ph, q, var_pos, variant_id)) return 0;
    return format_twice(buf, cap, [&](TextOut &o) {
        o.put("group_id\tgroup_size\tphenotype_id\tnum_var\tbeta_shape1\tbeta_shape2\tdof\tvariant_id\tdistance\tr\tslope\tslope_se\ttstat\tpval_nominal\t"
              "pval_perm\tpval_beta\n");
        for (uint64_t g = 0; q && g < q->n_groups; ++g) {
            if (!q->group_n_cis[g]) continue;
            const uint32_t i = ph->row[q->best_row[g]], v = q->best_variant[g];
            const double t = rgx_qtl_tstat(q->best_r[g], q->dof);
            put_clu(o, m, cl, ph->row[q->grp_row[q->grp_begin[g]]]);
            o.fmt("\t%u\t", q->grp_begin[g + 1] - q->grp_begin[g]);
            put_intron_id(o, m, cl, i);
            o.fmt("\t%llu\t", (unsigned long long)q->group_n_cis[g]);
            o.g17(q->beta_shape1[g], '\t'); o.g17(q->beta_shape2[g], '\t');
            o.fmt("%u\t", q->dof);
            o.put(variant_id[v]);
            o.fmt("\t%lld\t", (long long)var_pos[v] - (long long)m->start[i]);
            o.g17(q->best_r[g], '\t'); o.g17(q->best_slope[g], '\t'); o.g17(q->best_slope[g] / t, '\t'); o.g17(t, '\t');
            o.g17(rgx_qtl_pvalue(t, q->dof), '\t'); o.g17(q->p_perm[g], '\t'); o.g17(q->p_beta[g], '\n');
        }
    });
}
