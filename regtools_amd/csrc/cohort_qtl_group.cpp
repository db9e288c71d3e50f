// cohort_qtl_group.cpp -- the grouped permutation pass of the cohort's cis-sQTL scan: rgx_cohort_qtl_permute_grouped (device), its host twin
// rgx_cohort_qtl_permute_grouped_host, rgx_cohort_pheno_groups and the text (contract in include/regtools_amd.h; FastQTL's --grp and tensorQTL's
// group_s, which the reference does not contain).  Device side: qtl_group_kernels.hip behind QtlRun's shared stages (qtl_run.h); the permutation
// checks and the beta approximation of one series are cohort_qtl_perm.cpp's; arithmetic: qtl_core.h.
//   QtlRun: inputs in HBM -> residuals -> the usable variants compacted -> Gt sample-major -> per row its range
//   -> the groups' member lists (host, counting sort) and the permutations sample-major in HBM -> one workgroup per (group, 64 permutations): perm_r
//   -> a thread per group: the best pair of permutation 0 -> ONE wait, the copies back -> on the host: n_ge, p_perm, the beta approximation
#include "qtl_run.h"

#include <cmath>

namespace {

// One block, every array 16-byte aligned.
struct GroupLayout { size_t yy, gg, perm_r, best_r, best_slope, p_perm, shape1, shape2, p_beta, group_n_cis, n_cis, grp_begin, grp_row, best_row,
                            best_variant, n_ge, verdict, status, bytes; };
GroupLayout group_layout(uint64_t K, uint32_t V, uint32_t B, uint64_t G, uint64_t n_members) {
    GroupLayout L; size_t o = 0;
    auto take = [&](size_t bytes) { const size_t at = o; o += (bytes + 15) & ~(size_t)15; return at; };
    L.yy = take((size_t)K * 8); L.gg = take((size_t)V * 8); L.perm_r = take((size_t)G * ((size_t)B + 1) * 8);
    L.best_r = take((size_t)G * 8); L.best_slope = take((size_t)G * 8); L.p_perm = take((size_t)G * 8); L.shape1 = take((size_t)G * 8);
    L.shape2 = take((size_t)G * 8); L.p_beta = take((size_t)G * 8); L.group_n_cis = take((size_t)G * 8);
    L.n_cis = take((size_t)K * 4); L.grp_begin = take(((size_t)G + 1) * 4); L.grp_row = take((size_t)n_members * 4);
    L.best_row = take((size_t)G * 4); L.best_variant = take((size_t)G * 4); L.n_ge = take((size_t)G * 4); L.verdict = take((size_t)V);
    L.status = take((size_t)G);
    L.bytes = o + 16;
    return L;
}
struct GroupBox { rgx_qtl_group_result q; void *block; size_t block_cap; bool pinned; };

rgx_qtl_group_result *group_alloc(uint64_t K, uint32_t S, uint32_t V, uint32_t n_cov, uint32_t B, uint32_t G, uint64_t n_members, bool pinned) {
    GroupBox *box = (GroupBox *)calloc(1, sizeof *box);
    if (!box) return nullptr;
    const GroupLayout L = group_layout(K, V, B, G, n_members);
    box->pinned = pinned;
    box->block = block_take(L.bytes, box->block_cap, pinned);
    if (!box->block && pinned) { box->pinned = false; box->block = block_take(L.bytes, box->block_cap, false); }
    if (!box->block) { free(box); return nullptr; }
    uint8_t *b = (uint8_t *)box->block;
    rgx_qtl_group_result *q = &box->q;
    q->n_rows = K; q->n_samples = S; q->n_variants = V; q->n_cov = n_cov; q->dof = S - n_cov - 2; q->n_perm = B; q->n_groups = G;
    q->yy = (double *)(b + L.yy); q->gg = (double *)(b + L.gg); q->perm_r = (double *)(b + L.perm_r); q->best_r = (double *)(b + L.best_r);
    q->best_slope = (double *)(b + L.best_slope); q->p_perm = (double *)(b + L.p_perm); q->beta_shape1 = (double *)(b + L.shape1);
    q->beta_shape2 = (double *)(b + L.shape2); q->p_beta = (double *)(b + L.p_beta); q->group_n_cis = (uint64_t *)(b + L.group_n_cis);
    q->n_cis = (uint32_t *)(b + L.n_cis); q->grp_begin = (uint32_t *)(b + L.grp_begin); q->grp_row = (uint32_t *)(b + L.grp_row);
    q->best_row = (uint32_t *)(b + L.best_row); q->best_variant = (uint32_t *)(b + L.best_variant); q->n_ge = (uint32_t *)(b + L.n_ge);
    q->variant_verdict = b + L.verdict; q->beta_status = b + L.status;
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
struct Members { std::vector<uint32_t> begin, row; };
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

// group_n_cis, n_pairs, the verdict counts and the tile count of a result whose arrays from steps (1)-(6), the member lists and perm_r, best_* are
// in place; then n_ge, p_perm and the beta approximation, sixteen groups a task (a group's sums do not depend on who runs it)
int group_finish(rgx_qtl_group_result *q, bool device, char *err, size_t errlen) {
    const uint64_t K = q->n_rows, G = q->n_groups; const uint32_t B = q->n_perm, S = q->n_samples, dof = q->dof;
    for (uint32_t v = 0; v < q->n_variants; ++v) { q->n_constant += q->variant_verdict[v] == 1; q->n_explained += q->variant_verdict[v] == 2; }
    for (uint64_t k = 0; k < K; ++k) q->n_flat_rows += !qtl_enough(q->yy[k], S);
    const uint64_t p_tiles = ((uint64_t)B + 1 + kQtlTile - 1) / kQtlTile;
    for (uint64_t g = 0; g < G; ++g) {
        uint64_t n = 0;
        for (uint32_t i = q->grp_begin[g]; i < q->grp_begin[g + 1]; ++i) {
            const uint32_t c = q->n_cis[q->grp_row[i]];
            n += c;
            if (device) q->n_tiles += p_tiles * (((uint64_t)c + kQtlTile - 1) / kQtlTile);
        }
        q->group_n_cis[g] = n; q->n_pairs += n;
    }
    const double t0 = now_ms();
    try {
        WorkerPool pool(G * B < 4096 ? 1 : qtl_host_threads());
        const uint64_t chunk = 16, n_tasks = (G + chunk - 1) / chunk;
        pool.run((size_t)n_tasks, [&](size_t task) {
            std::vector<double> p(B);
            for (uint64_t g = task * chunk; g < G && g < (task + 1) * chunk; ++g)
                qtl_series_finish(q->perm_r + g * ((size_t)B + 1), B, q->best_r[g], dof, q->group_n_cis[g] != 0, p.data(), q->n_ge[g], q->p_perm[g],
                                  q->beta_shape1[g], q->beta_shape2[g], q->p_beta[g], q->beta_status[g]);
        });
    } catch (const std::exception &) { return fail(err, errlen, RGX_ERR_ARG, "regtools_amd: no memory or threads for the beta approximation\n"); }
    q->ms_beta = now_ms() - t0;
    return RGX_OK;
}

// The device run: QtlRun's shared stages with the grouped permutation stage behind them.
struct GroupRun {
    QtlRun run; uint32_t B; const uint16_t *perm; size_t ldp; uint32_t G; const Members &mem;
    std::vector<uint16_t> permT;
    uint16_t *d_permT = nullptr; uint32_t *d_begin = nullptr, *d_row = nullptr;
    double *perm_r = nullptr, *best_r = nullptr, *best_slope = nullptr; uint32_t *best_row = nullptr, *best_u = nullptr, *best_variant = nullptr;

    GroupRun(rgx_cohort *co, const QtlArgs &a, uint32_t B_, const uint16_t *perm_, uint32_t G_, const Members &mem_, char *err, size_t errlen)
        : run(co, a, err, errlen), B(B_), perm(perm_), ldp(((size_t)B_ + 1 + kQtlTile - 1) / kQtlTile * kQtlTile), G(G_), mem(mem_) {
        run.best_only = true; }

    // 5. the member lists and the permutations sample-major in HBM, the products, the best pairs
    int products() {
        rgx_cohort *co = run.co; char *err = run.err; const size_t errlen = run.errlen; hipStream_t st = run.st;
        const uint32_t S = run.S;
        if ((uint64_t)G * (ldp / kQtlTile) > 0x7fffffffull) return fail(err, errlen, RGX_ERR_ARG,
            "regtools_amd: %u groups x %zu blocks of 64 permutations are more than 2^31 - 1 workgroups\n", G, ldp / kQtlTile);
        try { permT.assign((size_t)S * ldp, 0); }
        catch (const std::bad_alloc &) { return fail(err, errlen, RGX_ERR_ARG, "regtools_amd: no memory for %u permutations of %u samples\n", B, S); }
        for (uint32_t b = 0; b <= B; ++b) for (uint32_t s = 0; s < S; ++s) permT[(size_t)s * ldp + b] = perm[(size_t)b * S + s];
        const size_t n_out = (size_t)G * ((size_t)B + 1), n_mem = mem.row.size();
        if (co->qp_in.ensure(permT.size() * 2 + ((size_t)G + 1 + n_mem) * 4 + 256) != hipSuccess ||
            co->qp_out.ensure(n_out * 8 + (size_t)G * 28 + 256) != hipSuccess) {
            (void)hipGetLastError();
            return fail(err, errlen, RGX_ERR_DEVICE, "regtools_amd: no device memory for %u permutations of %u groups\n", B, G); }
        Carve in(co->qp_in);
        d_permT = in.take<uint16_t>(permT.size()); d_begin = in.u32((size_t)G + 1); d_row = in.u32(n_mem);
        CARVE_TRY(in, "grouped sQTL permutation");
        Carve o(co->qp_out);
        perm_r = o.take<double>(n_out); best_r = o.take<double>(G); best_slope = o.take<double>(G); best_row = o.u32(G); best_u = o.u32(G);
        best_variant = o.u32(G);
        CARVE_TRY(o, "grouped sQTL permutation result");
        HIP_TRY(hipMemcpyAsync(d_permT, permT.data(), permT.size() * 2, hipMemcpyHostToDevice, st));
        HIP_TRY(hipMemcpyAsync(d_begin, mem.begin.data(), ((size_t)G + 1) * 4, hipMemcpyHostToDevice, st));
        if (n_mem) { HIP_TRY(hipMemcpyAsync(d_row, mem.row.data(), n_mem * 4, hipMemcpyHostToDevice, st)); }
        run.mark("members + permutations in HBM");
        HIP_TRY(hipEventRecord(run.ev[2], st));
        launch_qtl_perm_group(run.Y, G, S, d_permT, ldp, B + 1, run.Gt, run.ldg, run.lo, run.count, run.yy, run.u_gg, d_begin, d_row, perm_r, best_row,
                              best_u, st);
        run.mark("grouped permuted products");
        launch_qtl_group_best(run.Y, run.G, G, S, best_row, best_u, run.u_var, run.yy, run.gg, best_variant, best_r, best_slope, st);
        HIP_TRY(hipEventRecord(run.ev[3], st));
        run.mark("best pairs");
        return RGX_OK;
    }
    // 6. the copies back behind the call's one wait, then the host's part
    int finish(rgx_qtl_group_result **out) {
        char *err = run.err; const size_t errlen = run.errlen; hipStream_t st = run.st;
        const uint32_t K = run.K, V = run.V;
        rgx_qtl_group_result *q = group_alloc(K, run.S, V, run.a.n_cov, B, G, mem.row.size(), /*pinned=*/true);
        if (!q) { (void)hipStreamSynchronize(st); return fail(err, errlen, RGX_ERR_DEVICE,
            "regtools_amd: no memory for the result of %u groups and %u permutations\n", G, B); }
        memcpy(q->grp_begin, mem.begin.data(), ((size_t)G + 1) * 4);
        if (!mem.row.empty()) memcpy(q->grp_row, mem.row.data(), mem.row.size() * 4);
        uint64_t h[4] = {0, 0, 0, 0};
        hipError_t e_ = hipMemcpyAsync(q->yy, run.yy, (size_t)K * 8, hipMemcpyDeviceToHost, st);
        auto copy = [&](void *dst, const void *src, size_t bytes) { if (e_ == hipSuccess && bytes) e_ = hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, st); };
        copy(q->gg, run.gg, (size_t)V * 8); copy(q->variant_verdict, run.verdict, V); copy(q->n_cis, run.count, (size_t)K * 4);
        copy(q->perm_r, perm_r, (size_t)G * ((size_t)B + 1) * 8); copy(q->best_r, best_r, (size_t)G * 8); copy(q->best_slope, best_slope, (size_t)G * 8);
        copy(q->best_row, best_row, (size_t)G * 4); copy(q->best_variant, best_variant, (size_t)G * 4); copy(h, run.head, 32);
        if (e_ == hipSuccess) e_ = hipStreamSynchronize(st);
        if (e_ == hipSuccess) e_ = rgx::pending_launch_error();
        float ms_res = 0, ms_pr = 0;
        if (e_ == hipSuccess) e_ = hipEventElapsedTime(&ms_res, run.ev[0], run.ev[1]);
        if (e_ == hipSuccess) e_ = hipEventElapsedTime(&ms_pr, run.ev[2], run.ev[3]);
        if (e_ != hipSuccess) { rgx_cohort_qtl_group_free(q); return fail(err, errlen, RGX_ERR_DEVICE, "HIP error %s in the grouped sQTL permutation pass\n",
            hipGetErrorString(e_)); }
        run.mark("copies");
        int rc = bad_flags((const uint32_t *)(h + 2), K, err, errlen);
        if (rc == RGX_OK) rc = group_finish(q, /*device=*/true, err, errlen);
        if (rc != RGX_OK) { rgx_cohort_qtl_group_free(q); return rc; }
        q->ms_residual = ms_res; q->ms_products = ms_pr; q->ms_perm = now_ms() - run.t0;
        *out = q;
        return RGX_OK;
    }
};

}  // namespace

extern "C" void rgx_cohort_qtl_group_free(rgx_qtl_group_result *q) {
    if (!q) return;
    GroupBox *box = (GroupBox *)q;                                      // q is the first member
    block_give(box->block, box->block_cap, box->pinned);
    free(box);
}

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
    const QtlArgs a{ph, regions, n_variants, var_tid, var_pos, dosage, n_cov, covariates, window};
    int rc = check_qtl(a, err, errlen);
    if (rc == RGX_OK) rc = check_groups(ph->n_rows, n_groups, group, err, errlen);
    if (rc == RGX_OK) rc = check_perm(n_groups, "groups", ph->n_samples, n_perm, perm, err, errlen);
    Members mem;
    if (rc == RGX_OK) rc = group_members(ph->n_rows, n_groups, group, mem, err, errlen);
    if (rc != RGX_OK) return rc;
    GroupRun p(co, a, n_perm, perm, n_groups, mem, err, errlen);
    rc = p.run.open();
    if (rc == RGX_OK) rc = p.run.residuals();
    if (rc == RGX_OK) rc = p.run.compact();
    if (rc == RGX_OK) rc = p.run.plan_launch();
    if (rc == RGX_OK) rc = p.products();
    if (rc == RGX_OK) rc = p.finish(out);
    if (rc != RGX_OK && p.run.st) (void)hipStreamSynchronize(p.run.st);   // (the uploads read the caller's arrays and this run's T, Q, permT and members)
    return rc;
}

extern "C" int rgx_cohort_qtl_permute_grouped_host(const rgx_pheno_table *ph, const rgx_qtl_region *regions, uint32_t n_variants,
                                                   const uint32_t *var_tid, const uint32_t *var_pos, const int8_t *dosage, uint32_t n_cov,
                                                   const double *covariates, uint32_t window, uint32_t n_perm, const uint16_t *perm,
                                                   uint32_t n_groups, const uint32_t *group, rgx_qtl_group_result **out, char *err, size_t errlen) {
    if (!ph || !out) return fail(err, errlen, RGX_ERR_ARG, "regtools_amd: rgx_cohort_qtl_permute_grouped_host needs a phenotype table\n");
    *out = nullptr;
    const double t0 = now_ms();
    const QtlArgs a{ph, regions, n_variants, var_tid, var_pos, dosage, n_cov, covariates, window};
    int rc = check_qtl(a, err, errlen);
    if (rc == RGX_OK) rc = check_groups(ph->n_rows, n_groups, group, err, errlen);
    if (rc == RGX_OK) rc = check_perm(n_groups, "groups", ph->n_samples, n_perm, perm, err, errlen);
    Members mem;
    if (rc == RGX_OK) rc = group_members(ph->n_rows, n_groups, group, mem, err, errlen);
    if (rc != RGX_OK) return rc;
    QtlHost h;
    rc = qtl_host_prepare(a, h, err, errlen);
    if (rc != RGX_OK) return rc;
    const uint64_t K = ph->n_rows; const uint32_t S = ph->n_samples, V = n_variants, B = n_perm, G = n_groups;
    rgx_qtl_group_result *q = group_alloc(K, S, V, n_cov, B, G, mem.row.size(), false);
    if (!q) return fail(err, errlen, RGX_ERR_ARG, "regtools_amd: no memory for the result of %u groups and %u permutations\n", G, B);
    memcpy(q->yy, h.yy.data(), K * 8);
    memcpy(q->n_cis, h.cnt.data(), K * 4);
    if (V) { memcpy(q->gg, h.gg.data(), (size_t)V * 8); memcpy(q->variant_verdict, h.verdict.data(), V); }
    memcpy(q->grp_begin, mem.begin.data(), ((size_t)G + 1) * 4);
    if (!mem.row.empty()) memcpy(q->grp_row, mem.row.data(), mem.row.size() * 4);
    try {
        uint64_t P = 0;
        for (uint32_t k : mem.row) P += h.cnt[k];
        WorkerPool pool(P * ((uint64_t)B + 1) * S < (1u << 20) ? 1 : qtl_host_threads());
        pool.run((size_t)G, [&](size_t g) {
            std::vector<double> yp(S);
            std::vector<uint64_t> top((size_t)B + 1, 0);
            q->best_row[g] = RGX_NO_PAIR; q->best_variant[g] = RGX_NO_PAIR; q->best_r[g] = 0.0; q->best_slope[g] = 0.0;
            // members in ascending row, variants in ascending order: a strictly larger |r| alone replaces, so the earliest of equals stays
            for (uint32_t i = mem.begin[g]; i < mem.begin[g + 1]; ++i) {
                const uint32_t k = mem.row[i];
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
                        if (!b && (q->best_variant[g] == RGX_NO_PAIR || bits > top[0])) {
                            q->best_row[g] = k; q->best_variant[g] = v; q->best_r[g] = r; q->best_slope[g] = qtl_slope(acc, h.gg[v]);
                        }
                        if (bits > top[b]) top[b] = bits;
                    }
                }
            }
            memcpy(q->perm_r + g * ((size_t)B + 1), top.data(), ((size_t)B + 1) * 8);
        });
    } catch (const std::exception &) { rgx_cohort_qtl_group_free(q); return fail(err, errlen, RGX_ERR_ARG,
                                           "regtools_amd: no memory or threads for the grouped permutation pass\n"); }
    const double t1 = now_ms();
    rc = group_finish(q, /*device=*/false, err, errlen);
    if (rc != RGX_OK) { rgx_cohort_qtl_group_free(q); return rc; }
    q->ms_residual = h.t_pairs - h.t_res; q->ms_products = t1 - h.t_pairs; q->ms_perm = now_ms() - t0;
    *out = q;
    return RGX_OK;
}

// ---- text ---------------------------------------------------------------------------------------------------------------------------------------------
extern "C" size_t rgx_cohort_format_qtl_group(const rgx_cohort_matrix *m, const rgx_cohort_clusters *cl, const rgx_pheno_table *ph,
                                              const rgx_qtl_group_result *q, const uint32_t *var_pos, const char *const *variant_id, char *buf,
                                              size_t cap) {
    if (!m || !cl || !ph || cl->n_rows != m->n || (q && (q->n_rows != ph->n_rows || (q->n_variants && (!var_pos || !variant_id))))) return 0;
    for (uint64_t k = 0; k < ph->n_rows; ++k) if (ph->row[k] >= m->n || cl->cluster[ph->row[k]] == RGX_NO_CLUSTER) return 0;
    auto run = [&](char *dst) {
        size_t need = 0;
        auto put = [&](const char *s, size_t n) { if (dst) memcpy(dst + need, s, n); need += n; };
        char num[256];
        auto put_g = [&](double x, char end) {
            if (x != x) put(num, (size_t)snprintf(num, sizeof num, "nan%c", end)); else put(num, (size_t)snprintf(num, sizeof num, "%.17g%c", x, end));
        };
        auto put_clu = [&](uint32_t i, char end) {
            const uint32_t cls = rgx::strand_class(m->strand[i]);
            put(num, (size_t)snprintf(num, sizeof num, "clu_%llu_%s%c", (unsigned long long)cl->cluster[i] + 1, cls == 0 ? "+" : cls == 1 ? "-" : "NA", end));
        };
        static const char head[] = "group_id\tgroup_size\tphenotype_id\tnum_var\tbeta_shape1\tbeta_shape2\tdof\tvariant_id\tdistance\tr\tslope\tslope_se\t"
                                   "tstat\tpval_nominal\tpval_perm\tpval_beta\n";
        put(head, sizeof head - 1);
        for (uint64_t g = 0; q && g < q->n_groups; ++g) {
            if (!q->group_n_cis[g]) continue;
            const uint32_t i = ph->row[q->best_row[g]], v = q->best_variant[g];
            const char *contig = m->ref_name[m->tid[i]];
            const double t = rgx_qtl_tstat(q->best_r[g], q->dof);
            put_clu(ph->row[q->grp_row[q->grp_begin[g]]], '\t');
            put(num, (size_t)snprintf(num, sizeof num, "%u\t", q->grp_begin[g + 1] - q->grp_begin[g]));
            put(contig, strlen(contig));
            put(num, (size_t)snprintf(num, sizeof num, ":%u:%u:", m->start[i], m->end[i]));
            put_clu(i, '\t');
            put(num, (size_t)snprintf(num, sizeof num, "%llu\t", (unsigned long long)q->group_n_cis[g]));
            put_g(q->beta_shape1[g], '\t'); put_g(q->beta_shape2[g], '\t');
            put(num, (size_t)snprintf(num, sizeof num, "%u\t", q->dof));
            put(variant_id[v], strlen(variant_id[v]));
            put(num, (size_t)snprintf(num, sizeof num, "\t%lld\t", (long long)var_pos[v] - (long long)m->start[i]));
            put_g(q->best_r[g], '\t'); put_g(q->best_slope[g], '\t'); put_g(q->best_slope[g] / t, '\t'); put_g(t, '\t');
            put_g(rgx_qtl_pvalue(t, q->dof), '\t'); put_g(q->p_perm[g], '\t'); put_g(q->p_beta[g], '\n');
        }
        return need;
    };
    const size_t need = run(nullptr);
    if (buf && need <= cap) run(buf);
    return need;
}
