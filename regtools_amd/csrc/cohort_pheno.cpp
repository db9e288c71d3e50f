// cohort_pheno.cpp -- the splicing phenotype table of a clustered cohort: rgx_cohort_phenotypes (device), its host twin
// rgx_cohort_phenotypes_host, the quantile function and the text (contract in include/regtools_amd.h; modelled on LeafCutter's
// prepare_phenotype_table.py, which the reference does not contain).  Device side: pheno_kernels.hip; per-entry arithmetic: pheno_core.h.
//   matrix + cluster result in HBM -> per row: missing samples, mean, sd, filters (a wave per row) -> scan = the kept rows' places, scatter
//   -> per kept (row, sample): the 64-bit key of z -> ONE stable sort by (sample, z) -> head flags of the tie runs, scan, run starts -> rank2
#include "cohort_internal.h"
#include "pheno_core.h"

#include <cmath>
#include <limits>

namespace {

rgx_pheno_table *pheno_alloc(uint64_t K, uint32_t S, bool pinned) {
    rgx_pheno_table *p = result_alloc<rgx_pheno_table>(pinned, [&](rgx_pheno_table &r, BlockTake &take) {
        take(r.mean, K); take(r.sd, K); take(r.row, K); take(r.n_na, K); take(r.rank2, (size_t)K * S);
    });
    if (!p) return nullptr;
    p->n_rows = K; p->n_samples = S;
    return p;
}

constexpr uint64_t kMaxPhenoEntries = (1ull << 32) - (1ull << 16);    // (the sort's tiles round the count up inside 32 bits)

// the arguments, the same for the device and the twin; *n_clustered = the candidates
int check_pheno(const rgx_cohort_matrix *m, const rgx_cohort_clusters *cl, const rgx_pheno_params &p, uint64_t *n_clustered, char *err, size_t errlen) {
    if (p.na_den == 0 || p.na_num > p.na_den) return fail(err, errlen, RGX_ERR_ARG, "regtools_amd: the missing share %u/%u is not a share between 0 and 1\n",
        p.na_num, p.na_den);
    if (!(p.min_sd >= 0)) return fail(err, errlen, RGX_ERR_ARG, "regtools_amd: the least deviation %g is negative or no number\n", p.min_sd);
    if (cl->n_rows != m->n) return fail(err, errlen, RGX_ERR_ARG, "regtools_amd: the clusters are of a matrix of %llu rows; this one has %llu\n",
        (unsigned long long)cl->n_rows, (unsigned long long)m->n);
    uint64_t k = 0;
    for (uint64_t i = 0; i < m->n; ++i) {
        const uint32_t c = cl->cluster[i];
        if (c == RGX_NO_CLUSTER) continue;
        if (c >= cl->n_clusters) return fail(err, errlen, RGX_ERR_ARG, "regtools_amd: row %llu is in cluster %u of %llu\n", (unsigned long long)i, c,
            (unsigned long long)cl->n_clusters);
        ++k;
    }
    if (m->n > kMaxPhenoEntries || k * (uint64_t)m->n_samples > kMaxPhenoEntries) return fail(err, errlen, RGX_ERR_ARG,
        "regtools_amd: a phenotype table takes at most %llu entries; %llu clustered rows of %u samples are more\n", (unsigned long long)kMaxPhenoEntries,
        (unsigned long long)k, m->n_samples);
    *n_clustered = k;
    return RGX_OK;
}

// what the scans leave at the front of the row workspace
struct PhenoScalars { uint32_t n_kept, n_drop_na, n_runs; };

// One device run, as the stages rgx_cohort_phenotypes is made of.  The caller holds the cohort's lock and has checked the arguments; every stage
// enqueues on the cohort's stream and returns RGX_OK or the failed call's code.
struct PhenoRun : CohortRun {
    const rgx_cohort_matrix *m; const rgx_cohort_clusters *cl; rgx_pheno_params prm; uint64_t n_clustered;
    uint32_t n = 0, S = 0, K = 0, n_drop_na = 0;
    PhenoIn in{};
    PhenoScalars *d_sc = nullptr;
    double *mean = nullptr, *sd = nullptr, *o_mean = nullptr, *o_sd = nullptr;
    uint32_t *keep = nullptr, *drop_na = nullptr, *pos = nullptr, *n_na = nullptr, *o_row = nullptr, *o_n_na = nullptr, *tmp = nullptr;
    const uint32_t *rank2 = nullptr;

    PhenoRun(rgx_cohort *co_, const rgx_cohort_matrix *m_, const rgx_cohort_clusters *cl_, const rgx_pheno_params &p_, uint64_t n_clustered_, char *err_,
             size_t errlen_)
        : CohortRun(co_, "phenotypes", err_, errlen_), m(m_), cl(cl_), prm(p_), n_clustered(n_clustered_) {}

    // 1. the matrix where the kernels read it (its image in HBM, or uploaded), the cluster result beside it, the row workspace
    int open() {
        co->cluster_path = matrix_serial(m) == co->image_serial ? 1 : 0;
        n = (uint32_t)m->n; S = m->n_samples;
        if (!n_clustered || !S) return RGX_OK;
        if (int rc = enter()) return rc;
        CohortImage img{};
        if (int rc = cohort_matrix_image(co, m, st, &img, err, errlen)) return rc;
        const size_t C = (size_t)cl->n_clusters, n_cs = (size_t)cl->cs_begin[C];
        if (int rc = grow(co->ph_in, (C + 1 + n_cs) * 8 + ((size_t)n + n_cs) * 4 + 256,
                  "regtools_amd: no device memory to upload the clusters (%zu clusters, %zu denominators)\n", C, n_cs)) return rc;
        Carve u = carve(co->ph_in);                          // (every array written whole by its upload; the denominators have no bytes when there are none)
        unsigned long long *cs_begin = (unsigned long long *)u.u64(C + 1), *cs_total = (unsigned long long *)u.u64(n_cs);
        uint32_t *cluster = u.u32(n), *cs_sample = u.u32(n_cs);
        CARVE_TRY(u, "phenotype clusters");
        if (int rc = carved(u, "phenotype clusters")) return rc;
        HIP_TRY(hipMemcpyAsync(cs_begin, cl->cs_begin, (C + 1) * 8, hipMemcpyHostToDevice, st));
        HIP_TRY(hipMemcpyAsync(cluster, cl->cluster, (size_t)n * 4, hipMemcpyHostToDevice, st));
        if (n_cs) {
            HIP_TRY(hipMemcpyAsync(cs_total, cl->cs_total, n_cs * 8, hipMemcpyHostToDevice, st));
            HIP_TRY(hipMemcpyAsync(cs_sample, cl->cs_sample, n_cs * 4, hipMemcpyHostToDevice, st));
        }
        in.cluster = cluster; in.row_begin = img.row_begin; in.col_sample = img.col_sample; in.val_count = img.val_count;
        in.cs_begin = cs_begin; in.cs_sample = cs_sample; in.cs_total = cs_total;
        mark("matrix + clusters in HBM");

        const size_t Nn = (size_t)n + 64, tmp_words = scan_tmp_words(n) + 64;
        if (int rc = grow(co->ph_rows, (Nn * (4 * 2 + 6) + 64 + tmp_words) * 4 + 256, "regtools_amd: no device memory for the statistics of %u rows\n", n)) return rc;
        // first writers: keep, drop_na k_pheno_row_stats (whole); n_na, mean, sd the same kernel, but for rows without a cluster, whose keep is 0:
        // k_pheno_scatter reads them for kept rows alone; pos and the scalars the scans; o_row, o_n_na, o_mean, o_sd k_pheno_scatter [0, K), the
        // rest left and not read: k_pheno_z and the copies stop at K; tmp: the scans' scratch.  The 64 pad elements of every array are never touched.
        Carve w = carve(co->ph_rows);
        mean = w.take<double>(Nn); sd = w.take<double>(Nn); o_mean = w.take<double>(Nn); o_sd = w.take<double>(Nn);
        d_sc = (PhenoScalars *)w.u32(64);
        keep = w.u32(Nn); drop_na = w.u32(Nn); pos = w.u32(Nn); n_na = w.u32(Nn); o_row = w.u32(Nn); o_n_na = w.u32(Nn); tmp = w.u32(tmp_words);
        CARVE_TRY(w, "phenotype rows");
        if (int rc = carved(w, "phenotype rows")) return rc;
        return RGX_OK;
    }

    // 2. + 3. per row: missing samples, mean, sd and the filters; the kept rows' places by a scan; their statistics side by side
    int row_stats() {
        launch_pheno_row_stats(in, n, S, prm.na_num, prm.na_den, prm.min_sd, n_na, mean, sd, keep, drop_na, st);
        launch_scan_u32(keep, pos, n, &d_sc->n_kept, tmp, st);
        launch_scan_u32(drop_na, drop_na, n, &d_sc->n_drop_na, tmp, st);
        PhenoScalars sc;
        HIP_TRY(read_back(st, &sc, d_sc, sizeof sc));
        K = sc.n_kept; n_drop_na = sc.n_drop_na;
        if (K > n_clustered) return fail(err, errlen, RGX_ERR_DEVICE, "regtools_amd: %u rows kept of %llu clustered ones\n", K, (unsigned long long)n_clustered);
        launch_pheno_scatter(keep, pos, n_na, mean, sd, n, o_row, o_n_na, o_mean, o_sd, st);
        mark("row statistics + kept rows");
        return RGX_OK;
    }

    // 4. - 6. the kept entries' keys, one stable sort by (sample, z) -- z low word first -- and the tie runs' ranks
    int ranks() {
        const uint32_t N = K * S;                                        // (at most n_clustered * S: checked)
        const size_t Nn = (size_t)N + 64, tmp_words = radix_tmp_words(N) + scan_tmp_words(N) + 64;
        if (int rc = grow(co->ph_entries, (Nn * 7 + tmp_words) * 4 + 256, "regtools_amd: no device memory to rank %u rows of %u samples\n", K, S)) return rc;
        // first writers: z_lo, z_hi, e_sample k_pheno_z [0, N); perm0, perm1, key0, key1 the sort's passes; then, the sort over, key0 (heads)
        // k_pheno_tie_heads, key1 (seg) the scan, the spare permutation (run starts) k_cohort_row_start, e_sample (rank2) k_pheno_rank, each
        // [0, N); etmp: the passes' and the scan's scratch.  The 64 pad elements of every array are never touched.
        Carve q = carve(co->ph_entries);
        uint32_t *z_lo = q.u32(Nn), *z_hi = q.u32(Nn), *e_sample = q.u32(Nn), *perm0 = q.u32(Nn), *perm1 = q.u32(Nn), *key0 = q.u32(Nn), *key1 = q.u32(Nn),
                 *etmp = q.u32(tmp_words);
        CARVE_TRY(q, "phenotype entries");
        if (int rc = carved(q, "phenotype entries")) return rc;
        launch_pheno_z(in, o_row, o_mean, o_sd, K, S, z_lo, z_hi, e_sample, st);
        RadixSort by_column{{perm0, perm1}, etmp, N, st, {key0, key1}};
        by_column.by_keyed(z_lo, 32); by_column.by_keyed(z_hi, 32); by_column.by_keyed(e_sample, std::max<uint32_t>(1, bitlen(S - 1)));
        mark("keys + column sort");
        uint32_t *head = key0, *seg = key1, *run_start = by_column.spare(), *out = e_sample;      // (the sort is over: its keys and the sample word are used up)
        launch_pheno_tie_heads(by_column.sorted(), z_lo, z_hi, N, K, head, st);
        launch_scan_u32(head, seg, N, &d_sc->n_runs, etmp, st);
        launch_cohort_row_start(head, seg, N, run_start, st);
        launch_pheno_rank(by_column.sorted(), head, seg, run_start, N, K, out, st);
        rank2 = out;
        mark("tie runs + ranks");
        return RGX_OK;
    }

    // 7. the result in host memory (K == 0: the counts alone)
    int finish(rgx_pheno_table **out) {
        rgx_pheno_table *p = pheno_alloc(K, S, /*pinned=*/K != 0);
        if (!p) { if (st) (void)hipStreamSynchronize(st); return fail(err, errlen, RGX_ERR_DEVICE, "regtools_amd: no memory for the phenotype table\n"); }
        if (K) {
            CopyBack back{st};
            guards_back(back);
            back(p->row, o_row, (size_t)K * 4); back(p->n_na, o_n_na, (size_t)K * 4); back(p->mean, o_mean, (size_t)K * 8);
            back(p->sd, o_sd, (size_t)K * 8); back(p->rank2, rank2, (size_t)K * S * 4);
            const hipError_t e_ = back.wait();
            if (e_ != hipSuccess) { rgx_cohort_phenotypes_free(p); return fail(err, errlen, RGX_ERR_DEVICE, "HIP error %s building the phenotype table\n",
                hipGetErrorString(e_)); }
            mark("copy");
            if (int rc = guards_check()) { rgx_cohort_phenotypes_free(p); return rc; }
        }
        p->n_clustered = n_clustered; p->n_drop_na = S ? n_drop_na : n_clustered; p->n_drop_sd = n_clustered - p->n_drop_na - K;
        p->ms_pheno = now_ms() - t0;
        *out = p;
        return RGX_OK;
    }
};

// the contract's halving of the 64 partials
double halve(double *P) {
    for (uint32_t off = kPhenoPartials / 2; off; off >>= 1) for (uint32_t l = 0; l < off; ++l) P[l] = pheno_add(P[l], P[l + off]);
    return P[0];
}

}  // namespace

extern "C" void rgx_pheno_params_default(rgx_pheno_params *p) { if (p) { p->na_num = 4; p->na_den = 10; p->min_sd = 0.005; } }

extern "C" void rgx_cohort_phenotypes_free(rgx_pheno_table *ph) { result_free(ph); }

extern "C" int rgx_cohort_phenotypes(rgx_cohort *co, const rgx_cohort_matrix *m, const rgx_cohort_clusters *cl, const rgx_pheno_params *p,
                                     rgx_pheno_table **out, char *err, size_t errlen) {
    if (!co || !m || !cl || !out) return fail(err, errlen, RGX_ERR_ARG, "regtools_amd: rgx_cohort_phenotypes needs a cohort, a matrix and its clusters\n");
    *out = nullptr;
    std::lock_guard<std::mutex> lock(co->mu);
    rgx_pheno_params prm; if (p) prm = *p; else rgx_pheno_params_default(&prm);
    uint64_t n_clustered = 0;
    int rc = check_pheno(m, cl, prm, &n_clustered, err, errlen);
    if (rc != RGX_OK) return rc;
    PhenoRun run(co, m, cl, prm, n_clustered, err, errlen);
    rc = run.open();
    if (rc == RGX_OK && n_clustered && run.S) rc = run.row_stats();
    if (rc == RGX_OK && run.K) rc = run.ranks();
    if (rc == RGX_OK) rc = run.finish(out);
    return rc;
}

extern "C" int rgx_cohort_phenotypes_host(const rgx_cohort_matrix *m, const rgx_cohort_clusters *cl, const rgx_pheno_params *p,
                                          rgx_pheno_table **out, char *err, size_t errlen) {
    if (!m || !cl || !out) return fail(err, errlen, RGX_ERR_ARG, "regtools_amd: rgx_cohort_phenotypes_host needs a matrix and its clusters\n");
    *out = nullptr;
    const double t0 = now_ms();
    rgx_pheno_params prm; if (p) prm = *p; else rgx_pheno_params_default(&prm);
    uint64_t n_clustered = 0;
    const int rc = check_pheno(m, cl, prm, &n_clustered, err, errlen);
    if (rc != RGX_OK) return rc;
    const uint32_t n = (uint32_t)m->n, S = m->n_samples;
    std::vector<uint32_t> row, n_na;
    std::vector<double> mean, sd, x(S);
    uint64_t n_drop_na = 0, n_drop_sd = 0;
    auto row_of = [&](uint32_t i) {
        const uint32_t c = cl->cluster[i];
        PhenoRow r;
        r.col_sample = m->col_sample; r.val_count = m->val_count; r.cs_sample = cl->cs_sample; r.cs_total = (const unsigned long long *)cl->cs_total;
        r.e0 = m->row_begin[i]; r.e1 = m->row_begin[i + 1]; r.d0 = cl->cs_begin[c]; r.d1 = cl->cs_begin[c + 1];
        return r;
    };
    for (uint32_t i = 0; i < n; ++i) {
        if (cl->cluster[i] == RGX_NO_CLUSTER) continue;
        const PhenoRow r = row_of(i);
        double P[kPhenoPartials];
        for (double &v : P) v = 0.0;
        uint32_t miss = 0;
        for (uint32_t s = 0; s < S; ++s) {
            const uint64_t den = r.den(s);
            if (!den) { ++miss; x[s] = -1.0; continue; }
            x[s] = pheno_ratio(r.num(s), den);
            P[s % kPhenoPartials] = pheno_add(P[s % kPhenoPartials], x[s]);
        }
        double mu = 0.0, dev = 0.0;
        if (miss < S) {
            mu = pheno_mean(halve(P), S - miss);
            for (double &v : P) v = 0.0;
            for (uint32_t s = 0; s < S; ++s) if (x[s] >= 0.0) P[s % kPhenoPartials] = pheno_add(P[s % kPhenoPartials], pheno_sq_dev(x[s], mu));
            dev = pheno_sd(halve(P), S);
        }
        const uint32_t verdict = pheno_verdict(miss, S, prm.na_num, prm.na_den, dev, prm.min_sd);
        if (verdict == 1) { ++n_drop_na; continue; }
        if (verdict == 2) { ++n_drop_sd; continue; }
        row.push_back(i); n_na.push_back(miss); mean.push_back(mu); sd.push_back(dev);
    }
    const size_t K = row.size();
    rgx_pheno_table *ph = pheno_alloc(K, S, false);
    if (!ph) return fail(err, errlen, RGX_ERR_ARG, "regtools_amd: no memory for the phenotype table\n");
    if (K) {
        memcpy(ph->row, row.data(), K * 4); memcpy(ph->n_na, n_na.data(), K * 4); memcpy(ph->mean, mean.data(), K * 8); memcpy(ph->sd, sd.data(), K * 8);
        // the columns one after the other: the kept rows in stable order of z, then the runs of equal values
        std::vector<uint64_t> key(K * (size_t)S);
        for (size_t k = 0; k < K; ++k) {
            const PhenoRow r = row_of(row[k]);
            for (uint32_t s = 0; s < S; ++s) {
                const uint64_t den = r.den(s);
                key[k * S + s] = pheno_key(den ? pheno_z(pheno_ratio(r.num(s), den), mean[k], sd[k]) : 0.0);
            }
        }
        std::vector<uint32_t> order(K);
        for (uint32_t s = 0; s < S; ++s) {
            for (size_t k = 0; k < K; ++k) order[k] = (uint32_t)k;
            std::stable_sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) { return key[(size_t)a * S + s] < key[(size_t)b * S + s]; });
            for (size_t lo = 0; lo < K;) {
                size_t hi = lo + 1;
                while (hi < K && key[(size_t)order[hi] * S + s] == key[(size_t)order[lo] * S + s]) ++hi;
                for (size_t j = lo; j < hi; ++j) ph->rank2[(size_t)order[j] * S + s] = (uint32_t)(lo + 1 + hi);
                lo = hi;
            }
        }
    }
    ph->n_clustered = n_clustered; ph->n_drop_na = n_drop_na; ph->n_drop_sd = n_drop_sd; ph->ms_pheno = now_ms() - t0;
    *out = ph;
    return RGX_OK;
}

// ---- the quantile: Wichura, "Algorithm AS 241: The Percentage Points of the Normal Distribution", Applied Statistics 37 (1988) 477-484, routine
// PPND16 (relative accuracy about 1e-16), restated from the paper's coefficients.  p = rank2 / (2 (K + 1)) never leaves the rationals before
// it has to: p - 1/2 and min(p, 1 - p) are quotients of exact integers, so the function is odd around the middle rank to the last bit.
extern "C" double rgx_pheno_quantile(uint32_t rank2, uint64_t n_rows) {
    const uint64_t two_n = 2 * (n_rows + 1);
    if (!n_rows || n_rows > (1ull << 40) || rank2 < 1 || rank2 >= two_n) return std::numeric_limits<double>::quiet_NaN();
    const bool low = (uint64_t)rank2 < n_rows + 1;
    const double q = (low ? -(double)(n_rows + 1 - rank2) : (double)(rank2 - (n_rows + 1))) / (double)two_n;
    if (fabs(q) <= 0.425) {
        const double r = 0.180625 - q * q;
        return q * (((((((2.5090809287301226727e+3 * r + 3.3430575583588128105e+4) * r + 6.7265770927008700853e+4) * r + 4.5921953931549871457e+4) * r +
                        1.3731693765509461125e+4) * r + 1.9715909503065514427e+3) * r + 1.3314166789178437745e+2) * r + 3.3871328727963666080e+0) /
                   (((((((5.2264952788528545610e+3 * r + 2.8729085735721942674e+4) * r + 3.9307895800092710610e+4) * r + 2.1213794301586595867e+4) * r +
                       5.3941960214247511077e+3) * r + 6.8718700749205790830e+2) * r + 4.2313330701600911252e+1) * r + 1.0);
    }
    double r = sqrt(-log((double)(low ? (uint64_t)rank2 : two_n - rank2) / (double)two_n)), v;
    if (r <= 5.0) {
        r -= 1.6;
        v = (((((((7.74545014278341407640e-4 * r + 2.27238449892691845833e-2) * r + 2.41780725177450611770e-1) * r + 1.27045825245236838258e+0) * r +
                3.64784832476320460504e+0) * r + 5.76949722146069140550e+0) * r + 4.63033784615654529590e+0) * r + 1.42343711074968357734e+0) /
            (((((((1.05075007164441684324e-9 * r + 5.47593808499534494600e-4) * r + 1.51986665636164571966e-2) * r + 1.48103976427480074590e-1) * r +
                6.89767334985100004550e-1) * r + 1.67638483018380384940e+0) * r + 2.05319162663775882187e+0) * r + 1.0);
    } else {
        r -= 5.0;
        v = (((((((2.01033439929228813265e-7 * r + 2.71155556874348757815e-5) * r + 1.24266094738807843860e-3) * r + 2.65321895265761230930e-2) * r +
                2.96560571828504891230e-1) * r + 1.78482653991729133580e+0) * r + 5.46378491116411436990e+0) * r + 6.65790464350110377720e+0) /
            (((((((2.04426310338993978564e-15 * r + 1.42151175831644588870e-7) * r + 1.84631831751005468180e-5) * r + 7.86869131145613259100e-4) * r +
                1.48753612908506148525e-2) * r + 1.36929880922735805310e-1) * r + 5.99832206555887937690e-1) * r + 1.0);
    }
    return low ? -v : v;
}

// ---- text ------------------------------------------------------------------------------------------------------------------------------
extern "C" size_t rgx_cohort_format_phenotypes(const rgx_cohort_matrix *m, const rgx_cohort_clusters *cl, const rgx_pheno_table *ph, char *buf,
                                               size_t cap) {
    if (!m || !cl || !ph || cl->n_rows != m->n || ph->n_samples != m->n_samples) return 0;
    for (uint64_t k = 0; k < ph->n_rows; ++k) if (ph->row[k] >= m->n || cl->cluster[ph->row[k]] == RGX_NO_CLUSTER) return 0;
    return format_twice(buf, cap, [&](TextOut &o) {
        o.put("#Chr\tstart\tend\tID");
        for (uint32_t g = 0; g < m->n_samples; ++g) { o.put("\t", 1); o.put(m->sample_name[g]); }
        o.put("\n", 1);
        for (uint64_t k = 0; k < ph->n_rows; ++k) {
            const uint32_t i = ph->row[k];
            o.put(m->ref_name[m->tid[i]]);
            o.fmt("\t%u\t%u\t", m->start[i], m->end[i]);
            put_intron_id(o, m, cl, i);
            for (uint32_t g = 0; g < m->n_samples; ++g) o.fmt("\t%.17g", rgx_pheno_quantile(ph->rank2[k * m->n_samples + g], ph->n_rows));
            o.put("\n", 1);
        }
    });
}
