// genotypes.cpp -- rgx_genotypes_load: the dosages of the cohort's samples from a VCF or BCF, in the order the sQTL calls want their variants
// (contract in include/regtools_amd.h), and rgx_genotypes_free.  Host only; the records come through VcfText (cse_host.h).
#include "api_internal.h"
#include "qtl_core.h"

namespace {
struct GenoBox { rgx_genotypes g; std::vector<uint32_t> tid, pos; std::vector<int8_t> dosage; std::vector<std::string> id; std::vector<char *> id_ptr; };

// the dosages of one record's GT values (kInts, v.count per file sample) for the cohort's samples; col[s] = the file's column of cohort sample s
void gt_dosages(const VcfValue &v, const std::vector<uint32_t> &col, int8_t *out) {
    const int32_t no_more = v.width == 1 ? -127 : v.width == 2 ? -32767 : INT32_MIN + 1;
    for (size_t s = 0; s < col.size(); ++s) {
        const int32_t *a = v.ints.data() + (size_t)col[s] * (size_t)v.count;
        int ploidy = 0, alt = 0; bool missing = false;
        for (; ploidy < v.count && a[ploidy] != no_more; ++ploidy) {
            const int32_t allele = (a[ploidy] >> 1) - 1;
            if (allele < 0 || allele > 1) missing = true; else alt += allele;
        }
        out[s] = ploidy == 2 && !missing ? (int8_t)alt : (int8_t)-1;
    }
}
}  // namespace

extern "C" void rgx_genotypes_free(rgx_genotypes *g) { delete (GenoBox *)g; }                  // g is the first member

extern "C" int rgx_genotypes_load(const char *path, const rgx_cohort_matrix *m, rgx_genotypes **out, char *err, size_t errlen) {
    if (!path || !m || !out) return fail(err, errlen, RGX_ERR_ARG, "regtools_amd: rgx_genotypes_load needs a path and a matrix\n");
    *out = nullptr;
    try {
        VcfText vcf;
        const std::string why = vcf.load(path, /*annotating=*/false);
        if (!why.empty()) return fail(err, errlen, RGX_ERR_OPEN, "%s", why.c_str());
        const std::vector<std::string> &have = vcf.hdr.sample_names();
        std::unordered_map<std::string, uint32_t> column;
        for (size_t j = have.size(); j-- > 0;) column[have[j]] = (uint32_t)j;            // (the first of equal names)
        const uint32_t S = m->n_samples;
        std::vector<uint32_t> col(S);
        for (uint32_t s = 0; s < S; ++s) {
            auto it = column.find(m->sample_name[s]);
            if (it == column.end()) return fail(err, errlen, RGX_ERR_ARG, "Sample %s has no genotypes in %s\n", m->sample_name[s], path);
            col[s] = it->second;
        }
        std::unordered_map<std::string, uint32_t> contig;
        for (int32_t t = m->n_ref; t-- > 0;) contig[m->ref_name[t]] = (uint32_t)t;
        std::unique_ptr<GenoBox> box(new GenoBox());
        rgx_genotypes &g = box->g;
        memset(&g, 0, sizeof g);
        VcfDictionary h = vcf.hdr;
        h.silence();
        struct Kept { uint32_t tid, pos; std::string id; std::vector<int8_t> d; };
        std::vector<Kept> kept;
        for (size_t i = 0; i < vcf.recs.size(); ++i) {
            VcfRecord r;
            if (vcf.typed(i, h, r) != ReadResult::kOk) break;
            ++g.n_records;
            auto c = contig.find(vcf.recs[i].chrom);
            if (c == contig.end()) { ++g.n_unknown_contig; continue; }
            if (r.alleles.size() != 2) { ++g.n_multiallelic; continue; }
            const VcfValue *gt = nullptr;
            for (const VcfRecord::Tagged &f : r.fields) if (h.id_name(f.key) == "GT" && f.v.store == VcfValue::kInts && f.v.count > 0) gt = &f.v;
            if (!gt || (size_t)r.n_samples < have.size() || gt->ints.size() < have.size() * (size_t)gt->count) { ++g.n_no_gt; continue; }
            Kept k;
            k.tid = c->second; k.pos = vcf.recs[i].pos0 + 1;
            k.id = !r.id.empty() && r.id != "." ? r.id : vcf.recs[i].chrom + ":" + std::to_string(k.pos) + ":" + r.alleles[0] + ":" + r.alleles[1];
            k.d.resize(S);
            gt_dosages(*gt, col, k.d.data());
            kept.push_back(std::move(k));
        }
        std::vector<uint32_t> order(kept.size());
        for (size_t i = 0; i < order.size(); ++i) order[i] = (uint32_t)i;
        std::stable_sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) {
            return qtl_key(kept[a].tid, kept[a].pos) < qtl_key(kept[b].tid, kept[b].pos); });
        const size_t V = kept.size();
        box->tid.resize(V); box->pos.resize(V); box->dosage.resize(V * S); box->id.resize(V); box->id_ptr.resize(V);
        for (size_t v = 0; v < V; ++v) {
            Kept &k = kept[order[v]];
            box->tid[v] = k.tid; box->pos[v] = k.pos; box->id[v] = std::move(k.id); box->id_ptr[v] = &box->id[v][0];
            if (S) memcpy(box->dosage.data() + v * S, k.d.data(), S);
        }
        g.n_variants = (uint32_t)V; g.n_samples = S;
        g.tid = box->tid.data(); g.pos = box->pos.data(); g.dosage = box->dosage.data(); g.id = box->id_ptr.data();
        *out = &box.release()->g;
        return RGX_OK;
    } catch (const std::bad_alloc &) { return fail(err, errlen, RGX_ERR_ARG, "regtools_amd: no memory for the genotypes of %s\n", path); }
}
