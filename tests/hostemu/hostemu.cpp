// tests/hostemu/hostemu.cpp -- TEST INFRASTRUCTURE ONLY.
// Compiles the per-lane device cores (inflate_core.h, bam_core.h) for the host so their logic can be
// unit-tested on a machine without a GPU.  Never linked into the product library.
#include "../../regtools_amd/csrc/inflate_core.h"

extern "C" int emu_inflate(const uint8_t *in, uint32_t in_len, uint8_t *out, uint32_t cap, uint32_t *out_len) {
    rgx::HostTab T;
    return rgx::inflate_raw(in, in_len, out, cap, out_len, T);
}
extern "C" int emu_inflate_lits(const uint8_t *in, uint32_t in_len, uint8_t *out, uint32_t cap, uint32_t *out_len) {
    rgx::HostTab T;
    return rgx::inflate_raw<4>(in, in_len, out, cap, out_len, T);
}

// the round-2 decoder (inflate_ring.h: per-lane LDS window, cooperative line flush) with a one-lane wave.  The member is inflated into
// a private buffer at destination phase `phase` (address % 128) with guard bytes around it: returns -100 / -101 if a byte in front of /
// behind the member's [0, cap) was written.
#include "../../regtools_amd/csrc/inflate_ring.h"
#include <vector>
extern "C" int emu_inflate_ring(const uint8_t *in, uint32_t in_len, uint8_t *out, uint32_t cap, uint32_t *out_len, uint32_t phase) {
    std::vector<uint8_t> ibuf((size_t)in_len + 64 + 32, 0);
    memcpy(ibuf.data() + 32, in, in_len);
    std::vector<uint8_t> obuf((size_t)cap + 1024, 0xA5);
    uint8_t *dst = (uint8_t *)(((uintptr_t)obuf.data() + 127) & ~(uintptr_t)127) + 256 + (phase & 127u);
    rgx::HostTab T; rgx::HostRing R; rgx::HostCoop C;
    memset(&R, 0xCC, sizeof R);
    const int st = rgx::inflate_ring(ibuf.data() + 32, in_len, dst, cap, out_len, T, R, C, true);
    for (uint8_t *q = obuf.data(); q < dst; ++q) if (*q != 0xA5) return -100;
    for (uint8_t *q = dst + cap; q < obuf.data() + obuf.size(); ++q) if (*q != 0xA5) return -101;
    memcpy(out, dst, *out_len <= cap ? *out_len : cap);
    return st;
}

// the round-3 decoder (inflate_coop.h: long matches handed to the wave) with a one-lane wave; same guard bytes, every destination phase
#include "../../regtools_amd/csrc/inflate_coop.h"
extern "C" int emu_inflate_coop(const uint8_t *in, uint32_t in_len, uint8_t *out, uint32_t cap, uint32_t *out_len, uint32_t phase, int pairs) {
    // (the payload at every phase of a 16-byte block too)
    std::vector<uint8_t> ibuf((size_t)in_len + 64 + 64, 0xEE);
    uint8_t *src = (uint8_t *)(((uintptr_t)ibuf.data() + 15) & ~(uintptr_t)15) + 16 + ((phase * 7u) & 15u);
    memcpy(src, in, in_len);
    memset(src + in_len, 0, 24);
    std::vector<uint8_t> obuf((size_t)cap + 1024, 0xA5);
    uint8_t *dst = (uint8_t *)(((uintptr_t)obuf.data() + 127) & ~(uintptr_t)127) + 256 + (phase & 127u);
    rgx::HostTab T; rgx::HostCopy C;
    // bit 0 of `pairs`: a literal and the symbol behind it per trip; bit 1 selects the windowed bit reader; bit 2 (with bit 0): two literals and a
    // match behind them per trip, bits counted exactly (the decoder's mode bit 1); bit 3: runs written from registers (mode bit 2)
    const uint32_t mode = (uint32_t)(pairs & 1) | ((pairs & 4) ? 2u : 0u) | ((pairs & 8) ? 4u : 0u);
    const int st = (pairs & 2) ? rgx::inflate_coop<rgx::BitReaderWin>(src, in_len, dst, cap, out_len, T, C, true, mode)
                               : rgx::inflate_coop<rgx::BitReader>(src, in_len, dst, cap, out_len, T, C, true, mode);
    for (uint8_t *q = obuf.data(); q < dst; ++q) if (*q != 0xA5) return -100;
    for (uint8_t *q = dst + cap; q < obuf.data() + obuf.size(); ++q) if (*q != 0xA5) return -101;
    memcpy(out, dst, *out_len <= cap ? *out_len : cap);
    return st;
}

// the small-input decoder (inflate_wave.h: one member per wave, whole member in LDS) with the host's one-thread wave
#include "../../regtools_amd/csrc/inflate_wave.h"
extern "C" int emu_inflate_wave(const uint8_t *in, uint32_t in_len, uint8_t *out, uint32_t cap, uint32_t *out_len, uint32_t phase) {
    std::vector<uint8_t> ibuf((size_t)in_len + 64, 0);
    memcpy(ibuf.data(), in, in_len);
    std::vector<uint8_t> obuf((size_t)cap + 1024, 0xA5);
    uint8_t *dst = (uint8_t *)(((uintptr_t)obuf.data() + 127) & ~(uintptr_t)127) + 256 + (phase & 127u);
    static rgx::WaveShared S;
    memset(&S, 0xCC, sizeof S);
    rgx::HostWave W;
    const int st = rgx::inflate_wave(W, S, ibuf.data(), in_len, dst, cap, out_len);
    for (uint8_t *q = obuf.data(); q < dst; ++q) if (*q != 0xA5) return -100;
    for (uint8_t *q = dst + cap; q < obuf.data() + obuf.size(); ++q) if (*q != 0xA5) return -101;
    memcpy(out, dst, *out_len <= cap ? *out_len : cap);
    return st;
}

// ---- the decoders IN PLACE: on the caller's own payload bytes, no copy of the input (inflate_inplace.h, shared with inflate_edges.cpp) ------------
// The output goes to a private buffer at destination phase `phase`, 16 spare bytes or more on both sides: -100 / -101 if a byte in front of / behind
// the member's [0, cap) was written.  What each decoder may READ around its payload is the contract written down in inflate_inplace.h.
#include "inflate_inplace.h"
extern "C" uint32_t emu_inflate_front_bytes(int variant) { return rgx_emu::front_bytes(variant); }
extern "C" int emu_inflate_inplace(int variant, const uint8_t *in, uint32_t in_len, uint8_t *out, uint32_t cap, uint32_t *out_len, uint32_t phase) {
    std::vector<uint8_t> obuf((size_t)cap + 128 + 128 + 128 + 16, 0xA5);      // alignment, front, phase, behind
    uint8_t *dst = (uint8_t *)(((uintptr_t)obuf.data() + 127) & ~(uintptr_t)127) + 128 + (phase & 127u);
    const int st = rgx_emu::run(variant, in, in_len, dst, cap, out_len);
    for (uint8_t *q = obuf.data(); q < dst; ++q) if (*q != 0xA5) return -100;
    for (uint8_t *q = dst + cap; q < obuf.data() + obuf.size(); ++q) if (*q != 0xA5) return -101;
    memcpy(out, dst, *out_len <= cap ? *out_len : cap);
    return st;
}

// ---- the per-alignment cores of bam_core.h / cse_core.h, as the kernels call them ---------------------------------------------
#include "../../regtools_amd/csrc/bam_core.h"
#include "../../regtools_amd/csrc/cse_core.h"

struct emu_candidate { uint32_t start, end, thick_start, thick_end; };

extern "C" int emu_cigar_walk(int32_t pos, const uint32_t *cigar, uint32_t n_cigar, emu_candidate *out, int max_out) {
    int n = 0;
    rgx::cigar_walk(pos, reinterpret_cast<const uint8_t *>(cigar), n_cigar, [&](uint32_t s, uint32_t e, uint32_t ts, uint32_t te) {
        if (n < max_out) out[n] = emu_candidate{s, e, ts, te};
        ++n;
    });
    return n;
}
extern "C" int emu_strand_from_flag(uint32_t flag, int strandness) { return rgx::strand_from_flag(flag, strandness); }
extern "C" int emu_strand_from_tag(const uint8_t *aux, uint32_t len, uint8_t t0, uint8_t t1) { return rgx::strand_from_tag(aux, aux + len, t0, t1); }
extern "C" uint32_t emu_ucsc_bin(uint32_t start, uint32_t end) { return rgx::ucsc_bin(start, end); }
extern "C" int32_t emu_rec_endpos(const uint32_t *cigar, uint32_t n_cigar, uint32_t flag, int32_t pos) {
    return rgx::rec_endpos(reinterpret_cast<const uint8_t *>(cigar), n_cigar, flag, pos);
}

// record_row over one record's bytes (from its block_size word), as the decode kernels call it: the scalar fields of ExtractCfg, and the three
// optional outputs as on / off flags (the rule only tests those pointers for null).  Returns 0, or -1 for bytes that are not one whole sane record.
struct emu_row_cfg {
    int32_t n_ref, strandness; uint8_t tag0, tag1, bc0, bc1; uint32_t min_intron, max_intron; int32_t region_tid, region_beg, region_end;
    uint32_t long_threshold, stop_index; int32_t stop_on, abort_on, odd_on;
};
struct emu_row { int32_t in_region, stop_candidate, is_long, abort_read, odd_read, strand; uint32_t nev; };
extern "C" int emu_record_row(const uint8_t *rec, size_t len, uint32_t i, const emu_row_cfg *c, emu_row *out) {
    rgx::RecHead h;
    if (len < 36) return -1;
    rgx::rec_head(rec, h);
    if (!rgx::rec_sane(h) || 4 + (size_t)(uint32_t)h.block_len != len) return -1;
    static uint32_t on[2];                                  // somewhere for the three pointers to point: never read, never written
    rgx::ExtractCfg cfg = {};
    cfg.n_ref = c->n_ref; cfg.strandness = c->strandness; cfg.tag0 = c->tag0; cfg.tag1 = c->tag1; cfg.bc0 = c->bc0; cfg.bc1 = c->bc1;
    cfg.min_intron = c->min_intron; cfg.max_intron = c->max_intron;
    cfg.region_tid = c->region_tid; cfg.region_beg = c->region_beg; cfg.region_end = c->region_end;
    cfg.long_threshold = c->long_threshold; cfg.stop_index = c->stop_index;
    cfg.stop_out = c->stop_on ? on : nullptr; cfg.abort_out = c->abort_on ? on : nullptr; cfg.odd_count = c->odd_on ? on : nullptr;
    const uint8_t *data = rec + 36;
    const rgx::RecordRow r = rgx::record_row(h, i, cfg,
        [&](uint32_t q) { return rgx::ld32(data + h.l_qname + 4 * (size_t)q); },
        [&](uint8_t t0, uint8_t t1, bool *unknown) { return rgx::strand_from_tag(data + h.aux_off, data + ((int64_t)h.block_len - 32), t0, t1, unknown); });
    *out = emu_row{r.in_region, r.stop_candidate, r.is_long, r.abort_read, r.odd_read, r.strand, r.nev};
    return 0;
}

// ---- index normalisation (host_io.cpp): BAI / CSI / BGZF-compressed -> what the pipeline reads from it ---------------------------------
#include "../../regtools_amd/csrc/host_io.h"
// out[0..4] = n_ref, have_start, start_voff, n_no_coor, n_anchors; got[k] = first listed record start >= targets[k].  0 = not an index
extern "C" int emu_index_summary(const uint8_t *idx, size_t n, uint64_t *out, const uint64_t *targets, int nt, uint64_t *got) {
    std::vector<uint8_t> image; const uint8_t *d; size_t len;
    if (!rgx::normalize_index(idx, n, image, d, len)) return 0;
    rgx::BaiInfo bi;
    if (!rgx::parse_bai(d, len, bi, true)) return 0;
    out[0] = (uint64_t)bi.n_ref; out[1] = bi.have_start; out[2] = bi.start_voff; out[3] = bi.n_no_coor; out[4] = bi.anchors.size();
    if (nt) rgx::bai_first_anchor_ge(d, len, targets, nt, got);
    return 1;
}

// ---- the REAL std::unordered_map<std::string,int> of this image's libstdc++: what oracle.c's restated container is pinned against -----
#include <string>
#include <unordered_map>
// insert keys[0..n) the way Junction::barcodes receives them (a repeated key increments); order[k] = index of the first occurrence of the
// k-th key in iteration order, counts[k] its count, buckets = final bucket_count; returns the number of distinct keys
extern "C" size_t emu_umap_order(const char *const *keys, size_t n, size_t *order, int *counts, size_t *buckets) {
    std::unordered_map<std::string, int> m, first;
    for (size_t i = 0; i < n; ++i) {
        auto it = m.find(keys[i]);
        if (it != m.end()) { std::unordered_map<std::string, int> c = m; c[it->first]++; m = c; }      // the reference's copy-then-bump (cc:207-210)
        else { std::unordered_map<std::string, int> c = m; c.insert(std::pair<std::string, int>(keys[i], 1)); m = c; first[keys[i]] = (int)i; }
    }
    size_t k = 0;
    for (auto it = m.begin(); it != m.end(); ++it, ++k) { order[k] = (size_t)first[it->first]; counts[k] = it->second; }
    *buckets = m.bucket_count();
    return k;
}

// region -> [lo, hi) virtual offsets from a BAI (host_io.cpp bai_region_span); returns 1 span, 0 nothing to read, -1 not usable
extern "C" int emu_region_span(const uint8_t *bai, size_t n, int32_t tid, int32_t beg, int32_t end, uint64_t *lo, uint64_t *hi) {
    std::vector<uint8_t> image; const uint8_t *d; size_t len;
    if (!rgx::normalize_index(bai, n, image, d, len)) return -2;          // as prepare_events sees it: .bai, .csi or BGZF-compressed
    bool usable = false;
    if (rgx::bai_region_span(d, len, tid, beg, end, *lo, *hi, usable)) return 1;
    return usable ? 0 : -1;
}
// the BAM header through the host decoder (host_io.cpp host_bam_header): number of contigs, or -1
extern "C" int emu_host_header(const uint8_t *bam, size_t n, char *first_name, size_t cap) {
    rgx::BamHeader h;
    if (!rgx::host_bam_header(bam, n, h)) return -1;
    if (!h.names.empty() && cap) { strncpy(first_name, h.names[0].c_str(), cap - 1); first_name[cap - 1] = 0; }
    return (int)h.names.size();
}

// the host's parallel BGZF member scan (host_io.cpp scan_members_parallel: what rgx_extract_mem's overlapped upload launches from): number of
// members and total inflated size, or -1 when the file is not one the scan vouches for; members[k] = {cpos, upos, clen, isize} as 4 x u64
extern "C" long emu_scan_members(const uint8_t *bam, size_t n, int threads, uint64_t *members, size_t cap, uint64_t *total) {
    std::vector<rgx::Member> m;
    if (!rgx::scan_members_parallel(bam, n, threads, m, *total)) return -1;
    for (size_t k = 0; k < m.size() && k < cap; ++k) { members[4 * k] = m[k].cpos; members[4 * k + 1] = m[k].upos; members[4 * k + 2] = m[k].clen; members[4 * k + 3] = m[k].isize; }
    return (long)m.size();
}

// the annotated-VCF writer (cse_host.cpp write_annotated_vcf_records over vcf_rewrite.cpp) with "NA" for every record: what
// `variants annotate` writes when no transcript is near any variant.  Returns 0, 1 = load error (message in err), 2 = writer error.
#include "../../regtools_amd/csrc/cse_host.h"
// returns 0, or how the reference's process ends: 1 = through the tool's own error path (message, status 1); 4 / 5 = htslib ends it while the header is read,
// with exit(1) / abort(); 2 / 3 = the same at a record (what was written in front of it is in the file)
extern "C" int emu_vcf_rewrite(const char *in_path, const char *out_path, char *err, size_t errlen) {
    rgx::VcfText vcf;
    std::string e = vcf.load(in_path);
    if (!e.empty()) { snprintf(err, errlen, "%s", e.c_str()); return vcf.death == 2 ? 5 : vcf.death == 1 ? 4 : 1; }
    FILE *f = fopen(out_path, "w");
    if (!f) return 2;
    std::vector<size_t> todo(vcf.recs.size());
    for (size_t i = 0; i < todo.size(); ++i) todo[i] = i;
    e = rgx::write_annotated_vcf_records(f, vcf, todo, [](size_t) { return rgx::VcfAnnot{nullptr, nullptr, nullptr, nullptr}; });
    fclose(f);
    if (!e.empty()) { snprintf(err, errlen, "%s", e.c_str()); return vcf.fatal_aborts ? 3 : 2; }
    return 0;
}

// GtfModel::load on the host (it has no device part): every table, as text, for tests/test_hostemu.py
extern "C" int emu_gtf_dump(const char *gtf_path, const char *out_path, char *err, size_t errlen) {
    rgx::GtfModel m;
    const std::string e = m.load(gtf_path);
    if (!e.empty()) { snprintf(err, errlen, "%s", e.c_str()); return 1; }
    FILE *f = fopen(out_path, "w");
    if (!f) return 2;
    for (size_t i = 0; i < m.chroms.size(); ++i) fprintf(f, "chrom %zu %s\n", i, m.chroms[i].c_str());
    for (size_t t = 0; t < m.tx_id.size(); ++t) {
        fprintf(f, "tx %s %s %s %d %c %u", m.tx_id[t].c_str(), m.tx_gene_name[t].c_str(), m.tx_gene_id[t].c_str(), m.tx_chrom[t], m.tx_strand[t], m.tx_bin[t]);
        for (uint32_t q = 0; q < m.tx_n_exons[t]; ++q) fprintf(f, " %u-%u", m.es[m.tx_exon_off[t] + q], m.ee[m.tx_exon_off[t] + q]);
        fputc('\n', f);
    }
    for (size_t i = 0; i < m.bin_key.size(); ++i) fprintf(f, "bin %llu %u %u\n", (unsigned long long)(m.bin_key[i] >> 32), (unsigned)(m.bin_key[i] & 0xffffffffu), m.bin_tx[i]);
    {   // the direct index must describe the table above exactly
        bool ok = m.bin_start.size() == m.chroms.size() * (size_t)m.bin_stride + 1 && m.bin_start.back() == m.bin_key.size() && m.bin_start[0] == 0;
        for (size_t k = 0; ok && k + 1 < m.bin_start.size(); ++k) {
            if (m.bin_start[k] > m.bin_start[k + 1]) ok = false;
            for (uint32_t j = m.bin_start[k]; ok && j < m.bin_start[k + 1]; ++j)
                if (m.bin_key[j] != ((uint64_t)(k / m.bin_stride) << 32 | (uint64_t)(k % m.bin_stride))) ok = false;
        }
        fprintf(f, "bin_start %s\n", ok ? "ok" : "BAD");
    }
    fclose(f);
    return 0;
}

// worker_pool.h / bigvec.h on their own: parallel_sort against std::sort, the pool's every-task-once contract, huge-page vectors
#include <stdexcept>
#include "../../regtools_amd/csrc/worker_pool.h"
#include "../../regtools_amd/csrc/bigvec.h"
extern "C" int emu_pool_selftest(uint32_t seed, uint32_t n, uint32_t threads) {
    rgx::WorkerPool pool(threads);
    uint64_t x = seed * 0x9e3779b97f4a7c15ull + 1;
    auto rnd = [&] { x ^= x << 13; x ^= x >> 7; x ^= x << 17; return x; };
    rgx::BigVec<uint64_t> a(n), b;
    for (auto &v : a) v = rnd() % (n / 3 + 2);                     // plenty of equal keys
    b.assign(a.begin(), a.end());
    std::sort(b.begin(), b.end());
    rgx::parallel_sort(pool, a.begin(), a.end(), [](uint64_t p, uint64_t q) { return p < q; });
    if (a.size() != b.size() || !std::equal(a.begin(), a.end(), b.begin())) return 1;
    // every task exactly once, whatever the task count
    for (size_t tasks : {(size_t)0, (size_t)1, (size_t)2, (size_t)threads, (size_t)threads * 7 + 3}) {
        std::vector<std::atomic<int>> hit(tasks);
        for (auto &h : hit) h = 0;
        pool.run(tasks, [&](size_t k) { hit[k].fetch_add(1); });
        for (auto &h : hit) if (h.load() != 1) return 2;
    }
    // a task that throws: the phase still runs every other task once, the first exception comes out of run(), the pool stays usable
    {
        const size_t tasks = (size_t)threads * 5 + 2;
        std::vector<std::atomic<int>> hit(tasks);
        for (auto &h : hit) h = 0;
        bool thrown = false;
        try { pool.run(tasks, [&](size_t k) { hit[k].fetch_add(1); if (k == tasks / 2) throw std::runtime_error("task"); }); }
        catch (const std::runtime_error &) { thrown = true; }
        if (!thrown) return 6;
        for (auto &h : hit) if (h.load() != 1) return 7;
        std::atomic<int> sum{0};
        pool.run(tasks, [&](size_t) { sum.fetch_add(1); });
        if (sum.load() != (int)tasks) return 8;
        // a run() from inside a task does its work on the calling thread instead of queueing behind itself
        std::atomic<int> inner{0};
        pool.run(4, [&](size_t) { pool.run(3, [&](size_t) { inner.fetch_add(1); }); });
        if (inner.load() != 12) return 9;
    }
    // a block above the huge-page threshold: aligned, writable end to end, survives growth
    rgx::BigVec<uint32_t> big;
    big.resize((3u << 20) / 4 + 5);
    if (((uintptr_t)big.data() & ((2u << 20) - 1)) != 0) return 3;
    for (size_t i = 0; i < big.size(); ++i) big[i] = (uint32_t)i;
    big.resize((9u << 20) / 4 + 1);
    for (size_t i = 0; i < (3u << 20) / 4 + 5; ++i) if (big[i] != (uint32_t)i) return 4;
    big.back() = 7;
    rgx::BigVec<std::string> names(1000);
    for (auto &s : names) if (!s.empty()) return 5;                 // strings ARE constructed (only trivial types are left untouched)
    return 0;
}

// (lab) wall time of GtfModel::load alone, in ms: what the call costs its caller including the teardown of its temporaries
#include <chrono>
extern "C" double emu_gtf_load_ms(const char *gtf_path) {
    const auto t0 = std::chrono::steady_clock::now();
    rgx::GtfModel *m = new rgx::GtfModel();
    const std::string e = m->load(gtf_path);
    const double ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    delete m;
    return e.empty() ? ms : -1.0;
}

// carve.h on its own, over a host array of `cap` bytes: take k asks for count[k] elements of width[k] bytes (1, 4 or 8); off[k] receives the offset of
// the pointer it returned.  Returns Carve::over behind the last take (-1: a width Carve has no form for).
#include "../../regtools_amd/csrc/carve.h"
extern "C" int emu_carve(size_t cap, size_t n_takes, const uint32_t *width, const size_t *count, size_t *off) {
    std::vector<uint8_t> mem(cap ? cap : 1);
    Carve w(mem.data(), cap);
    for (size_t k = 0; k < n_takes; ++k) {
        const uint8_t *r = nullptr;
        if (width[k] == 1) r = w.u8(count[k]);
        else if (width[k] == 4) r = (const uint8_t *)w.u32(count[k]);
        else if (width[k] == 8) r = (const uint8_t *)w.u64(count[k]);
        else return -1;
        off[k] = (size_t)(r - mem.data());
    }
    return w.over ? 1 : 0;
}

// The same with a log attached.  type[k]: 1, 2, 4, 8 an integer of that width, 16 a float, 17 a double.  Returns `over` (bit 0) and the log's `full`
// (bit 1), -1 for a type there is none of; off as emu_carve; the log's arrays as (offset, bytes, kind) in log_rows (room for log_cap rows, *n_log
// receives the log's count) and where its last array ends in *end.  The log starts out dirty: the Carve has to reset it.
extern "C" int emu_carve_log(size_t cap, size_t n_takes, const uint32_t *type, const size_t *count, size_t *off, size_t *log_rows, size_t log_cap,
                             size_t *n_log, size_t *end) {
    std::vector<uint8_t> mem(cap ? cap : 1);
    CarveLog lg; lg.n = 7; lg.end = 99; lg.full = true;
    Carve w(mem.data(), cap, &lg);
    for (size_t k = 0; k < n_takes; ++k) {
        const uint8_t *r = nullptr;
        if (type[k] == 1) r = (const uint8_t *)w.take<int8_t>(count[k]);
        else if (type[k] == 2) r = (const uint8_t *)w.take<uint16_t>(count[k]);
        else if (type[k] == 4) r = (const uint8_t *)w.u32(count[k]);
        else if (type[k] == 8) r = (const uint8_t *)w.u64(count[k]);
        else if (type[k] == 16) r = (const uint8_t *)w.take<float>(count[k]);
        else if (type[k] == 17) r = (const uint8_t *)w.take<double>(count[k]);
        else return -1;
        off[k] = (size_t)(r - mem.data());
    }
    *n_log = lg.n; *end = lg.end;
    for (uint32_t i = 0; i < lg.n && i < log_cap; ++i) { log_rows[3 * i] = lg.a[i].off; log_rows[3 * i + 1] = lg.a[i].bytes; log_rows[3 * i + 2] = (size_t)lg.a[i].kind; }
    return (w.over ? 1 : 0) | (lg.full ? 2 : 0);
}
extern "C" uint32_t emu_carve_log_cap() { return CarveLog::kCap; }

// carve_guard_check over a window of n bytes: 1 untouched, 0 touched with the message in msg
extern "C" int emu_carve_guard(const uint8_t *window, size_t n, const char *what, char *msg, size_t msglen) {
    return carve_guard_check(window, n, what, msg, msglen) ? 1 : 0;
}

// cse_table.h on its own: the first-insert junction table of `identify` / `associate`.  names / vnames: contig names of the junctions and of the variants
// (equal names may repeat); cand: n_cand x (contig, start, end, variant contig, variant pos, src), indices into names / vnames, in arrival order.
// threads: the pool finish() sorts on (0 = none given: its own).  rows: per junction in table order (contig, start, end, src of the row that stayed,
// v0, v1) with [v0, v1) its variants in vars: (variant contig, pos) -- contigs as the first index that bears the name.  Returns the number of rows, -1 when
// they do not fit, -2 when a junction's fields were asked for more than once.
#include "../../regtools_amd/csrc/cse_table.h"
extern "C" long emu_jtable(size_t n_names, const char *const *names, size_t n_vnames, const char *const *vnames, size_t n_cand, const uint32_t *cand,
                           uint32_t threads, uint32_t *rows, size_t rows_cap, uint32_t *vars, size_t vars_cap, size_t *n_vars) {
    std::vector<std::string> nm(names, names + n_names), vnm(vnames, vnames + n_vnames);
    JTable t;
    std::vector<uint32_t> crank_of, vrank_of;
    string_ranks(nm, crank_of, t.chrom_name);
    run_string_ranks(n_cand, [&](size_t k) -> const std::string & { return vnm[cand[6 * k + 3]]; }, vrank_of, t.vchrom_name);
    for (size_t k = 0; k < n_cand; ++k) t.add(crank_of[cand[6 * k]], cand[6 * k + 1], cand[6 * k + 2], vrank_of[k], cand[6 * k + 4], cand[6 * k + 5]);
    size_t asked = 0;
    auto entry_of = [&](uint32_t src) { ++asked; return JEntry{src, 0, 0, "+", "", 2}; };
    if (threads) { rgx::WorkerPool pool(threads); t.finish(entry_of, &pool); }
    else t.finish(entry_of, nullptr);
    if (asked != t.size()) return -2;
    if (t.size() > rows_cap || t.vars.size() > vars_cap) return -1;
    auto first_index = [](const std::vector<std::string> &v, const std::string &s) { return (uint32_t)(std::find(v.begin(), v.end(), s) - v.begin()); };
    for (size_t i = 0; i < t.size(); ++i) {
        const JTable::Row &r = t.rows[i];
        const uint32_t out[6] = {first_index(nm, t.chrom_name[r.crank]), r.js, r.jend, r.e.ts, r.v0, r.v1};
        memcpy(rows + 6 * i, out, sizeof out);
    }
    for (size_t k = 0; k < t.vars.size(); ++k) { vars[2 * k] = first_index(vnm, t.vchrom_name[t.vars[k].first]); vars[2 * k + 1] = t.vars[k].second; }
    *n_vars = t.vars.size();
    return (long)t.size();
}

// The two annotation cores of cse_core.h over host memory (tests/test_cse_edges_host.py): GtfModel::load, a GtfView over its vectors in whichever
// index form the model chose (bin_start empty: the kernels' binary search), then junction_scan / variant_scan junction by junction -- the raw lists
// rgx_k_junction_scan and rgx_variant_windows return.  Outputs beyond `cap` items are counted, not written; the return value is the item count.
struct emu_gtf { rgx::GtfModel m; rgx::GtfView v; };
extern "C" void *emu_gtf_open(const char *gtf_path, char *err, size_t errlen) {
    emu_gtf *g = new emu_gtf();
    const std::string e = g->m.load(gtf_path);
    if (!e.empty()) { snprintf(err, errlen, "%s", e.c_str()); delete g; return nullptr; }
    const rgx::GtfModel &m = g->m;
    g->v.tx_strand = m.tx_strand.data(); g->v.tx_exon_off = m.tx_exon_off.data(); g->v.tx_n_exons = m.tx_n_exons.data();
    g->v.es = m.es.data(); g->v.ee = m.ee.data(); g->v.bin_key = m.bin_key.data(); g->v.bin_tx = m.bin_tx.data(); g->v.n_bin = (uint32_t)m.bin_key.size();
    g->v.bin_start = m.bin_start.size() ? m.bin_start.data() : nullptr; g->v.bin_stride = m.bin_start.size() ? m.bin_stride : 0;
    g->v.keep_single = 0;
    return g;
}
extern "C" void emu_gtf_close(void *h) { delete (emu_gtf *)h; }
extern "C" int emu_gtf_bin_index(const void *h) { return ((const emu_gtf *)h)->v.bin_start ? 1 : 0; }
extern "C" uint32_t emu_gtf_n_tx(const void *h) { return (uint32_t)((const emu_gtf *)h)->m.tx_id.size(); }
extern "C" uint32_t emu_gtf_n_chroms(const void *h) { return (uint32_t)((const emu_gtf *)h)->m.chroms.size(); }
extern "C" const char *emu_gtf_tx_id(const void *h, uint32_t t) { return ((const emu_gtf *)h)->m.tx_id[t].c_str(); }
extern "C" uint32_t emu_gtf_tx_bin(const void *h, uint32_t t) { return ((const emu_gtf *)h)->m.tx_bin[t]; }
extern "C" int32_t emu_gtf_chrom_of(const void *h, const char *name) { return ((const emu_gtf *)h)->m.chrom_of(name); }

extern "C" long emu_junction_scan(const void *h, uint32_t n, const int32_t *contig, const uint32_t *js, const uint32_t *je, const char *strand, int keep_single,
                                  uint32_t *flags, uint32_t *visits, uint32_t *item_off, size_t cap, uint32_t *kind, uint32_t *a, uint32_t *b) {
    rgx::GtfView v = ((const emu_gtf *)h)->v;
    v.keep_single = keep_single ? 1u : 0u;
    size_t k = 0;
    for (uint32_t i = 0; i < n; ++i) {
        if (contig[i] >= (int64_t)((const emu_gtf *)h)->m.chroms.size()) return -1;
        rgx::JunctionFlags f;
        item_off[i] = (uint32_t)k;
        rgx::junction_scan(v, contig[i], js[i], je[i], strand[i], f, visits[i], [&](uint32_t kd, uint32_t x, uint32_t y) {
            if (k < cap) { kind[k] = kd; a[k] = x; b[k] = y; }
            ++k;
        });
        flags[i] = f.known_donor | f.known_acceptor << 1 | f.known_junction << 2;
    }
    item_off[n] = (uint32_t)k;
    return (long)k;
}

extern "C" long emu_variant_scan(const void *h, uint32_t n, const int32_t *contig, const uint32_t *pos0, uint32_t intronic_min, uint32_t exonic_min,
                                 int all_intronic, int all_exonic, int skip_single, uint32_t *ces, uint32_t *cee, uint32_t *visits, uint32_t *hit_off,
                                 size_t cap, uint32_t *tx, uint32_t *ann, uint32_t *dist) {
    const rgx::GtfView &v = ((const emu_gtf *)h)->v;
    const rgx::VariantOpts o{intronic_min, exonic_min, all_intronic, all_exonic, skip_single};
    size_t k = 0;
    for (uint32_t i = 0; i < n; ++i) {
        if (contig[i] >= (int64_t)((const emu_gtf *)h)->m.chroms.size()) return -1;
        hit_off[i] = (uint32_t)k;
        rgx::variant_scan(v, contig[i], pos0[i], o, ces[i], cee[i], visits[i], [&](uint32_t t, uint32_t an, uint32_t d) {
            if (k < cap) { tx[k] = t; ann[k] = an; dist[k] = d; }
            ++k;
        });
    }
    hit_off[n] = (uint32_t)k;
    return (long)k;
}

// front_plan.h on its own: the plan of an extract call's front (upload range and chunks, the gate, member ranges, pieces, early-tail parts).  Member lists
// are arrays of rgx::Member (cpos, upos: u64; clen, isize: u32); lists come back in the caller's arrays, the function's value is their length.
#include "../../regtools_amd/csrc/front_plan.h"
extern "C" int emu_front_region_kind(const char *region) { return (int)rgx::region_kind(region); }       // 0 whole, 1 rest, 2 query
extern "C" void emu_front_shard_cut_targets(size_t bam_len, int shard, int n_shards, uint64_t floor_voff, uint64_t *tgt) {
    rgx::shard_cut_targets(bam_len, shard, n_shards, floor_voff, tgt);
}
extern "C" void emu_front_shard_upload_range(size_t bam_len, int shard, int n_shards, const uint64_t *got, size_t header_bytes, size_t fourth_member_end,
                                             size_t *out3) {
    const rgx::UploadRange r = rgx::shard_upload_range(bam_len, shard, n_shards, got, header_bytes, fourth_member_end);
    out3[0] = r.lo; out3[1] = r.hi; out3[2] = r.hdr_hi;
}
extern "C" int emu_front_payload_takes_gate(const uint8_t *bam, size_t n) { return rgx::payload_takes_gate(bam, n) ? 1 : 0; }
extern "C" int emu_front_inflate_plan_for(uint64_t compressed, uint64_t inflated) { return rgx::inflate_plan_for(compressed, inflated); }
extern "C" size_t emu_front_upload_chunks(size_t up_lo, size_t up_hi, int gated, unsigned gate_chunks, int one_shot, size_t *gate_chunk, size_t *end,
                                          size_t cap) {
    const rgx::UploadChunks u = rgx::plan_upload_chunks(up_lo, up_hi, gated != 0, gate_chunks, one_shot != 0);
    *gate_chunk = u.gate_chunk;
    for (size_t k = 0; k < u.end.size() && k < cap; ++k) end[k] = u.end[k];
    return u.end.size();
}
extern "C" void emu_front_member_query(const rgx::Member *hm, uint32_t n, const uint64_t *q, uint32_t *q_index, uint64_t *q_upos, uint32_t *stop) {
    const rgx::MemberQuery r = rgx::host_member_query(hm, n, q);
    for (int k = 0; k < 3; ++k) { q_index[k] = r.q_index[k]; q_upos[k] = r.q_upos[k]; }
    *stop = r.stop;
}
extern "C" void emu_front_member_range(uint64_t cut_lo, uint64_t cut_hi, const uint32_t *q_index, uint32_t stop, uint32_t n_members_all, int chunked,
                                       int region_to_file_end, uint32_t *out2) {
    rgx::member_range(cut_lo, cut_hi, q_index, stop, n_members_all, chunked != 0, region_to_file_end != 0, out2[0], out2[1]);
}
extern "C" uint32_t emu_front_lookahead(int gate) { return gate ? rgx::kGateLookahead : rgx::kPieceLookahead; }
extern "C" uint32_t emu_front_first_member_reading_past(const rgx::Member *hm, uint32_t lo, uint32_t hi, uint64_t lim_b, uint32_t lookahead) {
    return rgx::first_member_reading_past(hm, lo, hi, lim_b, lookahead);
}
extern "C" uint32_t emu_front_gate_chunk_needed(uint64_t cpos, uint32_t clen, uint64_t gate_lo, uint64_t chunk_bytes, uint32_t n_chunks) {
    return rgx::gate_chunk_needed(cpos, clen, gate_lo, chunk_bytes, n_chunks);
}
extern "C" int emu_front_upload_covers_members(const rgx::Member *hm, uint32_t m_lo, uint32_t m_hi, size_t up_lo, size_t up_hi) {
    return rgx::upload_covers_members(hm, m_lo, m_hi, up_lo, up_hi) ? 1 : 0;
}
extern "C" size_t emu_front_pieces(const rgx::Member *hm, uint32_t m_lo, uint32_t m_hi, const size_t *end, size_t n_end, uint32_t *out3, size_t cap) {
    const std::vector<rgx::Piece> v = rgx::plan_pieces(hm, m_lo, m_hi, end, n_end);
    for (size_t k = 0; k < v.size() && k < cap; ++k) { out3[3 * k] = v[k].chunk; out3[3 * k + 1] = v[k].g_lo; out3[3 * k + 2] = v[k].g_hi; }
    return v.size();
}
extern "C" size_t emu_front_early_cuts(const char *env_text, unsigned *out, size_t cap) {
    const std::vector<unsigned> v = rgx::parse_early_cuts(env_text);
    for (size_t k = 0; k < v.size() && k < cap; ++k) out[k] = v[k];
    return v.size();
}
extern "C" size_t emu_front_early_parts(const rgx::Member *hm, uint32_t m_lo, uint32_t m_hi, uint64_t upos_lo, const size_t *end, size_t n_end,
                                        const unsigned *cuts, size_t n_cuts, uint32_t early_min, uint32_t align, uint32_t *members, uint32_t *waves,
                                        uint64_t *upos, size_t cap) {
    const std::vector<rgx::EarlyPart> v = rgx::plan_early_parts(hm, m_lo, m_hi, upos_lo, end, n_end, std::vector<unsigned>(cuts, cuts + n_cuts), early_min,
                                                                align);
    for (size_t k = 0; k < v.size() && k < cap; ++k) { members[k] = v[k].members; waves[k] = v[k].waves; upos[k] = v[k].upos; }
    return v.size();
}
extern "C" uint32_t emu_front_early_prefix_segments(uint64_t part_upos, uint64_t pos0, uint32_t seg_bytes, uint32_t n_seg, uint32_t s_done, int small_ok) {
    return rgx::early_prefix_segments(part_upos, pos0, seg_bytes, n_seg, s_done, small_ok != 0);
}

// call_path.h on its own: the path of an attempt of an extract call as five bits (1 device_resident, 2 own_scan, 4 true_sizes, 8 to_file_end, 16 strict_walk)
#include "../../regtools_amd/csrc/call_path.h"
static rgx::CallPath call_path_of(unsigned bits) {
    rgx::CallPath p;
    p.device_resident = bits & 1; p.own_scan = bits & 2; p.true_sizes = bits & 4; p.to_file_end = bits & 8; p.strict_walk = bits & 16;
    return p;
}
static unsigned call_path_bits(const rgx::CallPath &p) {
    return (p.device_resident ? 1u : 0u) | (p.own_scan ? 2u : 0u) | (p.true_sizes ? 4u : 0u) | (p.to_file_end ? 8u : 0u) | (p.strict_walk ? 16u : 0u);
}
extern "C" unsigned emu_call_first_path(int device_bytes, int shared_list) { return call_path_bits(rgx::first_path(device_bytes != 0, shared_list != 0)); }
// why: 1..7 in the order of enum Restart.  The function's value: 1 and *next, or 0 (the flag the reason sets is set already)
extern "C" int emu_call_next_path(unsigned cur, int why, unsigned *next) {
    rgx::CallPath n;
    const bool ok = rgx::next_path(call_path_of(cur), (rgx::Restart)(why - 1), n);
    *next = call_path_bits(n);
    return ok ? 1 : 0;
}
extern "C" const char *emu_call_restart_name(int why) { return rgx::restart_name((rgx::Restart)(why - 1)); }
