// cse_table.h -- the first-insert junction table of `identify` / `associate` and the ranking of names it is keyed by.  Plain C++ and worker_pool.h, nothing
// from HIP: the CPU tests drive it on its own (tests/hostemu emu_jtable).
#pragma once
#include <stdint.h>

#include <algorithm>
#include <string>
#include <thread>
#include <unordered_map>
#include <utility>
#include <vector>

#include "worker_pool.h"

// unique_junctions_ / junction_to_variant_ (identifier.cc:292-299, associator.cc:266-270): first-inserted row wins per (chrom, start, end)
// Upstream: std::map<Junction-by-(chrom string, start, end), ...> filled with insert (the first row of a key stays) and, per junction, a
// std::set of variants ordered by (chrom string, start, end).  Here: the candidate rows as flat records keyed by the RANK of the contig name
// in string order, sorted once -- (key, arrival order) for the rows, (key, variant) for the links -- which visits keys, first rows and
// variants in exactly the order those containers iterate.  (The containers themselves, keyed on strings, were 25 of identify's 280 ms.)
struct JEntry { uint32_t ts, te, count; std::string strand, color; int nblocks; };
struct JTable {
    struct Cand { uint32_t crank, js, jend, order; uint32_t vrank, vpos, src; };     // src: where the caller finds the row's fields
    std::vector<std::string> chrom_name, vchrom_name;        // by rank
    std::vector<Cand> cand;                                  // every (row, variant) link in arrival order
    // after finish(): one entry per junction in map order, its variants in set order
    struct Row { uint32_t crank, js, jend; JEntry e; uint32_t v0, v1; };
    std::vector<Row> rows;
    std::vector<std::pair<uint32_t, uint32_t>> vars;         // (variant contig rank, pos0)
    void add(uint32_t crank, uint32_t js, uint32_t jend, uint32_t vrank, uint32_t vpos, uint32_t src) { cand.push_back(Cand{crank, js, jend,
        (uint32_t)cand.size(), vrank, vpos, src}); }
    // pool: the threads the sort runs on (nullptr = threads of its own, where there are candidates enough to be worth them)
    template <class F> void finish(F entry_of /* src -> JEntry, asked once per junction */, rgx::WorkerPool *pool) {
        std::vector<uint32_t> idx(cand.size());
        for (uint32_t i = 0; i < idx.size(); ++i) idx[i] = i;
        rgx::WorkerPool own(pool || cand.size() < (1u << 14) ? 1 : std::min(16u, std::max(2u, std::thread::hardware_concurrency())));
        rgx::parallel_sort(pool ? *pool : own, idx.begin(), idx.end(), [&](uint32_t a, uint32_t b) {
            const Cand &x = cand[a], &y = cand[b];
            if (x.crank != y.crank) return x.crank < y.crank;
            if (x.js != y.js) return x.js < y.js;
            if (x.jend != y.jend) return x.jend < y.jend;
            return x.order < y.order;
        });
        rows.clear(); vars.clear();
        for (size_t i = 0; i < idx.size();) {
            const Cand &f = cand[idx[i]];                       // the first arrival of this key: its fields stay (map::insert)
            size_t j = i;
            const uint32_t v0 = (uint32_t)vars.size();
            while (j < idx.size() && cand[idx[j]].crank == f.crank && cand[idx[j]].js == f.js &&
                cand[idx[j]].jend == f.jend) { vars.push_back({cand[idx[j]].vrank, cand[idx[j]].vpos}); ++j; }
            std::sort(vars.begin() + v0, vars.end());
            vars.erase(std::unique(vars.begin() + v0, vars.end()), vars.end());
            rows.push_back(Row{f.crank, f.js, f.jend, entry_of(f.src), v0, (uint32_t)vars.size()});
            i = j;
        }
    }
    size_t size() const { return rows.size(); }
};

// ranks of names in string order (equal names share a rank)
inline void string_ranks(const std::vector<std::string> &names, std::vector<uint32_t> &rank_of, std::vector<std::string> &name_of_rank) {
    std::vector<uint32_t> order(names.size());
    for (uint32_t i = 0; i < order.size(); ++i) order[i] = i;
    std::sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) { return names[a] < names[b]; });
    rank_of.assign(names.size(), 0); name_of_rank.clear();
    for (size_t k = 0; k < order.size(); ++k) {
        if (k == 0 || names[order[k]] != names[order[k - 1]]) name_of_rank.push_back(names[order[k]]);
        rank_of[order[k]] = (uint32_t)name_of_rank.size() - 1;
    }
}

// the same for a sequence that repeats few names many times (the variants' contigs): rank_of[w] for name_at(w), w in [0, n)
// (records of a VCF come contig by contig: one table lookup per run of equal names)
template <class NameAt> void run_string_ranks(size_t n, NameAt name_at, std::vector<uint32_t> &rank_of, std::vector<std::string> &name_of_rank) {
    std::vector<std::string> names; std::unordered_map<std::string, uint32_t> idx; std::vector<uint32_t> name_of(n), rank_of_name;
    const std::string *last = nullptr; uint32_t last_idx = 0;
    for (size_t w = 0; w < n; ++w) {
        const std::string &cn = name_at(w);
        if (!last || *last != cn) { auto it = idx.find(cn); if (it == idx.end()) { it = idx.emplace(cn, (uint32_t)names.size()).first; names.push_back(cn); }
            last = &cn; last_idx = it->second; }
        name_of[w] = last_idx;
    }
    string_ranks(names, rank_of_name, name_of_rank);
    rank_of.resize(n);
    for (size_t w = 0; w < n; ++w) rank_of[w] = rank_of_name[name_of[w]];
}
