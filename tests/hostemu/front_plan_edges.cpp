// TEST INFRASTRUCTURE ONLY: front_plan.h over the edge inputs of tests/test_front_plan_host.py, as a program of its own for the sanitizers
// (make -C tests/hostemu front_plan_edges: g++ -fsanitize=address,undefined; run it as it is, no GPU, no Python).  Member lists are exactly as long
// as the calls say, on the heap, so that a read beside one is the sanitizer's to report; the checks here are only what keeps the calls honest.
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "../../regtools_amd/csrc/front_plan.h"

using namespace rgx;

static int g_bad = 0;
#define CHECK(x) do { if (!(x)) { fprintf(stderr, "front_plan_edges: %s:%d: %s\n", __FILE__, __LINE__, #x); ++g_bad; } } while (0)

static std::vector<Member> member_list(const std::vector<uint32_t> &clens, uint32_t isize = 0xff00) {
    std::vector<Member> ms;
    uint64_t cpos = 18, upos = 0;
    for (uint32_t clen : clens) { ms.push_back(Member{cpos, upos, clen, isize}); cpos += clen + 26; upos += isize; }
    return ms;
}

static std::vector<uint8_t> bgzf28(uint32_t isize, unsigned bsize = 27) {
    std::vector<uint8_t> m = {0x1f, 0x8b, 8, 4, 0, 0, 0, 0, 0, 0xff, 6, 0, 'B', 'C', 2, 0, (uint8_t)bsize, (uint8_t)(bsize >> 8), 3, 0, 0, 0, 0, 0};
    for (int k = 0; k < 4; ++k) m.push_back((uint8_t)(isize >> (8 * k)));
    return m;
}

int main() {
    const std::vector<std::vector<uint32_t>> lists = {{100}, {100, 50, 200}, {30, 30, 30, 30, 30, 30, 30}, {500, 1, 2, 700, 64, 64, 64, 1000, 3, 3, 900, 10}};
    for (const auto &clens : lists) {
        const std::vector<Member> ms = member_list(clens);
        const uint32_t n = (uint32_t)ms.size();
        const size_t end = (size_t)(ms.back().cpos + ms.back().clen + 8);
        for (uint32_t la : {kPieceLookahead, kGateLookahead})
            for (const Member &m : ms)
                for (int d = -1; d <= 1; ++d)
                    for (uint32_t lo = 0; lo <= n; ++lo)
                        for (uint32_t hi = lo; hi <= n; ++hi) {
                            const uint32_t k = first_member_reading_past(ms.data(), lo, hi, m.cpos + m.clen + la + d, la);
                            CHECK(k >= lo && k <= hi);
                        }
        // pieces: a single chunk, every member in the first, ends around every member's reach, a chunk that completes no member
        std::vector<std::vector<size_t>> ends = {{end}, {end + 8, end + 40, end + 80}};
        for (const Member &m : ms) {
            for (int d = -1; d <= 1; ++d) { ends.push_back({(size_t)(m.cpos + m.clen + 16 + d), end}); ends.push_back({19, (size_t)(m.cpos + m.clen + 16 + d), end}); }
            ends.push_back({(size_t)m.cpos, (size_t)m.cpos + 1, end});
        }
        for (const auto &e : ends)
            for (uint32_t m_lo : {0u, n > 1 ? 1u : 0u}) {
                const std::vector<Piece> pc = plan_pieces(ms.data(), m_lo, n, e.data(), e.size());
                CHECK(!pc.empty() && pc.front().g_lo == m_lo && pc.back().g_hi == n);
                for (size_t k = 0; k + 1 < pc.size(); ++k) CHECK(pc[k].g_hi == pc[k + 1].g_lo && pc[k].chunk < pc[k + 1].chunk);
            }
        // the gate's rule: clamped, floored, never behind the last chunk
        for (uint64_t gate_lo : {(uint64_t)0, (uint64_t)7, (uint64_t)end + 100})
            for (uint64_t cb : {(uint64_t)1, (uint64_t)64, (uint64_t)ms[0].cpos + ms[0].clen + 24, (uint64_t)4096})
                for (uint32_t nc : {1u, 2u, 16u, 64u})
                    for (const Member &m : ms) CHECK(gate_chunk_needed(m.cpos, m.clen, gate_lo, cb, nc) < nc);
        CHECK(upload_covers_members(ms.data(), 0, n, 0, end + 8));
        CHECK(!upload_covers_members(ms.data(), 0, n, 1, end + 8));
        // member queries: hits, misses, a stop in front of and behind the first answer
        for (uint32_t stop_at : {0xffffffffu, 0u, n - 1}) {
            std::vector<Member> q_ms = ms;
            if (stop_at < n) q_ms[stop_at].isize = 0;
            for (const Member &m : ms) {
                const uint64_t q[3] = {m.cpos - 18, m.cpos - 17, UINT64_MAX - 64};
                const MemberQuery r = host_member_query(q_ms.data(), n, q);
                CHECK(r.q_index[0] < n && r.q_index[1] == n && r.q_index[2] == n && r.q_upos[1] == ~0ull);
                CHECK(r.stop == 0xffffffffu || (r.stop >= r.q_index[0] && r.stop < n));
            }
        }
    }
    { const uint64_t q[3] = {0, 0, 0}; const MemberQuery r = host_member_query(nullptr, 0, q); CHECK(r.q_index[0] == 0 && r.stop == 0xffffffffu); }

    // early tail: forty members of 126 bytes, sixteen chunks; then three thousand at the product's alignment
    {
        const std::vector<Member> ms = member_list(std::vector<uint32_t>(40, 100));
        std::vector<size_t> ends;
        for (size_t j = 0; j < 16; ++j) ends.push_back(315 * (j + 1));
        const std::vector<std::vector<unsigned>> cut_lists = {{6, 9, 12, 14}, {6, 15}, {5, 6}, {2, 4, 6, 8, 10, 12, 14}, {1, 6}, {15}, {}};
        for (const auto &cuts : cut_lists)
            for (uint32_t early_min : {1u, 4u, 6u, 10u, 40u, 41u})
                for (uint32_t m_lo : {0u, 5u, 39u}) {
                    const std::vector<EarlyPart> parts = plan_early_parts(ms.data(), m_lo, 40, ms[m_lo].upos, ends.data(), ends.size(), cuts, early_min, 4);
                    CHECK(parts.size() <= cuts.size());
                    for (const EarlyPart &ep : parts) CHECK(ep.members % 4 == 0 && ep.waves == ep.members / 64 && m_lo + ep.members < 40);
                }
        std::vector<uint32_t> clens;
        uint32_t x = 12345;
        for (int k = 0; k < 3000; ++k) { x = x * 1664525u + 1013904223u; clens.push_back(2000 + (x >> 8) % 18000); }
        const std::vector<Member> big = member_list(clens);
        const size_t end = (size_t)(big.back().cpos + big.back().clen + 8);
        const UploadChunks uc = plan_upload_chunks(0, end, true, 16, false);
        CHECK(uc.end.size() == 16 && uc.end.back() == end);
        const std::vector<EarlyPart> parts = plan_early_parts(big.data(), 0, 3000, 0, uc.end.data(), uc.end.size(), parse_early_cuts(nullptr), 1, 1024);
        CHECK(parts.size() == 2 && parts[0].members == 1024 && parts[1].members == 2048 && parts[1].waves == 32);
        for (const Member &m : big) CHECK(gate_chunk_needed(m.cpos, m.clen, 0, uc.gate_chunk, 16) < 16);
    }

    for (const char *text : {(const char *)nullptr, "0", "9,6,12", "6,16,20,14", "1,2,3,4,5,6,7,8,9", "garbage", "", "6,x,9", "4294967295,15"})
        CHECK(parse_early_cuts(text).size() <= 7);
    CHECK(parse_early_cuts(nullptr) == (std::vector<unsigned>{6, 9, 12, 14}) && parse_early_cuts("0").empty());

    for (unsigned n : {2u, 7u, 16u, 64u})
        for (size_t len : {(size_t)4096 * n * 3, (size_t)4096 * n * 3 + 1234, (size_t)2 * 4096 * n, (size_t)533000001})
            for (size_t lo : {(size_t)0, (size_t)8192}) {
                const UploadChunks u = plan_upload_chunks(lo, lo + len, true, n, false);
                CHECK(u.end.back() == lo + len && u.end.size() <= n && u.gate_chunk % 4096 == 0);
                for (size_t k = 0; k + 1 < u.end.size(); ++k) CHECK(u.end[k] < u.end[k + 1]);
            }
    CHECK(plan_upload_chunks(0, 5000, false, 16, false).end == (std::vector<size_t>{4096, 5000}));
    CHECK(plan_upload_chunks(0, 4000, false, 16, false).end == (std::vector<size_t>{4000}));
    CHECK(plan_upload_chunks(4096, 4096, false, 16, false).end == (std::vector<size_t>{4096}));
    CHECK(plan_upload_chunks(0, (size_t)100 << 20, false, 16, true).end.size() == 1);

    for (int n : {2, 3})
        for (int shard = 0; shard < n; ++shard)
            for (size_t bam_len : {(size_t)28, (size_t)533000001, ((size_t)1 << 40) + 3}) {
                uint64_t tgt[2];
                shard_cut_targets(bam_len, shard, n, 1, tgt);
                CHECK(tgt[0] <= tgt[1] && tgt[0] >= 1);
                const uint64_t gots[][2] = {{tgt[0], tgt[1]}, {UINT64_MAX, UINT64_MAX}, {tgt[1], tgt[0]}, {(uint64_t)90100 << 16, UINT64_MAX}, {0, 0}};
                for (const auto &got : gots) {
                    const UploadRange r = shard_upload_range(bam_len, shard, n, got, 3000, 90000);
                    CHECK(r.lo <= r.hi && r.hi <= bam_len && r.lo % 4096 == 0 && (r.lo ? r.hdr_hi <= r.lo : r.hdr_hi == 0));
                }
            }

    {
        uint32_t m_lo = 0, m_hi = 0;
        const uint32_t qi[3] = {9, 9, 98};
        member_range((uint64_t)9 << 16, ((uint64_t)700 << 16) | 1, qi, 99, 100, true, false, m_lo, m_hi);
        CHECK(m_lo == 9 && m_hi == 100);
        const uint32_t q2[3] = {0, 80, 50};
        member_range((uint64_t)80 << 16, (uint64_t)700 << 16, q2, 99, 100, false, false, m_lo, m_hi);
        CHECK(m_lo == 50 && m_hi == 50);
        const uint32_t q3[3] = {0, 4, 0xffffffffu};
        member_range(1, UINT64_MAX - 1, q3, 0xffffffffu, 0xffffffffu, true, false, m_lo, m_hi);        // (hi_m + 2 is made in 64 bits)
        CHECK(m_lo == 0 && m_hi == 0xffffffffu);
    }

    const uint64_t pos0 = 1000;
    CHECK(early_prefix_segments(pos0 + 2 * 65536, pos0, 16384, 100, 0, true) == 0 && early_prefix_segments(pos0 + 2 * 65536 + 1, pos0, 16384, 100, 0, true) == 4);
    CHECK(early_prefix_segments(pos0 + 65536 + 1024 * 16384, pos0, 16384, 2000, 0, false) == 1024);
    CHECK(early_prefix_segments(pos0 + 65536 + 1024 * 16384 - 1, pos0, 16384, 2000, 0, false) == 0);
    CHECK(early_prefix_segments(UINT64_MAX, pos0, 16384, 100, 4, true) == 0 && early_prefix_segments(0, pos0, 16384, 100, 4, true) == 0);

    {
        std::vector<uint8_t> a = bgzf28(896), b = bgzf28(895), c = bgzf28(5000, 28), d = bgzf28(5000);
        CHECK(!payload_takes_gate(a.data(), a.size()) && payload_takes_gate(b.data(), b.size()) && payload_takes_gate(c.data(), c.size()));
        CHECK(payload_takes_gate(d.data(), 27));                     // fewer than 28 bytes: nothing is read
        std::vector<uint8_t> two = d, second = bgzf28(0, 40);
        two.insert(two.end(), second.begin(), second.end());
        CHECK(!payload_takes_gate(two.data(), two.size()));          // the second BSIZE runs past the end: its footer is not read
        std::vector<uint8_t> many;
        for (int k = 0; k < 70; ++k) many.insert(many.end(), b.begin(), b.end());
        CHECK(payload_takes_gate(many.data(), many.size()));
    }
    CHECK(region_kind(nullptr) == RegionKind::whole && region_kind(".") == RegionKind::whole && region_kind("*") == RegionKind::rest &&
          region_kind("") == RegionKind::query && region_kind("chr1:5-9") == RegionKind::query);

    printf("front_plan_edges: %s\n", g_bad ? "FAILED" : "ok");
    return g_bad ? 1 : 0;
}
