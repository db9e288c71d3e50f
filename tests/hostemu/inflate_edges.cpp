// tests/hostemu/inflate_edges.cpp -- TEST INFRASTRUCTURE ONLY.  A program of its own (make inflate_edges; not part of the default build, not run from
// pytest): the DEFLATE decoders of regtools_amd/csrc in place (inflate_inplace.h) under the host sanitizers, on heap buffers that are exactly as large as
// the decoders' read / write contract says -- a byte more read or written is the sanitizer's report.
//
//     python tests/deflate_craft.py --dump catalogue.bin && tests/hostemu/inflate_edges catalogue.bin
//
// Every catalogue entry (and every third cut of every legal one) goes through every variant at sixteen destination phases:
//   input    front_bytes(variant) + payload + kBackBytes, the payload's first byte that far behind the allocation's start
//   output   the member at phase a of a 16-byte block, the block's a bytes in front of it (the ring decoder: kOutFrontBytes, or a + 16 where that is
//            less than the phase needs), and behind it the rest of its last aligned block (the lane and coop decoders: kOutBackBytes if that is more);
//            preset to 0xA5, and every byte outside [0, cap) must still be 0xA5 afterwards.
// Exit status 0 and one line when every legal entry came out byte for byte and every malformed one was refused with a code of its set.
#include "inflate_inplace.h"
#include <stdio.h>
#include <stdlib.h>
#include <string>
#include <vector>

struct Entry { std::string name; uint32_t mask, cap; std::vector<uint8_t> payload, expect; };

static bool read_u32(FILE *f, uint32_t &v) { return fread(&v, 4, 1, f) == 1; }

static std::vector<Entry> load(const char *path) {
    std::vector<Entry> v;
    FILE *f = fopen(path, "rb");
    char magic[4];
    uint32_t n = 0;
    if (!f || fread(magic, 1, 4, f) != 4 || memcmp(magic, "DFLC", 4) != 0 || !read_u32(f, n)) { fprintf(stderr, "inflate_edges: %s is no catalogue\n", path); exit(2); }
    for (uint32_t k = 0; k < n; ++k) {
        Entry e;
        uint16_t nl = 0;
        uint32_t pl = 0, el = 0;
        bool ok = fread(&nl, 2, 1, f) == 1;
        e.name.resize(nl);
        ok = ok && fread(&e.name[0], 1, nl, f) == nl && read_u32(f, e.mask) && read_u32(f, e.cap) && read_u32(f, pl);
        e.payload.resize(pl);
        ok = ok && fread(e.payload.data(), 1, pl, f) == pl && read_u32(f, el);
        e.expect.resize(el);
        ok = ok && fread(e.expect.data(), 1, el, f) == el;
        if (!ok) { fprintf(stderr, "inflate_edges: %s ends inside entry %u\n", path, k); exit(2); }
        v.push_back(e);
    }
    fclose(f);
    return v;
}

static const int kVariants[] = {rgx_emu::kLane, rgx_emu::kLane4, rgx_emu::kRing, rgx_emu::kWave, rgx_emu::kCoop + 0, rgx_emu::kCoop + 1, rgx_emu::kCoop + 2,
                                rgx_emu::kCoop + 3, rgx_emu::kCoop + 5, rgx_emu::kCoop + 7, rgx_emu::kCoop + 8, rgx_emu::kCoop + 10, rgx_emu::kCoop + 13,
                                rgx_emu::kCoop + 15};

static unsigned long g_runs = 0;

// one decoder over one payload (its first `len` bytes) on exact buffers; returns the status, or -100 - k for a broken promise
static int run_exact(int variant, const uint8_t *payload, uint32_t len, uint32_t cap, uint32_t a, uint8_t tail, std::vector<uint8_t> &got) {
    const uint32_t front = rgx_emu::front_bytes(variant);
    uint8_t *ibuf = (uint8_t *)malloc((size_t)front + len + rgx_emu::kBackBytes);
    memset(ibuf, tail, (size_t)front + len + rgx_emu::kBackBytes);
    memcpy(ibuf + front, payload, len);
    const bool ring = variant == rgx_emu::kRing, wave = variant == rgx_emu::kWave;
    uint32_t F = a, B = (16u - ((a + cap) & 15u)) & 15u;
    if (ring) { if (F < rgx_emu::kOutFrontBytes) F += 16; }
    else if (!wave && B < rgx_emu::kOutBackBytes) B = rgx_emu::kOutBackBytes;
    if (wave) B = 0;
    const size_t total = (size_t)F + cap + B;
    uint8_t *obuf = (uint8_t *)malloc(total ? total : 1);       // 16-byte aligned: the member starts at phase F % 16 == a
    memset(obuf, 0xA5, total);
    uint32_t out_len = 0;
    int st = rgx_emu::run(variant, ibuf + front, len, obuf + F, cap, &out_len);
    ++g_runs;
    for (size_t i = 0; i < F; ++i) if (obuf[i] != 0xA5) st = -100;
    for (size_t i = (size_t)F + cap; i < total; ++i) if (obuf[i] != 0xA5) st = -101;
    if (out_len > cap) st = -102;
    got.assign(obuf + F, obuf + F + (out_len <= cap ? out_len : cap));
    free(obuf);
    free(ibuf);
    return st;
}

int main(int argc, char **argv) {
    if (argc != 2) { fprintf(stderr, "usage: inflate_edges CATALOGUE (python tests/deflate_craft.py --dump CATALOGUE)\n"); return 2; }
    const std::vector<Entry> cat = load(argv[1]);
    unsigned legal = 0, bad = 0, cuts = 0, failures = 0;
    std::vector<uint8_t> got;
    for (const Entry &e : cat) {
        const bool is_legal = (e.mask & 1u) != 0;
        (is_legal ? legal : bad)++;
        const uint32_t phases = e.cap < 4096 ? 16 : 3;
        for (int variant : kVariants) {
            for (uint32_t k = 0; k < phases; ++k) {
                const uint32_t a = phases == 16 ? k : (k * 7 + 1 + (uint32_t)e.name.size()) & 15u;
                const int st = run_exact(variant, e.payload.data(), (uint32_t)e.payload.size(), e.cap, a, 0, got);
                const bool ok = is_legal ? (st == 0 && got == e.expect) : (st >= 1 && st < 32 && ((e.mask >> st) & 1u));
                if (!ok) { ++failures; fprintf(stderr, "inflate_edges: %s variant %d phase %u: status %d, %zu bytes\n", e.name.c_str(), variant, a, st, got.size()); }
            }
            // cuts of a legal stream, foreign bytes behind them: refused, whatever the code
            if (is_legal && e.payload.size() < 1200 && e.name.find("trailing") == std::string::npos)
                for (uint32_t cut = 0; cut < e.payload.size(); cut += 3) {
                    const int st = run_exact(variant, e.payload.data(), cut, e.cap, (cut * 5) & 15u, (uint8_t)(cut * 37 + 11), got);
                    if (variant == kVariants[0]) ++cuts;
                    if (st < 1 || st > 11) { ++failures; fprintf(stderr, "inflate_edges: %s cut at %u variant %d: status %d\n", e.name.c_str(), cut, variant, st); }
                }
        }
    }
    if (failures) { fprintf(stderr, "inflate_edges: %u failures\n", failures); return 1; }
    printf("inflate_edges: %u legal and %u malformed entries, %u cuts, %zu variants, %lu decoder runs on exact-size buffers: all as the catalogue says\n",
           legal, bad, cuts, sizeof kVariants / sizeof kVariants[0], g_runs);
    return 0;
}
