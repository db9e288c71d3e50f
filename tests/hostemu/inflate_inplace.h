// tests/hostemu/inflate_inplace.h -- TEST INFRASTRUCTURE ONLY.
// The DEFLATE decoders of regtools_amd/csrc (inflate_core.h, inflate_ring.h, inflate_coop.h, inflate_wave.h) run IN PLACE on the caller's bytes with
// the host's one-lane "wave": nothing is copied, so what a decoder touches around its payload and its member is what the caller's buffers must hold.
//
// The read / write contract, as tested (tests/test_deflate_conformance_host.py under a PROT_NONE page, tests/hostemu/inflate_edges.cpp under the host
// sanitizers on exact-size heap buffers):
//   payload   every decoder reads at most kBackBytes = 16 bytes behind the payload's last byte, whatever the stream says (the bit readers' look-ahead
//             and the 16-byte loads of a stored block's source).  Nothing in front of it -- except the ring decoder, whose stored-block copy loads its
//             source from up to 15 bytes in front of the block's first raw byte (the destination's phase in a 16-byte chunk); that byte lies at least
//             5 bytes into the payload (3 header bits, LEN, NLEN), so the ring decoder needs kRingFrontBytes = 10 readable bytes in front of the payload.
//             In a BGZF file the member's 18 header bytes stand there.
//   member    writes stay inside the member's [0, cap).  READS of the output may leave it: resync and flush read the aligned 16-byte blocks that the
//             member's two ends cut; the copy loads of the lane and coop decoders take 16 bytes at a time from a match's source and so reach up to
//             kOutBackBytes = 12 bytes behind the member (a 3-byte match at distance 1 that ends it: 16 bytes from cap - 4); the ring decoder's far copies start up to
//             kOutFrontBytes = 15 bytes in front of their source, for a source at the member's start in front of the member (kArenaFrontPad).  The wave
//             decoder reads nothing of the output.
#pragma once
#include "../../regtools_amd/csrc/inflate_core.h"
#include "../../regtools_amd/csrc/inflate_ring.h"
#include "../../regtools_amd/csrc/inflate_coop.h"
#include "../../regtools_amd/csrc/inflate_wave.h"
#include <string.h>

namespace rgx_emu {

constexpr uint32_t kBackBytes = 16, kRingFrontBytes = 10, kOutFrontBytes = 15, kOutBackBytes = 12;

// variants: 0 lane, 1 lane with four literals per trip, 2 ring, 3 wave, 16 + pairs = coop (pairs as emu_inflate_coop: bit 0 a literal and the symbol
// behind it per trip, bit 1 the windowed bit reader, bit 2 two literals and a match per trip, bit 3 runs written from registers)
constexpr int kLane = 0, kLane4 = 1, kRing = 2, kWave = 3, kCoop = 16;

inline uint32_t front_bytes(int variant) { return variant == kRing ? kRingFrontBytes : 0u; }

inline int run(int variant, const uint8_t *in, uint32_t in_len, uint8_t *out, uint32_t cap, uint32_t *out_len) {
    rgx::HostTab T;
    memset(&T, 0xEE, sizeof T);                         // stale tables: a lookup that no block's header filled must not pass for a symbol
    if (variant == kLane) return rgx::inflate_raw(in, in_len, out, cap, out_len, T);
    if (variant == kLane4) return rgx::inflate_raw<4>(in, in_len, out, cap, out_len, T);
    if (variant == kRing) {
        rgx::HostRing R; rgx::HostCoop C;
        memset(&R, 0xCC, sizeof R);
        return rgx::inflate_ring(in, in_len, out, cap, out_len, T, R, C, true);
    }
    if (variant == kWave) {
        static rgx::WaveShared S;
        memset(&S, 0xCC, sizeof S);
        rgx::HostWave W;
        return rgx::inflate_wave(W, S, in, in_len, out, cap, out_len);
    }
    const int pairs = variant - kCoop;
    const uint32_t mode = (uint32_t)(pairs & 1) | ((pairs & 4) ? 2u : 0u) | ((pairs & 8) ? 4u : 0u);
    rgx::HostCopy C;
    return (pairs & 2) ? rgx::inflate_coop<rgx::BitReaderWin>(in, in_len, out, cap, out_len, T, C, true, mode)
                       : rgx::inflate_coop<rgx::BitReader>(in, in_len, out, cap, out_len, T, C, true, mode);
}

}  // namespace rgx_emu
