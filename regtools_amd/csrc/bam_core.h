// bam_core.h -- per-record / per-read device cores of the junctions-extract hot path (host-compilable for
// the CPU unit tests).  file:line citations are relative to /root/reference.
#pragma once
#include "common.h"

namespace rgx {

// ---- BAM record framing (src/utils/htslib/sam.c:399-433 bam_read1) ------------------------------------
struct RecHead {
    int32_t  block_len;   // bytes after the length word
    int32_t  tid, pos;
    uint32_t l_qname, n_cigar, flag;
    int32_t  l_qseq;
    int32_t  mtid;
    int64_t  aux_off;     // offset of the aux area from the start of the variable data
};

// The fixed part from its eight little-endian words (the eighth, next_pos, is not kept).
RGX_HD void rec_head_words(const uint32_t x[8], RecHead &h) {
    h.block_len = (int32_t)x[0]; h.tid = (int32_t)x[1]; h.pos = (int32_t)x[2];
    h.l_qname = x[3] & 0xff; h.n_cigar = x[4] & 0xffff; h.flag = x[4] >> 16;
    h.l_qseq = (int32_t)x[5]; h.mtid = (int32_t)x[6];
    h.aux_off = (int64_t)h.l_qname + 4 * (int64_t)h.n_cigar + (((int64_t)h.l_qseq + 1) >> 1) + h.l_qseq;
}
// Reads the fixed part at arena offset o (caller guarantees o+36 <= lim).
RGX_HD void rec_head(const uint8_t *a, RecHead &h) {
    uint32_t x[8];
    for (int q = 0; q < 8; ++q) x[q] = ld32(a + 4 * q);
    rec_head_words(x, h);
}

// bam_read1's own acceptance test (sam.c:421-423): anything else ends iteration silently.
RGX_HD bool rec_sane(const RecHead &h) {
    int64_t l_data = (int64_t)h.block_len - 32;
    if (l_data < 0 || h.l_qseq < 0 || h.l_qname < 1) return false;
    return h.aux_off <= l_data;
}

// Speculation filter used ONLY to guess where a segment's first record starts; every guess is verified
// against the exact chain afterwards, so this predicate affects speed, never results.
RGX_HD bool rec_plausible(const uint8_t *arena, uint64_t o, uint64_t lim, int32_t n_ref) {
    if (o + 36 > lim) return false;
    RecHead h; rec_head(arena + o, h);
    if (!rec_sane(h)) return false;
    if (h.block_len > (1 << 27)) return false;
    if (h.tid < -1 || h.tid >= n_ref || h.mtid < -1 || h.mtid >= n_ref) return false;
    if (h.pos < -1 || h.pos > (1 << 29)) return false;       // a .bai cannot index beyond 2^29 (hts.c:1517)
    uint64_t q_end = o + 36 + h.l_qname - 1;
    if (q_end < lim && arena[q_end] != 0) return false;     // qname is NUL-terminated
    return true;
}

// ---- strand rules -----------------------------------------------------------------------------------------
// src/junctions/junctions_extractor.cc:297-322 set_junction_strand_flag (strandness 1 = RF, 2 = FR; 3 acts as b=2)
RGX_HD char strand_from_flag(uint32_t flag, int strandness) {
    int rev = (flag >> 4) & 1, mrev = (flag >> 5) & 1, r1 = (flag >> 6) & 1, r2 = (flag >> 7) & 1;
    int nb = (strandness - 1) == 0 ? 1 : 0;        // !bool_strandness
    int f = nb ^ r1 ^ rev, s = nb ^ r2 ^ mrev;
    return f != s ? '?' : (f ? '+' : '-');
}

// junctions_extractor.cc:283-294 + sam.c:1254-1266 bam_aux_get / :1233-1252 skip_aux / :1301-1307 bam_aux2A.
// First tag equal to `tag`: type 'A' with a non-NUL value gives that char, anything else '?'.
// *unknown (optional) is set when a tag of a type skip_aux does not know stands in front of the one looked for: upstream abort()s there (sam.c:1248).
RGX_HD char strand_from_tag(const uint8_t *aux, const uint8_t *end, uint8_t t0, uint8_t t1, bool *unknown = nullptr) {
    const uint8_t *s = aux;
    while (s + 3 <= end) {
        bool hit = s[0] == t0 && s[1] == t1;
        s += 2;
        if (hit) return (s[0] == 'A' && s + 2 <= end && s[1] != 0) ? (char)s[1] : '?';
        uint8_t t = *s++;
        uint32_t sz;
        switch (t) {
            case 'A': case 'c': case 'C': sz = 1; break;
            case 's': case 'S': sz = 2; break;
            case 'i': case 'I': case 'f': sz = 4; break;
            case 'd': sz = 8; break;
            case 'Z': case 'H': { while (s < end && *s) ++s; sz = 1; break; }
            case 'B': {
                if (s + 5 > end) return '?';
                uint8_t st = *s++; uint32_t n = (uint32_t)s[0] | (uint32_t)s[1] << 8 | (uint32_t)s[2] << 16 | (uint32_t)s[3] << 24; s += 4;   // bytes: s may point into LDS
                uint32_t es = (st == 'c' || st == 'C' || st == 'A') ? 1 : (st == 's' || st == 'S') ? 2 : (st == 'i' || st == 'I' || st == 'f') ? 4 : (st == 'd') ? 8 : 0;
                if ((uint64_t)es * n > (uint64_t)(end - s)) return '?';
                sz = es * n; break;
            }
            default: if (unknown) *unknown = true; return '?';   // upstream abort()s on an unknown type (the caller is told; the strand reads "not found")
        }
        s += sz;
    }
    return '?';
}

// junctions_extractor.cc:362-374 set_junction_barcode: bam_aux_get(tag) (sam.c:1254-1266) + bam_aux2Z (sam.c:1309-1315).
// 1 = found, the value is aux[*val, *val + *len) (its NUL excluded); 0 = no such tag (the barcode is then "?"); -1 = the tag is there
// but is not a Z/H string (upstream builds a std::string from NULL there and dies).
RGX_HD int aux_find_string(const uint8_t *aux, const uint8_t *end, uint8_t t0, uint8_t t1, uint32_t *val, uint32_t *len) {
    const uint8_t *s = aux;
    while (s + 3 <= end) {
        const bool hit = s[0] == t0 && s[1] == t1;
        s += 2;
        const uint8_t t = *s++;
        if (hit) {
            if (t != 'Z' && t != 'H') return -1;
            const uint8_t *e = s;
            while (e < end && *e) ++e;
            *val = (uint32_t)(s - aux); *len = (uint32_t)(e - s);
            return 1;
        }
        uint32_t sz;
        switch (t) {
            case 'A': case 'c': case 'C': sz = 1; break;
            case 's': case 'S': sz = 2; break;
            case 'i': case 'I': case 'f': sz = 4; break;
            case 'd': sz = 8; break;
            case 'Z': case 'H': { while (s < end && *s) ++s; sz = 1; break; }
            case 'B': {
                if (s + 5 > end) return 0;
                uint8_t st = *s++; uint32_t n = (uint32_t)s[0] | (uint32_t)s[1] << 8 | (uint32_t)s[2] << 16 | (uint32_t)s[3] << 24; s += 4;
                uint32_t es = (st == 'c' || st == 'C' || st == 'A') ? 1 : (st == 's' || st == 'S') ? 2 : (st == 'i' || st == 'I' || st == 'f') ? 4 : (st == 'd') ? 8 : 0;
                if ((uint64_t)es * n > (uint64_t)(end - s)) return 0;
                sz = es * n; break;
            }
            default: return 0;
        }
        s += sz;
    }
    return 0;
}
// grouping key of a barcode string: 64 bits, two independently seeded 32-bit lanes; equal strings are CHECKED byte for byte afterwards
// (k_bc_heads), the hash only brings them together
RGX_HD void barcode_hash(const uint8_t *s, uint32_t len, uint32_t *lo, uint32_t *hi) {
    uint32_t a = 0x811c9dc5u ^ len, b = 0x9747b28cu + len * 0x85ebca6bu;
    for (uint32_t i = 0; i < len; ++i) {
        a = (a ^ s[i]) * 0x01000193u;
        b = (b + s[i]) * 0xcc9e2d51u; b = (b << 15 | b >> 17) * 0x1b873593u;
    }
    a ^= a >> 16; a *= 0x7feb352du; a ^= a >> 15;
    b ^= b >> 13; b *= 0xc2b2ae35u; b ^= b >> 16;
    *lo = a; *hi = b;
}

// ---- intron-motif strand rule (junctions_extractor.cc:325-342, :564-584; faidx.c:341-413) --------------------------------
// FASTA file bytes live in HBM; one descriptor per BAM contig (matched by name on the host).
struct FaContig { int64_t offset, len; int32_t line_blen, line_len; int32_t present; int32_t pad; };

// fai_fetch("chr:beg1-end1") for a two-base window: returns the number of bases (0..2) and the bases in b[0..1]
RGX_HD int fa_fetch2(const uint8_t *fa, const FaContig &c, uint32_t beg1, uint32_t end1, uint8_t *b) {
    int64_t beg = beg1, end = end1;
    if (beg > 0) --beg;
    if (beg >= c.len) beg = c.len;
    if (end >= c.len) end = c.len;
    if (beg > end) beg = end;
    int n = 0;
    if (c.line_blen <= 0) return 0;
    for (int64_t p = beg; p < end && n < 2; ++p) b[n++] = fa[c.offset + p / c.line_blen * c.line_len + p % c.line_blen];
    return n;
}
RGX_HD uint8_t base_comp(uint8_t c) { return c == 'A' ? 'T' : c == 'C' ? 'G' : c == 'G' ? 'C' : c == 'T' ? 'A' : 'N'; }   // utils/common.h:59-83

// strand of the junction [start,end) from its splice-site motif; `carried` is the strand of the previous junction of the same
// read (upstream reuses the Junction object, cc:576-579).  '?' when the motif is not canonical.
RGX_HD char strand_from_motif(const uint8_t *fa, const FaContig &c, uint32_t start, uint32_t end, char carried) {
    uint8_t s1[2], s2[2];
    const int l1 = fa_fetch2(fa, c, start + 1u, start + 2u, s1);
    const int l2 = fa_fetch2(fa, c, end + 1u - 2u, end + 1u - 1u, s2);
    if (l1 != 2 || l2 != 2) return '?';
    uint8_t d0, d1, a0, a1;                       // motif = d0 d1 '-' a0 a1
    if (carried == '-') { d0 = base_comp(s2[1]); d1 = base_comp(s2[0]); a0 = base_comp(s1[1]); a1 = base_comp(s1[0]); }
    else { d0 = s1[0]; d1 = s1[1]; a0 = s2[0]; a1 = s2[1]; }
    const uint32_t m = (uint32_t)d0 << 24 | (uint32_t)d1 << 16 | (uint32_t)a0 << 8 | a1;
    if (m == 0x47544147u /*GT-AG*/ || m == 0x47434147u /*GC-AG*/ || m == 0x41544143u /*AT-AC*/) return '+';
    if (m == 0x43544143u /*CT-AC*/ || m == 0x43544743u /*CT-GC*/ || m == 0x47544154u /*GT-AT*/) return '-';
    return '?';
}

// key class of a strand char (junctions_extractor.cc:186-193)
RGX_HD uint32_t strand_class(char c) { return c == '+' ? 0u : c == '-' ? 1u : 2u; }

// ---- CIGAR (htslib/sam.h:75-104) ----------------------------------------------------------------------------
// op classes: N; M,= extend an anchor; D,X break it and advance the reference; I,S break it; H,P,B,10-15 are inert.
RGX_HD uint32_t cig_ref_len(uint32_t c) {          // bam_cigar_type bit 1 (0x3C1A7)
    uint32_t op = c & 0xf;
    return ((0x3C1A7u >> (op << 1)) & 2u) ? (c >> 4) : 0u;
}
RGX_HD bool cig_is_N(uint32_t c) { return (c & 0xf) == 3; }
RGX_HD bool cig_is_breaker(uint32_t c) { uint32_t op = c & 0xf; return op == 3 || op == 2 || op == 8 || op == 1 || op == 4; }
RGX_HD bool cig_advances_junction_state(uint32_t c) {   // ref-advancing for the junction machine: M,=,D,X,N
    uint32_t op = c & 0xf; return op == 0 || op == 7 || op == 2 || op == 8 || op == 3;
}

// bam_endpos (sam.c:336-342); cigar_at(q) = the record's q-th CIGAR word, wherever it lies
template <class CigarAt>
RGX_HD int32_t rec_endpos_at(CigarAt &&cigar_at, uint32_t n_cigar, uint32_t flag, int32_t pos) {
    if (!(flag & 4) && n_cigar > 0) {
        int32_t l = 0;
        for (uint32_t k = 0; k < n_cigar; ++k) l += (int32_t)cig_ref_len(cigar_at(k));
        return pos + l;
    }
    return pos + 1;
}
RGX_HD int32_t rec_endpos(const uint8_t *cig, uint32_t n_cigar, uint32_t flag, int32_t pos) {
    return rec_endpos_at([&](uint32_t k) { return ld32(cig + 4 * (size_t)k); }, n_cigar, flag, pos);
}

// The serial state machine of junctions_extractor.cc:377-497.  `emit(start,end,ts,te)` is
// called once per N op, in order.  Used by the lane-per-read kernel and by the unit tests; the
// wave-per-read kernel computes the same four numbers with prefix sums (see k_emit_long in emit_kernels.hip).
template <class Emit>
RGX_HD void cigar_walk(int32_t pos, const uint8_t *cig, uint32_t n_cigar, Emit &&emit) {
    uint32_t start = (uint32_t)pos, ts = (uint32_t)pos, end = 0, te = 0;
    bool started = false;
    for (uint32_t i = 0; i < n_cigar; ++i) {
        uint32_t c = ld32(cig + 4 * (size_t)i), op = c & 0xf, len = c >> 4;
        if (op == 3) {
            if (!started) { end = start + len; te = end; started = true; }
            else { emit(start, end, ts, te); ts = end; start = te; end = start + len; te = end; }
        } else if (op == 0 || op == 7) {
            if (!started) start += len; else te += len;
        } else if (op == 2 || op == 8) {
            if (!started) { start += len; ts = start; }
            else { emit(start, end, ts, te); start = te + len; ts = start; }
            started = false;
        } else if (op == 1 || op == 4) {
            if (!started) ts = start;
            else { emit(start, end, ts, te); start = te; ts = start; }
            started = false;
        }
    }
    if (started) emit(start, end, ts, te);
}

// junction_qc (junctions_extractor.cc:160-170), the intron-length half: unsigned compare
RGX_HD bool intron_ok(uint32_t start, uint32_t end, uint32_t min_intron, uint32_t max_intron) {
    uint32_t l = end - start;
    return !(l < min_intron || l > max_intron);
}

// ---- the decode rule: one BAM record -> one row of the read table --------------------------------------------------------
struct ExtractCfg {
    int32_t  n_ref;
    int32_t  strandness;           // 0 tag, 1 RF, 2 FR, 3 intron-motif
    uint8_t  tag0, tag1;
    uint32_t min_anchor, min_intron, max_intron;
    int32_t  region_tid;           // -2 = whole file
    int32_t  region_beg, region_end;
    uint32_t long_threshold;       // reads with more CIGAR ops than this go to the wave-per-read kernel
    // intron-motif strand rule (a FASTA was given): file bytes + one descriptor per BAM contig, both in HBM
    const uint8_t *fa_data;
    const FaContig *fa_tab;
    uint32_t *fa_missing;          // [0] set to 1+tid when a junction lies on a contig the FASTA does not have
    // the iterator's end rule (hts_itr_next, hts.c:1946-1950: the first record read whose tid is not the region's or whose pos is not below
    // its end finishes the iteration, whatever follows).  stop_out (null = off): [0] = smallest index of such a record (preset ~0),
    // [1] = 1 + largest index of a record that passed the overlap test (preset 0); records at or behind stop_index are not iterated.
    uint32_t *stop_out;
    uint32_t stop_index;
    uint32_t *insane_out;          // null = the framing made bam_read1's acceptance test itself; else [0] is set when a decoded record fails it (SegGeom::lite_walk)
    // -s XS: the smallest index of an iterated read with an N operation whose strand tag lies behind an aux field of unknown type (preset ~0; null =
    // off): the reference's bam_aux_get abort()s on it (sam.c:1233-1252) when the read's first junction asks for its strand (junctions_extractor.cc:283-286)
    uint32_t *abort_out;
    uint8_t  bc0, bc1;             // -b: the barcode tag (0 = no -b).  set_junction_barcode asks for it on every read with more than one CIGAR operation, before the
                                   // CIGAR is looked at (junctions_extractor.cc:393-395): a field of unknown type in front of it (or anywhere, without it) is abort_out's too
    // `identify -s XS` (one extraction for every window): such reads are COUNTED here (null = off) and marked in bit 7 of their row's strand byte; upstream
    // abort()s in the first window -- in the order of the variants -- that reads one of them (launch_collect_odd_aux, cse_api.cpp)
    uint32_t *odd_count;
};

// What record i of the file means to the extraction: the answers the decode kernels store and count.  Pure: nothing is written, and the
// pointers of ExtractCfg are only tested for null.
struct RecordRow {
    bool in_region;        // the iterator returns the record
    bool stop_candidate;   // a record of the end rule (ExtractCfg::stop_out): in front of stop_index and not below the region's end
    bool is_long;          // goes to the wave-per-read emitter
    bool abort_read;       // ExtractCfg::abort_out's read
    bool odd_read;         // ExtractCfg::odd_count's read (bit 7 of `strand`)
    uint8_t strand;
    uint32_t nev;          // junction events inside -m / -M
};
// cigar_at(q) = the q-th CIGAR word; tag_strand(t0, t1, &unknown) = strand_from_tag over the record's aux area -- the two things a kernel reads
// where the record's bytes lie.  `h` has passed rec_sane (or has been made inert: n_cigar = 0).  The questions are asked in the reference's
// order, which decides where it aborts: barcode tag, CIGAR, strand tag.
template <class CigarAt, class TagStrand>
RGX_HD RecordRow record_row(const RecHead &h, uint32_t i, const ExtractCfg &cfg, CigarAt &&cigar_at, TagStrand &&tag_strand) {
    RecordRow r = {true, false, false, false, false, (uint8_t)'?', 0};
    if (cfg.region_tid != -2) {
        r.in_region = h.tid == cfg.region_tid && h.pos < cfg.region_end;
        if (cfg.stop_out) {                                // hts_itr_next's end rule (hts.c:1946-1950), see ExtractCfg
            if (i >= cfg.stop_index) r.in_region = false;
            else r.stop_candidate = !r.in_region;
        }
        if (r.in_region) r.in_region = rec_endpos_at(cigar_at, h.n_cigar, h.flag, h.pos) > cfg.region_beg;
    }
    if (!(r.in_region && h.n_cigar > 1 && h.tid >= 0 && h.tid < cfg.n_ref)) return r;
    if (cfg.bc0 && cfg.abort_out) {                        // -b: the barcode tag is asked for first (the walk is strand_from_tag's; what it finds is the barcode kernels' business)
        bool unknown = false;
        (void)tag_strand(cfg.bc0, cfg.bc1, &unknown);
        r.abort_read = unknown;
    }
    bool has_n = false;
    for (uint32_t q = 0; q < h.n_cigar; ++q) {
        const uint32_t c = cigar_at(q);
        if (cig_is_N(c)) { r.nev += intron_ok(0, c >> 4, cfg.min_intron, cfg.max_intron) ? 1u : 0u; has_n = true; }
    }
    // (the tag is asked for by every junction the walk reaches, also one junction_qc then drops: any N operation, cc:415 / :447 / :467 / :490)
    if (r.nev || (has_n && (cfg.abort_out || cfg.odd_count) && cfg.strandness == 0)) {
        if (cfg.strandness == 0) {
            bool unknown = false;
            r.strand = (uint8_t)tag_strand(cfg.tag0, cfg.tag1, &unknown);
            if (unknown && cfg.abort_out) r.abort_read = true;
            if (unknown && cfg.odd_count) { r.odd_read = true; r.strand |= 0x80; }
        } else r.strand = (uint8_t)strand_from_flag(h.flag, cfg.strandness);
        r.is_long = r.nev && h.n_cigar > cfg.long_threshold;
    }
    return r;
}

}  // namespace rgx
