"""A bit-level DEFLATE writer (RFC 1951 and nothing else) and a catalogue of hand-built streams: legal ones that zlib's compressor never
writes, and malformed ones that name the decoder's rejection code.  The catalogue is what tests/test_deflate_conformance_host.py (CPU),
tests/hostemu/inflate_edges.cpp (host sanitizers, `python tests/deflate_craft.py --dump FILE`) and tests/test_gpu_deflate_conformance.py feed
to every form of the decoder; zlib's inflate is the referee of every entry.

Tokens of a compressed block:
    b                    a literal byte (int 0..255)
    (length, distance)   a match, 3..258 bytes from 1..32768 back
    ("ll", s)            literal/length symbol s as it stands, no extra bits           } raw escapes: what a malformed stream is made of;
    ("d", s)             distance symbol s as it stands, no extra bits                 } the token interpreter refuses them
    ("bits", v, k)       k raw bits of v, LSB first                                    }
"""
import struct
import sys
import zlib

# InflateStatus of regtools_amd/csrc/inflate_core.h
INF_OK, INF_BAD_BTYPE, INF_BAD_STORED, INF_BAD_HEADER, INF_OVERSUBSCRIBED, INF_INCOMPLETE, INF_BAD_REPEAT = 0, 1, 2, 3, 4, 5, 6
INF_NO_EOB, INF_BAD_CODE, INF_BAD_DIST, INF_OUT_OVERFLOW, INF_IN_OVERRUN, INF_SIZE_MISMATCH = 7, 8, 9, 10, 11, 12

CL_ORDER = [16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15]                 # RFC 1951 3.2.7
LEN_BASE = [3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258]
LEN_EXTRA = [0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0]
DIST_BASE = [1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145, 8193, 12289,
             16385, 24577]
DIST_EXTRA = [0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13]
FIXED_LL = [8] * 144 + [9] * 112 + [7] * 24 + [8] * 8                                         # RFC 1951 3.2.6
FIXED_D = [5] * 32


def length_symbol(length):
    """(symbol, extra bits, their value) of a match length; 258 is symbol 285."""
    assert 3 <= length <= 258
    c = 28 if length == 258 else max(k for k in range(28) if LEN_BASE[k] <= length)
    return 257 + c, LEN_EXTRA[c], length - LEN_BASE[c]


def distance_symbol(dist):
    assert 1 <= dist <= 32768
    c = max(k for k in range(30) if DIST_BASE[k] <= dist)
    return c, DIST_EXTRA[c], dist - DIST_BASE[c]


def canonical(lens):
    """RFC 1951 3.2.2: {symbol: (code, length)} of a list of code lengths (0 = unused).  An over-subscribed list still gets codes (cut to
    their length): the decoder under test must refuse it from the header alone."""
    count = [0] * 17
    for l in lens:
        count[l] += 1
    count[0] = 0
    nxt, code = [0] * 17, 0
    for bits in range(1, 17):
        code = (code + count[bits - 1]) << 1
        nxt[bits] = code
    out = {}
    for s, l in enumerate(lens):
        if l:
            out[s] = (nxt[l] & ((1 << l) - 1), l)
            nxt[l] += 1
    return out


def complete_lens(k):
    """Code lengths of a complete code over k >= 2 symbols, as flat as they come: 2^(m+1) - k codes of m bits, then 2 (k - 2^m) of m + 1."""
    assert k >= 2
    m = k.bit_length() - 1
    return [m] * ((2 << m) - k) + [m + 1] * (2 * (k - (1 << m)))


class BitSink:
    """Bits leave LSB first; Huffman codes go in MSB first (RFC 1951 3.1.1)."""

    def __init__(self):
        self.out, self.acc, self.n = bytearray(), 0, 0

    def put(self, v, n):
        assert 0 <= v < (1 << n) or n == 0
        self.acc |= v << self.n
        self.n += n
        if self.n >= 64:
            k = self.n >> 3
            self.out += (self.acc & ((1 << (8 * k)) - 1)).to_bytes(k, "little")
            self.acc >>= 8 * k
            self.n -= 8 * k

    def code(self, code, length):
        self.put(int(format(code, "0%db" % length)[::-1], 2), length)

    def align(self):
        if self.n & 7:
            self.put(0, 8 - (self.n & 7))

    def raw(self, data):
        assert self.n & 7 == 0
        self.out += self.acc.to_bytes(self.n >> 3, "little") + data
        self.acc = self.n = 0

    def value(self):
        return bytes(self.out) + self.acc.to_bytes((self.n + 7) >> 3, "little")


def interpret(tokens, history=b""):
    """The bytes a token list stands for, behind `history` (a match may reach into it)."""
    out = bytearray(history)
    for t in tokens:
        if isinstance(t, int):
            out.append(t)
        else:
            assert len(t) == 2 and isinstance(t[0], int), "raw escape %r has no meaning" % (t,)
            length, dist = t
            assert 1 <= dist <= len(out)
            for _ in range(length):
                out.append(out[-dist])
    return bytes(out[len(history):])


class Stream:
    """One raw-DEFLATE stream being written block by block; .data is what the interpreter makes of the blocks so far (None once a raw
    escape was written)."""

    def __init__(self):
        self.w, self.data = BitSink(), bytearray()

    def payload(self, trailing=b""):
        return self.w.value() + trailing

    def stored(self, last, data, nlen=None, claim=None):
        """claim: the LEN field when it is not len(data) (a block that runs past the input); nlen: the NLEN field when it is not ~LEN."""
        n = len(data) if claim is None else claim
        self.w.put(last, 1); self.w.put(0, 2); self.w.align()
        self.w.put(n, 16); self.w.put((n ^ 0xffff) if nlen is None else nlen, 16)
        self.w.raw(data)
        self.data += data
        return self

    def _tokens(self, tokens, ll, dd, eob):
        put = self.w.put
        rl = {s: (int(format(c, "0%db" % l)[::-1], 2), l) for s, (c, l) in ll.items()}        # codes as the sink takes them: bit-reversed
        rd = {s: (int(format(c, "0%db" % l)[::-1], 2), l) for s, (c, l) in dd.items()}
        for t in tokens:
            if isinstance(t, int):
                put(*rl[t])
            elif t[0] == "ll":
                put(*rl[t[1]])
            elif t[0] == "d":
                put(*rd[t[1]])
            elif t[0] == "bits":
                put(t[1], t[2])
            else:
                s, eb, ev = length_symbol(t[0])
                put(*rl[s]); put(ev, eb)
                s, eb, ev = distance_symbol(t[1])
                put(*rd[s]); put(ev, eb)
        if eob:
            put(*rl[256])
        if self.data is not None and all(isinstance(t, int) or isinstance(t[0], int) for t in tokens):
            self.data += interpret(tokens, bytes(self.data))
        else:
            self.data = None

    def fixed(self, last, tokens, eob=True):
        self.w.put(last, 1); self.w.put(1, 2)
        self._tokens(tokens, canonical(FIXED_LL), canonical(FIXED_D), eob)
        return self

    def header_bits(self, last, btype):
        self.w.put(last, 1); self.w.put(btype, 2)
        return self

    def dynamic(self, last, ll_lens, d_lens, tokens, cl_lens=None, hclen=None, cl_seq=None, eob=True):
        """HLIT = len(ll_lens), HDIST = len(d_lens).  cl_seq spells the code-length symbols: 0..15, (16, 3..6), (17, 3..10), (18, 11..138);
        by default every length stands for itself.  cl_lens: the 19 lengths of the code-length code (default: a flat complete code over the symbols
        cl_seq uses); hclen: how many of them are sent (default: up to the last non-zero one)."""
        if cl_seq is None:
            cl_seq = list(ll_lens) + list(d_lens)
        used = sorted({s if isinstance(s, int) else s[0] for s in cl_seq})
        if cl_lens is None:
            cl_lens = [0] * 19
            if len(used) == 1:
                used = used + [(used[0] + 1) % 19]                       # a one-code code-length code is no code: lend it a neighbour
            for s, l in zip(used, complete_lens(len(used))):
                cl_lens[s] = l
        if hclen is None:
            hclen = max([4] + [k + 1 for k in range(19) if cl_lens[CL_ORDER[k]]])
        assert 257 <= len(ll_lens) <= 288 and 1 <= len(d_lens) <= 32 and 4 <= hclen <= 19
        self.w.put(last, 1); self.w.put(2, 2)
        self.w.put(len(ll_lens) - 257, 5); self.w.put(len(d_lens) - 1, 5); self.w.put(hclen - 4, 4)
        for k in range(hclen):
            self.w.put(cl_lens[CL_ORDER[k]], 3)
        cl = canonical(cl_lens)
        for s in cl_seq:
            if isinstance(s, int):
                self.w.code(*cl[s])
            else:
                self.w.code(*cl[s[0]])
                self.w.put(s[1] - (3 if s[0] < 18 else 11), 2 if s[0] == 16 else 3 if s[0] == 17 else 7)
        self._tokens(tokens, canonical(ll_lens), canonical(d_lens), eob)
        return self


# ---- small deterministic encoders (the end-to-end dialects of tests/test_gpu_deflate_conformance.py) -----------------------------------------

def run_tokens(data):
    """Literals, and distance-1 matches for the tail of every run of 4 or more equal bytes."""
    out, i, n = [], 0, len(data)
    while i < n:
        j = i
        while j < n and data[j] == data[i]:
            j += 1
        out.append(data[i])
        left = j - i - 1
        while left >= 3:
            k = min(258, left)
            out.append((k, 1)); left -= k                                # (a rest of 1 or 2 goes out as literals below)
        out += [data[i]] * left
        i = j
    return out


def flat_ll_lens(tokens):
    """A flat complete literal/length code over the symbols a token list uses and end-of-block, cut to HLIT entries."""
    used = {256}
    for t in tokens:
        used.add(t if isinstance(t, int) else length_symbol(t[0])[0])
    if len(used) == 1:
        return [0] * 256 + [1]
    lens = [0] * 286
    for s, l in zip(sorted(used), complete_lens(len(used))):
        lens[s] = l
    return lens[:max(257, max(used) + 1)]


def seven_short_lens(data):
    """The '7 short + 256 fifteen-bit' code for literals-only data: the six most frequent bytes and end-of-block get 1..7 bits, the other 250 bytes and
    the length symbols 257..262 fifteen (1/2 + .. + 1/128 + 256 / 32768 = 1)."""
    freq = sorted(range(256), key=lambda b: (-data.count(bytes([b])), b))
    lens = [15] * 263
    for l, s in zip((1, 2, 3, 4, 5, 6), freq):
        lens[s] = l
    lens[256] = 7
    return lens


def dialect(name, data):
    """One member's worth of `data` as raw DEFLATE in a dialect zlib never writes."""
    s = Stream()
    if name == "fixed_literals":
        s.fixed(1, list(data))
    elif name == "dynamic_no_distance":
        s.dynamic(1, flat_ll_lens(list(data)), [0], list(data))
    elif name == "dynamic_one_distance":
        t = run_tokens(data)
        s.dynamic(1, flat_ll_lens(t), [1], t)
    elif name == "block_every_200":
        pieces = [data[i:i + 200] for i in range(0, len(data), 200)] or [b""]
        for k, p in enumerate(pieces):
            last = 1 if k == len(pieces) - 1 else 0
            if k % 3 == 0:
                s.stored(0, b"").stored(last, p)
            elif k % 3 == 1:
                s.dynamic(0, [0] * 256 + [1], [0], []).fixed(last, run_tokens(p))
            else:
                t = run_tokens(p)
                s.dynamic(last, flat_ll_lens(t), [1], t)
    elif name == "seven_short":
        s.dynamic(1, seven_short_lens(data), [0], list(data))
    else:
        raise KeyError(name)
    assert bytes(s.data) == data
    return s.payload()


DIALECTS = ["fixed_literals", "dynamic_no_distance", "dynamic_one_distance", "block_every_200", "seven_short"]


# ---- the catalogue ----------------------------------------------------------------------------------------------------------------------

class Entry:
    """name, payload and either expect (bytes: a legal stream; interp is what the token interpreter made of the same blocks) or code (the
    InflateStatus every decoder must give; accept = the set where a form legitimately differs, why = the line that says why), zmsg (a piece of
    zlib's message, or "truncated": zlib wants more input) and size (the capacity the member claims)."""

    def __init__(self, name, payload, expect=None, interp=None, code=None, zmsg=None, size=300, accept=None, why=None):
        self.name, self.payload, self.expect, self.interp = name, payload, expect, interp
        self.code, self.zmsg, self.size = code, zmsg, size
        self.accept = frozenset(accept) if accept else frozenset([code])
        self.why = why
        assert (expect is None) != (code is None) and len(payload) < 65536
        assert accept is None or why


def _legal(name, stream, expect, trailing=b""):
    return Entry(name, stream.payload(trailing), expect=bytes(expect), interp=bytes(stream.data))


def _bad(name, stream, code, zmsg, size=300, trailing=b"", **kw):
    return Entry(name, stream.payload(trailing) if isinstance(stream, Stream) else stream, code=code, zmsg=zmsg, size=size, **kw)


def _noise(n, seed):
    x, out = (seed * 2654435761 + 12345) & 0xffffffff, bytearray()
    for _ in range(n):
        x = (x * 1103515245 + 12345) & 0x7fffffff
        out.append((x >> 16) & 255)
    return bytes(out)


HOT_SLOTS = 160                     # kHotSyms of kernels.hip: literal/length list slots held in LDS; the rest in the global scratch column


def list_slots(ll_lens):
    """{symbol: its slot in the list sorted by (code length, symbol)}: what build_code hands to set_ll_sym."""
    order = sorted((l, s) for s, l in enumerate(ll_lens) if l)
    return {s: k for k, (_, s) in enumerate(order)}


def rotated(lens, k):
    return lens[-k:] + lens[:-k] if k else list(lens)


ALL286_VECTORS = {"226x8+60x9": [9] * 60 + [8] * 226, "126x7+96x13+64x14": [7] * 126 + [13] * 96 + [14] * 64}
ALL286_SHIFTS = (0, 72, 143, 214)


def _all286_tokens():
    t = list(range(256))
    for c in range(29):                                                  # every length symbol, base length and its last
        t.append((LEN_BASE[c], 1 + c % 4))
        if LEN_EXTRA[c]:
            t.append((LEN_BASE[c] + (1 << LEN_EXTRA[c]) - 1, 5 + c % 2))
    return t


def _hclen_ll(h):
    """A complete literal/length code whose lengths are all among the values that HCLEN = h can name, and use the last of them (CL_ORDER[h - 1])."""
    L = CL_ORDER[h - 1]
    if L == 8:
        return [8] * 255 + [0, 8]
    if L < 8:
        return [8] * (256 - (1 << (8 - L))) + [0] * (1 << (8 - L)) + [L]
    return [8] * 255 + [0] + list(range(9, L + 1)) + [L]


def legal_entries():
    E = []
    abc = b"abcabcabcabcab"
    # ---- distance tree
    E.append(_legal("dist_one_code_len1", Stream().dynamic(1, flat_ll_lens([120, (20, 1)]), [1], [120, (20, 1)]), b"x" * 21))
    E.append(_legal("dist_one_code_is_symbol_3", Stream().dynamic(1, flat_ll_lens(list(b"wxyz") + [(9, 4)]), [0, 0, 0, 1], list(b"wxyz") + [(9, 4)]),
                    b"wxyzwxyzwxyzw"))
    t = list(b"no matches here")
    E.append(_legal("hdist1_zero_length_literals_only", Stream().dynamic(1, flat_ll_lens(t), [0], t), b"no matches here"))
    pre = _noise(32768, 1)
    t, want = [], bytearray(pre)
    for c in range(30):
        d = DIST_BASE[c] + (1 << DIST_EXTRA[c]) - 1 if c == 29 else DIST_BASE[c]
        t.append((3 + c % 5, d)); t.append(65 + c)
    for tok in t:
        want += interpret([tok], bytes(want))
    E.append(_legal("dist_all_30_symbols_back_to_32768", Stream().stored(0, pre).dynamic(1, flat_ll_lens(t), [4, 4] + [5] * 28, t), want))
    d15 = list(range(1, 16)) + [15]
    pre = _noise(300, 2)
    t = [(4 + c, DIST_BASE[c]) for c in range(16)]
    E.append(_legal("dist_codes_up_to_15_bits", Stream().stored(0, pre).dynamic(1, flat_ll_lens(t), d15, t), pre + interpret(t, pre)))
    # ---- literal/length code
    eob_only = [0] * 256 + [1]
    E.append(_legal("ll_eob_alone_final", Stream().dynamic(1, eob_only, [0], []), b""))
    E.append(_legal("ll_eob_alone_then_fixed", Stream().dynamic(0, eob_only, [0], []).fixed(1, list(b"after")), b"after"))
    E.append(_legal("ll_eob_alone_between_stored", Stream().stored(0, b"left").dynamic(0, eob_only, [1], []).stored(1, b"right"), b"leftright"))
    ll = [0] * 286
    for l, s in zip(list(range(1, 16)) + [15], [97, 256, 98] + list(range(257, 269)) + [285]):
        ll[s] = l
    t = [97, 98] + [(n, 1 + n % 2) for n in range(3, 19)] + [(258, 2), 97, (258, 1)]
    E.append(_legal("ll_lengths_1_to_15_15_len258_tails_3_to_18", Stream().dynamic(1, ll, [1, 1], t), interpret(t)))
    for vname, vec in sorted(ALL286_VECTORS.items()):
        for k in ALL286_SHIFTS:
            t = _all286_tokens()
            E.append(_legal("ll_all_286_%s_rot%d" % (vname, k), Stream().dynamic(1, rotated(vec, k), [2, 2, 2, 3, 3], t), interpret(t)))
    ll = [15] * 256 + [1, 2, 3, 4, 5, 6, 7]
    t = list(range(256)) + [(3, 1), (8, 257), 0, 255, (5, 2)]
    E.append(_legal("ll_seven_short_256_fifteen_bit", Stream().dynamic(1, ll, [1, 2, 3, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 3], t), interpret(t)))
    # ---- code-length code
    ll = [0] * 256 + [2, 2]                                               # a, b: 3 bits, c, end-of-block, length 3: 2 bits; four distance codes of 2 bits
    ll[97], ll[98], ll[99] = 3, 3, 2
    t = list(b"abcabc") + [(3, 3), (3, 1), (3, 4)]
    seq = ll[:257] + [(16, 5)]                                            # the repeat 16 copies end-of-block's 2 onto symbol 257 and the four distance codes
    E.append(_legal("cl_repeat16_across_hlit_boundary", Stream().dynamic(1, ll, [2, 2, 2, 2], t, cl_seq=seq), interpret(t)))
    ll = [8] * 254 + [0, 0, 8, 8] + [0] * 8                               # 256 codes of 8 bits, HLIT 266; the distance code is symbol 5 alone
    seq = ll[:258] + [(18, 13)] + [1]                                     # the repeat 18 zeroes literal/length 258..265 and distance 0..4
    t = list(b"hello, world") + [(3, 7)]
    E.append(_legal("cl_repeat18_across_hlit_boundary", Stream().dynamic(1, ll, [0] * 5 + [1], t, cl_seq=seq), interpret(t)))
    for h in range(5, 20):
        ll = _hclen_ll(h)
        t = [0, 1, 2, 3, 100]
        s = Stream().dynamic(1, ll, [0], t, hclen=h)
        E.append(_legal("cl_hclen_%d" % h, s, bytes(t)))
    # HCLEN 4 can name only 16, 17, 18 and 0 -- every length would be zero, no end-of-block: RFC 1951 has no legal block with it (malformed list)
    t = list(b"skewed code-length code")
    ll = flat_ll_lens(t)
    used = sorted(set(ll) | {1})
    cl = [0] * 19
    for s_, l in zip(used, list(range(1, len(used))) + [len(used) - 1]):
        cl[s_] = l
    E.append(_legal("cl_skewed_hclen_below_19", Stream().dynamic(1, ll, [1], t, cl_lens=cl), bytes(t)))
    # ---- block sequences
    s = Stream().stored(0, b"data-1 ").stored(0, b"").stored(0, b"").stored(0, b"").fixed(0, []).stored(0, b"").fixed(0, list(b"data-2 ")).fixed(0, [])
    s.stored(1, b"data-3")
    E.append(_legal("empty_stored_run_and_empty_fixed_between_data", s, b"data-1 data-2 data-3"))
    E.append(_legal("match_across_block_boundary", Stream().fixed(0, list(b"abcdef")).fixed(0, [(6, 6)]).stored(0, b"-").fixed(1, [(13, 13)]),
                    b"abcdefabcdef-abcdefabcdef-"))
    E.append(_legal("distance_equals_bytes_written", Stream().fixed(1, list(b"12345") + [(5, 5), (10, 10), (258, 20)]),
                    b"12345" * 4 + (b"12345" * 52)[:258]))
    far = _noise(400, 5)                                                  # (beyond the ring decoder's LDS window: a copy whose source is the member's first byte)
    E.append(_legal("distance_equals_bytes_written_far", Stream().stored(0, far).fixed(1, [(20, 400)] + [33] * 13 + [(258, 433)]),
                    far + far[:20] + b"!" * 13 + far[:258]))
    E.append(_legal("final_block_then_trailing_bytes", Stream().fixed(1, list(b"the end")), b"the end", trailing=b"\x07\xff\x00 not deflate \xfe" * 2))
    E.append(_legal("final_stored_then_trailing_bytes", Stream().stored(1, b"stored end"), b"stored end", trailing=b"\xff" * 9))
    for n in (0, 1, 15, 16, 17):
        d = bytes(range(48, 48 + n))
        E.append(_legal("out_%d_bytes_fixed" % n, Stream().fixed(1, list(d)), d))
        E.append(_legal("out_%d_bytes_stored" % n, Stream().stored(1, d), d))
    half = _noise(32768, 3)
    E.append(_legal("out_65536_bytes_stored_half_then_its_copy", Stream().stored(0, half).fixed(1, [(258, 32768)] * 126 + [(257, 32768), (3, 32768)]),
                    half + half))
    for n in (0, 1, 15, 16, 17):
        d = bytes((7 * k) % 5 + 65 for k in range(n))
        E.append(_legal("out_%d_bytes_dynamic_one_distance" % n, Stream().dynamic(1, flat_ll_lens(run_tokens(d)), [1], run_tokens(d)), d))
    text = (b"@read/1 ACGTTTTTTTTGCA IIIIIIIIIIIIII\n" * 9 + bytes(range(256)) + b"\0" * 700 + b"tail")
    for name in DIALECTS:
        E.append(Entry("dialect_" + name, dialect(name, text), expect=text, interp=text))
    t = list(b"abcdefgh") + [(8, 8), (16, 16), (32, 32), (64, 64), (128, 128), (258, 256)]
    E.append(_legal("distance_equals_bytes_written_dynamic", Stream().dynamic(1, flat_ll_lens(t), complete_lens(16), t), (b"abcdefgh" * 80)[:514]))
    t = list(b"0123456789abcdefg") + [(n, 1 + n % 17) for n in range(3, 259)]
    E.append(_legal("fixed_every_match_length_3_to_258", Stream().fixed(1, t), interpret(t)))
    t = [7] + [(258, 1)] * 254 + [(3, 1)]
    E.append(_legal("out_65536_bytes_one_run", Stream().fixed(1, t), b"\x07" * 65536))
    return E


def malformed_entries():
    E = []
    lit5 = list(b"hello")
    ok_ll = flat_ll_lens(lit5)
    # ---- 1..3
    E.append(_bad("btype_3_first", Stream().header_bits(1, 3), INF_BAD_BTYPE, "invalid block type"))
    E.append(_bad("btype_3_after_data", Stream().fixed(0, lit5).header_bits(0, 3), INF_BAD_BTYPE, "invalid block type"))
    E.append(_bad("stored_nlen_wrong", Stream().stored(1, b"0123456789", nlen=0xfff4), INF_BAD_STORED, "invalid stored block lengths"))
    E.append(_bad("stored_nlen_equals_len", Stream().fixed(0, lit5).stored(1, b"", nlen=0), INF_BAD_STORED, "invalid stored block lengths"))
    E.append(_bad("hlit_287", Stream().dynamic(1, ok_ll + [0] * (287 - len(ok_ll)), [0], lit5), INF_BAD_HEADER, "too many length or distance symbols"))
    E.append(_bad("hdist_31", Stream().dynamic(1, ok_ll, [1] + [0] * 30, lit5), INF_BAD_HEADER, "too many length or distance symbols"))
    # ---- 4, 5
    seq = ok_ll + [0]
    used = sorted(set(seq))

    def cl_with(lens_for_used):
        cl = [0] * 19
        for s_, l in zip(used, lens_for_used):
            cl[s_] = l
        return cl
    assert len(used) == 3                                                  # 0 and two code lengths
    E.append(_bad("cl_code_oversubscribed", Stream().dynamic(1, ok_ll, [0], lit5, cl_lens=cl_with([1, 1, 1])), INF_OVERSUBSCRIBED, "invalid code lengths set"))
    E.append(_bad("cl_code_incomplete", Stream().dynamic(1, ok_ll, [0], lit5, cl_lens=cl_with([2, 2, 2])), INF_INCOMPLETE, "invalid code lengths set"))
    E.append(_bad("cl_code_one_symbol", Stream().dynamic(1, [0] * 256 + [1], [1], [], cl_lens=[0, 1] + [0] * 17, cl_seq=[1] * 258), INF_INCOMPLETE,
                  "invalid code lengths set"))
    over = [0] * 256 + [1, 1, 1]
    E.append(_bad("ll_set_oversubscribed", Stream().dynamic(1, over, [0], []), INF_OVERSUBSCRIBED, "invalid literal/lengths set"))
    E.append(_bad("ll_set_oversubscribed_by_one_15_bit", Stream().dynamic(1, [15] * 256 + [1, 2, 3, 4, 5, 6, 7, 15], [0], []), INF_OVERSUBSCRIBED,
                  "invalid literal/lengths set"))
    E.append(_bad("ll_set_incomplete", Stream().dynamic(1, [2] + [0] * 255 + [2, 2], [0], []), INF_INCOMPLETE, "invalid literal/lengths set"))
    E.append(_bad("ll_set_one_2_bit_code", Stream().dynamic(1, [0] * 256 + [2], [0], []), INF_INCOMPLETE, "invalid literal/lengths set"))
    E.append(_bad("dist_set_oversubscribed", Stream().dynamic(1, ok_ll, [1, 1, 1], lit5), INF_OVERSUBSCRIBED, "invalid distances set"))
    E.append(_bad("dist_set_incomplete", Stream().dynamic(1, ok_ll, [2, 2, 2], lit5), INF_INCOMPLETE, "invalid distances set"))
    E.append(_bad("dist_set_one_2_bit_code", Stream().dynamic(1, ok_ll, [2], lit5), INF_INCOMPLETE, "invalid distances set"))
    E.append(_bad("dist_set_two_codes_one_bit_and_two", Stream().dynamic(1, ok_ll, [1, 2], lit5), INF_INCOMPLETE, "invalid distances set"))
    # ---- 6
    E.append(_bad("repeat16_first", Stream().dynamic(1, ok_ll, [0], lit5, cl_seq=[(16, 3)] + ok_ll[3:] + [0]),
                  INF_BAD_REPEAT, "invalid bit length repeat"))
    E.append(_bad("repeat18_overruns_hlit_plus_hdist", Stream().dynamic(1, ok_ll, [0], lit5, cl_seq=ok_ll[:-1] + [(18, 11)]), INF_BAD_REPEAT,
                  "invalid bit length repeat"))
    E.append(_bad("repeat16_overruns_hlit_plus_hdist", Stream().dynamic(1, ok_ll, [ok_ll[-1]], lit5, cl_seq=ok_ll + [(16, 3)]), INF_BAD_REPEAT,
                  "invalid bit length repeat"))
    E.append(_bad("hclen_4_all_zero_lengths_overrun", Stream().dynamic(1, [0] * 257, [0], [], cl_seq=[(18, 138), (18, 138)], cl_lens=[1] + [0] * 17 + [1],
                                                                       hclen=4, eob=False), INF_BAD_REPEAT, "invalid bit length repeat"))
    # ---- 7
    E.append(_bad("no_end_of_block_code", Stream().dynamic(1, [1, 1] + [0] * 255, [0], [0, 1, 0], eob=False), INF_NO_EOB, "missing end-of-block"))
    E.append(_bad("hclen_4_all_zero_lengths", Stream().dynamic(1, [0] * 257, [0], [], cl_seq=[(18, 138), (18, 120)], cl_lens=[1] + [0] * 17 + [1], hclen=4,
                                                               eob=False), INF_NO_EOB, "missing end-of-block"))
    # ---- 8
    m = flat_ll_lens([97, (3, 1)])
    E.append(_bad("one_code_distance_tree_other_half", Stream().dynamic(1, m, [1], [97, ("ll", 257), ("bits", 1, 1)]), INF_BAD_CODE, "invalid distance code"))
    E.append(_bad("match_without_a_distance_code", Stream().dynamic(1, m, [0], [97, ("ll", 257), ("bits", 0, 1)]), INF_BAD_CODE, "invalid distance code"))
    E.append(_bad("fixed_symbol_286", Stream().fixed(1, [97, ("ll", 286)]), INF_BAD_CODE, "invalid literal/length code"))
    E.append(_bad("fixed_symbol_287", Stream().fixed(1, [97, ("ll", 287)]), INF_BAD_CODE, "invalid literal/length code"))
    E.append(_bad("fixed_distance_symbol_30", Stream().fixed(1, [97, ("ll", 257), ("d", 30)]), INF_BAD_CODE, "invalid distance code"))
    E.append(_bad("fixed_distance_symbol_31", Stream().fixed(1, [97, 98, 99, ("ll", 285), ("d", 31)]), INF_BAD_CODE, "invalid distance code"))
    E.append(_bad("fifteen_ones_no_code_owns", Stream().dynamic(0, [0] * 256 + [1], [0], [("bits", 0x7fff, 15)], eob=False), INF_BAD_CODE,
                  "invalid literal/length code"))
    # ... and the same three holes behind a fixed block, whose full symbol lists are still in the tables, with bits behind the hole that spell a small
    # number: a decoder that took "no code owns this" for a list index would find a symbol of the block before and go on
    def pre():
        return Stream().fixed(0, list(b"0123456789abcdef" * 3))
    E.append(_bad("one_code_distance_tree_other_half_then_zeros", pre().dynamic(1, m, [1], [97, ("ll", 257), ("bits", 1, 15), ("bits", 0, 15)]),
                  INF_BAD_CODE, "invalid distance code"))
    E.append(_bad("match_without_a_distance_code_then_zeros", pre().dynamic(1, m, [0], [97, ("ll", 257), ("bits", 0, 15), ("bits", 0, 15)]),
                  INF_BAD_CODE, "invalid distance code"))
    E.append(_bad("eob_alone_other_half_then_zeros", pre().dynamic(1, [0] * 256 + [1], [0], [("bits", 1, 15), ("bits", 0, 15)]), INF_BAD_CODE,
                  "invalid literal/length code"))
    for k in (1, 2, 5, 30):                                               # (MSB first behind the hole's one bit)
        E.append(_bad("one_code_distance_tree_other_half_then_%d" % k,
                      pre().dynamic(1, m, [1], [97, ("ll", 257), ("bits", 1, 1), ("bits", int(format(k, "014b")[::-1], 2), 14), ("bits", 0, 15)]),
                      INF_BAD_CODE, "invalid distance code"))
        E.append(_bad("eob_alone_other_half_then_%d" % (24 + k), pre().dynamic(1, [0] * 256 + [1], [0],
                                                                          [("bits", 1, 1), ("bits", int(format(24 + k, "014b")[::-1], 2), 14)]),
                      INF_BAD_CODE, "invalid literal/length code"))
    # ---- 9
    E.append(_bad("distance_one_past_the_start", Stream().fixed(1, [97, ("ll", 257), ("d", 1)]), INF_BAD_DIST, "invalid distance too far back"))
    E.append(_bad("distance_first_symbol", Stream().fixed(1, [("ll", 257), ("d", 0)]), INF_BAD_DIST, "invalid distance too far back"))
    s = Stream().stored(0, _noise(32767, 4))
    s.fixed(1, [("ll", 257), ("d", 29), ("bits", 8191, 13)])
    E.append(_bad("distance_32768_after_32767_bytes", s, INF_BAD_DIST, "invalid distance too far back", size=40000))
    # ---- 11
    E.append(_bad("stored_runs_past_the_input", Stream().stored(1, b"only ten b", claim=100), INF_IN_OVERRUN, "truncated", size=100))
    E.append(_bad("stored_runs_past_the_input_after_data", Stream().fixed(0, lit5).stored(1, b"past", claim=60000), INF_IN_OVERRUN, "truncated", size=65536))
    E.append(_bad("no_final_block", Stream().fixed(0, lit5).stored(0, b"more").header_bits(0, 1), INF_IN_OVERRUN, "truncated"))
    return [e for e in E if e is not None]


# the counts DESIGN.md states; tests/test_deflate_conformance_host.py asserts the catalogue is at least this large
MIN_LEGAL, MIN_MALFORMED = 66, 47

_cache = {}


def catalogue():
    if not _cache:
        _cache["legal"], _cache["bad"] = legal_entries(), malformed_entries()
        names = [e.name for e in _cache["legal"] + _cache["bad"]]
        assert len(set(names)) == len(names)
    return _cache["legal"], _cache["bad"]


def zlib_verdict(payload):
    """("ok", bytes) when zlib's inflate reaches the end of the stream, ("truncated", None) when it wants more input, ("error", message)."""
    d = zlib.decompressobj(-15)
    try:
        out = d.decompress(payload)
    except zlib.error as e:
        return "error", str(e)
    return ("ok", out) if d.eof else ("truncated", None)


def dump(path):
    """The catalogue as one file for tests/hostemu/inflate_edges.cpp: "DFLC", u32 count, then per entry u16 name length, name, u32 accepted codes as a
    bit set (bit 0 = legal), u32 capacity, u32 payload length, payload, u32 expected length, expected bytes."""
    legal, bad = catalogue()
    with open(path, "wb") as f:
        f.write(b"DFLC" + struct.pack("<I", len(legal) + len(bad)))
        for e in legal + bad:
            exp = e.expect if e.expect is not None else b""
            mask = 1 if e.expect is not None else sum(1 << c for c in e.accept)
            cap = len(exp) if e.expect is not None else e.size
            f.write(struct.pack("<H", len(e.name)) + e.name.encode() + struct.pack("<III", mask, cap, len(e.payload)) + e.payload)
            f.write(struct.pack("<I", len(exp)) + exp)
    return len(legal), len(bad)


if __name__ == "__main__":
    if len(sys.argv) == 3 and sys.argv[1] == "--dump":
        print("%d legal, %d malformed entries" % dump(sys.argv[2]))
    else:
        sys.exit("usage: deflate_craft.py --dump FILE")
