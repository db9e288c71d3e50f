"""BGZF member discovery restated serially (what rgx_k_members must return, include/regtools_amd.h), and the files the discovery tests run it on.

The restatement is plain Python over the file's bytes; nothing in it knows about tiles, threads or jump rounds.  The builders write members whose
payload is one stored DEFLATE block: 18 bytes of header, 5 of block header, the data, 8 of footer -- 31 + n bytes for n data bytes.  Discovery never
inflates, so the footers' sizes are chosen freely and the data may hold anything, decoy headers included."""
import struct
import zlib

import numpy as np

NONE = 0xffffffffffffffff
MAX_BLOCK = 65536
FIXED = bytes([0x1f, 0x8b, 8, 4, 0, 0, 0, 0, 0, 0xff, 6, 0, 0x42, 0x43, 2, 0])        # bytes 0-3 and 10-15 are the ten the magic test reads
_TAIL = FIXED[10:16]


def u16(d, o):
    return d[o] | d[o + 1] << 8


def u32(d, o):
    return struct.unpack_from("<I", d, o)[0]


# ---- the restatement ------------------------------------------------------------------------------------------------------------------
def candidates(d):
    """Every offset o with o + 18 <= len(d) and the ten fixed header bytes, found with an overlapping search."""
    out = []
    i = d.find(b"\x1f\x8b\x08")
    while i != -1:
        if i + 18 <= len(d) and (d[i + 3] & 4) and d[i + 10:i + 16] == _TAIL:
            out.append(i)
        i = d.find(b"\x1f\x8b\x08", i + 1)
    return out


def discover(d, root2=NONE, true_sizes=None, q=(0, 0, 0)):
    d = bytes(d)
    n = len(d)
    cand = candidates(d)
    cset = set(cand)
    reached = {}                                     # offset -> (block length, footer size)
    for root in (0, root2):
        o = root
        while o in cset and o not in reached:
            blen = u16(d, o + 16) + 1
            if blen < 26 or o + blen > n:
                reached[o] = (blen, 0xffffffff)      # listed, ends its chain
                break
            isz = u32(d, o + blen - 4)
            reached[o] = (blen, 0xfffffffe if isz == 0xffffffff else isz)
            o += blen
    members = []
    up = 0
    for k, o in enumerate(sorted(reached)):
        blen, isz = reached[o]
        cpos = o + 18
        clen = blen - 18 if blen >= 26 else 0        # (a header too short to be a member holds nothing)
        if cpos + clen + 8 > n:
            clen = n - 8 - cpos if n > cpos + 8 else 0
        if true_sizes is not None:
            isz = int(true_sizes[k])
        members.append((cpos, up, clen, isz))
        up += isz if isz <= MAX_BLOCK else 0
    index_of = {m[0]: k for k, m in enumerate(members)}
    q_index, q_upos = [], []
    for qq in q:
        k = index_of.get(qq + 18)
        q_index.append(len(members) if k is None else k)
        q_upos.append(NONE if k is None else members[k][1])
    stop = 0xffffffff
    for k in range(q_index[0], len(members)):
        if members[k][3] == 0 or members[k][3] > MAX_BLOCK:
            stop = k
            break
    return {"candidates": cand, "members": members, "total": up, "q_index": q_index, "q_upos": q_upos, "stop": stop}


def members_array(members):
    a = np.zeros((len(members), 4), dtype=np.uint64)
    if members:
        a[:] = np.array(members, dtype=np.uint64)
    return a


# ---- members no compressor writes -----------------------------------------------------------------------------------------------------
def header(blen):
    return FIXED + struct.pack("<H", blen - 1)


def member(data, isize=None, blen_delta=0):
    """A stored-block member of 31 + len(data) bytes; the footer says isize (default: the truth); BSIZE is off by blen_delta."""
    n = len(data)
    body = b"\x01" + struct.pack("<HH", n, n ^ 0xffff) + data
    return header(18 + len(body) + 8 + blen_delta) + body + struct.pack("<II", zlib.crc32(data) & 0xffffffff, n if isize is None else isize)


DATA_AT = 23                                          # where a member's data starts


def decoy(blen=27):
    """18 bytes that pass the magic test; as a member's data they sit DATA_AT bytes behind its start.  blen 27 lands one byte in front of the next
    member of a run of 51-byte members, 28 exactly on it."""
    return header(blen)


def plain_run(n_members, isizes=None):
    """n members of 33 bytes (two data bytes that cannot start a header)."""
    return b"".join(member(b"ab", None if isizes is None else int(isizes[k])) for k in range(n_members))


def decoy_run(n_members, isizes=None, land_on_next=(), blen_delta=None):
    """n members of 51 bytes, each with a decoy header at the start of its data.  land_on_next: the members whose decoy's BSIZE + 1 reaches the next
    member exactly; blen_delta: {member: delta} for members whose own BSIZE is wrong."""
    out = []
    for k in range(n_members):
        out.append(member(decoy(28 if k in land_on_next else 27) + b"xy", None if isizes is None else int(isizes[k]), (blen_delta or {}).get(k, 0)))
    return b"".join(out)


EOF_MEMBER = FIXED + struct.pack("<H", 27) + b"\x03\x00" + bytes(8)       # the 28 bytes that end every BAM


def two_in_one_thread():
    """A 22-byte pattern with the magic at k and at k + 6 (the second header starts in the first one's free bytes), as member data, once for every
    k % 16.  Returns the file and the sixteen k."""
    pat = FIXED[:6] + FIXED[:4] + _TAIL + _TAIL
    assert len(pat) == 22 and pat[6:22] == FIXED[:4] + _TAIL + _TAIL
    out, at, ks = [], 0, []
    for phase in range(16):
        pad = (phase - at - DATA_AT) % 16
        m = member(bytes(pad) + pat + b"\x07\x00")      # (the two bytes behind it are the second header's BSIZE: 8 bytes, no member)
        ks.append(at + DATA_AT + pad)
        out.append(m)
        at += len(m)
    return b"".join(out) + EOF_MEMBER, ks


def small_file():
    """Twelve members of mixed kinds and the EOF member: the file that is cut at every length near its end."""
    parts = [member(b"ab"), member(decoy() + b"xy"), member(b"abc"), member(decoy(28) + b"xy"), member(b"ab", 0), member(decoy() + b"xyz")] * 2
    return b"".join(parts) + EOF_MEMBER


FOOTER_KINDS = [0, 1, 65535, 65536, 65537, 0xffffffff]


def drawn_footers(n, seed):
    """Footer sizes for n members: the six edge values and random ones, mixed."""
    rng = np.random.default_rng(seed)
    kinds = rng.integers(0, 10, n)
    rnd = np.where(rng.integers(0, 2, n) == 0, rng.integers(0, MAX_BLOCK + 1, n), rng.integers(0, 1 << 32, n))
    out = np.where(kinds < 6, np.array(FOOTER_KINDS, dtype=np.int64)[np.minimum(kinds, 5)], rnd).astype(np.int64)
    if n >= 6:
        out[:6] = FOOTER_KINDS
    return out


def drawn_true_sizes(n, seed):
    """What a probe launch would report: lengths up to 65536, and a few above (members that hold nothing)."""
    rng = np.random.default_rng(seed)
    out = rng.integers(0, MAX_BLOCK + 1, n).astype(np.int64)
    if n > 4:
        out[n // 3] = 65537
        out[n // 2] = 0xfffffffe
        out[0] = 65536
        out[n - 1] = 0
    return out


CHAIN_LENGTHS = [1, 2, 3, 4, 5, 255, 256, 257, 1023, 1024, 1025, 2047, 2048, 2049, 4097]
UPOS_LENGTHS = [2047, 2048, 2049, 4096, 4097]
BIG_N, BIG_TOTAL = 70000, 4587520000
