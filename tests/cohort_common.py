"""What the cohort tests share (tests/test_cohort_host.py, tests/test_gpu_cohort.py): hand-made tables through rgx_table_unpack, the synthetic
ten-sample cohort, and the EXPECTATION -- each sample's BED12 from the oracle, merged with a dict here.  The restatement shares no code with the
product: it reads BED text and BAM headers and writes the two cohort texts itself."""
import ctypes as C
import os
import struct
import subprocess
import zlib

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ORACLE = os.path.join(ROOT, "oracle", "oracle_cli")

# (name, shape, seed, n_introns, n_reads, -s)
SPECS = [("s30k", "short", 7, 20000, 30_000, "XS"), ("s60k", "short", 7, 20000, 60_000, "XS"), ("s120k", "short", 7, 20000, 120_000, "XS"),
         ("s250k", "short", 7, 20000, 250_000, "XS"), ("s500k", "short", 7, 20000, 500_000, "XS"), ("s90k", "short", 7, 20000, 90_000, "XS"),
         ("other", "short", 8, 5000, 80_000, "XS"), ("fuzz", "fuzz", 41, 0, 20_000, "XS"), ("long", "long", 42, 0, 1_500, "XS"),
         ("rf40k", "short", 7, 20000, 40_000, "RF")]
STRANDNESS = {"XS": 0, "RF": 1, "FR": 2}


def table_from_rows(rows, contigs=(("chrA", 1000000), ("chrB", 1000000))):
    """rows: (tid, start, end, thick_start, thick_end, count, strand) -> JunctionTable* through rgx_table_unpack (name_index and the anchor
    flag bytes stay unset, as on every unpacked table)."""
    from regtools_amd import _ffi
    L = _ffi.lib()
    raw = b"".join(struct.pack("<12I", r[0] & 0xffffffff, r[1], r[2], r[3], r[4], r[5], 0, 0, 0, 0, ord(r[6]), 0) for r in rows)
    proto = _ffi.JunctionTable()
    arr = (C.c_char_p * max(1, len(contigs)))(*[c[0].encode() for c in contigs])
    lens = (C.c_uint32 * max(1, len(contigs)))(*[c[1] for c in contigs])
    proto.n_ref, proto.ref_name, proto.ref_len = len(contigs), arr, lens
    t = C.POINTER(_ffi.JunctionTable)()
    buf = (C.c_uint8 * max(1, len(raw))).from_buffer_copy(raw or b"\0")
    assert L.rgx_table_unpack(buf, len(rows), C.byref(proto), C.byref(t)) == 0
    return t


class HostMatrix(object):
    """rgx_cohort_merge_host over raw table pointers."""

    def __init__(self, tables, anchors, names, only_anchored=True, min_samples=1, min_total=1):
        from regtools_amd import _ffi
        self.L = L = _ffi.lib()
        n = len(tables)
        tabs = (C.POINTER(_ffi.JunctionTable) * max(1, n))(*tables)
        anc = (C.c_uint32 * max(1, n))(*anchors)
        nm = (C.c_char_p * max(1, n))(*[s.encode() for s in names])
        p = _ffi.CohortParams()
        L.rgx_cohort_params_default(C.byref(p))
        self.defaults = (p.only_anchored, p.min_samples, p.min_total)
        p.only_anchored, p.min_samples, p.min_total = int(only_anchored), min_samples, min_total
        self.h = C.POINTER(_ffi.CohortMatrix)()
        self.err = C.create_string_buffer(512)
        self.rc = L.rgx_cohort_merge_host(tabs, anc, nm, n, C.byref(p), C.byref(self.h), self.err, len(self.err))

    def _text(self, fn):
        n = fn(self.h, None, 0)
        buf = C.create_string_buffer(n + 1)
        assert fn(self.h, buf, n) == n
        return buf.raw[:n]

    def bed12(self):
        return self._text(self.L.rgx_cohort_format_bed12)

    def counts(self):
        return self._text(self.L.rgx_cohort_format_counts)

    def free(self):
        if self.h:
            self.L.rgx_cohort_matrix_free(self.h)
            self.h = None


def read_contigs(path):
    """[(name, length)] of a BAM's header, in header order."""
    d = open(path, "rb").read()
    data, off = b"", 0

    def need(k):
        nonlocal data, off
        while len(data) < k:
            bl = struct.unpack_from("<H", d, off + 16)[0] + 1
            data += zlib.decompress(d[off + 18: off + bl - 8], -15)
            off += bl
    need(12)
    assert data[:4] == b"BAM\1"
    l_text = struct.unpack_from("<i", data, 4)[0]
    need(12 + l_text)
    n_ref = struct.unpack_from("<i", data, 8 + l_text)[0]
    q, out = 12 + l_text, []
    for _ in range(n_ref):
        need(q + 4)
        l_name = struct.unpack_from("<i", data, q)[0]
        need(q + 4 + l_name + 4)
        out.append((data[q + 4: q + 4 + l_name - 1].decode(), struct.unpack_from("<i", data, q + 4 + l_name)[0]))
        q += 8 + l_name
    return out


def parse_bed12(text):
    """{(chrom, start, end, strand): (score, thick_start, thick_end)} with start = chromStart + blockSize0, end = chromEnd - blockSize1."""
    rows = {}
    for line in text.decode().splitlines():
        f = line.split("\t")
        b0, b1 = [int(x) for x in f[10].split(",")[:2]]
        key = (f[0], int(f[1]) + b0, int(f[2]) - b1, f[5])
        assert key not in rows
        rows[key] = (int(f[4]), int(f[1]), int(f[2]))
    return rows


@pytest.fixture(scope="module")
def cohort_files(tmp_path_factory):
    """The synthetic cohort on disk: [dict(name, path, strand, contigs, rows)], rows = the sample's `junctions extract` BED12 by the oracle."""
    from regtools_amd import synth
    d = str(tmp_path_factory.mktemp("cohort"))
    out = []
    for name, shape, seed, n_introns, n_reads, strand in SPECS:
        path = os.path.join(d, name + ".bam")
        synth.write(path, n_reads, shape=shape, seed=seed, n_introns=n_introns)
        if not os.path.exists(path + ".bai"):
            synth.index(path)
        bed = subprocess.run([ORACLE, "extract", "-s", strand, path], stdout=subprocess.PIPE, stderr=subprocess.PIPE, check=True).stdout
        out.append(dict(name=name, path=path, strand=strand, contigs=read_contigs(path), rows=parse_bed12(bed)))
    return out


def cls_of(strand):
    return 0 if strand == "+" else 1 if strand == "-" else 2


def expected_texts(samples, min_samples=1, min_total=1):
    """(BED12 bytes, counts bytes, stats) of the cohort of `samples` (dicts with name, contigs, rows as parse_bed12 gives them), by a dict."""
    contigs = {}
    for s in samples:
        for nm, ln in s["contigs"]:
            assert contigs.setdefault(nm, (len(contigs), ln))[1] == ln
    merged = {}
    for k, s in enumerate(samples):
        for (chrom, start, end, strand), (score, ts, te) in s["rows"].items():
            merged.setdefault((contigs[chrom][0], start, end, cls_of(strand)), {})[k] = (score, ts, te, strand, chrom)
    bed, tsv = [], ["chrom\tstart\tend\tstrand" + "".join("\t" + s["name"] for s in samples) + "\n"]
    n_with_hist = {}
    for key in sorted(merged):
        per = merged[key]
        total = sum(v[0] for v in per.values())
        n_with_hist[len(per)] = n_with_hist.get(len(per), 0) + 1
        if len(per) < min_samples or total < min_total:
            continue
        ts, te = min(v[1] for v in per.values()), max(v[2] for v in per.values())
        _, _, _, strand, chrom = per[max(per)]
        _, start, end, _ = key
        bed.append("%s\t%d\t%d\tJUNC%08d\t%d\t%s\t%d\t%d\t255,0,0\t2\t%d,%d\t0,%d\n" % (chrom, ts, te, len(bed) + 1, total, strand, ts, te, start - ts,
                                                                                       te - end, end - ts))
        tsv.append("%s\t%d\t%d\t%s" % (chrom, start, end, strand) + "".join("\t%d" % (per[k][0] if k in per else 0) for k in range(len(samples))) + "\n")
    stats = dict(rows_in=sum(len(s["rows"]) for s in samples), union=len(merged), n_with_hist=n_with_hist)
    return "".join(bed).encode(), "".join(tsv).encode(), stats
