"""Deterministic builders of the inputs that aim at the edges of cse_kernels.hip / cse_core.h (TEST INFRASTRUCTURE): annotations whose junctions
have an exact number of candidate transcripts, a flag-setting transcript at an exact candidate index, transcripts filed at every one of the seven bin
levels; variants around every exon edge; event lists and windows with an exact number of candidates; contig buckets of exact sizes.

Every builder states what it aims at in `claims`; tests/test_cse_edges_host.py re-derives each claim with arithmetic of its own.  Transcript ids are
zero-padded, so byte order of the ids is the order the builder planted them in.

An annotation case comes in two layouts of the same loci: "direct" (3 contigs: the model builds its direct (contig, bin) index) and "search" (230
contigs, the loci on the first, the middle and the last one: contigs x bins exceeds 2^23 and the kernels binary-search the bin table).  Every contig
holds one short filler transcript, so a contig's index is its place in the layout."""
import hashlib
import os

import numpy as np

BIN = 16384
X29 = 1 << 29
LAYOUTS = ("direct", "search")


def contig_layout(layout):
    """(all contig names in GTF order, the three that hold loci: first, middle, last)"""
    names = ["k%03d" % i for i in range(3 if layout == "direct" else 230)]
    return names, [names[0], names[len(names) // 2], names[-1]]


# ---- transcript shapes around a junction (js, je); all of them mean the same on either strand unless said ------------------------------------
def span(js, je):          # reaches its exon loop, sets nothing, skips nothing
    return [(js - 300, js - 200), (je + 200, je + 300)]


def known(js, je):         # the junction itself: all three flags
    return [(js - 300, js), (je, je + 300)]


def at_start(js, je):      # an exon ends at the junction's start: known donor on '+', known acceptor on '-'
    return [(js - 300, js), (je + 200, je + 300)]


def at_end(js, je):        # an exon starts at the junction's end: known acceptor on '+', known donor on '-'
    return [(js - 300, js - 200), (je, je + 300)]


def inner(js, je, m):      # m exons inside the junction: 3 items each (exon, donor, acceptor)
    assert 100 + 60 * m < je - js
    return [(js - 300, js - 200)] + [(js + 100 + 60 * k, js + 130 + 60 * k) for k in range(m)] + [(je + 200, je + 300)]


def one_item(js, je):      # its last exon starts inside the junction: one skipped acceptor ('+') / donor ('-')
    return [(js - 300, js - 200), (js + 50, je + 300)]


def outside(js, je):       # same bin, left of the junction: returns before its loop
    return [(js - 900, js - 800), (js - 700, js - 600)]


def single_start(js, je):  # one exon that ends at the junction's start: takes part only with keep_single
    return [(js - 300, js)]


SHAPES = dict(span=span, known=known, at_start=at_start, at_end=at_end, one_item=one_item, outside=outside, single_start=single_start)


class Case:
    pass


class AnnBuilder:
    def __init__(self, name, layout):
        self.name, self.layout = name, layout
        self.contigs, self.cand = contig_layout(layout)
        self.txs = [dict(id="F%03d" % i, contig=c, strand="+", exons=[(1000, 1100), (1200, 1300)]) for i, c in enumerate(self.contigs)]
        self.junctions = []                  # (contig index, start, end1, strand)
        self.claims = dict(totals={}, setter={}, levels={})

    def add(self, tid, contig, strand, exons):
        self.txs.append(dict(id=tid, contig=contig, strand=strand, exons=list(exons)))

    def junction(self, contig, js, je, strand):
        self.junctions.append((self.contigs.index(contig) if contig is not None else -1, js, je, strand))
        return len(self.junctions) - 1

    def locus(self, tag, k, spec, strands="+-"):
        """spec: [(strand, shape name or ('inner', m))] in id order, all in the level-0 bin k of the k-th locus' contig; one junction per strand"""
        contig = self.cand[k % 3]
        js, je = BIN * (1 + k // 3) + 2000, BIN * (1 + k // 3) + 6000
        for i, (sd, shape) in enumerate(spec):
            ex = inner(js, je, shape[1]) if isinstance(shape, tuple) else SHAPES[shape](js, je)
            self.add("%s%02d_%04d" % (tag, k, i), contig, sd, ex)
        return [self.junction(contig, js, je, sd) for sd in strands]

    def finish(self, outdir, fasta=False):
        c = Case()
        c.name, c.layout, c.contigs, c.transcripts, c.claims = self.name, self.layout, self.contigs, self.txs, self.claims
        j = self.junctions
        c.j_contig = np.array([x[0] for x in j], dtype=np.int32)
        c.j_start = np.array([x[1] for x in j], dtype=np.uint32)
        c.j_end1 = np.array([x[2] for x in j], dtype=np.uint32)
        c.j_strand = "".join(x[3] for x in j)
        os.makedirs(str(outdir), exist_ok=True)
        pre = os.path.join(str(outdir), "%s_%s" % (self.name, self.layout))
        c.gtf = pre + ".gtf"
        lines = []
        for cn in self.contigs:                              # contig by contig, so that first-seen order is the layout's
            for t in self.txs:
                if t["contig"] != cn:
                    continue
                for n, (s, e) in enumerate(t["exons"]):
                    lines.append("\t".join([cn, "edge", "exon", str(s), str(e), ".", t["strand"], ".",
                                            'gene_id "G_%s"; gene_name "N_%s"; transcript_id "%s"; exon_number "%d";' % (t["id"], t["id"], t["id"], n + 1)]))
        with open(c.gtf, "w") as f:
            f.write("\n".join(lines) + "\n")
        c.gtf_lines = len(lines)
        c.digest = hashlib.sha256(("\n".join(lines) + "|" + ",".join("%d:%d:%d:%s" % x for x in j)).encode()).hexdigest()
        c.fasta = c.bed = None
        top = max(e for t in self.txs for _, e in t["exons"])
        if fasta and top <= 200_000:
            # `junctions annotate` reads the two splice-site dinucleotides of every junction: a FASTA of fixed bases is enough (the motif column is not compared)
            c.fasta = pre + ".fa"
            with open(c.fasta, "w") as f, open(c.fasta + ".fai", "w") as fi:
                off = 0
                for cn in self.contigs:
                    length = 200_000 if cn in self.cand else 2_000
                    hdr = ">%s\n" % cn
                    f.write(hdr)
                    off += len(hdr)
                    fi.write("%s\t%d\t%d\t50\t51\n" % (cn, length, off))
                    f.write(("ACGTTGCAAC" * 5 + "\n") * (length // 50))
                    off += length + length // 50
            c.bed = pre + ".bed"
            with open(c.bed, "w") as f:                      # adjust_junction_ends: start += block 1, end -= block 2 - 1
                for n, (ci, js, je, sd) in enumerate(j):
                    if ci >= 0:
                        f.write("%s\t%d\t%d\tJ%05d\t1\t%s\t%d\t%d\t255,0,0\t2\t10,10\t0,%d\n" % (self.contigs[ci], js - 10, je + 9, n, sd, js - 10, je + 9, je - 1 - (js - 10)))
        return c


def _mixed(i):
    """what stands at candidate index i of a filler stretch: two of three on '+', the shapes in turn"""
    return ("-" if i % 3 == 1 else "+"), ["span", ("inner", 2), "one_item", "outside", "span"][i % 5]


def _flip(sd):
    return "-" if sd == "+" else "+"


def j_totals(outdir, layout):
    """Candidate totals (bin-table entries over the seven ranges, both strands: a third of the lanes of a turn are idle) of exactly 0, 1, 63, 64, 65,
    127, 128, 129 and 200; a known junction of either strand half way, so that what is visited before is not listed and what comes after is."""
    b = AnnBuilder("J_totals", layout)
    for k, total in enumerate([0, 1, 63, 64, 65, 127, 128, 129, 200]):
        spec = [_mixed(i) for i in range(total)]
        if total == 1:
            spec[0] = ("+", "known")
        elif total:
            spec[total // 2], spec[total // 2 + 1] = ("+", "known"), ("-", "known")
        for jn in b.locus("T", k, spec):
            b.claims["totals"][jn] = total
    return b.finish(outdir, fasta=True)


SETTER_AT = [0, 62, 63, 64, 65, 127, 128]


def j_setter(outdir, layout, kind):
    """The only transcript that sets a flag sits at candidate index 0, 62, 63, 64, 65, 127 or 128: everything before it reaches its loop (or is idle:
    other strand, outside) and is not listed, everything from it on is.  kind: the junction itself, its donor alone, its acceptor alone; per strand."""
    b = AnnBuilder("J_setter_" + kind, layout)
    k = 0
    for sd in "+-":
        shape = "known" if kind == "known" else ("at_start" if (kind == "donor") == (sd == "+") else "at_end")
        for p in SETTER_AT:
            spec = []
            for i in range(p):
                o, sh = _mixed(i)
                spec.append((o if sd == "+" else _flip(o), sh))
            spec.append((sd, shape))
            spec += [(sd, "span"), (sd, ("inner", 2)), (_flip(sd), "span"), (sd, "one_item")]
            jn = b.locus("S", k, spec, strands=sd)[0]
            b.claims["totals"][jn] = p + 5
            b.claims["setter"][jn] = p
            k += 1
    return b.finish(outdir, fasta=True)


def j_items(outdir, layout):
    """Item counts per transcript of 0, 1, 3 and many, laid so that a junction's items straddle the turns of 64: a listed stretch behind a known
    junction at index 0 (locus 0), a stretch in which nothing is listed (locus 1: the last transcript of the first turn has 21 items, the first of the
    second returns before its loop; a single exon at index 10 that sets a flag only with keep_single), the same on the other strand (2, 3).
    129 junctions over these loci, with a '?' strand and a contig of -1 inside the first workgroup of four and near the end."""
    b = AnnBuilder("J_items", layout)
    jn = []
    for k in range(4):
        sd = "+" if k < 2 else "-"
        spec = []
        for i in range(132):
            o, sh = ("+", [("inner", 3), "one_item", "span", ("inner", 5)][i % 4]) if i % 5 else ("-", ("inner", 2))
            spec.append((o if sd == "+" else _flip(o), sh))
        spec[63], spec[64], spec[127], spec[128] = (sd, ("inner", 7)), (sd, "outside" if k % 2 else "span"), (sd, ("inner", 20)), (sd, "one_item")
        if k % 2 == 0:
            spec[0] = (sd, "known")
        else:
            spec[10] = (sd, "single_start")
        jn += b.locus("I", k, spec)
        b.claims["totals"][jn[-2]] = b.claims["totals"][jn[-1]] = 132
    base = list(b.junctions)
    b.junctions = []
    for n in range(129):
        c, js, je, sd = base[(n * 3) % len(base)]
        if n in (1, 6, 126):
            sd = "?"
        if n in (2, 127):
            c = -1
        b.junctions.append((c, js, je, sd))
    b.claims["totals"] = {}
    for n, (c, js, je, sd) in enumerate(b.junctions):
        if c >= 0:
            b.claims["totals"][n] = 132
    return b.finish(outdir, fasta=True)


def _geometry(b):
    """the bin geometry both annotation scans walk: transcripts filed at each of the levels 0 to 6, each crossing the border that puts it there"""
    hi, lo = b.cand[0], b.cand[1]
    border = {1: X29 + 3 * (1 << 14), 2: X29 + 3 * (1 << 17), 3: X29 + 3 * (1 << 20), 4: X29 + 3 * (1 << 23), 5: X29 + (1 << 26), 6: X29}
    b.border = border
    for lvl, bd in border.items():
        for sd, tag in (("+", "p"), ("-", "m")):
            b.add("G_L%d_known_%s" % (lvl, tag), hi, sd, [(bd - 500, bd - 300), (bd + 300, bd + 500)])
            b.claims["levels"]["G_L%d_known_%s" % (lvl, tag)] = lvl
            b.add("G_L%d_after_%s" % (lvl, tag), hi, sd, [(bd + 100, bd + 200), (bd + 250, bd + 290)])
            b.add("G_L%d_before_%s" % (lvl, tag), hi, sd, [(bd - 290, bd - 250), (bd - 200, bd - 100)])
            b.claims["levels"]["G_L%d_after_%s" % (lvl, tag)] = b.claims["levels"]["G_L%d_before_%s" % (lvl, tag)] = 0
    for sd, tag in (("+", "p"), ("-", "m")):
        b.add("A_span6_" + tag, hi, sd, [(X29 - 2000, X29 - 1900), (X29 + (1 << 26) + 5000, X29 + (1 << 26) + 5100)])
        b.add("A_span5_" + tag, hi, sd, [(border[5] - 3000, border[5] - 2900), (border[5] + 3000, border[5] + 3100)])
        b.claims["levels"]["A_span6_" + tag], b.claims["levels"]["A_span5_" + tag] = 6, 5


def j_geometry(outdir, layout):
    """Junctions on the borders of every bin level (the known junction is filed one level per border coarser and is visited after the level-0
    transcripts of lower AND higher ids, a level-6 transcript of the lowest id last of all); a start on a multiple of 16,384 (the bin before is not
    walked, though a transcript in it ends on the junction's start); end1 - 1 one short of, on and one past a multiple; junctions over 2 and 9
    level-0 bins (two level-1 bins); a flag-setter of the lowest id filed at level 1 behind level-0 transcripts; a contig that is not the first;
    requested bins at and beyond the direct index's stride."""
    b = AnnBuilder("J_geometry", layout)
    _geometry(b)
    hi, lo = b.cand[0], b.cand[1]
    for lvl, bd in b.border.items():
        for sd in "+-":
            b.junction(hi, bd - 300, bd + 300, sd)
    # start on a multiple of 16,384
    js = BIN * 10
    b.add("S_prev", lo, "+", [(js - 300, js - 200), (js - 100, js)])
    b.add("S_here", lo, "+", [(js + 10, js + 20), (js + 3000, js + 3300)])
    b.claims["levels"]["S_prev"] = b.claims["levels"]["S_here"] = 0
    b.junction(lo, js, js + 3000, "+")
    # end1 - 1 around a multiple of 16,384
    m = BIN * 20
    b.add("E_m0", lo, "+", [(m, m + 100), (m + 200, m + 300)])
    b.add("E_m1", lo, "+", [(m + 1, m + 90), (m + 210, m + 310)])
    b.add("E_m2", lo, "+", [(m + 2, m + 80), (m + 220, m + 320)])
    b.add("E_in", lo, "+", [(m - 3300, m - 3000), (m - 2500, m - 2400)])
    for je in (m, m + 1, m + 2):
        b.junction(lo, m - 3000, je, "+")
    # 2 and 9 level-0 bins from bin 52 (level-1 bins 6 and 7)
    k0 = 52
    for q in range(k0, k0 + 9):
        for sd in "+-":
            b.add("R_%02d_%s" % (q, "p" if sd == "+" else "m"), lo, sd, [(BIN * q + 9000, BIN * q + 9100), (BIN * q + 9200, BIN * q + 9300)])
    js, je2, je9 = BIN * k0 + 8000, BIN * (k0 + 1) + 9150, BIN * (k0 + 8) + 9150
    for sd, tag in (("+", "p"), ("-", "m")):
        b.add("R_l1a_" + tag, lo, sd, [(BIN * 53 - 500, BIN * 53 - 400), (BIN * 53 + 400, BIN * 53 + 500)])
        b.add("R_l1b_" + tag, lo, sd, [(BIN * 59 - 500, BIN * 59 - 400), (BIN * 59 + 400, BIN * 59 + 500)])
        b.add("R_known9_" + tag, lo, sd, [(js - 300, js), (je9, je9 + 300)])
        b.claims["levels"]["R_l1a_" + tag] = b.claims["levels"]["R_l1b_" + tag] = 1
        b.claims["levels"]["R_known9_" + tag] = 2
        b.junction(lo, js, je2, sd)
        b.junction(lo, js, je9, sd)
    # the flag-setter has the lowest id and is filed at level 1
    bd = BIN * 30
    js, je = bd + 1000, bd + 3000
    b.add("C_000", lo, "+", [(bd - 200, js), (je, je + 300)])
    for i in range(1, 6):
        b.add("C_%03d" % i, lo, "+", span(js, je))
    b.add("C_006", lo, "+", [(bd - 250, bd - 220), (je + 200, je + 300)])
    b.claims["levels"]["C_000"] = b.claims["levels"]["C_006"] = 1
    b.claims["levels"]["C_001"] = 0
    jn = b.junction(lo, js, je, "+")
    b.claims["totals"][jn], b.claims["setter"][jn] = 9, 5      # (5 at level 0, C_000 and C_006 at level 1, the two R_known9 at level 2)
    # bins at and beyond the stride (the largest bin any transcript has is A_span6's): all of them, then only the far end of the range
    b.junction(lo, X29 + (1 << 28), X29 + (1 << 28) + 5000, "+")
    b.junction(hi, X29 + (1 << 26) + 4000, X29 + (1 << 26) + 4000 + 5 * BIN, "+")
    b.junction(hi, X29 + (1 << 26) + 4000, X29 + (1 << 26) + 4000 + 5 * BIN, "-")
    # a third contig: the last one of the layout
    js, je = BIN * 3 + 2000, BIN * 3 + 6000
    b.add("Z_known", b.cand[2], "-", known(js, je))
    b.add("Z_span", b.cand[2], "-", span(js, je))
    b.junction(b.cand[2], js, je, "-")
    b.junction(b.cand[2], js, je, "+")
    return b.finish(outdir)


JUNCTION_CASES = {"J_totals": j_totals, "J_setter_known": lambda o, l: j_setter(o, l, "known"), "J_setter_donor": lambda o, l: j_setter(o, l, "donor"),
                  "J_setter_acceptor": lambda o, l: j_setter(o, l, "acceptor"), "J_items": j_items, "J_geometry": j_geometry}


# ---- variants ---------------------------------------------------------------------------------------------------------------------------------
VARIANT_OPTS = [dict(intronic_min=i, exonic_min=e, all_intronic=ai, all_exonic=ae, skip_single=ss)
                for (i, e) in ((0, 0), (2, 3), (50, 50)) for (ai, ae) in ((0, 0), (1, 0), (0, 1)) for ss in (1, 0)]


def v_edges(outdir, layout):
    """Positions on both sides of every exon edge +- 0, 1, 2, 3, 4, 49, 50, 51 (first, inner and last exons of a '+' and a '-' transcript with an
    exon of 40 and an intron of 60 among them, a single-exon transcript), the seven-level transcripts of the junction geometry, positions below
    intronic_min (the bin range wraps: only level 6 is walked), position +- intronic_min astride a 16 KiB border, a position that 70 transcripts hit,
    positions nothing is near, an unknown contig."""
    b = AnnBuilder("V_edges", layout)
    _geometry(b)
    hi, lo = b.cand[0], b.cand[1]
    var = []                                         # (contig name, 1-based position)
    deltas = [0, 1, 2, 3, 4, 49, 50, 51]
    base = BIN * 5 + 3000
    exons = [(base, base + 200), (base + 500, base + 540), (base + 600, base + 800), (base + 1100, base + 1300)]
    b.add("V_plus", lo, "+", exons)
    b.add("V_minus", lo, "-", [(s + 4000, e + 4000) for s, e in exons])
    b.add("V_single", lo, "+", [(base + 9000, base + 9200)])
    for off in (0, 4000):
        for s, e in exons:
            for x in (s + off, e + off):
                for d in deltas:
                    var += [(lo, x + d), (lo, x - d)]
    for d in deltas:
        var += [(lo, base + 9000 + d), (lo, base + 9000 - d), (lo, base + 9200 + d), (lo, base + 9200 - d)]
    for lvl, bd in b.border.items():
        var += [(hi, bd - 300), (hi, bd - 299), (hi, bd + 300), (hi, bd + 298), (hi, bd), (hi, bd - 501)]
    # below intronic_min: W_low is filed at level 0 and not walked once the subtraction wraps; W_six starts at 1 and is filed at level 6
    b.add("W_low", lo, "+", [(1, 100), (200, 300)])
    b.add("W_six", hi, "+", [(1, 50), (X29 + 100, X29 + 200)])
    var += [(lo, 1), (lo, 2), (lo, 3), (lo, 11), (lo, 51), (lo, 52), (hi, 1), (hi, 2), (hi, 50), (hi, 51), (hi, 52)]
    # astride a 16 KiB border: B_after lives in the bin behind the border alone and starts on it, B_before in the bin in front and ends on it
    bd = BIN * 40
    b.add("B_after", lo, "+", [(bd, bd + 2), (bd + 300, bd + 400)])
    b.add("B_before", lo, "-", [(bd - 400, bd - 300), (bd - 2, bd)])
    b.claims["levels"]["B_after"] = b.claims["levels"]["B_before"] = 0
    for d in (-51, -50, -3, -2, -1, 0, 1, 2, 3, 50, 51):
        var.append((lo, bd + d))
    # 70 hits
    m0 = BIN * 45 + 1000
    for i in range(70):
        b.add("M_%03d" % i, lo, "+-"[i % 2], [(m0, m0 + 200), (m0 + 500 + i, m0 + 700), (m0 + 1000, m0 + 1200)])
    var += [(lo, m0 + 200), (lo, m0 + 201), (lo, m0 + 499), (lo, m0 + 700), (lo, m0 + 5000), (lo, BIN * 70 + 5)]
    var += [("nope", 1000), ("nope", m0 + 200)]
    c = b.finish(outdir)
    c.v_contig = [v[0] for v in var]
    c.v_pos0 = np.array([v[1] - 1 for v in var], dtype=np.uint32)
    c.vcf = c.gtf[:-4] + ".vcf"
    with open(c.vcf, "w") as f:
        f.write("##fileformat=VCFv4.1\n")
        for cn in c.contigs + ["nope"]:
            f.write("##contig=<ID=%s,length=%d>\n" % (cn, 1 << 30))
        f.write("#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\n")
        for cn, p in var:
            f.write("%s\t%d\t.\tA\tC\t50\tPASS\t.\n" % (cn, p))
    c.digest = hashlib.sha256((c.digest + "|" + ",".join("%s:%d" % v for v in var)).encode()).hexdigest()
    return c


# ---- window pairs -----------------------------------------------------------------------------------------------------------------------------
P0 = 100_000
DENSE = 8300
WINDOW_CANDIDATES = [0, 1, 2, 3, 4, 5, 63, 64, 65, 255, 256, 257, 4095, 4096, 4097, 8197]


def window_events():
    """tid 0: a few short reads from position 0 on and THE long read (span 20,000); tid 1: 8,300 reads, one per position from 100,000, the even ones
    1 to 3 bases long, the odd ones 9,000; tid 2: the reads of the edge compares; tid 3: none; tid 4: the last reads of the list"""
    tid = [0] * 40 + [0] + [1] * DENSE + [2, 2, 2] + [4] * 5
    rpos = list(range(0, 80, 2)) + [30_000] + [P0 + i for i in range(DENSE)] + [1000, 1000, 5000] + [700 + i for i in range(5)]
    rend = [p + 30 for p in range(0, 80, 2)] + [50_000] + [P0 + i + (9000 if i % 2 else 1 + i % 3) for i in range(DENSE)] + [2000, 2001, 5010] + \
           [800 + i for i in range(5)]
    return np.array(tid, dtype=np.uint32), np.array(rpos, dtype=np.uint32), np.array(rend, dtype=np.uint32)


def w_sizes():
    """windows with exactly 0 .. 8197 candidates (candidates = events of the contig from beg - longest span, clamped to 0, up to end): in the large
    ones half of the candidates end in front of beg; the edge compares; the clamp; contigs without events; a window twice; an empty window first"""
    c = Case()
    c.name = "W_sizes"
    c.tid, c.rpos, c.rend = window_events()
    w = [(1, P0 - 10, P0)]                                        # no candidate, first in its batch
    c.claims = dict(candidates={})
    for n in WINDOW_CANDIDATES:
        c.claims["candidates"][len(w)] = n
        w.append((1, max(P0 + n - 50, 0), P0 + n))
    w += [(2, 2000, 3000), (2, 1999, 3000), (2, 1999, 2000), (2, 500, 1001), (2, 500, 1000), (2, 2001, 2002), (2, 2000, 2001)]
    w += [(0, 0, 50), (0, 0, 1), (0, 100, 200), (0, 19_999, 30_001), (0, 49_999, 50_000), (0, 50_000, 50_001)]
    w += [(3, 0, 1_000_000), (5, 0, 1_000_000), (4, 0, 1_000_000), (4, 702, 703), (-1, 0, 1000)]
    w += [(1, P0 + 100, P0 + 120), (1, P0 + 100, P0 + 120), (1, P0 + 8299, P0 + 8300), (1, P0 + 8300, P0 + 8400), (1, P0 + 17_000, P0 + 17_300)]
    c.w_tid, c.w_beg, c.w_end = (np.array([x[k] for x in w], dtype=np.int32) for k in range(3))
    return c


def w_300():
    """300 overlapping windows over the dense stretch: more than the large kernel's grid of 256, with windows of more than 4096 candidates at the
    indexes 0, 255, 256 and 299 and small ones between"""
    c = Case()
    c.name = "W_300"
    c.tid, c.rpos, c.rend = window_events()
    big = {0: 4500, 255: 5000, 256: 6000, 299: 8197}
    w = []
    for i in range(300):
        n = big.get(i, 1 + (i * 37) % 900)
        w.append((1, P0 + n - 20, P0 + n))
    c.claims = dict(candidates={i: big.get(i, 1 + (i * 37) % 900) for i in range(300)}, big=sorted(big))
    c.w_tid, c.w_beg, c.w_end = (np.array([x[k] for x in w], dtype=np.int32) for k in range(3))
    return c


def w_span():
    """270,000 events (k_max_span strides its grid from 262,144 on); the longest read is event 265,000, and one window only it reaches into"""
    c = Case()
    c.name = "W_span"
    n, at = 270_000, 265_000
    c.tid = np.zeros(n, dtype=np.uint32)
    c.rpos = (1000 + np.arange(n)).astype(np.uint32)
    c.rend = c.rpos + 5
    c.rend[at] = c.rpos[at] + 50_000
    p = int(c.rpos[at])
    w = [(0, p + 40_000, p + 40_010), (0, p - 3, p + 1), (0, 1000, 1001), (0, p + 50_000, p + 50_001), (0, p + 49_999, p + 50_000)]
    c.claims = dict(longest=at, only_longest=[0, 4])
    c.w_tid, c.w_beg, c.w_end = (np.array([x[k] for x in w], dtype=np.int32) for k in range(3))
    return c


WINDOW_CASES = {"W_sizes": w_sizes, "W_300": w_300, "W_span": w_span}
PAIR_BATCHES = [0, 5000, 1000, 1]            # the product's (one batch), several windows a batch, large windows alone, every non-empty window alone


# ---- assoc pairs ------------------------------------------------------------------------------------------------------------------------------
BUCKETS = [0, 1, 63, 64, 65, 129]


def assoc_case(n_windows):
    """contig buckets of 0, 1, 63, 64, 65 and 129 junctions (the last contig's is the largest); windows on every contig and on -1, with ces > cee
    (0xffffffff, 0: a variant nothing hit), with a junction's start or end ON ces and ON cee, inside a junction that covers them; 1 or 1000 windows"""
    c = Case()
    c.name = "A_%d" % n_windows
    rng = np.random.RandomState(7)
    off = np.concatenate([[0], np.cumsum(BUCKETS)]).astype(np.uint32)
    n = int(off[-1])
    c.j_start = rng.randint(1000, 50_000, n).astype(np.uint32)
    c.j_end = (c.j_start + rng.randint(1, 3000, n)).astype(np.uint32)
    c.contig_off = off
    w = []
    last = len(BUCKETS) - 1
    j = int(off[last]) + 64                                       # a junction of the last bucket's second trip
    s, e = int(c.j_start[j]), int(c.j_end[j])
    w += [(last, s, s), (last, s + 1, s + 1), (last, s - 1, s - 1), (last, e, e), (last, e + 1, e + 1), (last, e - 1, e - 1), (last, s - 5, s), (last, s, s + 5),
          (last, e - 5, e), (last, e, e + 5), (last, 0xffffffff, 0), (-1, 0, 0xffffffff), (0, 0, 0xffffffff), (1, 0, 0xffffffff), (last, 0, 0xffffffff)]
    c.j_start[int(off[2])], c.j_end[int(off[2])] = 100, 900       # covers [200, 800] without an end inside
    w += [(2, 200, 800), (2, 100, 100), (2, 900, 900), (2, 101, 899)]
    while len(w) < n_windows:
        k = len(w)
        a = int(rng.randint(0, 52_000))
        w.append(((k % 7) - 1, a, a + int(rng.randint(0, 4000))) if k % 11 else ((k % 7) - 1, 0xffffffff, 0))
    w = w[:n_windows] if n_windows >= 19 else [w[6]]
    c.w_contig = np.array([x[0] for x in w], dtype=np.int32)
    c.w_ces = np.array([x[1] for x in w], dtype=np.uint32)
    c.w_cee = np.array([x[2] for x in w], dtype=np.uint32)
    return c


_built = {}


def build(name, outdir, layout="direct"):
    """a case by name, built once per (name, layout, directory)"""
    key = (name, layout, str(outdir))
    if key not in _built:
        if name in JUNCTION_CASES:
            _built[key] = JUNCTION_CASES[name](outdir, layout)
        elif name == "V_edges":
            _built[key] = v_edges(outdir, layout)
        elif name in WINDOW_CASES:
            _built[key] = WINDOW_CASES[name]()
        else:
            _built[key] = assoc_case(int(name.split("_")[1]))
    return _built[key]
