"""Plain Python / numpy references of the four interval operations behind `cis-splice-effects identify`, `associate`, `junctions annotate` and
`variants annotate` (TEST INFRASTRUCTURE), written from SURVEY.md 9.6 (quirks 4, 6-10, 14, 16) and the upstream functions it cites --
JunctionsAnnotator::overlap_ps / overlap_ns / annotate_junction_with_gtf (junctions_annotator.cc:128-363), VariantsAnnotator::
get_variant_overlaps_spliceregion_* / set_variant_cis_effect_limits_* / annotate_record_with_transcripts (variants_annotator.cc:169-518), getBin
(bedFile.h:339-354), hts_itr's overlap test (hts.c:1946-1957) and the associator's keep test (cis_splice_effects_associator.cc:261-272).  They share no
code and no shape with regtools_amd/csrc/cse_core.h: the annotation is a dictionary (contig, bin) -> transcripts, a transcript against a junction is
a handful of numpy masks over its exons, a transcript against a variant is a table of rules read top to bottom, the two joins are their definitions.

An annotation is made from the transcripts a case builder planted, never from the GTF text: [{"id", "contig", "strand", "exons": [(start, end), ...]}]
with 1-based inclusive coordinates as a GTF writes them, and the contig names in first-seen order.  Transcript numbers are ranks of the ids in byte
order (upstream keeps them in a std::map)."""
import bisect

import numpy as np

M32 = 0xffffffff
OFFSETS = (32678 + 4096 + 512 + 64 + 8 + 1, 4681, 585, 73, 9, 1, 0)          # bedFile.h:59, the 32678 typo included
ITEM_TX, ITEM_EXON, ITEM_DONOR, ITEM_ACCEPTOR = 0, 1, 2, 3
ANN_EXONIC, ANN_INTRONIC, ANN_SPL_EXONIC, ANN_SPL_INTRONIC = 1, 2, 3, 4


def level_and_bin(start, end):
    """getBin(start, end): (level, bin id); the shifted pair is only tested for equality, so start > end is accepted"""
    a, b = (start & M32) >> 14, ((end - 1) & M32) >> 14
    for lvl in range(7):
        if a == b:
            return lvl, OFFSETS[lvl] + a
        a >>= 3
        b >>= 3
    return 7, 0


class Annotation:
    def __init__(self, transcripts, contigs):
        self.contigs = list(contigs)
        self.contig_index = {c: i for i, c in enumerate(self.contigs)}
        txs = sorted(transcripts, key=lambda t: t["id"].encode())
        assert len({t["id"] for t in txs}) == len(txs)
        self.ids = [t["id"] for t in txs]
        self.strand = [t["strand"] for t in txs]
        self.s, self.e, self.level, self.bin = [], [], [], []
        self.table = {}                                  # (contig index, bin id) -> transcript numbers, ascending
        for k, t in enumerate(txs):
            ex = sorted(t["exons"], key=lambda x: x[0], reverse=t["strand"] == "-")      # sort_exons_within_transcripts (stable; starts are distinct here)
            self.s.append(np.array([x[0] for x in ex], dtype=np.int64))
            self.e.append(np.array([x[1] for x in ex], dtype=np.int64))
            lvl, b = level_and_bin(ex[0][0], ex[-1][1])                                  # gtf_parser.cc:154-160
            self.level.append(lvl)
            self.bin.append(b)
            self.table.setdefault((self.contig_index[t["contig"]], b), []).append(k)
        self.occupied = {}                               # contig index -> its occupied bin ids, ascending
        for (c, b) in sorted(self.table):
            self.occupied.setdefault(c, []).append(b)

    def walk(self, contig, first_bin, last_bin):
        """transcripts in visiting order: level fine to coarse, bin ascending, transcript id ascending; first_bin > last_bin: a level without bins"""
        occ = self.occupied.get(contig, [])
        a, b = first_bin & M32, last_bin & M32
        for lvl in range(7):
            if a <= b:
                lo, hi = bisect.bisect_left(occ, a + OFFSETS[lvl]), bisect.bisect_right(occ, b + OFFSETS[lvl])
                for q in occ[lo:hi]:
                    for t in self.table[(contig, q)]:
                        yield t
            a >>= 3
            b >>= 3


# ---- junctions -------------------------------------------------------------------------------------------------------------------------------
def _transcript_vs_junction(s, e, strand, js, je, keep_single):
    """None when the transcript returns before its exon loop (:131, :135-137 / :231, :235-238), else (own flags, items in writing order)"""
    n = len(s)
    if n == 1 and not keep_single:
        return None
    plus = strand == "+"
    if (s[0] > je or e[-1] < js) if plus else (e[0] < js or s[-1] > je):
        return None
    idx = np.arange(n)
    beyond = (s > je) if plus else (e < js)                       # "the rest of the exons are outside the junction": the loop ends at the first
    inside = idx < (int(np.argmax(beyond)) if beyond.any() else n)
    if plus:
        nxt = np.append(s[1:], -1)
        known = inside & (e == js) & (nxt == je)                  # (exons[i + 1] behind the last exon: "no match")
        reaches = e >= js
    else:
        nxt = np.append(e[1:], -1)
        known = inside & (s == je) & (nxt == js)
        reaches = s <= je
    rest = inside & ~known
    hit = rest & reaches
    active = rest & (idx >= int(np.argmax(hit))) if hit.any() else np.zeros(n, dtype=bool)
    interior = (idx > 0) & (idx < n - 1)
    skipped = active & (s > js) & (e < je) & interior
    end_in = active & (e > js) & (e < je) & (idx < n - 1)
    start_in = active & (s > js) & (s < je) & ((idx > 0) if plus else True)
    at_start, at_end = bool((active & (e == js)).any()), bool((active & (s == je)).any())
    flags = 7 if known.any() else 0
    if plus:
        flags |= (1 if at_start else 0) | (2 if at_end else 0)    # exon.end == junction.start: known donor; exon.start == junction.end: known acceptor
        end_kind, start_kind = ITEM_DONOR, ITEM_ACCEPTOR
    else:
        flags |= (2 if at_start else 0) | (1 if at_end else 0)
        end_kind, start_kind = ITEM_ACCEPTOR, ITEM_DONOR
    items = []
    for i in np.nonzero(skipped | end_in | start_in)[0]:
        if skipped[i]:
            items.append((ITEM_EXON, int(s[i]), int(e[i])))
        if end_in[i]:
            items.append((end_kind, int(e[i]), 0))
        if start_in[i]:
            items.append((start_kind, int(s[i]), 0))
    return flags, items


def junction_scan(ann, contig, start, end1, strand, keep_single=False):
    """per junction (contig index or -1, start, end1 = Junction.end + 1, strand character): flags, exon records of the same-strand candidates, and
    the raw item list -- a transcript's skipped elements, then the transcript itself when its loop ran and a flag is set by then"""
    flags, visits, off, items = [], [], [0], []
    for c, js, je, sd in zip(contig, start, end1, strand):
        f, v = 0, 0
        if c >= 0 and sd in "+-":                                 # '?' matches no transcript (9.6-14)
            for t in ann.walk(int(c), (int(js) & M32) >> 14, ((int(je) - 1) & M32) >> 14):
                if ann.strand[t] != sd:
                    continue
                v += len(ann.s[t])
                r = _transcript_vs_junction(ann.s[t], ann.e[t], sd, int(js), int(je), keep_single)
                if r is None:
                    continue
                f |= r[0]
                items.extend(r[1])
                if f:
                    items.append((ITEM_TX, t, 0))
        flags.append(f)
        visits.append(v)
        off.append(len(items))
    it = np.array(items, dtype=np.uint32).reshape(-1, 3)
    return dict(flags=np.array(flags, dtype=np.uint32), visits=np.array(visits, dtype=np.uint32), off=np.array(off, dtype=np.uint32),
                kind=it[:, 0].copy(), a=it[:, 1].copy(), b=it[:, 2].copy())


def unique_counts(r, i):
    """(acceptors, exons, donors skipped, sorted transcript numbers) of junction i as upstream's sets leave them"""
    k = slice(int(r["off"][i]), int(r["off"][i + 1]))
    kind, a, b = r["kind"][k], r["a"][k], r["b"][k]
    return (len(set(a[kind == ITEM_ACCEPTOR].tolist())), len(set(zip(a[kind == ITEM_EXON].tolist(), b[kind == ITEM_EXON].tolist()))),
            len(set(a[kind == ITEM_DONOR].tolist())), sorted(set(a[kind == ITEM_TX].tolist())))


# ---- variants ---------------------------------------------------------------------------------------------------------------------------------
def _transcript_vs_variant(s, e, strand, v, I, E, all_intronic, all_exonic):
    """(annotation, distance, exon index) or None; v = the variant's 1-based position; every sum and difference is a uint32, as upstream"""
    n = len(s)
    plus = strand == "+"
    if (s[0] > v or e[-1] < v) if plus else (s[-1] > v or e[0] < v):
        return None
    u = lambda x: int(x) & M32
    for i in range(n):
        si, ei = int(s[i]), int(e[i])
        first, last = i == 0, i == n - 1
        in_exon = si <= v <= ei
        d_exon = min(u(v - si), u(ei - v))
        # the neighbouring exon across the intron at this exon's 3' side (towards higher indexes) and at its 5' side
        if plus:
            gap3 = None if last else (ei, int(s[i + 1]))          # intron (exon end, next start), genomic order
            gap5 = None if first else (int(e[i - 1]), si)
        else:
            gap3 = None if last else (int(e[i + 1]), si)
            gap5 = None if first else (ei, int(s[i - 1]))
        in_gap = lambda g: g is not None and g[0] < v < g[1]
        d_gap = lambda g: min(u(v - g[0]), u(g[1] - v))
        if all_exonic and in_exon:
            return ANN_EXONIC, d_exon, i
        if all_intronic and in_gap(gap3):
            return ANN_INTRONIC, d_gap(gap3), i
        if (u(si - I) > v) if plus else (u(ei + I) < v):          # "the rest of the exons are outside"
            return None
        # genomic left edge of the exon (its start) and right edge (its end); which one needs a neighbour depends on the strand
        left_gap, right_gap = (gap5, gap3) if plus else (gap3, gap5)
        rules = [
            (left_gap is not None and in_exon and v <= u(si + E), ANN_SPL_EXONIC, d_exon),
            (v < si and v >= u(si - I) and in_gap(left_gap), ANN_SPL_INTRONIC, d_gap(left_gap) if left_gap else 0),
            (right_gap is not None and in_exon and v >= u(ei - E), ANN_SPL_EXONIC, d_exon),
            (v > ei and v <= u(ei + I) and in_gap(right_gap), ANN_SPL_INTRONIC, d_gap(right_gap) if right_gap else 0),
        ]
        for ok, ann, dist in rules:
            if ok:
                return ann, dist, i
    return None


def variant_scan(ann, contig, pos0, intronic_min=2, exonic_min=3, all_intronic=False, all_exonic=False, skip_single=True):
    """per variant (contig index or -1, 0-based position): cis window (0xffffffff, 0 when nothing hit), exon records of the candidates looked at,
    hits (transcript, annotation, distance) in visiting order"""
    ces, cee, visits, off, hits = [], [], [], [0], []
    for c, p in zip(contig, pos0):
        lo, hi, nv = M32, 0, 0
        if c >= 0:
            p = int(p)
            for t in ann.walk(int(c), ((p - intronic_min) & M32) >> 14, ((p + intronic_min) & M32) >> 14):
                s, e, n = ann.s[t], ann.e[t], len(ann.s[t])
                if skip_single and n == 1:
                    continue
                nv += n
                r = _transcript_vs_variant(s, e, ann.strand[t], (p + 1) & M32, intronic_min, exonic_min, all_intronic, all_exonic)
                if r is None:
                    continue
                kind, dist, i = r
                hits.append((t, kind, dist))
                # set_variant_cis_effect_limits_*: the neighbouring exons' far edges for a cassette exon, the intron's own edges for "intronic"
                if kind == ANN_INTRONIC:
                    a, b = sorted((i, i + 1), key=lambda q: s[q])
                    lo, hi = min(lo, int(e[a])), max(hi, int(s[b]))
                else:
                    order = np.argsort(s, kind="stable")                     # genomic order of the exons
                    g = int(np.nonzero(order == i)[0][0])
                    left, right = order[max(g - 1, 0)], order[min(g + 1, n - 1)]
                    lo, hi = min(lo, int(s[left])), max(hi, int(e[right]))
        ces.append(lo)
        cee.append(hi)
        visits.append(nv)
        off.append(len(hits))
    h = np.array(hits, dtype=np.uint32).reshape(-1, 3)
    return dict(ces=np.array(ces, dtype=np.uint32), cee=np.array(cee, dtype=np.uint32), visits=np.array(visits, dtype=np.uint32),
                off=np.array(off, dtype=np.uint32), tx=h[:, 0].copy(), ann=h[:, 1].copy(), dist=h[:, 2].copy())


# ---- the two joins ----------------------------------------------------------------------------------------------------------------------------
def window_pairs(tid, rpos, rend, w_tid, w_beg, w_end):
    """(event, window) for window w in order: the events, in file order, with tid == t, rpos < end, rend > beg (signed 32-bit, hts.c:1946-1957).
    By definition: neither a candidate range nor the longest span."""
    tid = np.asarray(tid, dtype=np.uint32)
    p, q = np.asarray(rpos, dtype=np.uint32).view(np.int32), np.asarray(rend, dtype=np.uint32).view(np.int32)
    ev, win, counts = [], [], []
    for w, (t, b, e) in enumerate(zip(w_tid, w_beg, w_end)):
        k = np.nonzero((tid == np.uint32(int(t) & M32)) & (p < np.int32(e)) & (q > np.int32(b)))[0]
        ev.append(k.astype(np.uint32))
        win.append(np.full(len(k), w, dtype=np.uint32))
        counts.append(len(k))
    cat = lambda v: np.concatenate(v) if v else np.zeros(0, dtype=np.uint32)
    return cat(ev), cat(win), counts


def pair_batches(counts, batch, n_events):
    """how many batches of whole windows hold at most `batch` pairs each (a window above it is a batch of its own)"""
    if not counts or not n_events:
        return 0
    n, w = 0, 0
    while w < len(counts):
        total = counts[w]
        w += 1
        while w < len(counts) and total + counts[w] <= batch:
            total += counts[w]
            w += 1
        n += 1
    return n


def assoc_pairs(w_contig, w_ces, w_cee, contig_off, j_start, j_end):
    """(junction, window) for window w in order: the junctions of its contig, in bucket order, whose start or end lies in [ces, cee]"""
    js, je = np.asarray(j_start, dtype=np.uint32), np.asarray(j_end, dtype=np.uint32)
    pj, pw = [], []
    for w, (c, a, b) in enumerate(zip(w_contig, w_ces, w_cee)):
        if c < 0:
            continue
        lo, hi = int(contig_off[c]), int(contig_off[c + 1])
        s, e = js[lo:hi], je[lo:hi]
        a, b = np.uint32(a), np.uint32(b)
        k = np.nonzero(((s >= a) & (s <= b)) | ((e >= a) & (e <= b)))[0] + lo
        pj.append(k.astype(np.uint32))
        pw.append(np.full(len(k), w, dtype=np.uint32))
    cat = lambda v: np.concatenate(v) if v else np.zeros(0, dtype=np.uint32)
    return cat(pj), cat(pw)
