"""The cohort junction-by-sample matrix on the device (csrc/cohort_kernels.hip, csrc/cohort.cpp): rows appended from a context's HBM or from an
uploaded table, one key-carrying sort, segmented reductions, the CSR image.  Expectations: the oracle's per-sample BED12 merged with a dict
(tests/cohort_common.py), the library's host twin, and a numpy.unique restatement.  Every comparison is exact."""
import os
import subprocess

import numpy as np
import pytest

import cohort_ref
from cohort_common import STRANDNESS, cohort_files, expected_texts, table_from_rows  # noqa: F401  (cohort_files is a fixture)

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "bin", "regtools-amd")


def _index_bytes(path):
    from regtools_amd import cohort
    return cohort._index_bytes(path)


def _extract(ctx, s):
    import regtools_amd
    je = regtools_amd.JunctionsExtractor(bam=s["path"], strandness=STRANDNESS[s["strand"]], ctx=ctx)
    je.identify_junctions_from_BAM()
    return je


def _items(samples):
    return [(s["path"], s["name"], dict(strandness=STRANDNESS[s["strand"]])) for s in samples]


def _same_matrix(a, b):
    assert (a.n, a.n_samples, a.n_triples, a.ref_name, a.ref_len, a.sample_name) == (b.n, b.n_samples, b.n_triples, b.ref_name, b.ref_len, b.sample_name)
    for k in ("tid", "start", "end", "thick_start", "thick_end", "strand", "n_with", "total", "row_begin", "col_sample", "val_count"):
        assert np.array_equal(getattr(a, k), getattr(b, k)), k


def test_sequential_adds_against_the_oracle_and_the_host_twin(gpu_ctx, cohort_files):  # noqa: F811
    import regtools_amd
    from regtools_amd import cohort
    bed, tsv, stats = expected_texts(cohort_files)
    assert stats["union"] > 10000 and max(stats["n_with_hist"]) >= 5
    names = [s["name"] for s in cohort_files]
    co = regtools_amd.Cohort(ctx=gpu_ctx)
    jes = []
    for s in cohort_files:
        jes.append(_extract(gpu_ctx, s))
        assert co.add(jes[-1], s["name"]) == len(jes) - 1          # (the next extraction on this context waits for the rows to be taken)
    assert co.add_paths == [1] * len(cohort_files)
    m = co.finish()
    assert (m.n, m.n_triples, m.n_samples) == (stats["union"], stats["rows_in"], len(cohort_files))
    assert m.bed12() == bed
    assert m.counts_tsv() == tsv
    d = m.dense()
    assert d.shape == (m.n, len(names)) and np.array_equal(d.sum(axis=1, dtype=np.uint64), m.total) and np.array_equal((d > 0).sum(axis=1), m.n_with)
    _same_matrix(m, cohort.merge_host(jes, names))
    for kw in (dict(min_samples=3), dict(min_samples=2, min_total=25)):
        cf = regtools_amd.Cohort(ctx=gpu_ctx, **kw)
        for je, nm in zip(jes, names):
            cf.add(je, nm)
        e_bed, e_tsv, _ = expected_texts(cohort_files, **kw)
        f = cf.finish()
        assert f.bed12() == e_bed and f.counts_tsv() == e_tsv
        cf.close()
    # every row, anchored or not: against the host twin over the same ten GPU tables (all but the last are no longer their context's last table)
    ca = regtools_amd.Cohort(ctx=gpu_ctx, only_anchored=False)
    for je, nm in zip(jes, names):
        ca.add(je, nm)
    assert ca.add_paths == [0] * (len(jes) - 1) + [1]
    a, h = ca.finish(), cohort.merge_host(jes, names, only_anchored=False)
    assert a.n_triples == sum(je.table.contents.n for je in jes) > m.n_triples and a.n > m.n
    assert a.bed12() == h.bed12() and a.counts_tsv() == h.counts_tsv()
    _same_matrix(a, h)
    co.close(); ca.close()


@pytest.mark.parametrize("depth", [1, 2])
def test_pipeline_run_takes_the_device_path(gpu_ctx, cohort_files, depth):  # noqa: F811
    import regtools_amd
    bed, tsv, _ = expected_texts(cohort_files)
    co = regtools_amd.Cohort(ctx=gpu_ctx)
    co.run(_items(cohort_files), depth=depth)
    assert co.add_paths == [1] * len(cohort_files)
    m = co.finish()
    assert m.bed12() == bed and m.counts_tsv() == tsv
    co.close()


def test_a_table_whose_context_has_moved_on_is_uploaded(gpu_ctx, cohort_files):  # noqa: F811
    import regtools_amd
    two = cohort_files[3:5]
    bed, tsv, _ = expected_texts(two)
    pl = regtools_amd.Pipeline(0, 1)
    try:
        jes = []
        for s in two:
            data, bai = open(s["path"], "rb").read(), _index_bytes(s["path"])
            jes.append(pl.wait(pl.submit(bam_bytes=data, bai_bytes=bai, strandness=STRANDNESS[s["strand"]])))
        co = regtools_amd.Cohort(ctx=gpu_ctx)
        for je, s in zip(jes, two):
            co.add(je, s["name"])
        assert co.add_paths == [0, 1]                  # the first file's rows were overwritten by the second's
        m = co.finish()
        assert m.bed12() == bed and m.counts_tsv() == tsv
        co.close()
    finally:
        pl.close()


@pytest.mark.parametrize("depth", [1, 2])
def test_an_unreadable_file_in_the_middle(gpu_ctx, cohort_files, tmp_path, depth):  # noqa: F811
    import regtools_amd
    junk, junk_bytes, junk_bai = str(tmp_path / "junk.bam"), b"this is not a BAM file, not even a gzip stream" * 10, _index_bytes(cohort_files[0]["path"])
    open(junk, "wb").write(junk_bytes)
    open(junk + ".bai", "wb").write(junk_bai)
    good = [cohort_files[0], cohort_files[6], cohort_files[2], cohort_files[7]]
    items = _items(good[:2]) + [(junk, "junk", dict(strandness=0))] + _items(good[2:])
    co = regtools_amd.Cohort(ctx=gpu_ctx)
    with pytest.raises(regtools_amd.RegtoolsError) as e:
        co.run(items, depth=depth)
    je = regtools_amd.JunctionsExtractor(strandness=0, ctx=gpu_ctx)
    with pytest.raises(regtools_amd.RegtoolsError) as alone:
        je.identify_junctions_from_BAM(bam_bytes=junk_bytes, bai_bytes=junk_bai)
    assert (e.value.code, str(e.value)) == (alone.value.code, str(alone.value))          # that file's own error
    bed, tsv, _ = expected_texts(good[:2])
    m = co.finish()
    assert m.sample_name == [s["name"] for s in good[:2]] and m.bed12() == bed and m.counts_tsv() == tsv
    # ... and the cohort goes on
    co.run(_items(good[2:]), depth=depth)
    bed, tsv, _ = expected_texts(good)
    m = co.finish()
    assert m.bed12() == bed and m.counts_tsv() == tsv
    # a file that is not there at all
    with pytest.raises(regtools_amd.RegtoolsError) as e:
        co.run([str(tmp_path / "absent.bam")], depth=depth, strandness=0)
    assert "Unable to open BAM/SAM file." in str(e.value) and co.finish().bed12() == bed
    co.close()


# ---- size: more triples than the radix sort's small tiles take ---------------------------------------------------------------------------
CONTIGS = [("c%02d" % k, 50_000_000 + k) for k in range(23)]
N_COMMON, N_POPULAR, PER, PRIVATE, ANCHOR = 20_000, 200_000, 100_000, 20_000, 8
LOOSE, LOOSE_BASE = 10_000, N_COMMON + N_POPULAR + 72 * PRIVATE          # ids from LOOSE_BASE on: rows with a left anchor of 3, on top of the 100,000


class _Sample(object):
    """What Cohort.add and cohort.merge_host read of an extractor, over a hand-made table."""

    def __init__(self, table):
        self.table, self.min_anchor_length_, self._ctx = table, ANCHOR, None


def _sample_ids(g, rng):
    """100,000 distinct key ids -- 20 k that every sample has, 60 k out of a pool of 200 k, 20 k nobody else has -- and 10,000 more whose rows have
    no left anchor, scattered among them."""
    pop = N_COMMON + rng.choice(N_POPULAR, PER - N_COMMON - PRIVATE, replace=False)
    own = N_COMMON + N_POPULAR + g * PRIVATE + np.arange(PRIVATE)
    loose = LOOSE_BASE + g * LOOSE + np.arange(LOOSE)
    return rng.permutation(np.concatenate([np.arange(N_COMMON), pop, own, loose])).astype(np.int64)


def _columns(g, ids):
    """The rows of sample g.  A key's coordinates and strand are functions of its id; bounds and counts also of the sample."""
    name = ids % 23
    start = 1000 + 3 * (ids // 23) + 40 * (ids % 2)
    end = start + 100 + ids % 50
    strand = np.array([ord("+"), ord("-"), ord("?"), ord(".")], np.uint32)[np.where(ids % 3 == 2, 2 + g % 2, ids % 3)]
    ts = np.where(ids >= LOOSE_BASE, start - 3, start - ANCHOR - (ids * 3 + g * 5) % 20)
    te = end + ANCHOR + (ids * 7 + g * 11) % 20
    count = 1 + (ids * 7 + g) % 9 + np.where(ids == 5, 4_000_000_000, 0)           # one key's total passes 2^32
    return name, start, end, ts, te, count, strand


def _table(g, cols):
    import ctypes as C
    from regtools_amd import _ffi
    name, start, end, ts, te, count, strand = cols
    order = CONTIGS[g % 3:] + CONTIGS[:g % 3]                            # the samples do not agree on the tids
    rows = np.zeros((len(name), 12), np.uint32)
    rows[:, 0] = (name - g % 3) % 23
    for k, col in enumerate((start, end, ts, te, count)):
        rows[:, 1 + k] = col
    rows[:, 10] = strand
    proto = _ffi.JunctionTable()
    arr = (C.c_char_p * 23)(*[c[0].encode() for c in order])
    lens = (C.c_uint32 * 23)(*[c[1] for c in order])
    proto.n_ref, proto.ref_name, proto.ref_len = 23, arr, lens
    t = C.POINTER(_ffi.JunctionTable)()
    raw = rows.tobytes()
    assert _ffi.lib().rgx_table_unpack(raw, len(rows), C.byref(proto), C.byref(t)) == 0
    return t


def _by_numpy(all_cols, first_names):
    """The matrix of the samples' anchored rows with numpy.unique.  Cohort tid = position of the contig's name in the order of first appearance."""
    ctid_of_name = np.array([first_names.index(c[0]) for c in CONTIGS])
    parts = []
    for g, (name, start, end, ts, te, count, strand) in enumerate(all_cols):
        keep = (start - ts >= ANCHOR) & (te - end >= ANCHOR)
        cls = np.where(strand == ord("+"), 0, np.where(strand == ord("-"), 1, 2))
        key = (((ctid_of_name[name] << 20 | start) << 8 | (end - start)) << 2 | cls)[keep]
        parts.append((key, np.full(keep.sum(), g), ts[keep], te[keep], count[keep], start[keep], end[keep], ctid_of_name[name][keep], strand[keep]))
    key, sample, ts, te, count, start, end, ctid, chars = [np.concatenate(x) for x in zip(*parts)]
    uniq, inv, n_with = np.unique(key, return_inverse=True, return_counts=True)
    order = np.lexsort((sample, inv))
    total = np.zeros(len(uniq), np.uint64); np.add.at(total, inv, count.astype(np.uint64))
    lo = np.full(len(uniq), 2**32 - 1, np.int64); np.minimum.at(lo, inv, ts)
    hi = np.zeros(len(uniq), np.int64); np.maximum.at(hi, inv, te)
    first = np.zeros(len(uniq), np.int64); first[inv[order][::-1]] = order[::-1]          # (any triple of the key: start / end / tid are the key's)
    return dict(n=len(uniq), n_triples=len(key), n_with=n_with, total=total, thick_start=lo, thick_end=hi, start=start[first], end=end[first], tid=ctid[first],
                strand=cohort_ref.last_sample_strand(inv, sample, chars, len(uniq)),          # the character of the highest-numbered sample that has the key
                row_begin=np.concatenate([[0], np.cumsum(n_with)]), col_sample=sample[order], val_count=count[order])


def _check(m, want):
    assert (m.n, m.n_triples) == (want["n"], want["n_triples"])
    for k in ("row_begin", "col_sample", "val_count", "total", "n_with", "thick_start", "thick_end", "start", "end", "tid"):
        assert np.array_equal(getattr(m, k).astype(np.int64), want[k].astype(np.int64)), k
    assert m.strand.shape == want["strand"].shape and np.array_equal(m.strand, want["strand"]), "strand"


def test_six_million_triples_twice(gpu_ctx):
    import regtools_amd
    from regtools_amd import _ffi, cohort
    rng = np.random.default_rng(17)
    cols = [_columns(g, _sample_ids(g, rng)) for g in range(72)]
    tables = [_table(g, c) for g, c in enumerate(cols)]
    samples = [_Sample(t) for t in tables]
    names = ["n%02d" % g for g in range(72)]
    first_names = [c[0] for c in CONTIGS]                                # sample 0 lists them in this order, the others add no name
    co = regtools_amd.Cohort(ctx=gpu_ctx)
    for s, nm in zip(samples[:64], names[:64]):
        co.add(s, nm)
    assert co.add_paths == [0] * 64
    m = co.finish()
    want = _by_numpy(cols[:64], first_names)
    assert m.n_triples == 64 * PER > 2 * 1024 * 1024 and 1_400_000 < m.n <= N_COMMON + N_POPULAR + 64 * PRIVATE and m.n_with.max() == 64 and (m.n_with == 1).sum() > 500_000
    assert m.total.max() > 2**32
    _check(m, want)
    _same_matrix(m, cohort.merge_host(samples[:64], names[:64]))
    # eight more samples, a second finish: equal to a fresh cohort of all 72
    for s, nm in zip(samples[64:], names[64:]):
        co.add(s, nm)
    m2 = co.finish()
    _check(m2, _by_numpy(cols, first_names))
    fresh = regtools_amd.Cohort(ctx=gpu_ctx)
    for s, nm in zip(samples, names):
        fresh.add(s, nm)
    f = fresh.finish()
    _same_matrix(m2, f)
    assert m2.bed12() == f.bed12() == cohort.merge_host(samples, names).bed12()
    co.close(); fresh.close()
    for t in tables:
        _ffi.lib().rgx_table_free(t)


def test_keys_that_most_samples_share(gpu_ctx):
    """48 samples over the same 5,000 keys and twenty of their own each: 40 samples per key on average, where finish reduces a row per wave
    (launch_cohort_reduce) instead of a row per lane."""
    import regtools_amd
    from regtools_amd import _ffi, cohort
    rng = np.random.default_rng(23)
    G = 48
    ids = [rng.permutation(np.concatenate([np.arange(5000), N_COMMON + N_POPULAR + g * PRIVATE + np.arange(20), LOOSE_BASE + g * LOOSE + np.arange(300)]))
           .astype(np.int64) for g in range(G)]
    cols = [_columns(g, ids[g]) for g in range(G)]
    tables = [_table(g, c) for g, c in enumerate(cols)]
    samples, names = [_Sample(t) for t in tables], ["w%02d" % g for g in range(G)]
    co = regtools_amd.Cohort(ctx=gpu_ctx)
    for s, nm in zip(samples, names):
        co.add(s, nm)
    m = co.finish()
    assert m.n == 5000 + 20 * G and m.n_triples >= 32 * m.n and m.n_with.max() == G and m.total.max() > 2**32
    _check(m, _by_numpy(cols, [c[0] for c in CONTIGS]))
    _same_matrix(m, cohort.merge_host(samples, names))
    co.close()
    for t in tables:
        _ffi.lib().rgx_table_free(t)


def test_limits_are_reported(gpu_ctx):
    import regtools_amd
    co = regtools_amd.Cohort(ctx=gpu_ctx)
    a = _Sample(table_from_rows([(0, 100, 200, 90, 230, 3, "+")], (("chrA", 1000),)))
    b = _Sample(table_from_rows([(0, 100, 200, 90, 230, 3, "+")], (("chrA", 1001),)))
    co.add(a, "first")
    with pytest.raises(regtools_amd.RegtoolsError) as e:
        co.add(b, "second")
    assert e.value.code == 7 and "chrA" in str(e.value) and "first" in str(e.value) and "second" in str(e.value)
    m = co.finish()                                                      # the refused sample left nothing behind
    assert m.sample_name == ["first"] and m.bed12() == b"chrA\t90\t230\tJUNC00000001\t3\t+\t90\t230\t255,0,0\t2\t10,30\t0,110\n"
    empty = regtools_amd.Cohort(ctx=gpu_ctx).finish()
    assert empty.n == 0 and empty.bed12() == b"" and empty.counts_tsv() == b"chrom\tstart\tend\tstrand\n" and list(empty.row_begin) == [0]
    co.close()


def test_tool_equals_the_python_result(gpu_ctx, cohort_files, tmp_path):  # noqa: F811
    import regtools_amd
    four = [cohort_files[1], cohort_files[6], cohort_files[7], cohort_files[3]]
    co = regtools_amd.Cohort(ctx=gpu_ctx)
    co.run(_items(four))
    m = co.finish()
    bed, tsv = str(tmp_path / "x.bed"), str(tmp_path / "x.tsv")
    r = subprocess.run([EXE, "junctions", "cohort", "-s", "XS", "-o", bed, "-c", tsv] + [s["path"] for s in four], stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert r.returncode == 0 and r.stdout == b"", r.stderr[-2000:]
    assert open(bed, "rb").read() == m.bed12() == expected_texts(four)[0] and open(tsv, "rb").read() == m.counts_tsv()
    co.close()
    # a list with names of its own, filters, BED12 on stdout
    lst = tmp_path / "list.txt"
    lst.write_text("".join("%s\tS%d\n" % (s["path"], k) for k, s in enumerate(four[:3])) + four[3]["path"] + "\n")
    renamed = [dict(s, name="S%d" % k) for k, s in enumerate(four[:3])] + [four[3]]
    e_bed, e_tsv, _ = expected_texts(renamed, min_samples=2, min_total=10)
    r = subprocess.run([EXE, "junctions", "cohort", "-s", "XS", "-n", "2", "-N", "10", "-c", tsv, "-L", str(lst)], stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert r.returncode == 0 and r.stdout == e_bed and open(tsv, "rb").read() == e_tsv and len(e_bed) > 0
    # a file that fails: its error, exit 1, no output files
    os.remove(bed); os.remove(tsv)
    r = subprocess.run([EXE, "junctions", "cohort", "-s", "XS", "-o", bed, "-c", tsv, four[0]["path"], str(tmp_path / "absent.bam"), four[1]["path"]],
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert r.returncode == 1 and b"Unable to open BAM/SAM file." in r.stderr and not os.path.exists(bed) and not os.path.exists(tsv)
