"""The cohort junction-by-sample matrix without a device: the contract of include/regtools_amd.h as rgx_cohort_merge_host (the library's plain C++
twin of rgx_cohort_add + rgx_cohort_finish) keeps it, the two text formats, and the option surface of `regtools-amd junctions cohort`.
Every comparison is between integers or bytes and exact."""
import ctypes as C
import os
import subprocess

from cohort_common import HostMatrix, cohort_files, expected_texts, table_from_rows  # noqa: F401  (cohort_files is a fixture)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "bin", "regtools-amd")


def _free(tables):
    from regtools_amd import _ffi
    for t in tables:
        _ffi.lib().rgx_table_free(t)


def test_defaults():
    m = HostMatrix([], [], [])
    assert m.rc == 0 and m.defaults == (1, 1, 1)
    m.free()


def test_keys_are_matched_by_contig_name():
    # s0 and s1 list the same contigs in different tid order; s2 has a contig the others lack, in front of one they have
    s0 = table_from_rows([(0, 100, 200, 90, 230, 3, "+"), (1, 50, 150, 20, 160, 2, "-")], (("chrA", 1000), ("chrB", 2000)))
    s1 = table_from_rows([(1, 100, 200, 80, 220, 2, "+"), (0, 50, 150, 30, 170, 5, "-"), (0, 70, 90, 60, 99, 1, "+")], (("chrB", 2000), ("chrA", 1000)))
    s2 = table_from_rows([(0, 10, 20, 1, 30, 7, "+"), (1, 100, 200, 92, 208, 1, "+")], (("chrC", 500), ("chrA", 1000)))
    m = HostMatrix([s0, s1, s2], [8, 8, 8], ["a", "b", "c"])
    assert m.rc == 0
    c = m.h.contents
    assert [c.ref_name[i] for i in range(c.n_ref)] == [b"chrA", b"chrB", b"chrC"] and [c.ref_len[i] for i in range(c.n_ref)] == [1000, 2000, 500]
    assert [c.sample_name[i] for i in range(c.n_samples)] == [b"a", b"b", b"c"] and c.n_triples == 7
    assert m.bed12().decode().splitlines() == [
        "chrA\t80\t230\tJUNC00000001\t6\t+\t80\t230\t255,0,0\t2\t20,30\t0,120",
        "chrB\t20\t170\tJUNC00000002\t7\t-\t20\t170\t255,0,0\t2\t30,20\t0,130",
        "chrB\t60\t99\tJUNC00000003\t1\t+\t60\t99\t255,0,0\t2\t10,9\t0,30",
        "chrC\t1\t30\tJUNC00000004\t7\t+\t1\t30\t255,0,0\t2\t9,10\t0,19",
    ]
    assert m.counts().decode().splitlines() == [
        "chrom\tstart\tend\tstrand\ta\tb\tc",
        "chrA\t100\t200\t+\t3\t2\t1",
        "chrB\t50\t150\t-\t2\t5\t0",
        "chrB\t70\t90\t+\t0\t1\t0",
        "chrC\t10\t20\t+\t0\t0\t7",
    ]
    n = int(c.n)
    assert [c.n_with[i] for i in range(n)] == [3, 2, 1, 1] and [c.row_begin[i] for i in range(n + 1)] == [0, 3, 5, 6, 7]
    assert [c.col_sample[i] for i in range(7)] == [0, 1, 2, 0, 1, 1, 2] and [c.val_count[i] for i in range(7)] == [3, 2, 1, 2, 5, 1, 7]
    m.free()
    _free([s0, s1, s2])


def test_strand_class_is_part_of_the_key():
    s0 = table_from_rows([(0, 100, 200, 90, 230, 3, "+"), (0, 100, 200, 85, 215, 4, "-"), (0, 300, 400, 280, 410, 1, "?")])
    s1 = table_from_rows([(0, 300, 400, 290, 450, 4, "."), (0, 100, 200, 95, 240, 1, "-")])
    m = HostMatrix([s0, s1], [8, 8], ["x", "y"], only_anchored=False)
    assert m.rc == 0
    assert m.bed12().decode().splitlines() == [
        "chrA\t90\t230\tJUNC00000001\t3\t+\t90\t230\t255,0,0\t2\t10,30\t0,110",
        "chrA\t85\t240\tJUNC00000002\t5\t-\t85\t240\t255,0,0\t2\t15,40\t0,115",
        "chrA\t280\t450\tJUNC00000003\t5\t.\t280\t450\t255,0,0\t2\t20,50\t0,120",
    ]
    assert m.counts().decode().splitlines()[1:] == ["chrA\t100\t200\t+\t3\t0", "chrA\t100\t200\t-\t4\t1", "chrA\t300\t400\t.\t1\t4"]
    m.free()
    # the later sample gives the character also when it is the '?'
    m = HostMatrix([s1, s0], [8, 8], ["y", "x"], only_anchored=False)
    assert m.bed12().decode().splitlines()[2] == "chrA\t280\t450\tJUNC00000003\t5\t?\t280\t450\t255,0,0\t2\t20,50\t0,120"
    m.free()
    _free([s0, s1])


def test_only_anchored_is_computed_from_the_rows_own_numbers():
    # anchors of (10, 30), (7, 30), (10, 7); the second sample is read with -a 5 (so its 7 counts) and has a row whose thick bounds lie INSIDE
    # the junction: the unsigned differences are huge, as in k_merge_table, and the row takes part
    s0 = table_from_rows([(0, 100, 200, 90, 230, 3, "+"), (0, 300, 400, 293, 430, 2, "+"), (0, 500, 600, 490, 607, 1, "-")])
    s1 = table_from_rows([(0, 300, 400, 293, 405, 4, "+"), (0, 700, 800, 701, 799, 6, "+")])
    on = HostMatrix([s0, s1], [8, 5], ["p", "q"])
    assert on.bed12().decode().splitlines() == [
        "chrA\t90\t230\tJUNC00000001\t3\t+\t90\t230\t255,0,0\t2\t10,30\t0,110",
        "chrA\t293\t405\tJUNC00000002\t4\t+\t293\t405\t255,0,0\t2\t7,5\t0,107",
        "chrA\t701\t799\tJUNC00000003\t6\t+\t701\t799\t255,0,0\t2\t4294967295,4294967295\t0,99",
    ]
    assert on.counts().decode().splitlines()[1:] == ["chrA\t100\t200\t+\t3\t0", "chrA\t300\t400\t+\t0\t4", "chrA\t700\t800\t+\t0\t6"]
    off = HostMatrix([s0, s1], [8, 5], ["p", "q"], only_anchored=False)
    assert off.bed12().decode().splitlines() == [
        "chrA\t90\t230\tJUNC00000001\t3\t+\t90\t230\t255,0,0\t2\t10,30\t0,110",
        "chrA\t293\t430\tJUNC00000002\t6\t+\t293\t430\t255,0,0\t2\t7,30\t0,107",
        "chrA\t490\t607\tJUNC00000003\t1\t-\t490\t607\t255,0,0\t2\t10,7\t0,110",
        "chrA\t701\t799\tJUNC00000004\t6\t+\t701\t799\t255,0,0\t2\t4294967295,4294967295\t0,99",
    ]
    assert off.h.contents.n_triples == 5 and on.h.contents.n_triples == 3
    on.free(); off.free()
    _free([s0, s1])


def test_min_samples_and_min_total():
    s0 = table_from_rows([(0, 100, 200, 90, 230, 3, "+"), (0, 300, 400, 280, 430, 9, "+")])
    s1 = table_from_rows([(0, 100, 200, 90, 230, 1, "+"), (0, 500, 600, 480, 630, 2, "+")])
    lines = lambda **kw: [x.split("\t")[1:5] for x in HostMatrix([s0, s1], [8, 8], ["p", "q"], **kw).bed12().decode().splitlines()]
    assert lines() == [["90", "230", "JUNC00000001", "4"], ["280", "430", "JUNC00000002", "9"], ["480", "630", "JUNC00000003", "2"]]
    assert lines(min_samples=2) == [["90", "230", "JUNC00000001", "4"]]
    assert lines(min_total=4) == [["90", "230", "JUNC00000001", "4"], ["280", "430", "JUNC00000002", "9"]]          # renamed after the drop
    assert lines(min_total=5) == [["280", "430", "JUNC00000001", "9"]]
    assert lines(min_samples=2, min_total=5) == []
    m = HostMatrix([s0, s1], [8, 8], ["p", "q"], min_total=5)
    c = m.h.contents
    assert (c.n, c.row_begin[0], c.row_begin[1], c.col_sample[0], c.val_count[0], c.n_triples) == (1, 0, 1, 0, 9, 4)
    m.free()
    _free([s0, s1])


def test_total_is_64_bit():
    s0 = table_from_rows([(0, 100, 200, 90, 230, 4000000000, "+")])
    s1 = table_from_rows([(0, 100, 200, 90, 230, 4000000000, "+")])
    m = HostMatrix([s0, s1], [8, 8], ["p", "q"])
    assert m.bed12() == b"chrA\t90\t230\tJUNC00000001\t8000000000\t+\t90\t230\t255,0,0\t2\t10,30\t0,110\n"
    assert m.h.contents.total[0] == 8000000000
    assert m.counts() == b"chrom\tstart\tend\tstrand\tp\tq\nchrA\t100\t200\t+\t4000000000\t4000000000\n"
    big = HostMatrix([s0, s1], [8, 8], ["p", "q"], min_total=8000000001)
    assert big.rc == 0 and big.h.contents.n == 0
    m.free(); big.free()
    _free([s0, s1])


def test_an_empty_sample_and_an_empty_cohort():
    s0 = table_from_rows([(0, 100, 200, 90, 230, 3, "+")])
    s1 = table_from_rows([], (("chrB", 1000000), ("chrQ", 77)))
    m = HostMatrix([s0, s1, s0], [8, 8, 8], ["p", "empty", "r"])
    assert m.rc == 0
    c = m.h.contents
    assert [c.ref_name[i] for i in range(c.n_ref)] == [b"chrA", b"chrB", b"chrQ"]          # an empty sample's contigs still count
    assert m.counts() == b"chrom\tstart\tend\tstrand\tp\tempty\tr\nchrA\t100\t200\t+\t3\t0\t3\n"
    m.free()
    for tables, names in (([s1], ["empty"]), ([], []), ([s0], ["unanchored"])):
        z = HostMatrix(tables, [200] * len(tables), names)          # (-a 200: s0's row has no anchors)
        assert z.rc == 0
        c = z.h.contents
        assert c.n == 0 and c.row_begin[0] == 0 and c.n_triples == 0 and z.bed12() == b""
        assert z.counts() == ("chrom\tstart\tend\tstrand" + "".join("\t" + s for s in names) + "\n").encode()
        z.free()
    _free([s0, s1])


def test_one_name_with_two_lengths_is_an_error():
    s0 = table_from_rows([(0, 100, 200, 90, 230, 3, "+")], (("chrA", 1000), ("chrB", 2000)))
    s1 = table_from_rows([(0, 100, 200, 90, 230, 3, "+")], (("chrB", 2001),))
    m = HostMatrix([s0, s1], [8, 8], ["first", "second"])
    msg = m.err.value.decode()
    assert m.rc == 7 and not m.h and "chrB" in msg and "first" in msg and "second" in msg and "2000" in msg and "2001" in msg
    bad = table_from_rows([(1, 100, 200, 90, 230, 3, "+")], (("chrA", 1000),))
    m = HostMatrix([bad], [8], ["tid"])
    assert m.rc == 7 and not m.h
    _free([s0, s1, bad])


def test_formatters_size_then_fill():
    from regtools_amd import _ffi
    L = _ffi.lib()
    s0 = table_from_rows([(0, 100, 200, 90, 230, 3, "+"), (1, 50, 150, 20, 160, 2, "-")])
    m = HostMatrix([s0], [8], ["only"])
    for fn, text in ((L.rgx_cohort_format_bed12, m.bed12()), (L.rgx_cohort_format_counts, m.counts())):
        n = fn(m.h, None, 0)
        assert n == len(text) > 0
        small = C.create_string_buffer(b"#" * n, n)
        assert fn(m.h, small, n - 1) == n and small.raw == b"#" * n          # too small: the size again, nothing written
        exact = C.create_string_buffer(b"#" * (n + 4), n + 4)
        assert fn(m.h, exact, n) == n and exact.raw == text + b"####"
    m.free()
    _free([s0])


def test_real_tables_against_the_oracle_and_a_dict(cohort_files):  # noqa: F811
    """Each sample's `junctions extract` BED12 by the oracle, merged here with a dict; the same rows as tables through rgx_cohort_merge_host."""
    bed, tsv, stats = expected_texts(cohort_files)
    print("cohort: %d anchored rows, %d keys, keys by number of samples %s" % (stats["rows_in"], stats["union"], sorted(stats["n_with_hist"].items())))
    assert stats["union"] > 10000 and max(stats["n_with_hist"]) >= 5
    tables = []
    for s in cohort_files:
        tid = {nm: k for k, (nm, _) in enumerate(s["contigs"])}
        tables.append(table_from_rows([(tid[chrom], start, end, ts, te, score, strand) for (chrom, start, end, strand), (score, ts, te) in s["rows"].items()],
                                      s["contigs"]))
    names = [s["name"] for s in cohort_files]
    m = HostMatrix(tables, [8] * len(tables), names)
    assert m.rc == 0 and m.h.contents.n_triples == stats["rows_in"] and m.h.contents.n == stats["union"]
    assert m.bed12() == bed
    assert m.counts() == tsv
    m.free()
    for kw in (dict(min_samples=3), dict(min_total=40), dict(min_samples=2, min_total=25)):
        m = HostMatrix(tables, [8] * len(tables), names, **kw)
        e_bed, e_tsv, _ = expected_texts(cohort_files, **kw)
        assert m.bed12() == e_bed and m.counts() == e_tsv and 0 < len(e_bed) < len(bed)
        m.free()
    _free(tables)


def _run(*args):
    return subprocess.run([EXE, "junctions", "cohort"] + list(args), stdout=subprocess.PIPE, stderr=subprocess.PIPE)


def test_tool_option_surface(tmp_path):
    h = _run("-h")
    assert h.returncode == 0 and h.stdout.startswith(b"Usage:\t\tregtools-amd junctions cohort") and b"Usage" not in h.stderr
    usage = h.stdout
    for args in (["-s", "XS"], ["a.bam"], ["-s", "XS", "-Z", "a.bam"], ["-s", "XS", "-L", str(tmp_path / "no_such_list.txt")]):
        r = _run(*args)          # no BAM, no -s, a bad option, a list that cannot be read
        assert r.returncode == 1 and r.stdout == b"" and usage in r.stderr, args
    lst = tmp_path / "list.txt"
    lst.write_text("x/a.bam\nb.bam\tother\ny/a.bam\n")
    r = _run("-s", "XS", "-L", str(lst))
    assert r.returncode == 1 and r.stdout == b"" and b"named a" in r.stderr and usage not in r.stderr
    r = _run("-s", "XS", "dir1/same.bam", "dir2/same.bam")
    assert r.returncode == 1 and b"named same" in r.stderr
    # the sub-command is not in the usage texts the reference pins
    j = subprocess.run([EXE, "junctions"], stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert j.returncode == 0 and b"cohort" not in j.stdout


def test_tool_fails_like_extract_on_a_file_it_cannot_run():
    """Without a device both tools end with the library's no-device message and exit 1; with one, with the reference's text for a file that cannot be opened."""
    import torch
    r = _run("-s", "XS", "a.bam")
    e = subprocess.run([EXE, "junctions", "extract", "-s", "XS", "a.bam"], stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    last = lambda x: [ln for ln in x.stderr.splitlines() if ln.strip()][-1]
    assert r.returncode == 1 and e.returncode == 1 and r.stdout == b"" and last(r) == last(e)
    if not torch.cuda.is_available():
        assert b"no CPU fallback" in r.stderr
