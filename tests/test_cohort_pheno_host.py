"""The splicing phenotype table of a clustered cohort without a device: the contract of rgx_cohort_phenotypes in include/regtools_amd.h as
rgx_cohort_phenotypes_host (the library's plain C++ twin) keeps it, the quantile function, the text and the -q / -x / -d options of
`regtools-amd junctions cohort`.  Expectations: literals for the hand-made cohort of tests/cluster_cases.py and the numpy restatement of
tests/pheno_ref.py.  Integers are compared exactly, mean and sd as bit patterns; the two tolerances below were measured, not chosen."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import cluster_cases
import pheno_cases as pc
import pheno_ref
import refine_cases
from cohort_common import HostMatrix, table_from_rows

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "bin", "regtools-amd")
RGX_ERR_ARG = 7
NO = 0xffffffff

# (a) rgx_pheno_quantile against scipy.stats.norm.ppf over every rank2 of K = 1, 2, 3, 64, 4097: the largest relative difference measured on the
# CPU this was written on is 5.713e-14 (K = 4097, rank2 = 4105: scipy is handed the rounded double rank2 / (2 (K + 1)) and takes its distance from
# 1/2, an absolute 5.5e-17 against 1.2e-4; the library takes that distance from the integers).  Times 4 for another machine's libm.
QUANTILE_MEASURED, QUANTILE_TOL = 5.72e-14, 4 * 5.72e-14
# (b) the contract's summation order against plain np.mean / np.std over the cohorts of this file: largest relative difference measured
# 6.02e-16 (mean) and 3.82e-16 (sd), rows whose sd is rounding noise (below 1e-9) aside.  Times 4.
ORDER_MEASURED, ORDER_TOL = (6.02e-16, 3.82e-16), (4 * 6.02e-16, 4 * 3.82e-16)


def _matrix(tables, names, **kw):
    from regtools_amd import cohort
    hm = HostMatrix(tables, [8] * len(tables), names, **kw)
    assert hm.rc == 0, hm.err.value
    m, hm.h = cohort.CohortMatrix(hm.h), None
    return m


def _cohort(count, **kw):
    """(tables, matrix, clusters) of pheno_cases' cohort with these counts; the clusters are what groups_of says."""
    from regtools_amd import cohort
    tables = pc.tables(count)
    m = cohort.merge_host([cluster_cases.Sample(t) for t in tables], pc.names(count.shape[1]), **kw)
    return tables, m, cohort.cluster_host(m)


def _check(m, cl, **kw):
    from regtools_amd import cohort
    ph, want = cohort.phenotypes_host(m, cl, **kw), pheno_ref.phenotypes(m, cl, **kw)
    pheno_ref.same(ph, want)
    assert ph.text(m, cl) == pheno_ref.text(m, cl, ph, cohort.quantile)
    return ph, want


def test_defaults():
    from regtools_amd import _ffi
    p = _ffi.PhenoParams(7, 7, 7.0)
    _ffi.lib().rgx_pheno_params_default(C.byref(p))
    assert (p.na_num, p.na_den, p.min_sd) == (4, 10, 0.005)


def test_hand_made_cohort_against_literals():
    from regtools_amd import cohort
    tables = [table_from_rows(cluster_cases.HAND_P), table_from_rows(cluster_cases.HAND_Q)]
    m = _matrix(tables, ["p", "q"], only_anchored=False, min_total=0)
    cl = cohort.cluster_host(m)
    assert [int(c) for c in cl.cluster] == cluster_cases.HAND["cluster"]
    # rows 1, 4 and 7 are alone in clusters that one sample has no reads on: 1 of 2 missing is over 4/10.  The ratios of the others, p then q:
    # row 0: 3.5/5.5, 1.5/5.5; row 2: 2.5/5.5, 0.5/5.5; row 3: 0.5/5.5, 4.5/5.5; row 5: 1.5/1.5, 0.5/2.5; row 6: 0.5/1.5, 2.5/2.5
    ph, _ = _check(m, cl)
    assert (ph.n_rows, ph.n_samples, ph.n_clustered, ph.n_drop_na, ph.n_drop_sd) == (5, 2, 8, 3, 0)
    assert ph.row.tolist() == [0, 2, 3, 5, 6] and ph.n_na.tolist() == [0, 0, 0, 0, 0]
    assert ph.mean.tolist() == [0.45454545454545453, 0.2727272727272727, 0.4545454545454546, 0.6, 0.6666666666666666]
    assert ph.sd.tolist() == [0.18181818181818182, 0.18181818181818182, 0.36363636363636365, 0.4, 0.33333333333333337]
    # with two samples every z is 1 or -1 up to its last bit: in column p rows 0, 2 and 5 come out equal (places 3 .. 5: rank2 8) and rows
    # 3 and 6 do not (2 and 4); in column q rows 2 and 5 tie (places 2 .. 3) and rows 3 and 6 (places 4 .. 5)
    assert ph.rank2.tolist() == [[8, 2], [8, 5], [2, 9], [8, 5], [4, 9]]
    assert ph.text(m, cl).decode().splitlines() == [
        "#Chr\tstart\tend\tID\tp\tq",
        "chrA\t100\t200\tchrA:100:200:clu_1_+\t0.43072729929545744\t-0.96742156610170105",
        "chrA\t100\t300\tchrA:100:300:clu_1_+\t0.43072729929545744\t-0.21042839424792475",
        "chrA\t150\t300\tchrA:150:300:clu_1_+\t-0.96742156610170105\t0.67448975019608171",
        "chrA\t500\t600\tchrA:500:600:clu_4_NA\t0.43072729929545744\t-0.21042839424792475",
        "chrA\t500\t700\tchrA:500:700:clu_4_NA\t-0.43072729929545744\t0.67448975019608171"]
    # every share of missing samples allowed: rows 1, 4 and 7 pass the first filter and fall to the second -- one present sample is its own mean
    ph, _ = _check(m, cl, max_missing=(1, 1))
    assert (ph.n_rows, ph.n_drop_na, ph.n_drop_sd) == (5, 0, 3) and ph.row.tolist() == [0, 2, 3, 5, 6]
    # the refined clusters of the same matrix are taken like the plain ones
    rc = cohort.refine_host(m, min_reads=2)
    assert [int(c) for c in rc.cluster] == [0, 1, 0, 0, 2, NO, 3, 4]
    ph, _ = _check(m, rc, max_missing=(1, 1))
    assert (ph.n_clustered, ph.n_rows) == (7, 3)
    m.close()
    cluster_cases.free_tables(tables)


@pytest.mark.parametrize("S, n_missing, kept", [(5, 2, True), (5, 3, False), (10, 4, True), (10, 5, False)])
def test_the_missing_share_is_an_exact_compare(S, n_missing, kept):
    count = pc.counts(S, 4, seed=S)
    count[:2, :n_missing] = 0                                # the first cluster has no reads in the first n_missing samples
    tables, m, cl = _cohort(count)
    ph, want = _check(m, cl)
    assert want["all_n_na"].tolist() == [n_missing, n_missing, 0, 0]
    assert ph.row.tolist() == ([0, 1, 2, 3] if kept else [2, 3]) and ph.n_drop_na == (0 if kept else 2) and ph.n_drop_sd == 0
    m.close()
    cluster_cases.free_tables(tables)


def test_a_row_missing_everywhere_is_dropped_whatever_the_share():
    from regtools_amd import cohort
    # rows 0 and 1 count 0 reads: with min_total = 0 they are rows of the matrix and a cluster that no sample has reads on
    p = [(0, 100, 200, 90, 230, 0, "+"), (0, 100, 300, 90, 330, 0, "+"), (0, 500, 600, 480, 630, 4, "+"), (0, 500, 700, 480, 730, 2, "+")]
    q = [(0, 500, 600, 480, 630, 1, "+"), (0, 500, 700, 480, 730, 5, "+")]
    tables = [table_from_rows(p), table_from_rows(q)]
    m = _matrix(tables, ["p", "q"], only_anchored=False, min_total=0)
    cl = cohort.cluster_host(m)
    assert [int(t) for t in m.total] == [0, 0, 5, 7] and cl.cluster.tolist() == [0, 0, 1, 1] and cl.cs_begin.tolist() == [0, 0, 2]
    ph, want = _check(m, cl, max_missing=(1, 1), min_sd=0.0)
    assert want["all_n_na"].tolist() == [2, 2, 0, 0] and (ph.n_drop_na, ph.n_drop_sd) == (2, 0) and ph.row.tolist() == [2, 3]
    m.close()
    cluster_cases.free_tables(tables)


def test_flat_rows():
    # rows 0, 1: counts near 1000 that move by a few reads -- sd 0.0015; rows 2, 3: sd 0.3; row 4 is alone in its cluster: its ratio is 1 in
    # every sample and its sd exactly 0
    count = np.array([[1000, 1004, 996, 1002], [1000, 996, 1004, 998], [10, 30, 5, 50], [20, 10, 40, 7]])
    tables = pc.tables(count)
    lone = [table_from_rows([(0, 5000, 5100, 4990, 5110, c, "+")], contigs=cluster_cases.CONTIGS) for c in (3, 9, 27, 81)]
    from regtools_amd import cohort
    both = [cluster_cases.Sample(t) for t in tables] + [cluster_cases.Sample(t) for t in lone]
    # (sample s and its `lone` twin would be two samples: give the lone row to four further samples, which then lack the clusters above)
    m = cohort.merge_host(both, pc.names(8))
    cl = cohort.cluster_host(m)
    assert cl.cluster.tolist() == [0, 0, 1, 1, 2]
    want = pheno_ref.phenotypes(m, cl, max_missing=(1, 1), min_sd=0.0)
    sd = want["all_sd"]
    assert sd[4] == 0.0 and want["all_mean"][4] == 1.0 and all(0 < s <= 0.0025 for s in sd[:2]) and all(s >= 0.01 for s in sd[2:4])
    ph, _ = _check(m, cl, max_missing=(1, 1), min_sd=0.0)
    assert ph.row.tolist() == [0, 1, 2, 3] and (ph.n_drop_na, ph.n_drop_sd) == (0, 1)             # sd exactly 0 goes at min_sd = 0
    ph, _ = _check(m, cl, max_missing=(1, 1))
    assert ph.row.tolist() == [2, 3] and (ph.n_drop_na, ph.n_drop_sd) == (0, 3)                   # 0.0015 < 0.005 <= 0.3
    m.close()
    cluster_cases.free_tables(tables + lone)


def test_one_row_kept():
    tables, m, cl = _cohort(pc.ONE_KEPT)
    ph, want = _check(m, cl)
    assert cl.cluster.tolist() == [0, 0] and ph.row.tolist() == [0] and ph.n_drop_sd == 1 and ph.rank2.tolist() == [[2, 2, 2]]
    assert [float(x) for x in ph.quantiles()[0]] == [0.0, 0.0, 0.0]
    m.close()
    cluster_cases.free_tables(tables)


def test_ties():
    # sample 0 has no reads in every third cluster (z = +0.0 there, a run of equal values in its column); sample 1 has none at all (its column
    # is one single tie); the first two pairs of clusters carry the same counts (equal rows: ties in every column)
    count = pc.counts(5, 60, seed=3, empty_clusters=[(0, 0, 3), (1, 0, 1)], duplicates=2)
    tables, m, cl = _cohort(count)
    ph, want = _check(m, cl, max_missing=(1, 1))
    assert ph.n_rows == 60 and (ph.rank2[:, 1] == 61).all() and (want["z"][:, 1] == 0).all()
    missing0 = np.flatnonzero(pc.groups_of(60) % 3 == 0)
    assert len(set(ph.rank2[missing0, 0].tolist())) == 1 and (ph.n_na[missing0] == 2).all()
    assert np.array_equal(ph.rank2[0:2], ph.rank2[6:8]) and np.array_equal(ph.rank2[12:14], ph.rank2[18:20])
    assert np.array_equal(pheno_ref.bits(ph.mean[0:2]), pheno_ref.bits(ph.mean[6:8]))
    m.close()
    cluster_cases.free_tables(tables)


@pytest.mark.parametrize("S", pc.SAMPLE_COUNTS)
def test_sample_counts_around_the_partials(S):
    count = pc.counts(S, 41, seed=S, absent=0.3, empty_clusters=[(0, 0, 3)], duplicates=2)
    tables, m, cl = _cohort(count)
    for kw in (dict(), dict(max_missing=(1, 1), min_sd=0.0)):
        ph, want = _check(m, cl, **kw)
        assert ph.n_clustered == m.n and (ph.n_rows > 0) == (S > 1)          # one sample: every row is its own mean
    # the restatement's column-at-a-time sums are the scalar loops, bit for bit
    for j in range(len(want["all_n_na"])):
        n_na, mean, sd = pheno_ref.row_stats_scalar(want["all_num"][j], want["all_den"][j])
        assert n_na == want["all_n_na"][j]
        if n_na < S:
            assert pheno_ref.bits(mean) == pheno_ref.bits(want["all_mean"][j]) and pheno_ref.bits(sd) == pheno_ref.bits(want["all_sd"][j])
    m.close()
    cluster_cases.free_tables(tables)


@pytest.fixture(scope="module")
def heavy():
    """The refined heavy-tailed random cohort of six samples (tests/test_cohort_refine_host.py): (matrix, refined clusters, the restatement)."""
    from regtools_amd import cohort
    G = 6
    tid, start, end, cls = cluster_cases.random_junctions()
    tables = refine_cases.heavy_tables(G, tid, start, end, cls)
    m = cohort.merge_host([cluster_cases.Sample(t) for t in tables], ["g%d" % g for g in range(G)])
    cl = cohort.refine_host(m, max_intron=200000, min_reads=30, min_ratio=(1, 100), min_rows=2, min_total=30)
    yield m, cl, pheno_ref.phenotypes(m, cl)
    cl.close(); m.close()
    cluster_cases.free_tables(tables)


def test_refined_heavy_tailed_random_cohort(heavy):
    from regtools_amd import cohort
    m, cl, want = heavy
    assert m.n == 199_998
    ph = cohort.phenotypes_host(m, cl)
    print("heavy-tailed cohort: %d clustered rows, %d dropped as missing, %d as flat, %d kept, twin %.1f ms" % (
        ph.n_clustered, ph.n_drop_na, ph.n_drop_sd, ph.n_rows, ph.ms_pheno))
    pheno_ref.same(ph, want)
    assert ph.n_rows >= 20_000 and ph.n_drop_na >= 100 and ph.n_drop_sd >= 1
    assert ph.text(m, cl)[:4000] == pheno_ref.text(m, cl, _Head(ph, 40), lambda r, K: cohort.quantile(r, ph.n_rows))[:4000]


class _Head(object):
    """The first rows of a table, for a writer that need not write 20,000 lines."""

    def __init__(self, ph, k):
        self.row, self.rank2 = ph.row[:k], ph.rank2[:k]


def test_the_summation_order_is_plausible(heavy):
    """(b): the contract's mean and sd against plain np.mean / np.std of the imputed rows.  The numbers compared are the restatement's, over every
    clustered row; the twin's, which it hands out for the kept rows only, are first shown to be the same bits."""
    from regtools_amd import cohort
    worst = [0.0, 0.0]
    wants = [heavy[2]]
    pheno_ref.same(cohort.phenotypes_host(heavy[0], heavy[1]), heavy[2])
    for S in pc.SAMPLE_COUNTS[1:]:
        tables, m, cl = _cohort(pc.counts(S, 41, seed=S, absent=0.3))
        wants.append(pheno_ref.phenotypes(m, cl, max_missing=(1, 1), min_sd=0.0))
        pheno_ref.same(cohort.phenotypes_host(m, cl, max_missing=(1, 1), min_sd=0.0), wants[-1])
        m.close()
        cluster_cases.free_tables(tables)
    for w in wants:
        num, den = w["all_num"].astype(np.float64), w["all_den"].astype(np.float64)
        present = den > 0
        ok = present.any(axis=1)
        with np.errstate(invalid="ignore", divide="ignore"):
            x = np.where(present, (num + 0.5) / (den + 0.5), np.nan)[ok]
        mean = np.nanmean(x, axis=1)
        sd = np.std(np.where(np.isnan(x), mean[:, None], x), axis=1)
        nz = w["all_sd"][ok] > 1e-9                                          # (a flat row's sd is rounding noise in either order)
        worst[0] = max(worst[0], float(np.max(np.abs(w["all_mean"][ok] - mean) / mean)))
        worst[1] = max(worst[1], float(np.max(np.abs(w["all_sd"][ok][nz] - sd[nz]) / sd[nz])))
    print("summation order against np.mean / np.std: largest relative difference %.3g (mean), %.3g (sd)" % tuple(worst))
    assert worst[0] <= ORDER_TOL[0] and worst[1] <= ORDER_TOL[1]


def test_quantile_against_scipy():
    """(a)"""
    from scipy.stats import norm
    from regtools_amd import cohort
    worst = 0.0
    for K in (1, 2, 3, 64, 4097):
        r = np.arange(2, 2 * K + 1)
        a, b = np.array([cohort.quantile(int(v), K) for v in r]), norm.ppf(r / (2.0 * (K + 1)))
        assert a[K - 1] == 0.0 and np.array_equal(a, -a[::-1]) and (np.diff(a) > 0).all()         # odd around the middle rank, increasing
        both_zero = (a == 0) & (b == 0)
        rel = np.where(both_zero, 0.0, np.abs(a - b) / np.where(both_zero, 1.0, np.abs(b)))
        worst = max(worst, float(rel.max()))
    print("rgx_pheno_quantile against scipy.stats.norm.ppf: largest relative difference %.3g" % worst)
    assert worst <= 1e-12                                    # (above that the approximation is mistyped)
    assert worst <= QUANTILE_TOL
    assert all(np.isnan(cohort.quantile(r, K)) for r, K in ((0, 5), (12, 5), (3, 0)))
    assert abs(cohort.quantile(1, 10**6) - norm.ppf(1 / (2.0 * (10**6 + 1)))) < 1e-9            # the far tail's branch (r > 5)


def test_argument_errors():
    from regtools_amd import RegtoolsError, _ffi, cohort
    tables, m, cl = _cohort(pc.counts(3, 6, seed=1))
    t2, m2, cl2 = _cohort(pc.counts(3, 8, seed=1))
    for kw in (dict(max_missing=(1, 0)), dict(max_missing=(3, 2)), dict(min_sd=-0.001), dict(min_sd=float("nan"))):
        with pytest.raises(RegtoolsError) as e:
            cohort.phenotypes_host(m, cl, **kw)
        assert e.value.code == RGX_ERR_ARG, kw
    with pytest.raises(RegtoolsError) as e:                  # the clusters of another matrix
        cohort.phenotypes_host(m, cl2)
    assert e.value.code == RGX_ERR_ARG
    cl.cluster[0] = cl.n_clusters                            # a cluster number the result does not have
    with pytest.raises(RegtoolsError) as e:
        cohort.phenotypes_host(m, cl)
    assert e.value.code == RGX_ERR_ARG
    cl.cluster[0] = 0
    m._h.contents.n_samples = 1 << 30                        # 6 clustered rows of 2^30 samples: past 2^32 - 2^16 entries, refused before anything is read
    with pytest.raises(RegtoolsError) as e:
        cohort.phenotypes_host(m, cl)
    assert e.value.code == RGX_ERR_ARG and "entries" in str(e.value)
    m._h.contents.n_samples = 3
    L, err, out = _ffi.lib(), C.create_string_buffer(256), C.POINTER(_ffi.PhenoTable)()
    assert L.rgx_cohort_phenotypes_host(None, cl._h, None, C.byref(out), err, len(err)) == RGX_ERR_ARG
    assert L.rgx_cohort_phenotypes_host(m._h, None, None, C.byref(out), err, len(err)) == RGX_ERR_ARG
    assert L.rgx_cohort_phenotypes(None, m._h, cl._h, None, C.byref(out), err, len(err)) == RGX_ERR_ARG and not out
    # no parameters: the defaults
    assert L.rgx_cohort_phenotypes_host(m._h, cl._h, None, C.byref(out), err, len(err)) == 0
    pheno_ref.same(cohort.CohortPhenotypes(out), pheno_ref.phenotypes(m, cl))
    # the text: a buffer that is too small gets nothing, a table of another cohort is refused
    ph, other = cohort.phenotypes_host(m, cl), cohort.phenotypes_host(m2, cl2)
    need = L.rgx_cohort_format_phenotypes(m._h, cl._h, ph._h, None, 0)
    buf = C.create_string_buffer(b"\xaa" * need, need)
    assert L.rgx_cohort_format_phenotypes(m._h, cl._h, ph._h, buf, need - 1) == need and buf.raw == b"\xaa" * need
    assert L.rgx_cohort_format_phenotypes(m._h, cl._h, ph._h, buf, need) == need and buf.raw == ph.text(m, cl)
    assert L.rgx_cohort_format_phenotypes(m._h, cl._h, other._h, None, 0) == 0 and L.rgx_cohort_format_phenotypes(m._h, cl2._h, ph._h, None, 0) == 0
    for x in (m, m2):
        x.close()
    cluster_cases.free_tables(tables + t2)


def test_empty_inputs():
    from regtools_amd import cohort
    m = _matrix([], [])
    cl = cohort.cluster_host(m)
    ph, _ = _check(m, cl)
    assert (ph.n_rows, ph.n_samples, ph.n_clustered, ph.n_drop_na, ph.n_drop_sd) == (0, 0, 0, 0, 0) and ph.rank2.shape == (0, 0)
    assert ph.text(m, cl) == b"#Chr\tstart\tend\tID\n"
    m.close()
    # rows, but none with a cluster
    tables, m, _ = _cohort(pc.counts(3, 6, seed=1))
    cl = cohort.cluster_host(m, min_rows=99)
    ph, _ = _check(m, cl)
    assert (ph.n_rows, ph.n_samples, ph.n_clustered, ph.n_drop_na, ph.n_drop_sd) == (0, 3, 0, 0, 0) and ph.rank2.shape == (0, 3)
    assert ph.text(m, cl) == b"#Chr\tstart\tend\tID\ts000\ts001\ts002\n"
    m.close()
    cluster_cases.free_tables(tables)


def _run(*args):
    return subprocess.run([EXE, "junctions", "cohort"] + list(args), stdout=subprocess.PIPE, stderr=subprocess.PIPE)


def test_tool_option_surface(tmp_path):
    h = _run("-h")
    assert h.returncode == 0
    for opt in (b"\t\t-q FILE\t", b"\t\t-x DEC\t", b"\t\t-d DEC\t", b"prepare_phenotype_table.py", b"\t\t-k FILE\t", b"\t\t-p DEC\t"):
        assert opt in h.stdout, opt
    q = str(tmp_path / "pheno.txt")
    # accepted values let the run get as far as the device it does not find or the file it cannot open
    for x, d in (("0.4", "0.005"), ("1", "0"), ("0", "1e-3"), (".5", "2.5"), ("1.000000000", "0.")):
        r = _run("-s", "XS", "-q", q, "-x", x, "-d", d, "a.bam")
        assert r.returncode == 1 and r.stdout == b"" and b"Unrecognized" not in r.stderr and h.stdout not in r.stderr, (x, d)
        assert not os.path.exists(q)
    for x in ("2", "x", "0.0000000001", "-1", "1.000000001", "", ".", "0.5x", "1e-3"):
        r = _run("-s", "XS", "-q", q, "-x", x, "a.bam")
        assert r.returncode == 1 and r.stdout == b"" and b"Unrecognized ratio argument!" in r.stderr and not os.path.exists(q), x
    for d in ("x", "-1", "-0.5", "", "0.5x", "nan", "1e", "0.005 "):
        r = _run("-s", "XS", "-q", q, "-d", d, "a.bam")
        assert r.returncode == 1 and r.stdout == b"" and b"Unrecognized deviation argument!" in r.stderr and not os.path.exists(q), d
