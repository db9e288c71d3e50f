"""The integer kernels between the stages on the device, at their edges: csrc/cohort_kernels.hip (append, key gather, heads, row start,
k_cohort_reduce<1|64>, rows out, CSR) and the denominator half of csrc/cluster_kernels.hip (k_cluster_row_len<1|64>, k_cluster_expand<1|64>,
k_cluster_cs_heads, k_cluster_cs_sum<8|64>, k_cluster_cs_begin, k_cluster_widen), through Cohort.add, finish, cluster and refine.  The inputs are
the cases of tests/cohort_edge_cases.py; the expectations are the numpy restatements (tests/cohort_ref.py, cluster_ref.py, refine_ref.py), which
tests/test_cohort_edge_cases_host.py holds against the library's host twins on the CPU.  Every comparison is exact, and every case proves its
claims -- the kernel form it takes, its distance from the threshold, its run lengths, its zeros -- again from the device's own matrix."""
import ctypes as C

import numpy as np
import pytest

import bamio
import cluster_ref
import cohort_edge_cases as cases
import cohort_ref
import refine_ref

pytestmark = pytest.mark.gpu

_WANT = {}


def _want(case, min_samples=1, min_total=0):
    """The restatement's matrix, computed once per case and filter pair."""
    key = (case.name, min_samples, min_total)
    if key not in _WANT:
        _WANT[key] = cohort_ref.matrix(case.samples, case.names, **case.params(min_samples, min_total))
    return _WANT[key]


@pytest.fixture(scope="module")
def loaded():
    """{case name: its samples as tables}, made once and freed at the end."""
    tables = {c.name: cases.load(c.samples) for c in cases.ALL}
    yield tables
    for t in tables.values():
        cases.free(t)


@pytest.fixture(scope="module")
def elsewhere(gpu_ctx):
    """A cohort without samples: a matrix it clusters is somebody else's, and is uploaded (cluster path 0)."""
    import regtools_amd
    co = regtools_amd.Cohort(ctx=gpu_ctx)
    yield co
    co.close()


def _cohort(gpu_ctx, samples, names, **params):
    import regtools_amd
    co = regtools_amd.Cohort(ctx=gpu_ctx, **params)
    for k, (s, nm) in enumerate(zip(samples, names)):
        assert co.add(s, nm) == k
    assert co.add_paths == [0] * len(names)
    return co


def _same_matrix(a, b):
    assert (a.n, a.n_samples, a.n_triples, a.ref_name, a.ref_len, a.sample_name) == (b.n, b.n_samples, b.n_triples, b.ref_name, b.ref_len, b.sample_name)
    for k in cohort_ref.FIELDS + ("strand",):
        assert np.array_equal(getattr(a, k), getattr(b, k)), k


def _clusters_on_both_paths(co, elsewhere, m, want, case, check=True):
    """cluster and refine of the matrix m of co's most recent finish: read in place (path 1), then uploaded through another cohort (path 0)."""
    for who, path in ((co, 1), (elsewhere, 0)):
        for kw in case.cluster_kw:
            cl = who.cluster(m, **kw)
            assert who.cluster_paths[-1] == path
            cluster_ref.same(cl, cluster_ref.clusters(want, **kw))
            if check:
                cases.check_clusters(case, m, cl, kw.get("min_rows", 1))
        for kw in case.refine_kw:
            rf = who.refine(m, **kw)
            assert who.cluster_paths[-1] == path
            ref = refine_ref.refine(want, **kw)
            refine_ref.same(rf, ref)
            if not set(kw) - {"min_rows", "min_total"}:                      # parameters that remove nothing: rgx_cohort_cluster's result
                cluster_ref.same_clusters(rf, who.cluster(m, **kw))
            if kw.get("min_reads") == 1:                                     # exactly the rows nobody has a read on
                zero = m.total == 0
                assert rf.n_weak == int(zero.sum()) and (rf.cluster[zero] == cases.NO).all()


@pytest.mark.parametrize("case", cases.ACCUMULATE + cases.CLUSTER, ids=repr)
def test_matrix_clusters_and_refinement(gpu_ctx, loaded, elsewhere, case):
    """Items 1, 2 (uploaded), 3 and 6 of the accumulate cases and 7 to 11 of the cluster cases: the whole chain of one case, both cluster paths."""
    want = _want(case)
    co = _cohort(gpu_ctx, loaded[case.name], case.names, **case.params())
    m = co.finish()
    cohort_ref.same(m, want)
    cases.check(case, m)
    _clusters_on_both_paths(co, elsewhere, m, want, case)
    co.close()


@pytest.mark.parametrize("case,f", [(c, f) for c in cases.FILTERS for f in c.filters], ids=lambda x: x["name"] if isinstance(x, dict) else repr(x))
def test_filters(gpu_ctx, loaded, elsewhere, case, f):
    """Item 4: min_samples and min_total on a lane-form and a wave-form matrix; the pair's claims come from the device's unfiltered matrix."""
    base = _cohort(gpu_ctx, loaded[case.name], case.names, **case.params())
    m = base.finish()
    cohort_ref.same(m, _want(case))
    cases.check(case, m)
    cases.check_filter(m, f)
    want = _want(case, f["min_samples"], f["min_total"])
    co = _cohort(gpu_ctx, loaded[case.name], case.names, **case.params(f["min_samples"], f["min_total"]))
    got = co.finish()
    assert got.n == f["n_kept"] and int(got.row_begin[-1]) == int(m.n_with[want.kept].sum()) and got.n_triples == m.n_triples
    cohort_ref.same(got, want)
    _clusters_on_both_paths(co, elsewhere, got, want, case, check=False)
    base.close(); co.close()


class _TableSample(object):
    """The rows of an extractor's table as cohort_ref.matrix reads a sample."""

    def __init__(self, je, contigs):
        t = je.table.contents
        n = int(t.n)
        self.contigs, self.min_anchor = contigs, je.min_anchor_length_
        assert [(t.ref_name[i].decode(), int(t.ref_len[i])) for i in range(t.n_ref)] == contigs
        self.tid, self.start, self.end, self.thick_start, self.thick_end, self.count = (
            np.ctypeslib.as_array(p, shape=(n,)).astype(np.int64) for p in (t.tid, t.start, t.end, t.thick_start, t.thick_end, t.read_count))
        self.strand = np.frombuffer(C.string_at(t.strand, n), np.uint8).astype(np.int64)


class _Uploaded(object):
    """An extractor's table without its context: Cohort.add uploads it."""

    def __init__(self, je):
        self.table, self.min_anchor_length_, self._ctx = je.table, je.min_anchor_length_, None


def test_append_waves_from_a_context_and_uploaded(gpu_ctx, tmp_path):
    """Item 2 on add path 1 (the ten-column block an extraction leaves in its context's HBM, strand column 9): the append-waves table as a
    small BAM extracted on the cohort's own context, then the same rows uploaded (strand column 6)."""
    import regtools_amd
    from regtools_amd import synth
    p = str(tmp_path / "waves.bam")
    bamio.write_bam(p, cases.WAVE_BAM_CONTIGS, cases.wave_bam_records())
    synth.index(p)
    je = regtools_amd.JunctionsExtractor(bam=p, strandness=0, ctx=gpu_ctx)
    je.identify_junctions_from_BAM()
    s = _TableSample(je, cases.WAVE_BAM_CONTIGS)
    rows = cases.wave_rows()
    for j, k in enumerate(("tid", "start", "end", "thick_start", "thick_end", "count")):
        assert getattr(s, k).tolist() == [r[j] for r in rows], k
    assert s.strand.tolist() == [ord(r[6]) for r in rows]
    assert cases.wave_masks(s)[:5] == cases.WAVE_MASKS and len(rows) % 64 == 37
    co = regtools_amd.Cohort(ctx=gpu_ctx)
    co.add(je, "bam")
    assert co.add_paths == [1]
    m1 = co.finish()
    up = regtools_amd.Cohort(ctx=gpu_ctx)
    up.add(_Uploaded(je), "bam")
    assert up.add_paths == [0]
    m0 = up.finish()
    _same_matrix(m1, m0)
    want = cohort_ref.matrix([s], ["bam"], only_anchored=True, min_samples=1, min_total=1)
    assert want.n == want.n_triples == int(cohort_ref.anchored(s).sum()) == 1 + 1 + 64 + 32 + 64 + 13
    cohort_ref.same(m1, want)
    co.close(); up.close()


@pytest.mark.parametrize("name,front", cases.SECOND_FINISH)
def test_a_second_finish_equals_a_fresh_cohort(gpu_ctx, loaded, name, front):
    """Item 5: three more adds behind a finish, on the shapes that reduce a row per wave."""
    case = cases.by_name(name)
    tables = loaded[name]
    co = _cohort(gpu_ctx, tables[:front], case.names[:front], **case.params())
    m1 = co.finish()
    cohort_ref.same(m1, cohort_ref.matrix(case.samples[:front], case.names[:front], **case.params()))
    for s, nm in zip(tables[front:], case.names[front:]):
        co.add(s, nm)
    m2 = co.finish()
    cohort_ref.same(m2, _want(case))
    cases.check(case, m2)
    fresh = _cohort(gpu_ctx, tables, case.names, **case.params())
    _same_matrix(m2, fresh.finish())
    co.close(); fresh.close()
