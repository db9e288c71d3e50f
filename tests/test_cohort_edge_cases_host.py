"""The cohort edge cases on the CPU (tests/cohort_edge_cases.py): for every case the library's host twins equal the restatements in every
array -- cohort.merge_host against cohort_ref.matrix, cohort.cluster_host against cluster_ref.clusters, cohort.refine_host against
refine_ref.refine -- and every case meets its own claims, computed from the restatement's matrix alone.  This is where the cases are proven to
reach the kernel forms, run lengths and filter positions that tests/test_gpu_cohort_edges.py then runs on the device."""
import numpy as np
import pytest

import cluster_ref
import cohort_edge_cases as cases
import cohort_ref
import refine_ref


@pytest.fixture(scope="module")
def loaded():
    """{case name: its samples as tables}, made once and freed at the end."""
    tables = {c.name: cases.load(c.samples) for c in cases.ALL}
    yield tables
    for t in tables.values():
        cases.free(t)


@pytest.mark.parametrize("case", cases.ALL, ids=repr)
def test_twin_equals_the_restatement_and_the_case_meets_its_claims(loaded, case):
    from regtools_amd import cohort
    want = cohort_ref.matrix(case.samples, case.names, **case.params())
    cases.check(case, want)
    m = cohort.merge_host(loaded[case.name], case.names, **case.params())
    cohort_ref.same(m, want)
    for f in case.filters:
        cases.check_filter(want, f)
        kw = case.params(f["min_samples"], f["min_total"])
        got, ref = cohort.merge_host(loaded[case.name], case.names, **kw), cohort_ref.matrix(case.samples, case.names, **kw)
        assert ref.n == f["n_kept"] and np.array_equal(ref.row_begin, np.concatenate([[0], np.cumsum(want.n_with[ref.kept])]))
        cohort_ref.same(got, ref)
    for kw in case.cluster_kw:
        ref = cluster_ref.clusters(want, **kw)
        cases.check_clusters(case, want, ref, kw.get("min_rows", 1))
        cluster_ref.same(cohort.cluster_host(m, **kw), ref)
    for kw in case.refine_kw:
        ref = refine_ref.refine(want, **kw)
        refine_ref.same(cohort.refine_host(m, **kw), ref)
        if not set(kw) - {"min_rows", "min_total"}:                          # parameters that remove nothing: rgx_cohort_cluster's result
            cluster_ref.same_clusters(cohort.refine_host(m, **kw), cohort.cluster_host(m, **kw))
        if kw.get("min_reads") == 1:                                         # exactly the rows nobody has a read on
            zero = want.total == 0
            assert ref["n_weak"] == int(zero.sum()) and (ref["cluster"][zero] == cases.NO).all() and (zero.any() or case not in cases.ZEROS)


def test_the_families_cover_what_they_are_for():
    """Across the cases: both sides of each of the three thresholds at distance 0 and 1, the run lengths of each reduction form, a dropped
    last row, a cluster without a run, a zero entry in a clustered row of a wave-form matrix."""
    claims = {c.name: c.claims for c in cases.ALL}
    for form, margin in (("reduce", "reduce_margin"), ("expand", "expand_margin"), ("sum", "sum_margin")):
        at = {(c[form], c[margin]) for c in claims.values() if form in c and margin in c}
        assert ("wave", 0) in at and ("lane", -1) in at, form
    wave_runs = set().union(*[set(c["runs"]) for c in claims.values() if c.get("reduce") == "wave" and "runs" in c])
    assert {1, 63, 64, 65, 129} <= wave_runs
    assert {7, 8, 9, 17} <= set().union(*[set(c["cs_runs"]) for c in claims.values() if c.get("sum") == "lane"])
    assert {63, 64, 65, 129} <= set().union(*[set(c["cs_runs"]) for c in claims.values() if c.get("sum") == "wave"])
    assert {p for c in claims.values() for p in c.get("run_of_two_at", ())} == {255, 511}
    assert {c["last_is_head"] for c in claims.values() if "last_is_head" in c} == {True, False}
    assert any(c.get("expand") == "wave" and c.get("zeros_in_clustered_rows") for c in claims.values())
    for c in cases.FILTERS:
        assert any(f.get("last_dropped") and f["n_kept"] for f in c.filters) and any(f["n_kept"] == 0 for f in c.filters)
        assert any(f.get("exact") and f["min_total"] > cases.P32 for f in c.filters) and any(f.get("exact") and f["min_total"] < cases.P32 for f in c.filters)
    middle = [z for c in cases.WIDTHS for z in c.claims["no_run_clusters"][1] if 0 < z < c.claims["n_clusters"][1] - 1]
    assert middle and all(0 in c.claims["no_run_clusters"][1] for c in cases.WIDTHS)


def test_second_finish_shapes_exist():
    for name, front in cases.SECOND_FINISH:
        assert len(cases.by_name(name).samples) == front + 3


# ---- Pipeline.wait keeps the ticket's buffers until the library has returned -------------------------------------------------------------
class _StandIn(object):
    """A library of which Pipeline.wait needs three functions; rgx_extract_wait records what the pipeline still holds during the call."""

    def __init__(self, rc):
        self.rc, self.pipeline, self.seen = rc, None, []

    def rgx_extract_wait(self, handle, ticket, tab, err, errlen):
        self.seen.append(self.pipeline._open.get(ticket))
        return self.rc

    def rgx_pipeline_ctx(self, handle, ticket):
        return 0

    def rgx_pipeline_destroy(self, handle):
        pass


@pytest.mark.parametrize("rc", [0, 3])
def test_wait_holds_the_buffers_until_the_library_returns(rc):
    import ctypes as C
    import regtools_amd
    from regtools_amd import extractor
    lib = _StandIn(rc)
    pl = extractor.Pipeline.__new__(extractor.Pipeline)
    pl._lib, pl._h, pl._open = lib, C.c_void_p(), {}
    lib.pipeline = pl
    je = extractor.JunctionsExtractor(strandness=0)
    bam, bai = bytes(bytearray(b"not really a BAM") * 4), bytes(bytearray(b"nor an index") * 4)
    pl._open[7] = (je, bam, bai)
    if rc:
        with pytest.raises(regtools_amd.RegtoolsError):
            pl.wait(7)
    else:
        with pytest.raises(ValueError):                                      # (the stand-in hands no table back: a NULL pointer is read)
            pl.wait(7)
    assert len(lib.seen) == 1 and lib.seen[0] is not None and lib.seen[0][1] is bam and lib.seen[0][2] is bai
    assert 7 not in pl._open                                                  # ... and let go of afterwards, whether the call succeeded or not
    with pytest.raises(KeyError):
        pl.wait(8)                                                            # a ticket this pipeline never gave out
    assert len(lib.seen) == 1
