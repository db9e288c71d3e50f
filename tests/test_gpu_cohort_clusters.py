"""The intron clusters of a cohort matrix on the device (csrc/cluster_kernels.hip, csrc/cohort_cluster.cpp): site sorts, edges, the hook + jump
component search, the per-cluster sums and the keyed sort of the count entries.  Expectations: the literals of tests/cluster_cases.py, the library's
host twin and the Python union-find of tests/cluster_ref.py.  Every comparison is exact."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import cluster_cases as cases
import cluster_ref
from cohort_common import STRANDNESS, cohort_files, table_from_rows  # noqa: F401  (cohort_files is a fixture)

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "bin", "regtools-amd")
ERRLEN = 512


def _cohort_of(gpu_ctx, tables, names, **kw):
    import regtools_amd
    co = regtools_amd.Cohort(ctx=gpu_ctx, **kw)
    for t, nm in zip(tables, names):
        co.add(cases.Sample(t), nm)
    return co


def _literal(cl, m, want):
    assert (cl.n_rows, cl.n_clusters, cl.n_components) == (len(want["cluster"]), len(want["cl_total"]), want["n_components"])
    for k in ("cluster", "cl_begin", "cl_row", "cl_total", "cs_begin", "cs_sample", "cs_total"):
        assert [int(x) for x in getattr(cl, k)] == want[k], k
    assert cl.counts_text(m).decode().splitlines() == want["text"]


def test_hand_made_cohort_on_both_paths(gpu_ctx):
    from regtools_amd import cohort
    tables = [table_from_rows(cases.HAND_P), table_from_rows(cases.HAND_Q)]
    co = _cohort_of(gpu_ctx, tables, ["p", "q"], only_anchored=False)
    m = co.finish()
    cl = co.cluster(m)                                        # straight behind the finish: read where it lies
    assert co.cluster_paths == [1] and cl.n_rounds >= 1
    _literal(cl, m, cases.HAND)
    twin = cohort.cluster_host(m)
    cluster_ref.same_clusters(cl, twin)
    f = co.cluster(m, min_rows=2)
    _literal(f, m, cases.HAND_MIN_ROWS_2)
    for kw in (dict(min_total=3), dict(min_total=4), dict(min_rows=2, min_total=4), dict(min_rows=3, min_total=11), dict(min_rows=4)):
        a, b = co.cluster(m, **kw), cohort.cluster_host(m, **kw)
        cluster_ref.same_clusters(a, b)
        assert a.counts_text(m) == b.counts_text(m)
    assert co.cluster_paths == [1] * 7
    # a merge_host matrix is uploaded, and so is the matrix of a finish that is no longer the most recent one
    h = cohort.merge_host([cases.Sample(t) for t in tables], ["p", "q"], only_anchored=False)
    up = co.cluster(h)
    assert co.cluster_paths[-1] == 0
    _literal(up, h, cases.HAND)
    co.add(cases.Sample(table_from_rows([(0, 100, 900, 90, 930, 2, "+")])), "r")          # joins the cluster of three through its start
    m2 = co.finish()
    old, new = co.cluster(m), co.cluster(m2)
    assert co.cluster_paths[-2:] == [0, 1]
    _literal(old, m, cases.HAND)
    assert list(new.cluster) == [0, 1, 0, 0, 0, 2, 3, 3, 4] and [int(x) for x in new.cl_total] == [12, 5, 6, 3, 7]
    cluster_ref.same_clusters(new, cohort.cluster_host(m2))
    cluster_ref.same(new, cluster_ref.clusters(m2))
    co.close()
    cases.free_tables(tables)


def test_filters_that_keep_no_cluster(gpu_ctx):
    """Rows and components, but no cluster, no member row and no denominator: every copy back but the rows' cluster numbers and the two
    begin arrays is empty."""
    from regtools_amd import cohort
    tables = [table_from_rows(cases.HAND_P), table_from_rows(cases.HAND_Q)]
    co = _cohort_of(gpu_ctx, tables, ["p", "q"], only_anchored=False)
    m = co.finish()
    for path, mat in ((1, m), (0, cohort.merge_host([cases.Sample(t) for t in tables], ["p", "q"], only_anchored=False))):
        a, b = co.cluster(mat, min_rows=99), cohort.cluster_host(mat, min_rows=99)
        assert co.cluster_paths[-1] == path
        cluster_ref.same_clusters(a, b)
        assert (a.n_clusters, len(a.cl_row), len(a.cs_sample), len(a.cs_total)) == (0, 0, 0, 0) and a.n_components > 0
        assert (a.cluster == 0xffffffff).all() and list(a.cl_begin) == [0] and list(a.cs_begin) == [0]
        assert a.counts_text(mat) == b.counts_text(mat) == b"chrom p q\n"
    co.close()
    cases.free_tables(tables)


def test_empty_matrix_and_a_cohort_without_samples(gpu_ctx):
    import regtools_amd
    from regtools_amd import cohort
    co = regtools_amd.Cohort(ctx=gpu_ctx)
    m = co.finish()
    cl = co.cluster(m)
    assert (cl.n_rows, cl.n_clusters, cl.n_components) == (0, 0, 0) and list(cl.cl_begin) == [0] and list(cl.cs_begin) == [0]
    assert cl.counts_text(m) == b"chrom\n" and co.cluster_paths == [1]
    # the cohort has no samples; the matrix it clusters is somebody else's
    tables = [table_from_rows(cases.HAND_P), table_from_rows(cases.HAND_Q)]
    h = cohort.merge_host([cases.Sample(t) for t in tables], ["p", "q"], only_anchored=False)
    _literal(co.cluster(h), h, cases.HAND)
    assert co.cluster_paths == [1, 0]
    # zero counts give no denominator
    z = [table_from_rows([(0, 100, 200, 90, 230, 0, "+"), (0, 100, 250, 90, 260, 0, "+")]), table_from_rows([(0, 100, 200, 90, 230, 2, "+")])]
    hz = cohort.merge_host([cases.Sample(t) for t in z], ["zero", "two"], only_anchored=False, min_total=0)
    cz = co.cluster(hz)
    assert list(cz.cs_sample) == [1] and list(cz.cs_total) == [2] and cz.counts_text(hz) == b"chrom zero two\nchrA:100:200:clu_1_+ 0/0 2/2\nchrA:100:250:clu_1_+ 0/0 0/2\n"
    cluster_ref.same_clusters(cz, cohort.cluster_host(hz))
    co.close()
    cases.free_tables(tables + z)


# ---- the random cohort: singletons, small clusters and giant ones in one input ---------------------------------------------------------
G = 24
FILTERS = [dict(), dict(min_rows=2, min_total=25)]


@pytest.fixture(scope="module")
def random_cohort(gpu_ctx):
    """(cohort, its matrix straight behind the finish, {filter index: the restatement})"""
    tid, start, end, cls = cases.random_junctions()
    label = cluster_ref.row_labels(tid, start, end, np.array([b"+", b"-", b"?"])[cls])
    sizes = np.bincount(label)
    big_row, second = [int(r) for r in np.flatnonzero(label == np.argmax(sizes))[:2]]          # the two lowest rows of the largest component
    assert sizes.max() > 1024
    # one row counts 4,000,000,000 in two samples (the cluster's total passes 2^32); 4,000,000,000 is itself below 2^32, so a second row of the
    # cluster counts as much in the first of the two samples: that sample's cs_total passes 2^32 as well
    tables = cases.sample_tables(G, tid, start, end, cls, big={big_row: (big_row % G, (big_row + 1) % G), second: (big_row % G,)})
    co = _cohort_of(gpu_ctx, tables, ["g%02d" % g for g in range(G)])
    m = co.finish()
    assert m.n == len(tid) == 199_998 and np.array_equal(m.start, start) and np.array_equal(m.end, end) and 2_000_000 < int(m.row_begin[-1]) < 3_000_000
    want = [cluster_ref.clusters(m, **kw) for kw in FILTERS]
    yield co, m, want, big_row
    co.close()
    cases.free_tables(tables)


@pytest.mark.parametrize("which", [0, 1])
def test_random_cohort(gpu_ctx, random_cohort, which):
    import regtools_amd
    from regtools_amd import cohort
    co, m, wants, big_row = random_cohort
    kw, want = FILTERS[which], wants[which]
    cl = co.cluster(m, **kw)
    assert co.cluster_paths[-1] == 1
    print("random cohort %s: %d components, %d clusters, %d rounds, %.3f ms" % (kw, cl.n_components, cl.n_clusters, cl.n_rounds, cl.ms_cluster))
    cluster_ref.same(cl, want)
    twin = cohort.cluster_host(m, **kw)
    cluster_ref.same_clusters(cl, twin)
    assert cl.counts_text(m) == twin.counts_text(m) == cluster_ref.counts_text(m, want)
    if which == 0:
        sizes = np.diff(cl.cl_begin)
        assert (sizes > 1024).sum() >= 5 and (sizes == 1).sum() >= 10_000 and (sizes >= 2).sum() >= 10_000
        assert sizes[int(cl.cluster[big_row])] == sizes.max()
        assert int(cl.cs_total.max()) > 2**32 and int(cl.cl_total.max()) > 2**32 and int(m.val_count.max()) == 4_000_000_000
    else:
        assert 0 < cl.n_clusters < cl.n_components and (cl.cluster == cases.NO).sum() >= 10_000
    # the same matrix through a cohort that never saw it: uploaded, same result
    other = regtools_amd.Cohort(ctx=gpu_ctx)
    up = other.cluster(m, **kw)
    assert other.cluster_paths == [0]
    cluster_ref.same_clusters(up, cl)
    other.close()


def test_scrambled_staircase_takes_few_rounds(gpu_ctx):
    """65,536 rows in one component of diameter 65,536: propagation by one hop per round would need that many rounds, pointer jumping about
    bitlen(L)."""
    tid, start, end, cls = cases.staircase()
    L = len(tid)
    t = cases.table_of(0, tid, start, end, 1 + np.arange(L) % 9, np.full(L, ord("+"), np.uint32))
    co = _cohort_of(gpu_ctx, [t], ["only"])
    m = co.finish()
    assert m.n == L
    # (the matrix is in (start, end) order and the starts are a permutation: along the staircase the row indices are scrambled)
    cl = co.cluster(m)
    print("staircase: n_rounds = %d for %d rows" % (cl.n_rounds, L))
    assert cl.n_clusters == cl.n_components == 1 and np.array_equal(cl.cl_row, np.arange(L)) and list(cl.cl_begin) == [0, L]
    assert cl.n_rounds * 16 <= L
    assert int(cl.cl_total[0]) == int(m.total.sum()) and list(cl.cs_sample) == [0] and int(cl.cs_total[0]) == int(m.total.sum())
    co.close()
    cases.free_tables([t])


# ---- rgx_k_components on the caller's edge list ------------------------------------------------------------------------------------------
def _dev(a):
    import torch
    a = np.ascontiguousarray(a, dtype=np.uint32)
    return torch.from_numpy(a.view(np.int32)).cuda()


def _components(gpu_ctx, n, a, b):
    import torch
    from regtools_amd import _ffi
    d_a, d_b = _dev(a), _dev(b)
    d_out = _dev(np.full(n, 0xdeadbeef, dtype=np.uint32))
    rounds = C.c_uint32(0)
    err = C.create_string_buffer(ERRLEN)
    torch.cuda.synchronize()                                 # the context's stream does not wait for torch's
    rc = _ffi.lib().rgx_k_components(gpu_ctx._h, n, len(a), d_a.data_ptr() if len(a) else None, d_b.data_ptr() if len(b) else None,
                                     d_out.data_ptr() if n else None, C.byref(rounds), err, ERRLEN)
    assert rc == 0, err.value                                # (RGX_ERR_DEVICE: a guard word behind the scratch changed)
    assert np.array_equal(d_a.cpu().numpy().view(np.uint32), np.asarray(a, np.uint32))
    return d_out.cpu().numpy().view(np.uint32), rounds.value


def _path(ids):
    return ids[:-1], ids[1:]


def _component_cases():
    rng = np.random.default_rng(31)
    none = np.zeros(0, np.uint32)
    out = [("no_vertices", 0, none, none), ("zero_edges", 5, none, none), ("one_edge", 4, [3], [1]), ("self_loops", 6, [0, 2, 5, 2], [0, 2, 5, 4]),
           ("duplicate_edges", 7, [1, 1, 6, 1, 6], [6, 6, 1, 6, 3]), ("star_centre_last", 3000, np.full(2999, 2999), np.arange(2999))]
    for n in (1, 2, 255, 256, 257, 65_537):
        out.append(("scrambled_path_%d" % n,) + (n,) + _path(rng.permutation(n)))
    ids = rng.permutation(1000)
    a0, b0 = _path(ids[:600])
    a1, b1 = _path(ids[600:])
    out.append(("two_disjoint_paths", 1000, np.concatenate([a0, a1]), np.concatenate([b0, b1])))
    return out


@pytest.mark.parametrize("case", _component_cases(), ids=lambda c: c[0])
def test_components_against_a_union_find(gpu_ctx, case):
    _, n, a, b = case
    a, b = np.asarray(a, np.uint32), np.asarray(b, np.uint32)
    got, rounds = _components(gpu_ctx, n, a, b)
    assert np.array_equal(got, cluster_ref.components(n, a, b))
    assert (rounds >= 1) == (n > 0) and rounds <= 64         # (pointer jumping: a path of 65,537 scrambled ids settles in well under 64 rounds)


# ---- real tables: the ten-BAM cohort through the pipeline, and the tool -------------------------------------------------------------------
def _items(samples):
    return [(s["path"], s["name"], dict(strandness=STRANDNESS[s["strand"]])) for s in samples]


def test_ten_bam_cohort_and_the_tool(gpu_ctx, cohort_files, tmp_path):  # noqa: F811
    import regtools_amd
    from regtools_amd import cohort
    co = regtools_amd.Cohort(ctx=gpu_ctx)
    co.run(_items(cohort_files))
    m = co.finish()
    cl = co.cluster(m)
    assert co.cluster_paths == [1] and cl.n_clusters == cl.n_components > 100
    want = cluster_ref.clusters(m)
    cluster_ref.same(cl, want)
    cluster_ref.same_clusters(cl, cohort.cluster_host(m))
    text = cl.counts_text(m)
    assert text == cluster_ref.counts_text(m, want)
    two = co.cluster(m, min_rows=2)
    cluster_ref.same_clusters(two, cohort.cluster_host(m, min_rows=2))
    # the tool: the ten files are all -s XS there, so compare against a cohort extracted the same way
    xs = [s for s in cohort_files if s["strand"] == "XS"][:4]
    cx = regtools_amd.Cohort(ctx=gpu_ctx)
    cx.run(_items(xs))
    mx = cx.finish()
    all_text, two_text = cx.cluster(mx).counts_text(mx), cx.cluster(mx, min_rows=2).counts_text(mx)
    bed, k = str(tmp_path / "x.bed"), str(tmp_path / "x.clusters")
    r = subprocess.run([EXE, "junctions", "cohort", "-s", "XS", "-o", bed, "-k", k] + [s["path"] for s in xs], stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert r.returncode == 0 and r.stdout == b"", r.stderr[-2000:]
    assert open(k, "rb").read() == all_text and open(bed, "rb").read() == mx.bed12()
    r = subprocess.run([EXE, "junctions", "cohort", "-s", "XS", "-o", bed, "-k", k, "-K", "2"] + [s["path"] for s in xs], stdout=subprocess.PIPE,
                       stderr=subprocess.PIPE)
    assert r.returncode == 0, r.stderr[-2000:]
    assert open(k, "rb").read() == two_text and 0 < len(two_text) < len(all_text)
    # a file that fails: its error, exit 1, no output files
    os.remove(bed); os.remove(k)
    r = subprocess.run([EXE, "junctions", "cohort", "-s", "XS", "-o", bed, "-k", k, xs[0]["path"], str(tmp_path / "absent.bam"), xs[1]["path"]],
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert r.returncode == 1 and b"Unable to open BAM/SAM file." in r.stderr and not os.path.exists(bed) and not os.path.exists(k)
    co.close(); cx.close()
