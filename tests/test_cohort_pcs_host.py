"""The principal components of the phenotype table without a device: the contract of rgx_cohort_pheno_pcs in include/regtools_amd.h as
rgx_cohort_pheno_pcs_host (the library's plain C++ twin) keeps it, and the text.  Expectations: the restatement of tests/pca_ref.py -- the Gram
matrix and the column sums as bit patterns against exact fused multiply-adds in the contract's order -- and sklearn's PCA, the library LeafCutter
calls, for the eigenvalues and the components.  The tolerance constant C_TOL: tests/pca_ref.py."""
import numpy as np
import pytest

import cluster_cases
import pca_cases as pca
import pca_ref as ref
import pheno_cases as pc

RGX_ERR_ARG = 7
EPS, C_TOL = ref.EPS, ref.C_TOL
same_bits, same_pcs, check_structure, check_residual = ref.same_bits, ref.same_pcs, ref.check_structure, ref.check_residual


def _twin(rank2, n_pcs):
    from regtools_amd import cohort
    return cohort.pheno_pcs_host(cohort.pheno_table_from_rank2(rank2), n_pcs)


@pytest.mark.parametrize("K, S", [(2, 2), (40, 5), (16, 1), (1025, 9)])
def test_gram_and_column_sums_are_the_contract_s_bits(K, S):
    """(1025, 9): two uneven chunks, 513 + 512 rows."""
    from regtools_amd import cohort
    r2 = pca.random_rank2(K, S, seed=K * 100 + S) if (K, S) != (1025, 9) else pca.shape(1025, 9, 4, True)
    if (K, S) == (1025, 9):
        assert ref.chunks(K) == [(0, 513), (513, 1025)]
    p = _twin(r2, 1)
    gram, col = ref.gram_exact(ref.quantiles(r2, cohort.quantile))
    same_bits(p.gram, gram)
    same_bits(p.col_sum, col)


@pytest.mark.parametrize("K, S, n_f, ties", pca.SHAPES)
def test_planted_components_against_sklearn(K, S, n_f, ties):
    from regtools_amd import cohort
    r2 = pca.shape(K, S, n_f, ties)
    n = min(n_f, S - 1)
    ev, comp = ref.sklearn_pca(ref.quantiles(r2, cohort.quantile))
    # the precondition: the compared components are well defined
    assert (-np.diff(ev[:n + 1]) >= pca.MIN_GAP * ev[0]).all()
    p = _twin(r2, n)
    assert (p.n_rows, p.n_samples, p.n_pcs) == (K, S, n) and p.component.shape == (n, S) and p.variance.shape == (S,)
    check_structure(p)
    scale = S * EPS * ev[0]
    d_ev = np.abs(p.variance - ev[:S]).max()
    print("(%d, %d)%s: eigenvalues off by %.3f S eps lambda_1" % (K, S, " ties" if ties else "", d_ev / scale))
    assert d_ev <= C_TOL * scale
    gaps = ref.neighbour_gaps(ev)
    for i in range(n):
        d = np.abs(ref.aligned(p.component[i], comp[i]) - comp[i]).max()
        print("  component %d off by %.3f S eps lambda_1 / gap" % (i + 1, d / (scale / gaps[i])))
        assert d <= C_TOL * scale / gaps[i], i
        assert np.dot(p.component[i], comp[i]) > 0             # (sklearn's sign rule is the contract's: no alignment was needed)
    check_residual(p, C_TOL * scale)


def test_all_components_and_a_table_without_structure():
    """n_pcs = min(K, S) both ways round; the residual does not need gaps."""
    for K, S in ((40, 5), (3, 7)):
        r2 = pca.random_rank2(K, S, seed=K + S)
        p = _twin(r2, min(K, S))
        check_structure(p)
        check_residual(p, C_TOL * S * EPS * p.variance[0])
        assert p.n_pcs == min(K, S)


def _cohort_table():
    from regtools_amd import cohort
    count = pc.counts(9, 41, seed=9, absent=0.2)
    tables = pc.tables(count)
    m = cohort.merge_host([cluster_cases.Sample(t) for t in tables], pc.names(9))
    cl = cohort.cluster_host(m)
    return tables, m, cohort.phenotypes_host(m, cl, max_missing=(1, 1), min_sd=0.0)


def test_a_cohort_s_table_and_the_text():
    from regtools_amd import cohort
    tables, m, ph = _cohort_table()
    assert ph.n_rows == 41 and ph.n_samples == 9
    p = cohort.pheno_pcs_host(ph, 4)
    same_pcs(p, _twin(ph.rank2, 4))                            # (the wrapped array is the same table)
    check_structure(p)
    check_residual(p, C_TOL * 9 * EPS * p.variance[0])
    gram, col = ref.gram_exact(ph.quantiles())
    same_bits(p.gram, gram)
    same_bits(p.col_sum, col)
    assert p.text(m) == ref.text(m.sample_name, p.component)
    assert p.text(m).count(b"\n") == 5 and p.text(m).startswith(b"id\ts000\ts001\t")
    # the buffer protocol: the size without a buffer, nothing written into one that is too small
    import ctypes as C
    from regtools_amd import _ffi
    fn = _ffi.lib().rgx_cohort_format_pheno_pcs
    n = fn(m._h, p._h, None, 0)
    small = C.create_string_buffer(b"\x7f" * 8, 8)
    assert n == len(p.text(m)) and fn(m._h, p._h, small, 8) == n and small.raw == b"\x7f" * 8
    assert _twin(pca.random_rank2(5, 3, 1), 1).text(m) == b""  # not of this matrix's samples
    cluster_cases.free_tables(tables)


def test_argument_errors():
    from regtools_amd import RegtoolsError
    r2 = pca.random_rank2(6, 4, seed=3)

    def refused(rank2, n_pcs):
        with pytest.raises(RegtoolsError) as e:
            _twin(rank2, n_pcs)
        assert e.value.code == RGX_ERR_ARG, (rank2.shape, n_pcs)
    refused(r2[:1], 1)                                           # K < 2
    refused(np.zeros((0, 4), np.uint32), 1)
    refused(np.zeros((6, 0), np.uint32), 1)                      # S == 0
    refused(r2, 0)
    refused(r2, 5)                                               # n_pcs > S
    refused(pca.random_rank2(3, 4, seed=3), 4)                   # n_pcs > K
    refused(np.full((2, 2049), 2, np.uint32), 1)                 # S > 2048
    for bad in (0, 1, 13, 0xffffffff):                           # rank2 outside [2, 2 K]
        b = r2.copy()
        b[4, 2] = bad
        refused(b, 2)
    for edge in (2, 12):                                         # ... and its two ends inside
        b = r2.copy()
        b[4, 2] = edge
        assert _twin(b, 2).n_pcs == 2
    assert _twin(np.full((2, 2048), 3, np.uint32), 1).n_samples == 2048      # (a constant table: every eigenvalue 0)
