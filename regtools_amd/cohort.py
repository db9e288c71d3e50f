"""The cohort junction-by-sample count matrix (rgx_cohort_* in include/regtools_amd.h): the union of many samples' junctions with one read-count
column per sample -- the table a cohort run builds after its loop around `regtools junctions extract` (junctions_main.cc:45-59); the reference has
no counterpart.  Rows are accumulated and merged in HBM (csrc/cohort_kernels.hip); `merge_host` is the library's plain C++ twin of the same contract.
"""
import ctypes as C
import os

from . import _ffi
from .extractor import Context, PinnedBuffer, Pipeline, RegtoolsError


def _params(only_anchored, min_samples, min_total):
    p = _ffi.CohortParams()
    _ffi.lib().rgx_cohort_params_default(C.byref(p))
    p.only_anchored, p.min_samples, p.min_total = (1 if only_anchored else 0), min_samples, min_total
    return p


def _text(fn, *args):
    """fn(*args, buf, cap) twice: once for the size, once into a buffer of it."""
    n = fn(*args, None, 0)
    buf = C.create_string_buffer(n + 1)
    fn(*args, buf, n)
    return buf.raw[:n]


def _call(fn, out_type, wrap, *args):
    """fn(*args, &out, err, len(err)) with out a pointer to out_type: RegtoolsError on a code, else wrap(out)."""
    out = C.POINTER(out_type)()
    err = C.create_string_buffer(512)
    rc = fn(*args, C.byref(out), err, len(err))
    if rc != 0:
        raise RegtoolsError(rc, err.value.decode())
    return wrap(out)


class _Owned(object):
    """A result handle the library allocated and this object owns: _free names the function that gives it back."""
    _free = None

    def __init__(self, handle):
        self._lib = _ffi.lib()
        self._h = handle

    @staticmethod
    def _view(ptr, k, dtype):
        import numpy as np               # (only the results need it: importing the package does not)
        return np.ctypeslib.as_array(ptr, shape=(k,)) if k else np.zeros(0, dtype)

    def close(self):
        if self._h:
            getattr(self._lib, self._free)(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def _qtl_text(fn, result, matrix, clusters, ph, var_pos, variant_ids):
    import numpy as np
    pos = np.ascontiguousarray(var_pos, dtype=np.uint32)
    ids = (C.c_char_p * max(len(variant_ids), 1))(*[v if isinstance(v, bytes) else v.encode() for v in variant_ids])
    if len(pos) != result.n_variants or len(variant_ids) != result.n_variants:
        raise ValueError("one position and one id per variant")
    return _text(fn, matrix._h, clusters._h, ph._h, result._h, pos.ctypes.data, ids)


class CohortMatrix(_Owned):
    """rgx_cohort_matrix.  The array attributes are numpy VIEWS of memory this object owns: copy what must outlive it."""

    _free = "rgx_cohort_matrix_free"

    def __init__(self, handle):
        import numpy as np
        _Owned.__init__(self, handle)
        m = handle.contents
        self.n, self.n_samples, self.n_triples = int(m.n), int(m.n_samples), int(m.n_triples)
        self.ms_add_total, self.ms_finish = m.ms_add_total, m.ms_finish
        self.ref_name = [m.ref_name[i].decode() for i in range(m.n_ref)]
        self.ref_len = [int(m.ref_len[i]) for i in range(m.n_ref)]
        self.sample_name = [m.sample_name[i].decode() for i in range(m.n_samples)]
        nnz = int(m.row_begin[self.n])
        view = self._view
        self.tid, self.start, self.end = view(m.tid, self.n, np.uint32), view(m.start, self.n, np.uint32), view(m.end, self.n, np.uint32)
        self.thick_start, self.thick_end = view(m.thick_start, self.n, np.uint32), view(m.thick_end, self.n, np.uint32)
        self.n_with, self.total = view(m.n_with, self.n, np.uint32), view(m.total, self.n, np.uint64)
        self.strand = np.frombuffer(C.string_at(m.strand, self.n), dtype="S1") if self.n else np.zeros(0, "S1")
        self.row_begin = np.ctypeslib.as_array(m.row_begin, shape=(self.n + 1,))
        self.col_sample, self.val_count = view(m.col_sample, nnz, np.uint32), view(m.val_count, nnz, np.uint32)

    def csr(self):
        return self.row_begin, self.col_sample, self.val_count

    def dense(self):
        """n x S uint32, 0 where a sample lacks the junction."""
        import numpy as np
        d = np.zeros((self.n, self.n_samples), np.uint32)
        rows = np.repeat(np.arange(self.n), np.diff(self.row_begin).astype(np.int64))
        d[rows, self.col_sample] = self.val_count
        return d

    def bed12(self):
        return _text(self._lib.rgx_cohort_format_bed12, self._h)

    def counts_tsv(self):
        return _text(self._lib.rgx_cohort_format_counts, self._h)


class CohortClusters(_Owned):
    """rgx_cohort_clusters: the intron clusters of a matrix (rows linked through a shared start or end) and, per cluster and sample, the reads on
    it.  The array attributes are numpy VIEWS of memory this object owns: copy what must outlive it."""

    _free = "rgx_cohort_clusters_free"

    def __init__(self, handle):
        import numpy as np
        _Owned.__init__(self, handle)
        c = handle.contents
        self.n_rows, self.n_clusters, self.n_components = int(c.n_rows), int(c.n_clusters), int(c.n_components)
        self.n_rounds, self.ms_cluster = int(c.n_rounds), c.ms_cluster
        self.n_ineligible, self.n_weak = int(c.n_ineligible), int(c.n_weak)          # (0, 0 unless the clusters are refined ones)
        view = self._view
        self.cluster = view(c.cluster, self.n_rows, np.uint32)
        self.cl_begin = np.ctypeslib.as_array(c.cl_begin, shape=(self.n_clusters + 1,))
        self.cs_begin = np.ctypeslib.as_array(c.cs_begin, shape=(self.n_clusters + 1,))
        self.cl_row, self.cl_total = view(c.cl_row, int(self.cl_begin[-1]), np.uint32), view(c.cl_total, self.n_clusters, np.uint64)
        self.cs_sample, self.cs_total = view(c.cs_sample, int(self.cs_begin[-1]), np.uint32), view(c.cs_total, int(self.cs_begin[-1]), np.uint64)

    def counts_text(self, matrix):
        """The cluster counts of `matrix` (the CohortMatrix these clusters were made from) in the layout of LeafCutter's perind.counts."""
        return _text(self._lib.rgx_cohort_format_cluster_counts, matrix._h, self._h)


def _cluster_params(min_rows, min_total):
    p = _ffi.ClusterParams()
    _ffi.lib().rgx_cluster_params_default(C.byref(p))
    p.min_rows, p.min_total = min_rows, min_total
    return p


def cluster_host(matrix, min_rows=1, min_total=0):
    """rgx_cohort_cluster_host: the clusters of a CohortMatrix by the library's plain C++ twin, no device involved."""
    p = _cluster_params(min_rows, min_total)
    return _call(_ffi.lib().rgx_cohort_cluster_host, _ffi.CohortClusters, CohortClusters, matrix._h, C.byref(p))


def _refine_params(max_intron, min_reads, min_ratio, min_rows, min_total):
    p = _ffi.RefineParams()
    _ffi.lib().rgx_refine_params_default(C.byref(p))
    p.max_intron, p.min_reads, (p.ratio_num, p.ratio_den), p.min_rows, p.min_total = max_intron, min_reads, min_ratio, min_rows, min_total
    return p


def refine_host(matrix, max_intron=0, min_reads=0, min_ratio=(0, 1), min_rows=1, min_total=0):
    """rgx_cohort_refine_host: the refined clusters of a CohortMatrix by the library's plain C++ twin, no device involved.  min_ratio is an exact
    fraction (numerator, denominator)."""
    p = _refine_params(max_intron, min_reads, min_ratio, min_rows, min_total)
    return _call(_ffi.lib().rgx_cohort_refine_host, _ffi.CohortClusters, CohortClusters, matrix._h, C.byref(p))


class CohortPhenotypes(_Owned):
    """rgx_pheno_table: the splicing phenotype table of a clustered matrix -- the kept rows, their missing samples, mean and sd of the
    intron-excision ratio, and rank2 (K x S), twice the average rank of each standardised entry in its sample's column.  The array attributes
    are numpy VIEWS of memory this object owns: copy what must outlive it."""

    _free = "rgx_cohort_phenotypes_free"

    def __init__(self, handle):
        import numpy as np
        _Owned.__init__(self, handle)
        p = handle.contents
        self.n_rows, self.n_samples = int(p.n_rows), int(p.n_samples)
        self.n_clustered, self.n_drop_na, self.n_drop_sd, self.ms_pheno = int(p.n_clustered), int(p.n_drop_na), int(p.n_drop_sd), p.ms_pheno
        view = self._view
        K = self.n_rows
        self.row, self.n_na = view(p.row, K, np.uint32), view(p.n_na, K, np.uint32)
        self.mean, self.sd = view(p.mean, K, np.float64), view(p.sd, K, np.float64)
        self.rank2 = view(p.rank2, K * self.n_samples, np.uint32).reshape(K, self.n_samples)

    def quantiles(self):
        """K x S float64: rgx_pheno_quantile of every entry (the numbers the text prints)."""
        import numpy as np
        q = self._lib.rgx_pheno_quantile
        table = np.array([q(r, self.n_rows) for r in range(2 * self.n_rows + 1)], np.float64) if self.n_rows else np.zeros(1)
        return table[self.rank2]

    def text(self, matrix, clusters):
        """The table as text: "#Chr start end ID" and the samples, one line per kept row.  matrix and clusters are what this came from."""
        return _text(self._lib.rgx_cohort_format_phenotypes, matrix._h, clusters._h, self._h)


def quantile(rank2, n_rows):
    """rgx_pheno_quantile: the standard normal quantile of rank2 / (2 (n_rows + 1)), on the host."""
    return _ffi.lib().rgx_pheno_quantile(rank2, n_rows)


def _pheno_params(max_missing, min_sd):
    p = _ffi.PhenoParams()
    _ffi.lib().rgx_pheno_params_default(C.byref(p))
    (p.na_num, p.na_den), p.min_sd = max_missing, min_sd
    return p


def phenotypes_host(matrix, clusters, max_missing=(4, 10), min_sd=0.005):
    """rgx_cohort_phenotypes_host: the phenotype table of a CohortMatrix and its CohortClusters by the library's plain C++ twin, no device
    involved.  max_missing is an exact fraction (numerator, denominator)."""
    p = _pheno_params(max_missing, min_sd)
    return _call(_ffi.lib().rgx_cohort_phenotypes_host, _ffi.PhenoTable, CohortPhenotypes, matrix._h, clusters._h, C.byref(p))


class CohortPCs(_Owned):
    """rgx_pheno_pcs: the principal components of a phenotype table -- col_sum (S) and gram (S x S) of its quantiles, variance (all S eigenvalues
    of their covariance, descending) and component (n_pcs x S, unit length, the largest entry positive).  The array attributes are numpy VIEWS of
    memory this object owns: copy what must outlive it."""

    _free = "rgx_cohort_pheno_pcs_free"

    def __init__(self, handle):
        import numpy as np
        _Owned.__init__(self, handle)
        p = handle.contents
        self.n_rows, self.n_samples, self.n_pcs = int(p.n_rows), int(p.n_samples), int(p.n_pcs)
        self.ms_pcs, self.ms_gram, self.ms_eigen = p.ms_pcs, p.ms_gram, p.ms_eigen
        S = self.n_samples
        self.col_sum = np.ctypeslib.as_array(p.col_sum, shape=(S,))
        self.gram = np.ctypeslib.as_array(p.gram, shape=(S, S))
        self.variance = np.ctypeslib.as_array(p.variance, shape=(S,))
        self.component = np.ctypeslib.as_array(p.component, shape=(self.n_pcs, S))

    def text(self, matrix):
        """The components as text, LeafCutter's .PCs layout: "id" and the samples of `matrix`, one line per component."""
        return _text(self._lib.rgx_cohort_format_pheno_pcs, matrix._h, self._h)


class CohortQTL(_Owned):
    """rgx_qtl_result: the nominal cis-sQTL scan of a phenotype table -- per variant its verdict (0 usable, 1 constant, 2 explained by the
    covariates) and gg, per row yy, the pairs as a CSR (pair_begin, pair_variant) with r and slope, and per row its best pair (NO_PAIR: none).
    The array attributes are numpy VIEWS of memory this object owns: copy what must outlive it."""
    NO_PAIR = 0xffffffff
    _free = "rgx_cohort_qtl_free"

    def __init__(self, handle):
        import numpy as np
        _Owned.__init__(self, handle)
        p = handle.contents
        self.n_rows, self.n_samples, self.n_variants = int(p.n_rows), int(p.n_samples), int(p.n_variants)
        self.n_cov, self.dof, self.n_pairs = int(p.n_cov), int(p.dof), int(p.n_pairs)
        self.n_constant, self.n_explained, self.n_flat_rows = int(p.n_constant), int(p.n_explained), int(p.n_flat_rows)
        self.n_tiles = int(p.n_tiles)
        self.ms_qtl, self.ms_residual, self.ms_pairs = p.ms_qtl, p.ms_residual, p.ms_pairs
        view = self._view
        K, V, n = self.n_rows, self.n_variants, self.n_pairs
        self.variant_verdict = view(p.variant_verdict, V, np.uint8)
        self.yy, self.gg = view(p.yy, K, np.float64), view(p.gg, V, np.float64)
        self.pair_begin, self.pair_variant = view(p.pair_begin, K + 1, np.uint32), view(p.pair_variant, n, np.uint32)
        self.r, self.slope, self.best = view(p.r, n, np.float64), view(p.slope, n, np.float64), view(p.best, K, np.uint32)

    def text(self, matrix, clusters, ph, var_pos, variant_ids):
        """The pairs as text: phenotype_id, variant_id, distance, r, slope, slope_se, tstat, pval_nominal, is_best; one line per pair.  matrix,
        clusters and ph are what the scan came from; var_pos and variant_ids (str or bytes) are per input variant."""
        return _qtl_text(self._lib.rgx_cohort_format_qtl, self, matrix, clusters, ph, var_pos, variant_ids)


class Genotypes(object):
    """rgx_genotypes: the dosages of a matrix's samples from a VCF or BCF -- tid, pos (V), dosage (V x S int8), ids (V, bytes), sorted by (tid, pos),
    and the counts of the records left out.  Copies: nothing here refers to the library's memory."""

    def __init__(self, path, matrix):
        import numpy as np
        lib = _ffi.lib()
        out = C.POINTER(_ffi.Genotypes)()
        err = C.create_string_buffer(1024)
        rc = lib.rgx_genotypes_load(os.fsencode(path), matrix._h, C.byref(out), err, len(err))
        if rc != 0:
            raise RegtoolsError(rc, err.value.decode())
        g = out.contents
        V, S = int(g.n_variants), int(g.n_samples)
        self.n_variants, self.n_samples = V, S
        self.n_records, self.n_multiallelic, self.n_no_gt, self.n_unknown_contig = (int(g.n_records), int(g.n_multiallelic), int(g.n_no_gt),
                                                                                   int(g.n_unknown_contig))
        self.tid = np.ctypeslib.as_array(g.tid, shape=(V,)).copy() if V else np.zeros(0, np.uint32)
        self.pos = np.ctypeslib.as_array(g.pos, shape=(V,)).copy() if V else np.zeros(0, np.uint32)
        self.dosage = np.ctypeslib.as_array(g.dosage, shape=(V * S,)).copy().reshape(V, S) if V * S else np.zeros((V, S), np.int8)
        self.ids = [g.id[v] for v in range(V)]
        lib.rgx_genotypes_free(out)


def genotypes(path, matrix):
    """rgx_genotypes_load: the genotypes of `matrix`'s samples, matched by name, from the VCF or BCF at `path`."""
    return Genotypes(path, matrix)


def qtl_tstat(r, dof):
    """rgx_qtl_tstat: r * sqrt(dof / (1 - r * r)), an infinity of r's sign when 1 - r * r <= 0."""
    return _ffi.lib().rgx_qtl_tstat(r, dof)


def qtl_pvalue(t, dof):
    """rgx_qtl_pvalue: the two-sided p of Student's t with dof degrees of freedom, on the host."""
    return _ffi.lib().rgx_qtl_pvalue(t, dof)


def pheno_regions(matrix, ph):
    """rgx_cohort_pheno_regions: K x 3 uint32 (tid, start, end) of the matrix rows the phenotype table kept."""
    import numpy as np
    out = np.zeros((ph.n_rows, 3), np.uint32)
    err = C.create_string_buffer(512)
    rc = _ffi.lib().rgx_cohort_pheno_regions(matrix._h, ph._h, out.ctypes.data, err, len(err))
    if rc != 0:
        raise RegtoolsError(rc, err.value.decode())
    return out


def _qtl_call(fn, front, ph, regions, var_tid, var_pos, dosage, covariates, window):
    import numpy as np
    S = ph.n_samples
    reg = np.ascontiguousarray(regions, dtype=np.uint32).reshape(-1, 3)
    tid, pos = np.ascontiguousarray(var_tid, dtype=np.uint32), np.ascontiguousarray(var_pos, dtype=np.uint32)
    dos = np.ascontiguousarray(dosage, dtype=np.int8).reshape(-1, S) if S else np.zeros((0, 0), np.int8)
    cov = np.ascontiguousarray(covariates, dtype=np.float64).reshape(-1, S) if covariates is not None and len(covariates) else np.zeros((0, S))
    if len(reg) != ph.n_rows or len(pos) != len(tid) or len(dos) != len(tid):
        raise ValueError("one region per table row, one position and one row of dosages per variant")
    if not 0 <= int(window) <= 0xffffffff:
        raise ValueError("window must fit 32 bits")
    return _call(fn, _ffi.QtlResult, CohortQTL, *(front + (ph._h, reg.ctypes.data, len(tid), tid.ctypes.data, pos.ctypes.data, dos.ctypes.data, len(cov),
                                                          cov.ctypes.data, int(window))))


def qtl_nominal_host(ph, regions, var_tid, var_pos, dosage, covariates=None, window=100000):
    """rgx_cohort_qtl_nominal_host: the nominal cis-sQTL scan by the library's plain C++ twin, no device involved.  regions: K x 3 (tid, start,
    end); var_tid, var_pos: V, ascending; dosage: V x S int8 in {0, 1, 2, -1}; covariates: n_cov x S or None."""
    return _qtl_call(_ffi.lib().rgx_cohort_qtl_nominal_host, (), ph, regions, var_tid, var_pos, dosage, covariates, window)


class CohortQTLPerm(_Owned):
    """rgx_qtl_perm_result: the permutation pass of the cis-sQTL scan -- per variant its verdict and gg, per row yy, n_cis (its pairs), perm_r
    (K x (B + 1): the largest |r| over its cis variants under the identity and the B permutations), the best pair of the identity (best_variant, an
    input variant or NO_PAIR; best_r, best_slope), n_ge, p_perm, and the beta approximation (beta_shape1, beta_shape2, p_beta, beta_status: 0
    converged, 1 moment estimates, 2 no fit).  The array attributes are numpy VIEWS of memory this object owns: copy what must outlive it."""
    NO_PAIR = 0xffffffff
    _free = "rgx_cohort_qtl_perm_free"

    def __init__(self, handle):
        import numpy as np
        _Owned.__init__(self, handle)
        p = handle.contents
        self.n_rows, self.n_samples, self.n_variants = int(p.n_rows), int(p.n_samples), int(p.n_variants)
        self.n_cov, self.dof, self.n_perm, self.n_pairs = int(p.n_cov), int(p.dof), int(p.n_perm), int(p.n_pairs)
        self.n_constant, self.n_explained, self.n_flat_rows = int(p.n_constant), int(p.n_explained), int(p.n_flat_rows)
        self.n_tiles = int(p.n_tiles)
        self.ms_perm, self.ms_residual, self.ms_products, self.ms_beta = p.ms_perm, p.ms_residual, p.ms_products, p.ms_beta
        view = self._view
        K, V, B1 = self.n_rows, self.n_variants, self.n_perm + 1
        self.variant_verdict = view(p.variant_verdict, V, np.uint8)
        self.yy, self.gg = view(p.yy, K, np.float64), view(p.gg, V, np.float64)
        self.n_cis, self.perm_r = view(p.n_cis, K, np.uint32), view(p.perm_r, K * B1, np.float64).reshape(K, B1)
        self.best_variant, self.best_r, self.best_slope = (view(p.best_variant, K, np.uint32), view(p.best_r, K, np.float64),
                                                           view(p.best_slope, K, np.float64))
        self.n_ge, self.p_perm = view(p.n_ge, K, np.uint32), view(p.p_perm, K, np.float64)
        self.beta_shape1, self.beta_shape2 = view(p.beta_shape1, K, np.float64), view(p.beta_shape2, K, np.float64)
        self.p_beta, self.beta_status = view(p.p_beta, K, np.float64), view(p.beta_status, K, np.uint8)

    def text(self, matrix, clusters, ph, var_pos, variant_ids):
        """One line per row that has pairs: phenotype_id, num_var, beta_shape1, beta_shape2, dof, variant_id, distance, r, slope, slope_se, tstat,
        pval_nominal, pval_perm, pval_beta.  The arguments are CohortQTL.text's."""
        return _qtl_text(self._lib.rgx_cohort_format_qtl_perm, self, matrix, clusters, ph, var_pos, variant_ids)


def qtl_permutations(n_samples, n_perm, seed=0):
    """rgx_qtl_permutations: (n_perm + 1) x n_samples uint16, row 0 the identity, rows 1 .. n_perm Fisher-Yates shuffles from one splitmix64
    stream that starts at `seed`."""
    import numpy as np
    out = np.zeros((int(n_perm) + 1, int(n_samples)), np.uint16)
    err = C.create_string_buffer(512)
    rc = _ffi.lib().rgx_qtl_permutations(int(n_samples), int(n_perm), int(seed) & 0xffffffffffffffff, out.ctypes.data, err, len(err))
    if rc != 0:
        raise RegtoolsError(rc, err.value.decode())
    return out


def qtl_digamma(x):
    """rgx_qtl_digamma: psi(x) for x > 0, on the host in long double."""
    return _ffi.lib().rgx_qtl_digamma(x)


def qtl_trigamma(x):
    """rgx_qtl_trigamma: psi'(x) for x > 0, on the host in long double."""
    return _ffi.lib().rgx_qtl_trigamma(x)


def qtl_betainc(x, a, b):
    """rgx_qtl_betainc: the regularised incomplete beta function I_x(a, b), on the host in long double."""
    return _ffi.lib().rgx_qtl_betainc(x, a, b)


def qtl_beta_fit(p):
    """rgx_qtl_beta_fit: (status, shape1, shape2) of the beta distribution fitted to the values p, each inside (0, 1), by maximum likelihood."""
    import numpy as np
    a = np.ascontiguousarray(p, dtype=np.float64)
    s1, s2 = C.c_double(), C.c_double()
    status = _ffi.lib().rgx_qtl_beta_fit(a.ctypes.data, len(a), C.byref(s1), C.byref(s2))
    return status, s1.value, s2.value


def _qtl_perm_call(fn, front, ph, regions, var_tid, var_pos, dosage, covariates, window, n_perm, seed, perms, groups=None, n_groups=None,
                   series=None, indep=None):
    import numpy as np
    S = ph.n_samples
    reg = np.ascontiguousarray(regions, dtype=np.uint32).reshape(-1, 3)
    tid, pos = np.ascontiguousarray(var_tid, dtype=np.uint32), np.ascontiguousarray(var_pos, dtype=np.uint32)
    dos = np.ascontiguousarray(dosage, dtype=np.int8).reshape(-1, S) if S else np.zeros((0, 0), np.int8)
    cov = np.ascontiguousarray(covariates, dtype=np.float64).reshape(-1, S) if covariates is not None and len(covariates) else np.zeros((0, S))
    if len(reg) != ph.n_rows or len(pos) != len(tid) or len(dos) != len(tid):
        raise ValueError("one region per table row, one position and one row of dosages per variant")
    if not 0 <= int(window) <= 0xffffffff:
        raise ValueError("window must fit 32 bits")
    if perms is None:
        if not 0 <= int(n_perm) <= 0xffffffff:
            raise ValueError("n_perm must fit 32 bits")
        n_perm = int(n_perm)
        pm = qtl_permutations(S, n_perm, seed) if 1 <= n_perm <= 65535 else np.zeros((1, S), np.uint16)     # (the library refuses the count)
    else:
        pm = np.ascontiguousarray(perms, dtype=np.uint16).reshape(-1, S)
        n_perm = len(pm) - 1
        if n_perm < 0:
            raise ValueError("perms needs the identity as its row 0")
    shared = front + (ph._h, reg.ctypes.data, len(tid), tid.ctypes.data, pos.ctypes.data, dos.ctypes.data, len(cov), cov.ctypes.data, int(window),
                      n_perm, pm.ctypes.data)
    if indep is not None:
        return _call(fn, _ffi.QtlIndepResult, CohortQTLIndep, *(shared + (float(indep[0]), int(indep[1]))))
    if series is not None:
        rows, begin, var = (np.ascontiguousarray(x, dtype=np.uint32) for x in series)
        if rows.ndim != 1 or begin.shape != (len(rows) + 1,) or var.ndim != 1 or (len(begin) and len(var) < int(begin.max())):
            raise ValueError("series_row (N), cond_begin (N + 1) and the cond_variant it indexes")
        pad = var if len(var) else np.zeros(1, np.uint32)                # (an empty list still has an address)
        return _call(fn, _ffi.QtlCondResult, CohortQTLCond, *(shared + (len(rows), rows.ctypes.data, begin.ctypes.data, pad.ctypes.data)))
    if groups is not None:
        grp = np.ascontiguousarray(groups, dtype=np.uint32)
        if grp.shape != (ph.n_rows,):
            raise ValueError("one group per table row")
        if not 0 <= int(n_groups) <= 0xffffffff:
            raise ValueError("n_groups must fit 32 bits")
        return _call(fn, _ffi.QtlGroupResult, CohortQTLGroup, *(shared + (int(n_groups), grp.ctypes.data)))
    return _call(fn, _ffi.QtlPermResult, CohortQTLPerm, *shared)


def qtl_permute_host(ph, regions, var_tid, var_pos, dosage, covariates=None, window=100000, n_perm=1000, seed=0, perms=None):
    """rgx_cohort_qtl_permute_host: the permutation pass by the library's plain C++ twin, no device involved.  The arguments are
    qtl_nominal_host's; perms: (B + 1) x S uint16 with the identity as row 0, or None for qtl_permutations(S, n_perm, seed)."""
    return _qtl_perm_call(_ffi.lib().rgx_cohort_qtl_permute_host, (), ph, regions, var_tid, var_pos, dosage, covariates, window, n_perm, seed, perms)


class CohortQTLGroup(_Owned):
    """rgx_qtl_group_result: the grouped permutation pass of the cis-sQTL scan -- per variant its verdict and gg, per row yy and n_cis, the
    groups' member lists (grp_begin, grp_row), and per group group_n_cis, perm_r (G x (B + 1): the largest |r| over all members' cis variants
    under the identity and the B permutations), the best pair of the identity (best_row, a table row, and best_variant, an input variant, or
    NO_PAIR; best_r, best_slope), n_ge, p_perm, and the beta approximation (beta_shape1, beta_shape2, p_beta, beta_status).  The array attributes
    are numpy VIEWS of memory this object owns: copy what must outlive it."""
    NO_PAIR = 0xffffffff
    NO_GROUP = 0xffffffff
    _free = "rgx_cohort_qtl_group_free"

    def __init__(self, handle):
        import numpy as np
        _Owned.__init__(self, handle)
        p = handle.contents
        self.n_rows, self.n_samples, self.n_variants = int(p.n_rows), int(p.n_samples), int(p.n_variants)
        self.n_cov, self.dof, self.n_perm, self.n_groups, self.n_pairs = int(p.n_cov), int(p.dof), int(p.n_perm), int(p.n_groups), int(p.n_pairs)
        self.n_constant, self.n_explained, self.n_flat_rows = int(p.n_constant), int(p.n_explained), int(p.n_flat_rows)
        self.n_tiles = int(p.n_tiles)
        self.ms_perm, self.ms_residual, self.ms_products, self.ms_beta = p.ms_perm, p.ms_residual, p.ms_products, p.ms_beta
        view = self._view
        K, V, G, B1 = self.n_rows, self.n_variants, self.n_groups, self.n_perm + 1
        self.variant_verdict = view(p.variant_verdict, V, np.uint8)
        self.yy, self.gg, self.n_cis = view(p.yy, K, np.float64), view(p.gg, V, np.float64), view(p.n_cis, K, np.uint32)
        self.grp_begin = view(p.grp_begin, G + 1, np.uint32)
        self.grp_row = view(p.grp_row, int(self.grp_begin[G]), np.uint32)
        self.group_n_cis, self.perm_r = view(p.group_n_cis, G, np.uint64), view(p.perm_r, G * B1, np.float64).reshape(G, B1)
        self.best_row, self.best_variant = view(p.best_row, G, np.uint32), view(p.best_variant, G, np.uint32)
        self.best_r, self.best_slope = view(p.best_r, G, np.float64), view(p.best_slope, G, np.float64)
        self.n_ge, self.p_perm = view(p.n_ge, G, np.uint32), view(p.p_perm, G, np.float64)
        self.beta_shape1, self.beta_shape2 = view(p.beta_shape1, G, np.float64), view(p.beta_shape2, G, np.float64)
        self.p_beta, self.beta_status = view(p.p_beta, G, np.float64), view(p.beta_status, G, np.uint8)

    def text(self, matrix, clusters, ph, var_pos, variant_ids):
        """One line per group that has pairs: group_id, group_size, then CohortQTLPerm.text's columns for the group's best pair with num_var =
        group_n_cis.  The arguments are CohortQTL.text's."""
        return _qtl_text(self._lib.rgx_cohort_format_qtl_group, self, matrix, clusters, ph, var_pos, variant_ids)


def pheno_groups(clusters, ph):
    """rgx_cohort_pheno_groups: (groups, n_groups) -- per row of the phenotype table its cluster, renumbered 0 .. n_groups - 1 in ascending order
    of each cluster's first table row."""
    import numpy as np
    out = np.zeros(ph.n_rows, np.uint32)
    n = C.c_uint32(0)
    err = C.create_string_buffer(512)
    rc = _ffi.lib().rgx_cohort_pheno_groups(clusters._h, ph._h, out.ctypes.data, C.byref(n), err, len(err))
    if rc != 0:
        raise RegtoolsError(rc, err.value.decode())
    return out, int(n.value)


def qtl_permute_grouped_host(ph, regions, groups, n_groups, var_tid, var_pos, dosage, covariates=None, window=100000, n_perm=1000, seed=0,
                             perms=None):
    """rgx_cohort_qtl_permute_grouped_host: the grouped permutation pass by the library's plain C++ twin, no device involved.  groups: per table
    row its group in [0, n_groups) or CohortQTLGroup.NO_GROUP; the other arguments are qtl_permute_host's."""
    return _qtl_perm_call(_ffi.lib().rgx_cohort_qtl_permute_grouped_host, (), ph, regions, var_tid, var_pos, dosage, covariates, window, n_perm,
                          seed, perms, groups, n_groups)


class CohortQTLCond(_Owned):
    """rgx_qtl_cond_result: the conditional permutation pass -- per variant its verdict and gg, per row yy, the series' lists echoed (series_row,
    cond_begin from 0, cond_variant), and per series cond_status (0, 1 collinear, 2 flat), yy_cond, dof, n_window (the row's usable cis variants),
    n_cis (those that take part), perm_r (N x (B + 1)), the best pair of the identity (best_variant, an input variant or NO_PAIR; best_r,
    best_slope), n_ge, p_perm and the beta approximation.  The array attributes are numpy VIEWS of memory this object owns."""
    NO_PAIR = 0xffffffff
    MAX_COND = 8
    _free = "rgx_cohort_qtl_cond_free"

    def __init__(self, handle):
        import numpy as np
        _Owned.__init__(self, handle)
        p = handle.contents
        self.n_rows, self.n_samples, self.n_variants = int(p.n_rows), int(p.n_samples), int(p.n_variants)
        self.n_cov, self.n_perm, self.n_series, self.n_cond, self.n_pairs = int(p.n_cov), int(p.n_perm), int(p.n_series), int(p.n_cond), int(p.n_pairs)
        self.n_constant, self.n_explained, self.n_flat_rows = int(p.n_constant), int(p.n_explained), int(p.n_flat_rows)
        self.n_collinear, self.n_flat_series, self.n_tiles = int(p.n_collinear), int(p.n_flat_series), int(p.n_tiles)
        self.ms_cond, self.ms_residual, self.ms_prepare, self.ms_products, self.ms_beta = (p.ms_cond, p.ms_residual, p.ms_prepare, p.ms_products,
                                                                                            p.ms_beta)
        view = self._view
        K, V, N, B1 = self.n_rows, self.n_variants, self.n_series, self.n_perm + 1
        self.variant_verdict = view(p.variant_verdict, V, np.uint8)
        self.yy, self.gg = view(p.yy, K, np.float64), view(p.gg, V, np.float64)
        self.series_row, self.cond_begin = view(p.series_row, N, np.uint32), view(p.cond_begin, N + 1, np.uint32)
        self.cond_variant, self.cond_status = view(p.cond_variant, self.n_cond, np.uint32), view(p.cond_status, N, np.uint8)
        self.yy_cond, self.dof = view(p.yy_cond, N, np.float64), view(p.dof, N, np.uint32)
        self.n_window, self.n_cis = view(p.n_window, N, np.uint32), view(p.n_cis, N, np.uint32)
        self.perm_r = view(p.perm_r, N * B1, np.float64).reshape(N, B1)
        self.best_variant, self.best_r, self.best_slope = (view(p.best_variant, N, np.uint32), view(p.best_r, N, np.float64),
                                                           view(p.best_slope, N, np.float64))
        self.n_ge, self.p_perm = view(p.n_ge, N, np.uint32), view(p.p_perm, N, np.float64)
        self.beta_shape1, self.beta_shape2 = view(p.beta_shape1, N, np.float64), view(p.beta_shape2, N, np.float64)
        self.p_beta, self.beta_status = view(p.p_beta, N, np.float64), view(p.beta_status, N, np.uint8)


def qtl_series(sets):
    """(series_row, cond_begin, cond_variant) of a list of (row, [variants]) pairs, as the conditional pass takes them."""
    import numpy as np
    rows = np.array([k for k, _ in sets], np.uint32)
    begin = np.concatenate([[0], np.cumsum([len(v) for _, v in sets])]).astype(np.uint32)
    var = np.array([x for _, v in sets for x in v], np.uint32)
    return rows, begin, var


def qtl_permute_conditional_host(ph, regions, series_row, cond_begin, cond_variant, var_tid, var_pos, dosage, covariates=None, window=100000,
                                 n_perm=1000, seed=0, perms=None):
    """rgx_cohort_qtl_permute_conditional_host: the conditional permutation pass by the library's plain C++ twin, no device involved.  Series c
    is table row series_row[c] conditioned on cond_variant[cond_begin[c]:cond_begin[c + 1]] (qtl_series builds the three); the other arguments are
    qtl_permute_host's."""
    return _qtl_perm_call(_ffi.lib().rgx_cohort_qtl_permute_conditional_host, (), ph, regions, var_tid, var_pos, dosage, covariates, window, n_perm,
                          seed, perms, series=(series_row, cond_begin, cond_variant))


class CohortQTLIndep(_Owned):
    """rgx_qtl_indep_result: the conditionally independent signals of every table row, CSR by row (sig_begin, K + 1) in (row, rank) order -- per
    signal variant, rank (its place in the row's forward order), n_cond, dof, n_cis, r, slope, p_perm, beta_shape1, beta_shape2, p_beta,
    beta_status -- and per row capped.  The array attributes are numpy VIEWS of memory this object owns."""
    _free = "rgx_cohort_qtl_indep_free"

    def __init__(self, handle):
        import numpy as np
        _Owned.__init__(self, handle)
        p = handle.contents
        self.n_rows, self.n_samples, self.n_variants = int(p.n_rows), int(p.n_samples), int(p.n_variants)
        self.n_cov, self.n_perm, self.max_signals, self.p_threshold = int(p.n_cov), int(p.n_perm), int(p.max_signals), p.p_threshold
        self.n_signals, self.n_entered, self.n_forward_rounds = int(p.n_signals), int(p.n_entered), int(p.n_forward_rounds)
        self.n_series_total, self.n_capped = int(p.n_series_total), int(p.n_capped)
        self.ms_indep, self.ms_round0, self.ms_forward, self.ms_backward = p.ms_indep, p.ms_round0, p.ms_forward, p.ms_backward
        view = self._view
        K, n = self.n_rows, self.n_signals
        self.sig_begin, self.capped = view(p.sig_begin, K + 1, np.uint32), view(p.capped, K, np.uint8)
        self.variant, self.rank, self.n_cond = view(p.variant, n, np.uint32), view(p.rank, n, np.uint32), view(p.n_cond, n, np.uint32)
        self.dof, self.n_cis = view(p.dof, n, np.uint32), view(p.n_cis, n, np.uint32)
        self.r, self.slope, self.p_perm = view(p.r, n, np.float64), view(p.slope, n, np.float64), view(p.p_perm, n, np.float64)
        self.beta_shape1, self.beta_shape2 = view(p.beta_shape1, n, np.float64), view(p.beta_shape2, n, np.float64)
        self.p_beta, self.beta_status = view(p.p_beta, n, np.float64), view(p.beta_status, n, np.uint8)

    def text(self, matrix, clusters, ph, var_pos, variant_ids):
        """One line per kept signal in (row, rank) order: CohortQTLPerm.text's columns, then rank and n_cond."""
        return _qtl_text(self._lib.rgx_cohort_format_qtl_indep, self, matrix, clusters, ph, var_pos, variant_ids)


def qtl_independent_host(ph, regions, var_tid, var_pos, dosage, covariates=None, window=100000, n_perm=1000, seed=0, perms=None, p_threshold=0.05,
                         max_signals=8):
    """rgx_cohort_qtl_independent_host: the forward-backward search for conditionally independent signals by the library's host twins, no device
    involved.  The arguments are qtl_permute_host's, then the threshold of p_beta and the most signals a row takes (1 to 8)."""
    return _qtl_perm_call(_ffi.lib().rgx_cohort_qtl_independent_host, (), ph, regions, var_tid, var_pos, dosage, covariates, window, n_perm, seed,
                          perms, indep=(p_threshold, max_signals))


class CohortQTLTrans(_Owned):
    """rgx_qtl_trans_result: the trans-sQTL scan of a phenotype table -- per variant its verdict and gg, per row yy, and the hits (the pairs whose
    |r| reaches r_min) as a CSR by row (hit_begin, hit_variant: an index into the input variants) with r and slope, a row's hits in ascending
    variant order; n_tested is the number of pairs that met.  The array attributes are numpy VIEWS of memory this object owns."""
    _free = "rgx_cohort_qtl_trans_free"

    def __init__(self, handle):
        import numpy as np
        _Owned.__init__(self, handle)
        p = handle.contents
        self.n_rows, self.n_samples, self.n_variants = int(p.n_rows), int(p.n_samples), int(p.n_variants)
        self.n_cov, self.dof, self.n_tested, self.n_hits = int(p.n_cov), int(p.dof), int(p.n_tested), int(p.n_hits)
        self.n_constant, self.n_explained, self.n_flat_rows = int(p.n_constant), int(p.n_explained), int(p.n_flat_rows)
        self.n_tiles, self.n_hit_tiles = int(p.n_tiles), int(p.n_hit_tiles)
        self.ms_trans, self.ms_residual, self.ms_count, self.ms_emit = p.ms_trans, p.ms_residual, p.ms_count, p.ms_emit
        view = self._view
        K, V, n = self.n_rows, self.n_variants, self.n_hits
        self.variant_verdict = view(p.variant_verdict, V, np.uint8)
        self.yy, self.gg = view(p.yy, K, np.float64), view(p.gg, V, np.float64)
        self.hit_begin, self.hit_variant = view(p.hit_begin, K + 1, np.uint32), view(p.hit_variant, n, np.uint32)
        self.r, self.slope = view(p.r, n, np.float64), view(p.slope, n, np.float64)

    def text(self, matrix, clusters, ph, var_pos, variant_ids):
        """The hits as text: phenotype_id, variant_id, r, slope, slope_se, tstat, pval; one line per hit.  Arguments as CohortQTL.text."""
        return _qtl_text(self._lib.rgx_cohort_format_qtl_trans, self, matrix, clusters, ph, var_pos, variant_ids)


def qtl_r_threshold(pval, dof):
    """rgx_qtl_r_threshold: the smallest |r| whose two-sided p with dof degrees of freedom is at most pval, by bisection on the host."""
    return _ffi.lib().rgx_qtl_r_threshold(pval, dof)


def _qtl_trans_call(fn, front, ph, regions, var_tid, var_pos, dosage, covariates, r_min, pval, exclude_window, max_hits):
    import numpy as np
    S = ph.n_samples
    reg = np.ascontiguousarray(regions, dtype=np.uint32).reshape(-1, 3)
    tid, pos = np.ascontiguousarray(var_tid, dtype=np.uint32), np.ascontiguousarray(var_pos, dtype=np.uint32)
    dos = np.ascontiguousarray(dosage, dtype=np.int8).reshape(-1, S) if S else np.zeros((0, 0), np.int8)
    cov = np.ascontiguousarray(covariates, dtype=np.float64).reshape(-1, S) if covariates is not None and len(covariates) else np.zeros((0, S))
    if len(reg) != ph.n_rows or len(pos) != len(tid) or len(dos) != len(tid):
        raise ValueError("one region per table row, one position and one row of dosages per variant")
    if exclude_window is not None and not 0 <= int(exclude_window) <= 0xffffffff:
        raise ValueError("exclude_window must fit 32 bits")
    if not 0 <= int(max_hits) < 1 << 64:
        raise ValueError("max_hits must fit 64 bits")
    if r_min is None:
        r_min = qtl_r_threshold(pval, max(S - len(cov) - 2, 0)) if S >= len(cov) + 3 else 0.0      # (too few samples: the call says so)
    return _call(fn, _ffi.QtlTransResult, CohortQTLTrans, *(front + (ph._h, reg.ctypes.data, len(tid), tid.ctypes.data, pos.ctypes.data,
                 dos.ctypes.data, len(cov), cov.ctypes.data, float(r_min), 0 if exclude_window is None else 1,
                 0 if exclude_window is None else int(exclude_window), int(max_hits))))


def qtl_trans_host(ph, regions, var_tid, var_pos, dosage, covariates=None, r_min=None, pval=1e-5, exclude_window=5000000, max_hits=0):
    """rgx_cohort_qtl_trans_host: the trans-sQTL scan by the library's plain C++ twin, no device involved.  The inputs are qtl_nominal_host's
    without the window; r_min: the smallest |r| kept, None for qtl_r_threshold(pval, dof); exclude_window: pairs within it of the row's intron are
    left out, None keeps them; max_hits: refuse more hits than this, 0 for the result's own limit."""
    return _qtl_trans_call(_ffi.lib().rgx_cohort_qtl_trans_host, (), ph, regions, var_tid, var_pos, dosage, covariates, r_min, pval,
                           exclude_window, max_hits)


class PlantedPhenotypes(object):
    """A K x S uint32 array as the rgx_pheno_table the principal component calls read (n_rows, n_samples and rank2 alone are set).  The memory is
    the array's own (a C-contiguous copy when it is not one already), kept alive by this object."""

    def __init__(self, rank2):
        import numpy as np
        a = np.ascontiguousarray(rank2, dtype=np.uint32)
        if a.ndim != 2:
            raise ValueError("rank2 must be a K x S array")
        self.rank2 = a
        self.n_rows, self.n_samples = int(a.shape[0]), int(a.shape[1])
        self._table = _ffi.PhenoTable()
        self._table.n_rows, self._table.n_samples = self.n_rows, self.n_samples
        self._table.rank2 = a.ctypes.data_as(C.POINTER(C.c_uint32))
        self._h = C.pointer(self._table)


def pheno_table_from_rank2(rank2):
    """Wraps a K x S array of rank2 values as a table for Cohort.pheno_pcs and pheno_pcs_host."""
    return PlantedPhenotypes(rank2)


def pheno_pcs_host(ph, n_pcs):
    """rgx_cohort_pheno_pcs_host: the first n_pcs principal components of a phenotype table by the library's plain C++ twin, no device involved."""
    return _call(_ffi.lib().rgx_cohort_pheno_pcs_host, _ffi.PhenoPCs, CohortPCs, ph._h, n_pcs)


def merge_host(extractors, names, only_anchored=True, min_samples=1, min_total=1):
    """rgx_cohort_merge_host over the tables the extractors hold (each with its own min_anchor_length_): no device involved."""
    lib = _ffi.lib()
    n = len(extractors)
    tabs = (C.POINTER(_ffi.JunctionTable) * max(n, 1))(*[je.table for je in extractors])
    anchors = (C.c_uint32 * max(n, 1))(*[je.min_anchor_length_ & 0xffffffff for je in extractors])
    nm = (C.c_char_p * max(n, 1))(*[s.encode() for s in names])
    p = _params(only_anchored, min_samples, min_total)
    return _call(lib.rgx_cohort_merge_host, _ffi.CohortMatrix, CohortMatrix, tabs, anchors, nm, n, C.byref(p))


def _index_bytes(path):
    """hts_idx_load's order (hts.c:2031-2042): <fn>.csi, <stem>.csi, <fn>.bai, <stem>.bai."""
    stem = os.path.splitext(path)[0]
    for cand in (path + ".csi", stem + ".csi", path + ".bai", stem + ".bai"):
        if os.path.exists(cand):
            with open(cand, "rb") as f:
                return f.read()
    raise RegtoolsError(2, "Unable to open BAM/SAM index. Make sure alignments are indexed\n\n")


class Cohort(object):
    """rgx_cohort: samples are numbered in the order they are added."""

    def __init__(self, ctx=None, device=0, only_anchored=True, min_samples=1, min_total=1):
        self._lib = _ffi.lib()
        self._ctx = ctx if ctx is not None else Context(device)
        self._device = device
        self._h = C.c_void_p()
        self.add_paths = []                      # per add: 1 = device to device, 0 = uploaded (rgx_cohort_add_path)
        self.cluster_paths = []                  # per cluster: 1 = the matrix was still in HBM, 0 = uploaded (rgx_cohort_cluster_path)
        p = _params(only_anchored, min_samples, min_total)
        err = C.create_string_buffer(512)
        rc = self._lib.rgx_cohort_create(self._ctx._h, C.byref(p), C.byref(self._h), err, len(err))
        if rc != 0:
            raise RegtoolsError(rc, err.value.decode())

    def add(self, je, name):
        """je: a JunctionsExtractor that holds a table.  Its context goes along, so a table that is still that context's last one (a
        Pipeline.wait result before the file `depth` tickets later is submitted; a sequential extraction) never leaves HBM."""
        idx = C.c_uint32()
        err = C.create_string_buffer(512)
        src = je._ctx._h if je._ctx is not None else None
        rc = self._lib.rgx_cohort_add(self._h, src, je.table, je.min_anchor_length_ & 0xffffffff, name.encode(), C.byref(idx), err, len(err))
        if rc != 0:
            raise RegtoolsError(rc, err.value.decode())
        self.add_paths.append(self._lib.rgx_cohort_add_path(self._h))
        return idx.value

    def finish(self):
        return _call(self._lib.rgx_cohort_finish, _ffi.CohortMatrix, CohortMatrix, self._h)

    def cluster(self, matrix, min_rows=1, min_total=0):
        """The intron clusters of `matrix` (any CohortMatrix) on this cohort's device.  The matrix of the most recent finish is read where it lies
        in HBM; any other one is uploaded."""
        p = _cluster_params(min_rows, min_total)
        cl = _call(self._lib.rgx_cohort_cluster, _ffi.CohortClusters, CohortClusters, self._h, matrix._h, C.byref(p))
        self.cluster_paths.append(self._lib.rgx_cohort_cluster_path(self._h))
        return cl

    def refine(self, matrix, max_intron=0, min_reads=0, min_ratio=(0, 1), min_rows=1, min_total=0):
        """The refined clusters of `matrix` on this cohort's device (rgx_cohort_refine): introns longer than max_intron take no part, junctions
        with fewer than min_reads reads or less than min_ratio = (numerator, denominator) of their cluster's reads are removed, and the rest is
        clustered again.  The matrix is found as in cluster()."""
        p = _refine_params(max_intron, min_reads, min_ratio, min_rows, min_total)
        cl = _call(self._lib.rgx_cohort_refine, _ffi.CohortClusters, CohortClusters, self._h, matrix._h, C.byref(p))
        self.cluster_paths.append(self._lib.rgx_cohort_cluster_path(self._h))
        return cl

    def phenotypes(self, matrix, clusters, max_missing=(4, 10), min_sd=0.005):
        """The splicing phenotype table of `matrix` and its `clusters` on this cohort's device (rgx_cohort_phenotypes): intron-excision ratios,
        rows dropped when more than max_missing = (numerator, denominator) of the samples have no reads on the cluster or when their sd is
        below min_sd, each row standardised, each sample's column ranked.  The matrix is found as in cluster()."""
        p = _pheno_params(max_missing, min_sd)
        ph = _call(self._lib.rgx_cohort_phenotypes, _ffi.PhenoTable, CohortPhenotypes, self._h, matrix._h, clusters._h, C.byref(p))
        self.cluster_paths.append(self._lib.rgx_cohort_cluster_path(self._h))
        return ph

    def pheno_pcs(self, ph, n_pcs):
        """The first n_pcs principal components of the phenotype table `ph` on this cohort's device (rgx_cohort_pheno_pcs): the Gram matrix of
        its quantiles in HBM, the eigen-decomposition of their covariance on the host."""
        return _call(self._lib.rgx_cohort_pheno_pcs, _ffi.PhenoPCs, CohortPCs, self._h, ph._h, n_pcs)

    def qtl_nominal(self, ph, regions, var_tid, var_pos, dosage, covariates=None, window=100000):
        """The nominal cis-sQTL scan of the phenotype table `ph` on this cohort's device (rgx_cohort_qtl_nominal): residuals of rows and variants
        against intercept + covariates, then r and slope of every (row, variant within `window` of its intron) pair.  Arguments as
        qtl_nominal_host."""
        return _qtl_call(self._lib.rgx_cohort_qtl_nominal, (self._h,), ph, regions, var_tid, var_pos, dosage, covariates, window)

    def qtl_permute(self, ph, regions, var_tid, var_pos, dosage, covariates=None, window=100000, n_perm=1000, seed=0, perms=None):
        """The permutation pass of the cis-sQTL scan on this cohort's device (rgx_cohort_qtl_permute): per row the largest |r| over its cis variants
        under the identity and n_perm permutations of the samples, the empirical p and its beta approximation.  Returns a CohortQTLPerm; the
        arguments are qtl_permute_host's."""
        return _qtl_perm_call(self._lib.rgx_cohort_qtl_permute, (self._h,), ph, regions, var_tid, var_pos, dosage, covariates, window, n_perm,
                              seed, perms)

    def qtl_permute_grouped(self, ph, regions, groups, n_groups, var_tid, var_pos, dosage, covariates=None, window=100000, n_perm=1000, seed=0,
                            perms=None):
        """The grouped permutation pass on this cohort's device (rgx_cohort_qtl_permute_grouped): per group of rows -- per intron cluster with
        pheno_groups -- the largest |r| over all its members' cis variants under the identity and n_perm permutations, the best (row, variant)
        of the identity, and on the host the empirical p and its beta approximation.  The arguments are qtl_permute_grouped_host's."""
        return _qtl_perm_call(self._lib.rgx_cohort_qtl_permute_grouped, (self._h,), ph, regions, var_tid, var_pos, dosage, covariates, window,
                              n_perm, seed, perms, groups, n_groups)

    def qtl_permute_conditional(self, ph, regions, series_row, cond_begin, cond_variant, var_tid, var_pos, dosage, covariates=None, window=100000,
                                n_perm=1000, seed=0, perms=None):
        """The conditional permutation pass on this cohort's device (rgx_cohort_qtl_permute_conditional): the permutation pass of table row
        series_row[c] with the variants cond_variant[cond_begin[c]:cond_begin[c + 1]] in the model, per series.  Returns a CohortQTLCond; the
        arguments are qtl_permute_conditional_host's."""
        return _qtl_perm_call(self._lib.rgx_cohort_qtl_permute_conditional, (self._h,), ph, regions, var_tid, var_pos, dosage, covariates, window,
                              n_perm, seed, perms, series=(series_row, cond_begin, cond_variant))

    def qtl_independent(self, ph, regions, var_tid, var_pos, dosage, covariates=None, window=100000, n_perm=1000, seed=0, perms=None,
                        p_threshold=0.05, max_signals=8):
        """The conditionally independent signals of every row on this cohort's device (rgx_cohort_qtl_independent): round 0 is the permutation
        pass, every further round one conditional pass behind the same preparation.  Returns a CohortQTLIndep; the arguments are
        qtl_independent_host's."""
        return _qtl_perm_call(self._lib.rgx_cohort_qtl_independent, (self._h,), ph, regions, var_tid, var_pos, dosage, covariates, window, n_perm,
                              seed, perms, indep=(p_threshold, max_signals))

    def qtl_trans(self, ph, regions, var_tid, var_pos, dosage, covariates=None, r_min=None, pval=1e-5, exclude_window=5000000, max_hits=0):
        """The trans-sQTL scan on this cohort's device (rgx_cohort_qtl_trans): every row against every usable variant, only the pairs whose |r|
        reaches r_min kept.  Returns a CohortQTLTrans; the arguments are qtl_trans_host's."""
        return _qtl_trans_call(self._lib.rgx_cohort_qtl_trans, (self._h,), ph, regions, var_tid, var_pos, dosage, covariates, r_min, pval,
                               exclude_window, max_hits)

    def run(self, files, depth=2, **extract_kw):
        """Extracts `files` through a Pipeline of `depth` and adds each.  An item is a path, or (path, name), or (path, name, kw) with that file's own
        JunctionsExtractor arguments over extract_kw; the default name is the base name without ".bam".  File k is added BEFORE file k + depth is
        submitted: that submit is what overwrites file k's rows in HBM.  When a file fails, the files in front of it are still added (the cohort
        stays usable), the ones behind it that were in flight are dropped, and the file's error is raised."""
        items = []
        for it in files:
            it = (it,) if isinstance(it, str) else tuple(it)
            path = it[0]
            base = os.path.basename(path)
            name = it[1] if len(it) > 1 and it[1] else (base[:-4] if base.endswith(".bam") else base)
            kw = dict(extract_kw)
            if len(it) > 2:
                kw.update(it[2])
            items.append((path, name, kw))
        pl = Pipeline(self._device, depth)
        flight = {}                              # file index -> (ticket, PinnedBuffer, index bytes): this run's own references, until wait returns

        def submit(k):
            path, _, kw = items[k]
            try:
                with open(path, "rb") as f:
                    data = f.read()
            except OSError:
                raise RegtoolsError(1, "[E::hts_open_format] fail to open file '%s'\nUnable to open BAM/SAM file.\n\n" % path)
            bai = _index_bytes(path)
            buf = PinnedBuffer(data)
            flight[k] = (pl.submit(bai_bytes=bai, host_ptr=buf.ptr, host_len=buf.size, bam=path, **kw), buf, bai)

        def wait(k, add):
            ticket, buf, _ = flight[k]
            try:
                je = pl.wait(ticket)
            finally:
                del flight[k]
                buf.close()
            if add:
                self.add(je, items[k][1])

        try:
            failed, error = None, None
            nxt = 0
            try:
                while nxt < min(depth, len(items)):
                    submit(nxt)
                    nxt += 1
            except RegtoolsError as e:
                failed, error = nxt, e
            k = 0
            while k < len(items) and (failed is None or k < failed):
                try:
                    wait(k, True)
                except RegtoolsError as e:
                    failed, error = k, e
                    break
                k += 1
                if failed is None and nxt < len(items):
                    try:
                        submit(nxt)
                        nxt += 1
                    except RegtoolsError as e:
                        failed, error = nxt, e
            for j in sorted(flight):             # behind a failed file: run to their end (their buffers were promised), results dropped
                try:
                    wait(j, False)
                except RegtoolsError:
                    pass
            if error is not None:
                raise error
        finally:
            pl.close()
        return self

    def close(self):
        if self._h:
            self._lib.rgx_cohort_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
