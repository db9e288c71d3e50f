"""The principal components of a phenotype table restated for the tests (contract: include/regtools_amd.h): the Gram matrix and the column sums in
the contract's summation order with exact fused multiply-adds, the covariance formula as written there, and two independent references for the
eigen-decomposition -- numpy.linalg.eigh of that covariance and sklearn's PCA (svd_solver="full", what LeafCutter calls) of the quantiles."""
from fractions import Fraction

import numpy as np

EPS = np.finfo(np.float64).eps

# The tolerance constant C.  The tests' bounds have the form C * S * eps * lambda_1 (eigenvalues, residuals) and C * S * eps * lambda_1 / gap_i
# (components).  C was measured between two references, neither of them the code under test: numpy.linalg.eigh of the covariance (the contract's
# formula over numpy's own Gram matrix q.T @ q) against sklearn's PCA(svd_solver="full") of the same quantiles, over the seven shapes of
# tests/pca_cases.py.  The largest ratio of their difference to S * eps * lambda_1 (eigenvalues) or to S * eps * lambda_1 / gap_i (compared
# components) was 1.525, in the eigenvalues of (65537, 3) with ties; the largest among the components alone 0.888, at the same shape.  C is four
# times the larger, the project's usual margin for another machine's libm.
C_MEASURED, C_TOL = 1.525, 4 * 1.525


def quantile_table(K, quantile):
    """T[r] = quantile(r, K) for r = 2 .. 2 K (NaN in front)."""
    T = np.full(2 * K + 1, np.nan)
    for r in range(2, 2 * K + 1):
        T[r] = quantile(r, K)
    return T


def quantiles(rank2, quantile):
    """q = T[rank2], K x S float64."""
    return quantile_table(rank2.shape[0], quantile)[rank2]


def chunks(K):
    """The contract's chunks of the rows: [(begin, end)]."""
    n = min(64, -(-K // 1024))
    L = -(-K // n)
    return [(j * L, min(K, (j + 1) * L)) for j in range(n)]


def fma(a, b, c):
    """a * b + c rounded once (Python 3.10 has no math.fma)."""
    return float(Fraction(a) * Fraction(b) + Fraction(c))


def gram_exact(q):
    """(gram, col_sum) of q (K x S) in the contract's order: per chunk and s <= t a chain of exact FMAs in ascending k from +0.0, the chunks added
    in order from +0.0 by rounded adds; col_sum likewise with plain adds."""
    K, S = q.shape
    gram, col = np.zeros((S, S)), np.zeros(S)
    for b, e in chunks(K):
        for s in range(S):
            acc = 0.0
            for k in range(b, e):
                acc = acc + float(q[k, s])
            col[s] = col[s] + acc
            for t in range(s, S):
                acc = 0.0
                for k in range(b, e):
                    acc = fma(float(q[k, s]), float(q[k, t]), acc)
                gram[s, t] = gram[s, t] + acc
                gram[t, s] = gram[s, t]
    return gram, col


def covariance(gram, col_sum, K):
    """cov[s][t] = (gram[s][t] - col_sum[s] * col_sum[t] / K) / (K - 1) for s <= t, mirrored; every operation rounded on its own."""
    S = len(col_sum)
    cov = np.zeros((S, S))
    for s in range(S):
        for t in range(s, S):
            cov[s, t] = cov[t, s] = (float(gram[s, t]) - float(col_sum[s]) * float(col_sum[t]) / float(K)) / float(K - 1)
    return cov


def flip(components):
    """Each row signed so that its entry of largest absolute value (the first on ties) is positive."""
    out = np.array(components, dtype=np.float64)
    for v in out:
        if v[np.argmax(np.abs(v))] < 0:
            v *= -1
    return out


def eigh(cov):
    """(eigenvalues descending, unit eigenvectors as rows, signed) by numpy.linalg.eigh."""
    w, v = np.linalg.eigh(cov)
    return w[::-1].copy(), flip(v.T[::-1])


def sklearn_pca(q):
    """(explained_variance_, components_) of sklearn's PCA(svd_solver="full") of q, K x S: rows are observations, samples are features."""
    from sklearn.decomposition import PCA
    p = PCA(svd_solver="full").fit(q)
    return p.explained_variance_.copy(), p.components_.copy()


def neighbour_gaps(ev):
    """gap_i = the distance from eigenvalue i to the nearer of its neighbours."""
    ev = np.asarray(ev)
    d = np.abs(np.diff(ev))
    return np.minimum(np.concatenate(([np.inf], d)), np.concatenate((d, [np.inf])))


def aligned(v, ref):
    """v or -v, whichever points along ref."""
    return v if np.dot(v, ref) >= 0 else -v


def text(sample_names, component):
    """The .PCs text: "id" and the sample names, one line per component with its 1-based number and %.17g entries."""
    lines = ["\t".join(["id"] + list(sample_names))]
    for i, v in enumerate(component):
        lines.append("\t".join([str(i + 1)] + ["%.17g" % x for x in v]))
    return ("\n".join(lines) + "\n").encode()


# ---- checks the host and the device tests share ----------------------------------------------------------------------------------------------
def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def same_bits(a, b):
    assert a.shape == b.shape and (_bits(a) == _bits(b)).all()


def same_pcs(a, b):
    """Two results of the library, every array as bit patterns."""
    assert (a.n_rows, a.n_samples, a.n_pcs) == (b.n_rows, b.n_samples, b.n_pcs)
    for name in ("col_sum", "gram", "variance", "component"):
        same_bits(getattr(a, name), getattr(b, name))


def check_structure(p):
    """gram symmetric, the components orthonormal to 64 eps, the sign rule, the eigenvalues descending."""
    same_bits(p.gram, p.gram.T.copy())
    assert np.abs(p.component @ p.component.T - np.eye(p.n_pcs)).max() <= 64 * EPS
    for v in p.component:
        assert v[np.argmax(np.abs(v))] > 0
    assert (np.diff(p.variance) <= 0).all()


def check_residual(p, bound):
    """|cov v - lambda v| <= bound for every component, whatever the gaps."""
    cov = covariance(p.gram, p.col_sum, p.n_rows)
    for i, v in enumerate(p.component):
        r = np.abs(cov @ v - p.variance[i] * v).max()
        assert r <= bound, (i, r, bound)
