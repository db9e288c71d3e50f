"""The contract of rgx_cohort_qtl_permute_grouped (include/regtools_amd.h) restated in scalar Python, for the grouped permutation pass tests
(tests/test_cohort_qtl_group_host.py, tests/test_gpu_cohort_qtl_group.py).  Steps (1)-(6) are tests/qtl_ref.py's and every permuted chain is
tests/qtl_perm_ref.py's, with its exact rational fma.
  restate()       a group's series = the largest bit pattern over its members' series, in Python integers; the best pair of the identity by the
                  tie rule (largest bits, then the lowest table row, then the earliest variant); n_ge
  max_identity()  what every grouped result owes the ungrouped result of the same input
  same_group_result()   two library results, every array
  text()          the Python writer of rgx_cohort_format_qtl_group
"""
import math
import struct

import numpy as np

import qtl_perm_ref as pref
import qtl_ref as ref

NO_PAIR = ref.NO_PAIR
NO_GROUP = 0xffffffff


def members_of(groups, G):
    """Per group its rows, ascending."""
    out = [[] for _ in range(G)]
    for k, g in enumerate(int(x) for x in groups):
        if g != NO_GROUP:
            out[g].append(k)
    return out


def as_double(b):
    return struct.unpack("<d", struct.pack("<Q", b))[0]


class Restated(object):
    pass


def restate(rows, groups, G):
    """rows: qtl_perm_ref.restate() of the same case and permutations, every (k, b).  The grouped contract on top of it."""
    K, B1 = rows.perm_r.shape
    mem = members_of(groups, G)
    o = Restated()
    o.rows = rows
    o.grp_begin = np.cumsum([0] + [len(m) for m in mem]).astype(np.uint32)
    o.grp_row = np.array([k for m in mem for k in m], np.uint32)
    o.group_n_cis = np.array([sum(int(rows.n_cis[k]) for k in m) for m in mem], np.uint64)
    o.n_pairs = int(o.group_n_cis.sum())
    o.perm_r = np.zeros((G, B1))
    o.best_row, o.best_variant = np.full(G, NO_PAIR, np.uint32), np.full(G, NO_PAIR, np.uint32)
    o.best_r, o.best_slope, o.n_ge = np.zeros(G), np.zeros(G), np.zeros(G, np.uint32)
    for g, m in enumerate(mem):
        with_pairs = [k for k in m if rows.n_cis[k]]
        for b in range(B1):
            o.perm_r[g, b] = as_double(max([pref.bits(rows.perm_r[k, b]) for k in with_pairs] or [0]))
        if with_pairs:
            top = max(pref.bits(rows.perm_r[k, 0]) for k in with_pairs)
            k = min(k for k in with_pairs if pref.bits(rows.perm_r[k, 0]) == top)      # (the row's own best is its earliest variant on ties)
            o.best_row[g], o.best_variant[g], o.best_r[g], o.best_slope[g] = k, rows.best_variant[k], rows.best_r[k], rows.best_slope[k]
        o.n_ge[g] = sum(1 for b in range(1, B1) if pref.bits(o.perm_r[g, b]) >= pref.bits(o.perm_r[g, 0]))
    return o


def restate_sampled(c, quantile, perms, groups, G, only, verdict):
    """perm_r[g][b] for the (g, b) of `only`, for tables too large to restate whole: {(g, b): the double}."""
    mem = members_of(groups, G)
    rows = pref.restate(c, quantile, perms, only=set((k, b) for g, b in only for k in mem[g]), verdict=verdict)
    return dict(((g, b), as_double(max([pref.bits(rows.perm_r[k, b]) for k in mem[g] if rows.n_cis[k]] or [0]))) for g, b in only), rows


def max_identity(q, ung, groups, G):
    """bits(perm_r[g][b]) == the largest of the members' bits(ungrouped perm_r[k][b]); hence n_ge[g] >= the ungrouped n_ge of best_row[g];
    group_n_cis sums n_cis.  q: a grouped result, ung: the ungrouped result of the same input (library or restatement)."""
    mem = members_of(groups, G)
    gb, ub = np.ascontiguousarray(q.perm_r).view(np.uint64), np.ascontiguousarray(ung.perm_r).view(np.uint64)
    assert np.array_equal(q.n_cis, ung.n_cis)
    for g, m in enumerate(mem):
        assert list(q.grp_row[q.grp_begin[g]:q.grp_begin[g + 1]]) == m
        want = ub[m].max(axis=0) if m else np.zeros(gb.shape[1], np.uint64)
        assert np.array_equal(gb[g], want), g
        assert int(q.group_n_cis[g]) == int(ung.n_cis[m].astype(np.int64).sum())
        if q.group_n_cis[g]:
            k = int(q.best_row[g])
            assert k in m and q.n_ge[g] >= ung.n_ge[k] and q.best_variant[g] == ung.best_variant[k]
            assert gb[g, 0] == ub[k, 0] and k == min(j for j in m if ub[j, 0] == gb[g, 0])
            ref.same_bits([q.best_r[g], q.best_slope[g]], [ung.best_r[k], ung.best_slope[k]])
        else:
            assert q.best_row[g] == NO_PAIR and q.best_variant[g] == NO_PAIR


def no_pairs(q, g):
    """What the contract says of a group without pairs."""
    B = q.n_perm
    assert q.group_n_cis[g] == 0 and q.best_row[g] == NO_PAIR and q.best_variant[g] == NO_PAIR
    assert not np.ascontiguousarray(q.perm_r[g]).view(np.uint64).any()                   # (+0.0 throughout, not -0.0)
    assert np.array_equal(np.array([q.best_r[g], q.best_slope[g]]).view(np.uint64), np.zeros(2, np.uint64))
    assert q.n_ge[g] == B and q.p_perm[g] == 1.0 and q.beta_status[g] == 2
    assert math.isnan(q.p_beta[g]) and math.isnan(q.beta_shape1[g]) and math.isnan(q.beta_shape2[g])


def same_group_result(a, b):
    """Every array of two results (library against library): the integers exactly, the doubles as bit patterns, NaN included."""
    assert (a.n_pairs, a.n_perm, a.dof, a.n_groups, a.n_rows) == (b.n_pairs, b.n_perm, b.dof, b.n_groups, b.n_rows)
    for f in ("variant_verdict", "n_cis", "grp_begin", "grp_row", "group_n_cis", "best_row", "best_variant", "n_ge", "beta_status"):
        assert np.array_equal(getattr(a, f), getattr(b, f)), f
    for f in ("yy", "gg", "perm_r", "best_r", "best_slope", "p_perm", "beta_shape1", "beta_shape2", "p_beta"):
        ref.same_bits(getattr(a, f), getattr(b, f))


def same_as_ungrouped(q, ung):
    """A result of singleton groups (group[k] = k) against the ungrouped result of the same input: every array."""
    K = ung.n_rows
    assert (q.n_groups, q.n_pairs, q.n_perm, q.dof) == (K, ung.n_pairs, ung.n_perm, ung.dof)
    assert np.array_equal(q.grp_begin, np.arange(K + 1)) and np.array_equal(q.grp_row, np.arange(K))
    assert np.array_equal(q.group_n_cis, ung.n_cis) and np.array_equal(q.best_row, np.where(ung.n_cis > 0, np.arange(K), NO_PAIR))
    for f in ("variant_verdict", "n_cis", "best_variant", "n_ge", "beta_status"):
        assert np.array_equal(getattr(q, f), getattr(ung, f)), f
    for f in ("yy", "gg", "perm_r", "best_r", "best_slope", "p_perm", "beta_shape1", "beta_shape2", "p_beta"):
        ref.same_bits(getattr(q, f), getattr(ung, f))


HEAD = ("group_id\tgroup_size\tphenotype_id\tnum_var\tbeta_shape1\tbeta_shape2\tdof\tvariant_id\tdistance\tr\tslope\tslope_se\ttstat\tpval_nominal\t"
        "pval_perm\tpval_beta\n")


def text(ids, variant_ids, var_pos, starts, q, tstat, pvalue):
    """The Python writer of rgx_cohort_format_qtl_group: ids[k] the phenotype IDs (their last field is the cluster's name), starts[k] the rows'
    starts; tstat and pvalue the library's host functions."""
    out = [HEAD]
    for g in range(q.n_groups if q is not None else 0):
        if not q.group_n_cis[g]:
            continue
        first, size = int(q.grp_row[q.grp_begin[g]]), int(q.grp_begin[g + 1]) - int(q.grp_begin[g])
        k, v = int(q.best_row[g]), int(q.best_variant[g])
        r, slope = float(q.best_r[g]), float(q.best_slope[g])
        t = tstat(r, q.dof)
        se = slope / t if not math.isinf(t) else math.copysign(0.0, slope * t)
        out.append("\t".join([ids[first].split(":")[-1], "%d" % size, ids[k], "%d" % q.group_n_cis[g], pref.g17(q.beta_shape1[g]),
                              pref.g17(q.beta_shape2[g]), "%d" % q.dof, variant_ids[v], "%d" % (int(var_pos[v]) - int(starts[k])), pref.g17(r),
                              pref.g17(slope), pref.g17(se), pref.g17(t), pref.g17(pvalue(t, q.dof)), pref.g17(q.p_perm[g]), pref.g17(q.p_beta[g])])
                   + "\n")
    return "".join(out).encode()
