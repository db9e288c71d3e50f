"""ctypes bindings of the C ABI declared in include/regtools_amd.h (libregtools_amd.so, HIP/gfx950)
and of the tooling library libregtools_synth.so (synthetic BAM writer).

The product library is loaded lazily and loading failures are NEVER swallowed: there is no Python or CPU
fallback for the hot path.
"""
import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libregtools_amd.so")
SYNTH_PATH = os.path.join(_HERE, "libregtools_synth.so")


class ExtractParams(C.Structure):
    _fields_ = [("region", C.c_char_p), ("strandness", C.c_int32), ("strand_tag", C.c_char * 2),
                ("min_anchor", C.c_uint32), ("min_intron", C.c_uint32), ("max_intron", C.c_uint32),
                ("fasta_path", C.c_char_p), ("shard", C.c_int32), ("n_shards", C.c_int32),
                ("barcodes", C.c_int32), ("barcode_tag", C.c_char * 2)]


class JunctionTable(C.Structure):
    _fields_ = [("n_ref", C.c_int32), ("ref_name", C.POINTER(C.c_char_p)), ("ref_len", C.POINTER(C.c_uint32)),
                ("n", C.c_uint64), ("tid", C.POINTER(C.c_int32)), ("start", C.POINTER(C.c_uint32)),
                ("end", C.POINTER(C.c_uint32)), ("thick_start", C.POINTER(C.c_uint32)),
                ("thick_end", C.POINTER(C.c_uint32)), ("read_count", C.POINTER(C.c_uint32)),
                ("name_index", C.POINTER(C.c_uint64)), ("strand", C.POINTER(C.c_char)),
                ("left_ok", C.POINTER(C.c_uint8)), ("right_ok", C.POINTER(C.c_uint8)),
                ("n_records", C.c_uint64), ("n_events", C.c_uint64), ("inflated_bytes", C.c_uint64),
                ("compressed_bytes", C.c_uint64), ("n_members", C.c_uint64),
                ("ms_total", C.c_double), ("ms_inflate", C.c_double), ("ms_records", C.c_double),
                ("ms_scan", C.c_double), ("ms_reduce", C.c_double),
                ("first_seen", C.POINTER(C.c_uint64)), ("last_seen", C.POINTER(C.c_uint64)), ("framing_sweeps", C.c_uint64),
                ("bc_row_begin", C.POINTER(C.c_uint64)), ("bc_count", C.POINTER(C.c_uint32)), ("bc_str_begin", C.POINTER(C.c_uint64)),
                ("bc_text", C.POINTER(C.c_char)), ("bc_insert_rank", C.POINTER(C.c_uint32)), ("ms_barcodes", C.c_double), ("stream_ended", C.c_uint64),
                ("ms_inflate_launch", C.c_double)]


class Member(C.Structure):
    _fields_ = [("cpos", C.c_uint64), ("upos", C.c_uint64), ("clen", C.c_uint32), ("isize", C.c_uint32)]


# every symbol include/regtools_amd.h declares (tests check the library exports all of them)
EXPORTS = ["rgx_extract_params_default", "rgx_ctx_create", "rgx_ctx_destroy", "rgx_extract", "rgx_extract_mem",
           "rgx_extract_device", "rgx_table_free", "rgx_table_merge", "rgx_table_pack", "rgx_table_unpack",
           "rgx_table_format_bed12", "rgx_table_format_barcodes", "rgx_version", "rgx_k_inflate",
           "rgx_identify_params_default", "rgx_identify", "rgx_gtf_load", "rgx_gtf_free", "rgx_gtf_info", "rgx_gtf_transcript_bin",
           "rgx_gtf_transcript_id", "rgx_variant_windows", "rgx_variant_hits_free", "rgx_annotate_junctions", "rgx_junction_annot_free",
           "rgx_associate", "rgx_variants_annotate", "rgx_junctions_annotate", "rgx_junctions_annotate_opts", "rgx_table_merge_device", "rgx_window_join", "rgx_window_rows_free", "rgx_last_table_pack_device",
           "rgx_host_alloc", "rgx_host_free", "rgx_extract_multi", "rgx_extract_multi_mem", "rgx_multi_exchange_kind", "rgx_k_inflate_form", "rgx_table_merge_barcodes",
           "rgx_table_pack_barcodes", "rgx_table_unpack_barcodes", "rgx_identify_multi", "rgx_ctx_arena_trials",
           "rgx_pipeline_create", "rgx_pipeline_depth", "rgx_pipeline_ctx", "rgx_extract_submit", "rgx_extract_wait", "rgx_pipeline_destroy",
           "rgx_cohort_params_default", "rgx_cohort_create", "rgx_cohort_add", "rgx_cohort_add_path", "rgx_cohort_finish", "rgx_cohort_destroy",
           "rgx_cohort_matrix_free", "rgx_cohort_merge_host", "rgx_cohort_format_bed12", "rgx_cohort_format_counts",
           "rgx_k_scan_u32", "rgx_k_members", "rgx_members_result_free", "rgx_k_radix_sort", "rgx_k_group_by",
           "rgx_cluster_params_default", "rgx_cohort_cluster", "rgx_cohort_cluster_path", "rgx_cohort_cluster_host", "rgx_cohort_clusters_free",
           "rgx_cohort_format_cluster_counts", "rgx_k_components",
           "rgx_refine_params_default", "rgx_cohort_refine", "rgx_cohort_refine_host",
           "rgx_pheno_params_default", "rgx_cohort_phenotypes", "rgx_cohort_phenotypes_host", "rgx_cohort_phenotypes_free", "rgx_pheno_quantile",
           "rgx_cohort_format_phenotypes",
           "rgx_cohort_pheno_pcs", "rgx_cohort_pheno_pcs_host", "rgx_cohort_pheno_pcs_free", "rgx_cohort_format_pheno_pcs",
           "rgx_cohort_pheno_regions", "rgx_cohort_qtl_nominal", "rgx_cohort_qtl_nominal_host", "rgx_cohort_qtl_free", "rgx_qtl_tstat",
           "rgx_qtl_pvalue", "rgx_cohort_format_qtl", "rgx_genotypes_load", "rgx_genotypes_free",
           "rgx_qtl_permutations", "rgx_cohort_qtl_permute", "rgx_cohort_qtl_permute_host", "rgx_cohort_qtl_perm_free", "rgx_qtl_digamma",
           "rgx_qtl_trigamma", "rgx_qtl_betainc", "rgx_qtl_beta_fit", "rgx_cohort_format_qtl_perm",
           "rgx_cohort_pheno_groups", "rgx_cohort_qtl_permute_grouped", "rgx_cohort_qtl_permute_grouped_host", "rgx_cohort_qtl_group_free",
           "rgx_cohort_format_qtl_group",
           "rgx_cohort_qtl_permute_conditional", "rgx_cohort_qtl_permute_conditional_host", "rgx_cohort_qtl_cond_free",
           "rgx_cohort_qtl_independent", "rgx_cohort_qtl_independent_host", "rgx_cohort_qtl_indep_free", "rgx_cohort_format_qtl_indep",
           "rgx_cohort_qtl_trans", "rgx_cohort_qtl_trans_host", "rgx_cohort_qtl_trans_free", "rgx_qtl_r_threshold", "rgx_cohort_format_qtl_trans",
           "rgx_gtf_bin_index", "rgx_k_junction_scan", "rgx_junction_items_free", "rgx_pair_list_free", "rgx_k_window_pairs", "rgx_k_assoc_pairs"]


class CohortParams(C.Structure):
    _fields_ = [("only_anchored", C.c_int32), ("min_samples", C.c_uint32), ("min_total", C.c_uint64)]


class CohortMatrix(C.Structure):
    _fields_ = [("n_ref", C.c_int32), ("ref_name", C.POINTER(C.c_char_p)), ("ref_len", C.POINTER(C.c_uint32)),
                ("n_samples", C.c_uint32), ("sample_name", C.POINTER(C.c_char_p)), ("n", C.c_uint64),
                ("tid", C.POINTER(C.c_uint32)), ("start", C.POINTER(C.c_uint32)), ("end", C.POINTER(C.c_uint32)),
                ("thick_start", C.POINTER(C.c_uint32)), ("thick_end", C.POINTER(C.c_uint32)), ("strand", C.POINTER(C.c_char)),
                ("n_with", C.POINTER(C.c_uint32)), ("total", C.POINTER(C.c_uint64)), ("row_begin", C.POINTER(C.c_uint64)),
                ("col_sample", C.POINTER(C.c_uint32)), ("val_count", C.POINTER(C.c_uint32)),
                ("ms_add_total", C.c_double), ("ms_finish", C.c_double), ("n_triples", C.c_uint64)]


class ClusterParams(C.Structure):
    _fields_ = [("min_rows", C.c_uint32), ("min_total", C.c_uint64)]


class CohortClusters(C.Structure):
    _fields_ = [("n_rows", C.c_uint64), ("n_clusters", C.c_uint64), ("cluster", C.POINTER(C.c_uint32)), ("cl_begin", C.POINTER(C.c_uint64)),
                ("cl_row", C.POINTER(C.c_uint32)), ("cl_total", C.POINTER(C.c_uint64)), ("cs_begin", C.POINTER(C.c_uint64)),
                ("cs_sample", C.POINTER(C.c_uint32)), ("cs_total", C.POINTER(C.c_uint64)),
                ("n_rounds", C.c_uint32), ("ms_cluster", C.c_double), ("n_components", C.c_uint64),
                ("n_ineligible", C.c_uint64), ("n_weak", C.c_uint64)]


class RefineParams(C.Structure):
    _fields_ = [("max_intron", C.c_uint32), ("min_reads", C.c_uint64), ("ratio_num", C.c_uint32), ("ratio_den", C.c_uint32),
                ("min_rows", C.c_uint32), ("min_total", C.c_uint64)]


class PhenoParams(C.Structure):
    _fields_ = [("na_num", C.c_uint32), ("na_den", C.c_uint32), ("min_sd", C.c_double)]


class PhenoTable(C.Structure):
    _fields_ = [("n_rows", C.c_uint64), ("n_samples", C.c_uint32), ("row", C.POINTER(C.c_uint32)), ("n_na", C.POINTER(C.c_uint32)),
                ("mean", C.POINTER(C.c_double)), ("sd", C.POINTER(C.c_double)), ("rank2", C.POINTER(C.c_uint32)),
                ("n_clustered", C.c_uint64), ("n_drop_na", C.c_uint64), ("n_drop_sd", C.c_uint64), ("ms_pheno", C.c_double)]


class PhenoPCs(C.Structure):
    _fields_ = [("n_rows", C.c_uint64), ("n_samples", C.c_uint32), ("n_pcs", C.c_uint32), ("col_sum", C.POINTER(C.c_double)),
                ("gram", C.POINTER(C.c_double)), ("variance", C.POINTER(C.c_double)), ("component", C.POINTER(C.c_double)),
                ("ms_pcs", C.c_double), ("ms_gram", C.c_double), ("ms_eigen", C.c_double)]


class Genotypes(C.Structure):
    _fields_ = [("n_variants", C.c_uint32), ("n_samples", C.c_uint32), ("tid", C.POINTER(C.c_uint32)), ("pos", C.POINTER(C.c_uint32)),
                ("dosage", C.POINTER(C.c_int8)), ("id", C.POINTER(C.c_char_p)),
                ("n_records", C.c_uint64), ("n_multiallelic", C.c_uint64), ("n_no_gt", C.c_uint64), ("n_unknown_contig", C.c_uint64)]


class QtlRegion(C.Structure):
    _fields_ = [("tid", C.c_uint32), ("start", C.c_uint32), ("end", C.c_uint32)]


class QtlResult(C.Structure):
    _fields_ = [("n_rows", C.c_uint64), ("n_samples", C.c_uint32), ("n_variants", C.c_uint32), ("n_cov", C.c_uint32), ("dof", C.c_uint32),
                ("n_pairs", C.c_uint64), ("variant_verdict", C.POINTER(C.c_uint8)), ("yy", C.POINTER(C.c_double)), ("gg", C.POINTER(C.c_double)),
                ("pair_begin", C.POINTER(C.c_uint32)), ("pair_variant", C.POINTER(C.c_uint32)), ("r", C.POINTER(C.c_double)),
                ("slope", C.POINTER(C.c_double)), ("best", C.POINTER(C.c_uint32)),
                ("n_constant", C.c_uint64), ("n_explained", C.c_uint64), ("n_flat_rows", C.c_uint64), ("n_tiles", C.c_uint64),
                ("ms_qtl", C.c_double), ("ms_residual", C.c_double), ("ms_pairs", C.c_double)]


class QtlTransResult(C.Structure):
    _fields_ = [("n_rows", C.c_uint64), ("n_samples", C.c_uint32), ("n_variants", C.c_uint32), ("n_cov", C.c_uint32), ("dof", C.c_uint32),
                ("n_tested", C.c_uint64), ("n_hits", C.c_uint64), ("variant_verdict", C.POINTER(C.c_uint8)), ("yy", C.POINTER(C.c_double)),
                ("gg", C.POINTER(C.c_double)), ("hit_begin", C.POINTER(C.c_uint32)), ("hit_variant", C.POINTER(C.c_uint32)),
                ("r", C.POINTER(C.c_double)), ("slope", C.POINTER(C.c_double)),
                ("n_constant", C.c_uint64), ("n_explained", C.c_uint64), ("n_flat_rows", C.c_uint64), ("n_tiles", C.c_uint64),
                ("n_hit_tiles", C.c_uint64), ("ms_trans", C.c_double), ("ms_residual", C.c_double), ("ms_count", C.c_double),
                ("ms_emit", C.c_double)]


class QtlPermResult(C.Structure):
    _fields_ = [("n_rows", C.c_uint64), ("n_samples", C.c_uint32), ("n_variants", C.c_uint32), ("n_cov", C.c_uint32), ("dof", C.c_uint32),
                ("n_perm", C.c_uint32), ("n_pairs", C.c_uint64), ("variant_verdict", C.POINTER(C.c_uint8)), ("yy", C.POINTER(C.c_double)),
                ("gg", C.POINTER(C.c_double)), ("n_cis", C.POINTER(C.c_uint32)), ("perm_r", C.POINTER(C.c_double)),
                ("best_variant", C.POINTER(C.c_uint32)), ("best_r", C.POINTER(C.c_double)), ("best_slope", C.POINTER(C.c_double)),
                ("n_ge", C.POINTER(C.c_uint32)), ("p_perm", C.POINTER(C.c_double)), ("beta_shape1", C.POINTER(C.c_double)),
                ("beta_shape2", C.POINTER(C.c_double)), ("p_beta", C.POINTER(C.c_double)), ("beta_status", C.POINTER(C.c_uint8)),
                ("n_constant", C.c_uint64), ("n_explained", C.c_uint64), ("n_flat_rows", C.c_uint64), ("n_tiles", C.c_uint64),
                ("ms_perm", C.c_double), ("ms_residual", C.c_double), ("ms_products", C.c_double), ("ms_beta", C.c_double)]


class QtlGroupResult(C.Structure):
    _fields_ = [("n_rows", C.c_uint64), ("n_samples", C.c_uint32), ("n_variants", C.c_uint32), ("n_cov", C.c_uint32), ("dof", C.c_uint32),
                ("n_perm", C.c_uint32), ("n_groups", C.c_uint32), ("n_pairs", C.c_uint64), ("variant_verdict", C.POINTER(C.c_uint8)),
                ("yy", C.POINTER(C.c_double)), ("gg", C.POINTER(C.c_double)), ("n_cis", C.POINTER(C.c_uint32)),
                ("grp_begin", C.POINTER(C.c_uint32)), ("grp_row", C.POINTER(C.c_uint32)), ("group_n_cis", C.POINTER(C.c_uint64)),
                ("perm_r", C.POINTER(C.c_double)), ("best_row", C.POINTER(C.c_uint32)), ("best_variant", C.POINTER(C.c_uint32)),
                ("best_r", C.POINTER(C.c_double)), ("best_slope", C.POINTER(C.c_double)),
                ("n_ge", C.POINTER(C.c_uint32)), ("p_perm", C.POINTER(C.c_double)), ("beta_shape1", C.POINTER(C.c_double)),
                ("beta_shape2", C.POINTER(C.c_double)), ("p_beta", C.POINTER(C.c_double)), ("beta_status", C.POINTER(C.c_uint8)),
                ("n_constant", C.c_uint64), ("n_explained", C.c_uint64), ("n_flat_rows", C.c_uint64), ("n_tiles", C.c_uint64),
                ("ms_perm", C.c_double), ("ms_residual", C.c_double), ("ms_products", C.c_double), ("ms_beta", C.c_double)]


class QtlCondResult(C.Structure):
    _fields_ = [("n_rows", C.c_uint64), ("n_samples", C.c_uint32), ("n_variants", C.c_uint32), ("n_cov", C.c_uint32), ("n_perm", C.c_uint32),
                ("n_series", C.c_uint32), ("n_cond", C.c_uint32), ("n_pairs", C.c_uint64), ("variant_verdict", C.POINTER(C.c_uint8)),
                ("yy", C.POINTER(C.c_double)), ("gg", C.POINTER(C.c_double)), ("series_row", C.POINTER(C.c_uint32)),
                ("cond_begin", C.POINTER(C.c_uint32)), ("cond_variant", C.POINTER(C.c_uint32)), ("cond_status", C.POINTER(C.c_uint8)),
                ("yy_cond", C.POINTER(C.c_double)), ("dof", C.POINTER(C.c_uint32)), ("n_window", C.POINTER(C.c_uint32)),
                ("n_cis", C.POINTER(C.c_uint32)), ("perm_r", C.POINTER(C.c_double)), ("best_variant", C.POINTER(C.c_uint32)),
                ("best_r", C.POINTER(C.c_double)), ("best_slope", C.POINTER(C.c_double)), ("n_ge", C.POINTER(C.c_uint32)),
                ("p_perm", C.POINTER(C.c_double)), ("beta_shape1", C.POINTER(C.c_double)), ("beta_shape2", C.POINTER(C.c_double)),
                ("p_beta", C.POINTER(C.c_double)), ("beta_status", C.POINTER(C.c_uint8)),
                ("n_constant", C.c_uint64), ("n_explained", C.c_uint64), ("n_flat_rows", C.c_uint64), ("n_collinear", C.c_uint64),
                ("n_flat_series", C.c_uint64), ("n_tiles", C.c_uint64),
                ("ms_cond", C.c_double), ("ms_residual", C.c_double), ("ms_prepare", C.c_double), ("ms_products", C.c_double),
                ("ms_beta", C.c_double)]


class QtlIndepResult(C.Structure):
    _fields_ = [("n_rows", C.c_uint64), ("n_samples", C.c_uint32), ("n_variants", C.c_uint32), ("n_cov", C.c_uint32), ("n_perm", C.c_uint32),
                ("max_signals", C.c_uint32), ("p_threshold", C.c_double), ("n_signals", C.c_uint64), ("sig_begin", C.POINTER(C.c_uint32)),
                ("capped", C.POINTER(C.c_uint8)), ("variant", C.POINTER(C.c_uint32)), ("rank", C.POINTER(C.c_uint32)),
                ("n_cond", C.POINTER(C.c_uint32)), ("dof", C.POINTER(C.c_uint32)), ("n_cis", C.POINTER(C.c_uint32)),
                ("r", C.POINTER(C.c_double)), ("slope", C.POINTER(C.c_double)), ("p_perm", C.POINTER(C.c_double)),
                ("beta_shape1", C.POINTER(C.c_double)), ("beta_shape2", C.POINTER(C.c_double)), ("p_beta", C.POINTER(C.c_double)),
                ("beta_status", C.POINTER(C.c_uint8)),
                ("n_entered", C.c_uint64), ("n_forward_rounds", C.c_uint32), ("n_series_total", C.c_uint64), ("n_capped", C.c_uint64),
                ("ms_indep", C.c_double), ("ms_round0", C.c_double), ("ms_forward", C.c_double), ("ms_backward", C.c_double)]


class IdentifyParams(C.Structure):
    _fields_ = [("vcf_path", C.c_char_p), ("bam_path", C.c_char_p), ("fasta_path", C.c_char_p), ("gtf_path", C.c_char_p),
                ("out_tsv", C.c_char_p), ("out_vcf", C.c_char_p), ("out_bed", C.c_char_p), ("window", C.c_uint32),
                ("intronic_min", C.c_uint32), ("exonic_min", C.c_uint32), ("all_intronic", C.c_int32), ("all_exonic", C.c_int32),
                ("skip_single", C.c_int32), ("strandness", C.c_int32), ("strand_tag", C.c_char * 2), ("min_anchor", C.c_uint32),
                ("min_intron", C.c_uint32), ("max_intron", C.c_uint32), ("override_motif", C.c_int32), ("bed_path", C.c_char_p), ("echo", C.c_int32)]


class IdentifyStats(C.Structure):
    _fields_ = [(n, C.c_uint64) for n in ("n_variants", "n_relevant", "n_windows", "n_pairs", "n_window_rows", "n_junctions", "n_records", "n_events",
                                          "exon_visits_variants", "exon_visits_junctions")] + \
               [(n, C.c_double) for n in ("ms_total", "ms_gtf", "ms_variants", "ms_extract", "ms_join", "ms_annotate", "ms_output",
                                          "ms_k_variant_scan", "ms_k_junction_scan", "ms_k_window_pairs")]


class VariantHits(C.Structure):
    _fields_ = [("n", C.c_uint64), ("cis_start", C.POINTER(C.c_uint32)), ("cis_end", C.POINTER(C.c_uint32)), ("hit_off", C.POINTER(C.c_uint32)),
                ("hit_transcript", C.POINTER(C.c_uint32)), ("hit_annotation", C.POINTER(C.c_uint32)), ("hit_distance", C.POINTER(C.c_uint32))]


class WindowRows(C.Structure):
    _fields_ = [("n", C.c_uint64)] + [(k, C.POINTER(C.c_uint32)) for k in ("window", "start", "end", "thick_start", "thick_end", "read_count", "name_index")] + \
               [("strand", C.POINTER(C.c_char))]


class JunctionAnnot(C.Structure):
    _fields_ = [("n", C.c_uint64), ("flags", C.POINTER(C.c_uint32)), ("n_acceptors_skipped", C.POINTER(C.c_uint32)),
                ("n_exons_skipped", C.POINTER(C.c_uint32)), ("n_donors_skipped", C.POINTER(C.c_uint32)), ("tx_off", C.POINTER(C.c_uint32)),
                ("tx", C.POINTER(C.c_uint32))]


class JunctionItems(C.Structure):
    _fields_ = [("n", C.c_uint64), ("visits_total", C.c_uint64)] + \
               [(k, C.POINTER(C.c_uint32)) for k in ("flags", "visits", "item_off", "item_kind", "item_a", "item_b")]


class PairList(C.Structure):
    _fields_ = [("n", C.c_uint64), ("n_batches", C.c_uint32), ("first", C.POINTER(C.c_uint32)), ("window", C.POINTER(C.c_uint32))]


class MembersResult(C.Structure):
    _fields_ = [("n_candidates", C.c_uint64), ("n_members", C.c_uint64), ("total_inflated", C.c_uint64), ("candidates", C.POINTER(C.c_uint64)),
                ("members", C.POINTER(Member)), ("q_upos", C.c_uint64 * 3), ("q_index", C.c_uint32 * 3), ("stop", C.c_uint32)]


_lib = None


def _preload_torch_hip_runtime():
    """PyTorch wheels bundle their own libamdhip64.so and ask for it by file name, while this library asks for
    the SONAME libamdhip64.so.7: loaded in the wrong order the process ends up with TWO HIP runtimes and the second
    one sees no GPU.  Loading torch's copy first (when torch is installed) makes both resolve to the same object."""
    try:
        import importlib.util
        spec = importlib.util.find_spec("torch")
        if spec and spec.submodule_search_locations:
            cand = os.path.join(list(spec.submodule_search_locations)[0], "lib", "libamdhip64.so")
            if os.path.exists(cand):
                C.CDLL(cand, mode=C.RTLD_GLOBAL)
    except Exception:
        pass


def lib():
    """Load libregtools_amd.so (raises if it was not built: no fallback)."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError("regtools_amd: %s is missing -- run `python -c 'import __graft_entry__ as g; g.build()'` "
                               "(hipcc --offload-arch=gfx950). There is no CPU fallback." % LIB_PATH)
        _preload_torch_hip_runtime()
        L = C.CDLL(LIB_PATH)
        P = C.POINTER
        L.rgx_version.restype = C.c_char_p
        L.rgx_extract_params_default.argtypes = [P(ExtractParams)]
        L.rgx_ctx_create.argtypes = [C.c_int, P(C.c_void_p), C.c_char_p, C.c_size_t]
        L.rgx_ctx_destroy.argtypes = [C.c_void_p]
        L.rgx_ctx_arena_trials.argtypes = [C.c_void_p, P(C.c_float), C.c_int]
        L.rgx_extract.argtypes = [C.c_void_p, C.c_char_p, P(ExtractParams), P(P(JunctionTable)), C.c_char_p, C.c_size_t]
        L.rgx_extract_mem.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, P(ExtractParams),
                                      P(P(JunctionTable)), C.c_char_p, C.c_size_t]
        L.rgx_extract_device.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t,
                                         P(ExtractParams), P(P(JunctionTable)), C.c_char_p, C.c_size_t]
        L.rgx_table_free.argtypes = [P(JunctionTable)]
        L.rgx_pipeline_create.argtypes = [C.c_int, C.c_int, P(C.c_void_p), C.c_char_p, C.c_size_t]
        L.rgx_pipeline_depth.argtypes = [C.c_void_p]
        L.rgx_pipeline_ctx.argtypes = [C.c_void_p, C.c_uint64]
        L.rgx_pipeline_ctx.restype = C.c_void_p
        L.rgx_extract_submit.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, P(ExtractParams), P(C.c_uint64), C.c_char_p, C.c_size_t]
        L.rgx_extract_wait.argtypes = [C.c_void_p, C.c_uint64, P(P(JunctionTable)), C.c_char_p, C.c_size_t]
        L.rgx_pipeline_destroy.argtypes = [C.c_void_p]
        L.rgx_extract_multi.argtypes = [P(C.c_int), C.c_int, C.c_char_p, P(ExtractParams), P(P(JunctionTable)), C.c_char_p, C.c_size_t]
        L.rgx_multi_exchange_kind.restype = C.c_char_p
        L.rgx_multi_exchange_kind.argtypes = []
        L.rgx_extract_multi_mem.argtypes = [P(C.c_int), C.c_int, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, P(ExtractParams), P(P(JunctionTable)), C.c_char_p, C.c_size_t]
        L.rgx_host_alloc.argtypes = [C.c_size_t]
        L.rgx_host_alloc.restype = C.c_void_p
        L.rgx_host_free.argtypes = [C.c_void_p]
        L.rgx_table_merge.argtypes = [P(P(JunctionTable)), C.c_int, C.c_uint32, P(P(JunctionTable)), C.c_char_p, C.c_size_t]
        L.rgx_table_merge_barcodes.argtypes = [P(P(JunctionTable)), C.c_int, P(JunctionTable), C.c_char_p, C.c_size_t]
        L.rgx_table_pack_barcodes.argtypes = [P(JunctionTable), C.c_void_p, C.c_size_t]
        L.rgx_table_pack_barcodes.restype = C.c_size_t
        L.rgx_table_unpack_barcodes.argtypes = [P(JunctionTable), C.c_void_p, C.c_size_t]
        L.rgx_table_pack.argtypes = [P(JunctionTable), C.c_void_p, C.c_size_t]
        L.rgx_table_pack.restype = C.c_size_t
        L.rgx_table_unpack.argtypes = [C.c_void_p, C.c_size_t, P(JunctionTable), P(P(JunctionTable))]
        L.rgx_last_table_pack_device.argtypes = [C.c_void_p, P(JunctionTable), C.c_void_p, C.c_uint64, C.c_char_p, C.c_size_t]
        L.rgx_table_merge_device.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, P(C.c_uint64), C.c_int, C.c_uint32, P(JunctionTable), P(P(JunctionTable)), C.c_char_p, C.c_size_t]
        L.rgx_table_format_bed12.argtypes = [P(JunctionTable), C.c_int, C.c_char_p, C.c_size_t]
        L.rgx_table_format_bed12.restype = C.c_size_t
        L.rgx_table_format_barcodes.argtypes = [P(JunctionTable), C.c_int, C.c_char_p, C.c_size_t]
        L.rgx_table_format_barcodes.restype = C.c_size_t
        L.rgx_k_inflate.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p]
        L.rgx_k_inflate_form.argtypes = [C.c_int, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p]
        L.rgx_k_scan_u32.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_char_p, C.c_size_t]
        L.rgx_k_members.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint64, C.c_void_p, P(C.c_uint64), P(P(MembersResult)), C.c_char_p, C.c_size_t]
        L.rgx_members_result_free.argtypes = [P(MembersResult)]
        L.rgx_k_radix_sort.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, P(C.c_void_p), P(C.c_uint32), C.c_int, C.c_void_p, C.c_char_p, C.c_size_t]
        L.rgx_k_group_by.argtypes = [C.c_void_p] + [C.c_void_p] * 6 + [C.c_uint32, C.c_uint32, C.c_uint32, P(C.c_uint32), C.c_uint32, C.c_int, C.c_void_p,
                                     P(C.c_uint64), C.c_void_p, C.c_void_p, C.c_char_p, C.c_size_t]
        L.rgx_identify_params_default.argtypes = [P(IdentifyParams)]
        L.rgx_identify.argtypes = [C.c_void_p, P(IdentifyParams), P(IdentifyStats), C.c_char_p, C.c_size_t]
        L.rgx_associate.argtypes = L.rgx_identify.argtypes
        L.rgx_identify_multi.argtypes = [P(C.c_int), C.c_int, P(IdentifyParams), P(IdentifyStats), C.c_char_p, C.c_size_t]
        L.rgx_variants_annotate.argtypes = L.rgx_identify.argtypes
        L.rgx_junctions_annotate_opts.argtypes = [C.c_void_p, C.c_char_p, C.c_char_p, C.c_char_p, C.c_char_p, C.c_int, P(C.c_uint64), C.c_char_p, C.c_size_t]
        L.rgx_junctions_annotate.argtypes = [C.c_void_p, C.c_char_p, C.c_char_p, C.c_char_p, C.c_char_p, P(C.c_uint64), C.c_char_p, C.c_size_t]
        L.rgx_gtf_load.argtypes = [C.c_void_p, C.c_char_p, P(C.c_void_p), C.c_char_p, C.c_size_t]
        L.rgx_gtf_free.argtypes = [C.c_void_p]
        L.rgx_gtf_info.argtypes = [C.c_void_p, P(C.c_uint32), P(C.c_uint32), P(C.c_uint32)]
        L.rgx_gtf_transcript_bin.argtypes = [C.c_void_p, C.c_char_p, P(C.c_uint32)]
        L.rgx_gtf_transcript_id.argtypes = [C.c_void_p, C.c_uint32]
        L.rgx_gtf_transcript_id.restype = C.c_char_p
        L.rgx_variant_windows.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, P(C.c_char_p), P(C.c_uint32), C.c_uint32, C.c_uint32, C.c_int, C.c_int, C.c_int,
                                          P(P(VariantHits)), C.c_char_p, C.c_size_t]
        L.rgx_variant_hits_free.argtypes = [P(VariantHits)]
        L.rgx_annotate_junctions.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, P(C.c_char_p), P(C.c_uint32), P(C.c_uint32), C.c_char_p,
                                             P(P(JunctionAnnot)), C.c_char_p, C.c_size_t]
        L.rgx_junction_annot_free.argtypes = [P(JunctionAnnot)]
        L.rgx_gtf_bin_index.argtypes = [C.c_void_p]
        L.rgx_k_junction_scan.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, P(C.c_int32), P(C.c_uint32), P(C.c_uint32), C.c_char_p, C.c_int, C.c_int,
                                          P(P(JunctionItems)), C.c_char_p, C.c_size_t]
        L.rgx_junction_items_free.argtypes = [P(JunctionItems)]
        L.rgx_pair_list_free.argtypes = [P(PairList)]
        L.rgx_k_window_pairs.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, P(C.c_int32), P(C.c_int32), P(C.c_int32),
                                         C.c_uint64, P(P(PairList)), C.c_char_p, C.c_size_t]
        L.rgx_k_assoc_pairs.argtypes = [C.c_void_p, C.c_uint32, P(C.c_int32), P(C.c_uint32), P(C.c_uint32), C.c_uint32, P(C.c_uint32), C.c_uint32,
                                        P(C.c_uint32), P(C.c_uint32), P(P(PairList)), C.c_char_p, C.c_size_t]
        L.rgx_window_join.argtypes = [C.c_void_p, C.c_char_p, P(ExtractParams), C.c_uint64, P(C.c_char_p), P(C.c_int32), P(C.c_int32), P(P(WindowRows)), C.c_char_p, C.c_size_t]
        L.rgx_window_rows_free.argtypes = [P(WindowRows)]
        L.rgx_cohort_params_default.argtypes = [P(CohortParams)]
        L.rgx_cohort_create.argtypes = [C.c_void_p, P(CohortParams), P(C.c_void_p), C.c_char_p, C.c_size_t]
        L.rgx_cohort_add.argtypes = [C.c_void_p, C.c_void_p, P(JunctionTable), C.c_uint32, C.c_char_p, P(C.c_uint32), C.c_char_p, C.c_size_t]
        L.rgx_cohort_add_path.argtypes = [C.c_void_p]
        L.rgx_cohort_finish.argtypes = [C.c_void_p, P(P(CohortMatrix)), C.c_char_p, C.c_size_t]
        L.rgx_cohort_destroy.argtypes = [C.c_void_p]
        L.rgx_cohort_matrix_free.argtypes = [P(CohortMatrix)]
        L.rgx_cohort_merge_host.argtypes = [P(P(JunctionTable)), P(C.c_uint32), P(C.c_char_p), C.c_int, P(CohortParams), P(P(CohortMatrix)),
                                            C.c_char_p, C.c_size_t]
        L.rgx_cohort_format_bed12.argtypes = [P(CohortMatrix), C.c_char_p, C.c_size_t]
        L.rgx_cohort_format_bed12.restype = C.c_size_t
        L.rgx_cohort_format_counts.argtypes = [P(CohortMatrix), C.c_char_p, C.c_size_t]
        L.rgx_cohort_format_counts.restype = C.c_size_t
        L.rgx_cluster_params_default.argtypes = [P(ClusterParams)]
        L.rgx_cohort_cluster.argtypes = [C.c_void_p, P(CohortMatrix), P(ClusterParams), P(P(CohortClusters)), C.c_char_p, C.c_size_t]
        L.rgx_cohort_cluster_path.argtypes = [C.c_void_p]
        L.rgx_cohort_cluster_host.argtypes = [P(CohortMatrix), P(ClusterParams), P(P(CohortClusters)), C.c_char_p, C.c_size_t]
        L.rgx_cohort_clusters_free.argtypes = [P(CohortClusters)]
        L.rgx_cohort_format_cluster_counts.argtypes = [P(CohortMatrix), P(CohortClusters), C.c_char_p, C.c_size_t]
        L.rgx_cohort_format_cluster_counts.restype = C.c_size_t
        L.rgx_refine_params_default.argtypes = [P(RefineParams)]
        L.rgx_cohort_refine.argtypes = [C.c_void_p, P(CohortMatrix), P(RefineParams), P(P(CohortClusters)), C.c_char_p, C.c_size_t]
        L.rgx_cohort_refine_host.argtypes = [P(CohortMatrix), P(RefineParams), P(P(CohortClusters)), C.c_char_p, C.c_size_t]
        L.rgx_pheno_params_default.argtypes = [P(PhenoParams)]
        L.rgx_cohort_phenotypes.argtypes = [C.c_void_p, P(CohortMatrix), P(CohortClusters), P(PhenoParams), P(P(PhenoTable)), C.c_char_p, C.c_size_t]
        L.rgx_cohort_phenotypes_host.argtypes = [P(CohortMatrix), P(CohortClusters), P(PhenoParams), P(P(PhenoTable)), C.c_char_p, C.c_size_t]
        L.rgx_cohort_phenotypes_free.argtypes = [P(PhenoTable)]
        L.rgx_pheno_quantile.argtypes = [C.c_uint32, C.c_uint64]
        L.rgx_pheno_quantile.restype = C.c_double
        L.rgx_cohort_format_phenotypes.argtypes = [P(CohortMatrix), P(CohortClusters), P(PhenoTable), C.c_char_p, C.c_size_t]
        L.rgx_cohort_format_phenotypes.restype = C.c_size_t
        L.rgx_cohort_pheno_pcs.argtypes = [C.c_void_p, P(PhenoTable), C.c_uint32, P(P(PhenoPCs)), C.c_char_p, C.c_size_t]
        L.rgx_cohort_pheno_pcs_host.argtypes = [P(PhenoTable), C.c_uint32, P(P(PhenoPCs)), C.c_char_p, C.c_size_t]
        L.rgx_cohort_pheno_pcs_free.argtypes = [P(PhenoPCs)]
        L.rgx_cohort_format_pheno_pcs.argtypes = [P(CohortMatrix), P(PhenoPCs), C.c_char_p, C.c_size_t]
        L.rgx_cohort_format_pheno_pcs.restype = C.c_size_t
        qtl_in = [P(PhenoTable), C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, P(P(QtlResult)),
                  C.c_char_p, C.c_size_t]
        L.rgx_cohort_qtl_nominal.argtypes = [C.c_void_p] + qtl_in
        L.rgx_cohort_qtl_nominal_host.argtypes = qtl_in
        L.rgx_cohort_qtl_free.argtypes = [P(QtlResult)]
        L.rgx_cohort_pheno_regions.argtypes = [P(CohortMatrix), P(PhenoTable), C.c_void_p, C.c_char_p, C.c_size_t]
        L.rgx_genotypes_load.argtypes = [C.c_char_p, P(CohortMatrix), P(P(Genotypes)), C.c_char_p, C.c_size_t]
        L.rgx_genotypes_free.argtypes = [P(Genotypes)]
        L.rgx_qtl_tstat.argtypes = [C.c_double, C.c_uint32]
        L.rgx_qtl_tstat.restype = C.c_double
        L.rgx_qtl_pvalue.argtypes = [C.c_double, C.c_uint32]
        L.rgx_qtl_pvalue.restype = C.c_double
        L.rgx_cohort_format_qtl.argtypes = [P(CohortMatrix), P(CohortClusters), P(PhenoTable), P(QtlResult), C.c_void_p, P(C.c_char_p), C.c_char_p,
                                            C.c_size_t]
        L.rgx_cohort_format_qtl.restype = C.c_size_t
        perm_in = [P(PhenoTable), C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, C.c_uint32,
                   C.c_void_p, P(P(QtlPermResult)), C.c_char_p, C.c_size_t]
        L.rgx_cohort_qtl_permute.argtypes = [C.c_void_p] + perm_in
        L.rgx_cohort_qtl_permute_host.argtypes = perm_in
        L.rgx_cohort_qtl_perm_free.argtypes = [P(QtlPermResult)]
        L.rgx_qtl_permutations.argtypes = [C.c_uint32, C.c_uint32, C.c_uint64, C.c_void_p, C.c_char_p, C.c_size_t]
        for fn in (L.rgx_qtl_digamma, L.rgx_qtl_trigamma):
            fn.argtypes = [C.c_double]
            fn.restype = C.c_double
        L.rgx_qtl_betainc.argtypes = [C.c_double, C.c_double, C.c_double]
        L.rgx_qtl_betainc.restype = C.c_double
        L.rgx_qtl_beta_fit.argtypes = [C.c_void_p, C.c_uint32, P(C.c_double), P(C.c_double)]
        L.rgx_cohort_format_qtl_perm.argtypes = [P(CohortMatrix), P(CohortClusters), P(PhenoTable), P(QtlPermResult), C.c_void_p, P(C.c_char_p),
                                                 C.c_char_p, C.c_size_t]
        L.rgx_cohort_format_qtl_perm.restype = C.c_size_t
        group_in = perm_in[:11] + [C.c_uint32, C.c_void_p, P(P(QtlGroupResult)), C.c_char_p, C.c_size_t]
        L.rgx_cohort_qtl_permute_grouped.argtypes = [C.c_void_p] + group_in
        L.rgx_cohort_qtl_permute_grouped_host.argtypes = group_in
        L.rgx_cohort_qtl_group_free.argtypes = [P(QtlGroupResult)]
        cond_in = perm_in[:11] + [C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, P(P(QtlCondResult)), C.c_char_p, C.c_size_t]
        L.rgx_cohort_qtl_permute_conditional.argtypes = [C.c_void_p] + cond_in
        L.rgx_cohort_qtl_permute_conditional_host.argtypes = cond_in
        L.rgx_cohort_qtl_cond_free.argtypes = [P(QtlCondResult)]
        indep_in = perm_in[:11] + [C.c_double, C.c_uint32, P(P(QtlIndepResult)), C.c_char_p, C.c_size_t]
        L.rgx_cohort_qtl_independent.argtypes = [C.c_void_p] + indep_in
        L.rgx_cohort_qtl_independent_host.argtypes = indep_in
        L.rgx_cohort_qtl_indep_free.argtypes = [P(QtlIndepResult)]
        L.rgx_cohort_format_qtl_indep.argtypes = [P(CohortMatrix), P(CohortClusters), P(PhenoTable), P(QtlIndepResult), C.c_void_p, P(C.c_char_p),
                                                  C.c_char_p, C.c_size_t]
        L.rgx_cohort_format_qtl_indep.restype = C.c_size_t
        L.rgx_cohort_pheno_groups.argtypes = [P(CohortClusters), P(PhenoTable), C.c_void_p, P(C.c_uint32), C.c_char_p, C.c_size_t]
        L.rgx_cohort_format_qtl_group.argtypes = [P(CohortMatrix), P(CohortClusters), P(PhenoTable), P(QtlGroupResult), C.c_void_p, P(C.c_char_p),
                                                  C.c_char_p, C.c_size_t]
        L.rgx_cohort_format_qtl_group.restype = C.c_size_t
        trans_in = qtl_in[:8] + [C.c_double, C.c_int, C.c_uint32, C.c_uint64, P(P(QtlTransResult)), C.c_char_p, C.c_size_t]
        L.rgx_cohort_qtl_trans.argtypes = [C.c_void_p] + trans_in
        L.rgx_cohort_qtl_trans_host.argtypes = trans_in
        L.rgx_cohort_qtl_trans_free.argtypes = [P(QtlTransResult)]
        L.rgx_qtl_r_threshold.argtypes = [C.c_double, C.c_uint32]
        L.rgx_qtl_r_threshold.restype = C.c_double
        L.rgx_cohort_format_qtl_trans.argtypes = [P(CohortMatrix), P(CohortClusters), P(PhenoTable), P(QtlTransResult), C.c_void_p, P(C.c_char_p),
                                                  C.c_char_p, C.c_size_t]
        L.rgx_cohort_format_qtl_trans.restype = C.c_size_t
        L.rgx_k_components.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, P(C.c_uint32), C.c_char_p, C.c_size_t]
        _lib = L
    return _lib


class SynthParams(C.Structure):
    _fields_ = [("shape", C.c_int), ("n_reads", C.c_uint64), ("seed", C.c_uint64), ("level", C.c_int),
                ("threads", C.c_int), ("n_introns", C.c_uint32), ("spliced_frac", C.c_double),
                ("realistic_payload", C.c_int), ("slice_index", C.c_int), ("n_slices", C.c_int), ("n_genes", C.c_uint32)]


class SynthResult(C.Structure):
    _fields_ = [("bam", C.c_void_p), ("bam_len", C.c_size_t), ("bai", C.c_void_p), ("bai_len", C.c_size_t),
                ("n_reads", C.c_uint64), ("n_spliced", C.c_uint64), ("n_blocks", C.c_uint64),
                ("inflated_bytes", C.c_uint64), ("cigar_ops", C.c_uint64)]


_synth = None


def synth():
    global _synth
    if _synth is None:
        if not os.path.exists(SYNTH_PATH):
            raise RuntimeError("regtools_amd: %s is missing -- run __graft_entry__.build()" % SYNTH_PATH)
        L = C.CDLL(SYNTH_PATH)
        P = C.POINTER
        L.rgx_synth_generate.argtypes = [P(SynthParams), P(SynthResult)]
        L.rgx_synth_free.argtypes = [P(SynthResult)]
        L.rgx_synth_write.argtypes = [P(SynthParams), C.c_char_p, P(SynthResult)]
        L.rgx_synth_index.argtypes = [C.c_char_p]
        L.rgx_synth_annotation.argtypes = [P(SynthParams), C.c_uint32, C.c_char_p, C.c_char_p, C.c_char_p]
        _synth = L
    return _synth


def format_bed12(table_ptr, only_anchored=True):
    """BED12 text of a table in ONE formatting pass (rgx_table_format_bed12 formats every row even for its size query): a row is its contig's
    name and at most 160 bytes of numbers (Junction::print, junctions_extractor.h:90-98), so n x (longest name + 160) bytes hold it; the exact
    two-call protocol only if that bound were ever short."""
    L = lib()
    t = table_ptr.contents
    longest = max([len(t.ref_name[i]) for i in range(t.n_ref)] or [0])
    cap = int(t.n) * (longest + 160) + 1
    buf = C.create_string_buffer(cap)
    n = L.rgx_table_format_bed12(table_ptr, 1 if only_anchored else 0, buf, cap)
    if n > cap:
        buf = C.create_string_buffer(n + 1)
        L.rgx_table_format_bed12(table_ptr, 1 if only_anchored else 0, buf, n)
    return buf.raw[:n]
