"""ctypes binding of libsrx_hip.so (include/srx.h, include/srx_synth.h).

This is plumbing: it loads the in-tree HIP library and declares its C ABI.  There is no
CPU fallback — if the library is missing, or no GPU is visible when a compute call is made,
the call raises (``SrxError``).
"""
from __future__ import annotations

import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "lib", "libsrx_hip.so")

# srx_status
OK, E_ARG, E_DTYPE, E_FORMAT, E_BOUNDS, E_HIP, E_RCCL, E_OOM, E_NAN, E_SHAPE, E_NOCONV = (
    0, -1, -2, -3, -4, -5, -6, -7, -8, -9, -10)
STATUS_NAMES = {0: "SRX_OK", -1: "SRX_E_ARG", -2: "SRX_E_DTYPE", -3: "SRX_E_FORMAT",
                -4: "SRX_E_BOUNDS", -5: "SRX_E_HIP", -6: "SRX_E_RCCL", -7: "SRX_E_OOM",
                -8: "SRX_E_NAN", -9: "SRX_E_SHAPE", -10: "SRX_E_NOCONV"}
# srx_dtype
I8, I16, I32, U8, U16, U32, F32, F64 = range(8)
ROW, COLUMN = 0, 1
STORE_AUTO, STORE_F32, STORE_F64 = 0, 1, 2
K_NORMALIZE, K_MOMENTS, K_COMPACT, K_SPMM_FWD, K_SPMM_T, K_GRAM, K_DENSE, K_ROWSUM, K_ITERATE, K_SELECT, K_BUCKET = range(11)
K_KNN = 11
K_GRAPH = 12
GRAPH_DISTANCES, GRAPH_CONNECTIVITIES = 0, 1
KNN_MAX_DIMS = 128
SOLVER_AUTO, SOLVER_GRAM, SOLVER_SPMM = 0, 1, 2
UNIQUE_ID_BYTES = 128


class SrxError(RuntimeError):
    def __init__(self, code: int, msg: str):
        super().__init__(f"{STATUS_NAMES.get(code, code)}: {msg}")
        self.code = code
        self.msg = msg


class Csr(C.Structure):
    _fields_ = [("n_rows", C.c_uint64), ("n_cols", C.c_uint64), ("nnz", C.c_uint64),
                ("indptr", C.c_void_p), ("indices", C.c_void_p), ("values", C.c_void_p),
                ("dtype", C.c_int32)]


class MatInfo(C.Structure):
    _fields_ = [("n_rows", C.c_uint64), ("n_cols", C.c_uint64), ("nnz", C.c_uint64),
                ("dtype", C.c_int32), ("store", C.c_int32), ("row_offset", C.c_uint64),
                ("n_rows_global", C.c_uint64)]


class PcaOpts(C.Structure):
    _fields_ = [("n_components", C.c_int32), ("center", C.c_int32), ("scale", C.c_int32),
                ("n_threads", C.c_int32), ("block", C.c_int32), ("max_iter", C.c_int32),
                ("solver", C.c_int32), ("tol", C.c_double), ("seed", C.c_uint64)]


class PcaInfo(C.Structure):
    _fields_ = [("n_cells_global", C.c_uint64), ("k", C.c_uint32), ("n_pc", C.c_uint32),
                ("block", C.c_uint32), ("n_iter", C.c_uint32), ("residual", C.c_double),
                ("nnz_selected", C.c_uint64), ("solver", C.c_uint32), ("reserved_", C.c_uint32)]


class PipelineResult(C.Structure):
    _fields_ = [("pca", PcaInfo), ("ms_normalize", C.c_double), ("ms_moments", C.c_double),
                ("ms_select", C.c_double), ("ms_compact", C.c_double), ("ms_pca", C.c_double)]


class KnnOpts(C.Structure):
    _fields_ = [("k", C.c_int32), ("n_dims", C.c_int32), ("include_self", C.c_int32), ("reserved_", C.c_int32)]


class KnnInfo(C.Structure):
    _fields_ = [("n_ref", C.c_uint64), ("n_query", C.c_uint64), ("d", C.c_uint32), ("k", C.c_uint32),
                ("n_candidates", C.c_uint32), ("reserved_", C.c_uint32), ("rows_certified", C.c_uint64),
                ("rows_recomputed", C.c_uint64)]


class GraphInfo(C.Structure):
    _fields_ = [("n", C.c_uint64), ("k", C.c_uint32), ("reserved_", C.c_uint32), ("nnz_distances", C.c_uint64),
                ("nnz_connectivities", C.c_uint64), ("n_mutual", C.c_uint64), ("rows_no_root", C.c_uint64),
                ("rows_clamped", C.c_uint64), ("rows_all_zero", C.c_uint64), ("entries_dropped", C.c_uint64),
                ("max_row_nnz", C.c_uint64)]


LOUVAIN_MAX_LEVELS = 32


class LouvainOpts(C.Structure):
    _fields_ = [("resolution", C.c_double), ("min_gain", C.c_double), ("max_levels", C.c_int32), ("max_sweeps", C.c_int32)]


class LouvainInfo(C.Structure):
    _fields_ = [("n", C.c_uint64), ("n_communities", C.c_uint64), ("n_levels", C.c_uint32), ("reserved_", C.c_uint32),
                ("sweeps", C.c_uint64), ("moves", C.c_uint64), ("modularity", C.c_double), ("ms", C.c_double),
                ("level_communities", C.c_uint64 * LOUVAIN_MAX_LEVELS), ("level_modularity", C.c_double * LOUVAIN_MAX_LEVELS)]


GROUPS_MAX = 4096
(MARKERS_CNT, MARKERS_SUM, MARKERS_SUMSQ, MARKERS_MEAN, MARKERS_VAR, MARKERS_MEAN_REST, MARKERS_VAR_REST, MARKERS_SCORE,
 MARKERS_LFC, MARKERS_PCT, MARKERS_PCT_REST) = range(11)
MARKERS_RANKSUM2 = 11


class RankGenesOpts(C.Structure):
    _fields_ = [("n_top", C.c_int32), ("logged", C.c_int32)]


class MarkersInfo(C.Structure):
    _fields_ = [("n_rows", C.c_uint64), ("n_cols", C.c_uint64), ("n_groups", C.c_uint32), ("n_top", C.c_uint32),
                ("sum_scale_log2", C.c_int32), ("sq_scale_log2", C.c_int32), ("groups_degenerate", C.c_uint32),
                ("reserved_", C.c_uint32), ("max_abs", C.c_double), ("ms", C.c_double)]


class WilcoxonOpts(C.Structure):
    _fields_ = [("n_top", C.c_int32), ("logged", C.c_int32), ("tie_correct", C.c_int32), ("reserved_", C.c_int32),
                ("scratch_bytes", C.c_uint64)]


class WilcoxonInfo(C.Structure):
    _fields_ = [("tie_correct", C.c_int32), ("n_chunks", C.c_uint32), ("scratch_bytes", C.c_uint64),
                ("segment_limit", C.c_uint64), ("segments_short", C.c_uint64), ("segments_long", C.c_uint64),
                ("ms_stage", C.c_double), ("ms_sort", C.c_double), ("ms_ranks", C.c_double)]


UMAP_GROUP = 8
UMAP_MAX_EPOCHS = 1 << 20
UMAP_INIT_GIVEN, UMAP_INIT_RANDOM, UMAP_INIT_PCA = 0, 1, 2


class UmapOpts(C.Structure):
    _fields_ = [("a", C.c_double), ("b", C.c_double), ("min_dist", C.c_double), ("spread", C.c_double), ("gamma", C.c_double),
                ("alpha0", C.c_double), ("seed", C.c_uint64), ("n_epochs", C.c_int32), ("stop_after", C.c_int32),
                ("n_components", C.c_int32), ("negative_sample_rate", C.c_int32), ("init", C.c_int32), ("reserved_", C.c_int32)]


class UmapInfo(C.Structure):
    _fields_ = [("n", C.c_uint64), ("nnz", C.c_uint64), ("entries_active", C.c_uint64), ("samples", C.c_uint64),
                ("negatives", C.c_uint64), ("negatives_skipped", C.c_uint64), ("n_epochs", C.c_uint32), ("epochs_run", C.c_uint32),
                ("dim", C.c_uint32), ("reserved_", C.c_uint32), ("a", C.c_double), ("b", C.c_double), ("w_max", C.c_double),
                ("ms", C.c_double)]


DIFFMAP_GROUP = 8
DIFFMAP_MAX_COMPS, DIFFMAP_MAX_NCV = 64, 129


class DiffmapOpts(C.Structure):
    _fields_ = [("tol", C.c_double), ("seed", C.c_uint64), ("n_comps", C.c_int32), ("ncv", C.c_int32), ("max_matvecs", C.c_int32),
                ("density_normalize", C.c_int32)]


class DiffmapInfo(C.Structure):
    _fields_ = [("n", C.c_uint64), ("nnz", C.c_uint64), ("n_comps", C.c_uint32), ("ncv", C.c_uint32), ("matvecs", C.c_uint32),
                ("restarts", C.c_uint32), ("breakdowns", C.c_uint32), ("reserved_", C.c_uint32), ("max_residual", C.c_double),
                ("max_ortho", C.c_double), ("ms", C.c_double)]


HARMONY_MAX_CLUSTERS, HARMONY_MAX_BATCHES, HARMONY_MAX_ROUNDS = 256, 256, 64
HARMONY_CORRECTED, HARMONY_R, HARMONY_CENTROIDS, HARMONY_OBSERVED, HARMONY_EXPECTED = range(5)


class HarmonyOpts(C.Structure):
    _fields_ = [("theta", C.c_double), ("sigma", C.c_double), ("lambda_", C.c_double), ("epsilon_cluster", C.c_double),
                ("epsilon_harmony", C.c_double), ("seed", C.c_uint64), ("n_clusters", C.c_int32), ("n_blocks", C.c_int32),
                ("max_rounds", C.c_int32), ("max_cluster_iters", C.c_int32), ("init_iters", C.c_int32), ("n_dims", C.c_int32)]


class HarmonyInfo(C.Structure):
    _fields_ = [("n", C.c_uint64), ("d", C.c_uint32), ("n_batches", C.c_uint32), ("n_clusters", C.c_uint32),
                ("n_blocks", C.c_uint32), ("rounds", C.c_uint32), ("converged", C.c_uint32), ("cluster_iters", C.c_uint64),
                ("round_iters", C.c_uint32 * HARMONY_MAX_ROUNDS), ("round_objective", C.c_double * HARMONY_MAX_ROUNDS),
                ("ms", C.c_double)]


class SynthParams(C.Structure):
    _fields_ = [("seed", C.c_uint64), ("n_rows_global", C.c_uint64), ("n_cols", C.c_uint64),
                ("density", C.c_double), ("lib_sigma", C.c_double), ("type_decay", C.c_double),
                ("n_types", C.c_uint32), ("marker_genes", C.c_uint32), ("expr_boost", C.c_uint32),
                ("value_boost", C.c_uint32), ("skew", C.c_uint32), ("reserved_", C.c_uint32)]


class Flex(C.Structure):            # srx_flex: FlexValue (src/shared/mod.rs:62-66)
    _fields_ = [("kind", C.c_int32), ("absolute", C.c_uint32), ("relative", C.c_double)]


HOST_ALLREDUCE_FN = C.CFUNCTYPE(C.c_int32, C.c_void_p, C.POINTER(C.c_double), C.c_uint64)
FLEX_NONE, FLEX_ABSOLUTE, FLEX_RELATIVE = 0, 1, 2
BACKED_NORMALIZE, BACKED_LOG1P = 1, 2
P = C.c_void_p
_SIGS = {
    # name: (restype, argtypes)
    "srx_abi_version": (C.c_int32, []),
    "srx_device_count": (C.c_int32, [C.POINTER(C.c_int32)]),
    "srx_ctx_create": (C.c_int32, [C.c_int32, C.POINTER(P)]),
    "srx_ctx_destroy": (None, [P]),
    "srx_ctx_synchronize": (C.c_int32, [P]),
    "srx_last_error": (C.c_char_p, [P]),
    "srx_comm_unique_id": (C.c_int32, [P]),
    "srx_comm_init": (C.c_int32, [P, C.c_int32, C.c_int32, P]),
    "srx_comm_init_host": (C.c_int32, [P, C.c_int32, C.c_int32, C.c_void_p, P]),
    "srx_comm_destroy": (C.c_int32, [P]),
    "srx_comm_info": (C.c_int32, [P, C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(C.c_int32)]),
    "srx_comm_overlap_info": (C.c_int32, [P, C.POINTER(C.c_int32), C.POINTER(C.c_int32)]),
    "srx_gram_mode_info": (C.c_int32, [P, C.POINTER(C.c_int32)]),
    "srx_gram_exchange_ranges": (C.c_int32, [C.c_uint64, P]),
    "srx_partition_rows": (C.c_int32, [P, C.c_uint64, C.c_int32, P]),
    "srx_matrix_upload": (C.c_int32, [P, C.POINTER(Csr), C.c_int32, C.POINTER(P)]),
    "srx_matrix_upload_csc": (C.c_int32, [P, C.POINTER(Csr), C.c_int32, C.POINTER(P)]),
    "srx_matrix_format": (C.c_int32, [P, C.POINTER(C.c_int32)]),
    "srx_matrix_to_csr": (C.c_int32, [P, C.POINTER(P)]),
    "srx_matrix_to_csc": (C.c_int32, [P, C.POINTER(P)]),
    "srx_matrix_alloc": (C.c_int32, [P, C.c_uint64, C.c_uint64, C.c_uint64, C.c_int32, C.c_int32, C.POINTER(P)]),
    "srx_matrix_device_ptrs": (C.c_int32, [P, C.POINTER(P), C.POINTER(P), C.POINTER(P)]),
    "srx_matrix_info": (C.c_int32, [P, C.POINTER(MatInfo)]),
    "srx_matrix_set_shard": (C.c_int32, [P, C.c_uint64]),
    "srx_matrix_download_values": (C.c_int32, [P, P, C.c_int32]),
    "srx_matrix_prepare": (C.c_int32, [P]),
    "srx_matrix_reserve_results": (C.c_int32, [P, C.c_uint64, C.c_int32]),
    "srx_matrix_clone": (C.c_int32, [P, C.POINTER(P)]),
    "srx_matrix_copy_values": (C.c_int32, [P, P]),
    "srx_matrix_free": (None, [P]),
    "srx_compute_number": (C.c_int32, [P, C.c_int32, P]),
    "srx_compute_sum": (C.c_int32, [P, C.c_int32, P]),
    "srx_compute_variance": (C.c_int32, [P, C.c_int32, P]),
    "srx_compute_std_dev": (C.c_int32, [P, C.c_int32, P]),
    "srx_compute_min_max": (C.c_int32, [P, C.c_int32, P, P]),
    "srx_compute_qc_variables": (C.c_int32, [P, P, P, P, P, P, P, P, P]),
    "srx_filter_cells": (C.c_int32, [P, Flex, Flex, C.POINTER(C.c_void_p), P]),
    "srx_filter_genes": (C.c_int32, [P, Flex, Flex, C.POINTER(C.c_void_p), P]),
    "srx_subset": (C.c_int32, [P, P, P, C.POINTER(C.c_void_p)]),
    "srx_matrix_download_pattern": (C.c_int32, [P, P, P]),
    "srx_gene_moments": (C.c_int32, [P, P, P, P]),
    "srx_normalize_total_inplace": (C.c_int32, [P, C.c_double, C.c_int32]),
    "srx_log1p_inplace": (C.c_int32, [P]),
    "srx_normalize_log1p_inplace": (C.c_int32, [P, C.c_double, P]),
    "srx_select_hvg": (C.c_int32, [P, C.c_uint64, P, C.POINTER(C.c_uint64)]),
    "srx_pca": (C.c_int32, [P, P, C.c_uint64, C.POINTER(PcaOpts), P, P, P, P, P, C.POINTER(PcaInfo)]),
    "srx_pca_loadings": (C.c_int32, [P, P, P, C.c_uint64, C.c_uint64, C.c_uint64, P]),
    "srx_pca_model_from_result": (C.c_int32, [P, C.POINTER(P)]),
    "srx_pca_model_create": (C.c_int32, [P, C.c_uint64, C.c_uint64, P, P, P, P, C.c_int32, C.c_int32, C.POINTER(P)]),
    "srx_pca_model_info": (C.c_int32, [P, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), P]),
    "srx_pca_model_free": (None, [P]),
    "srx_pca_transform": (C.c_int32, [P, P, P, C.c_double, C.c_int32, P]),
    "srx_knn_result": (C.c_int32, [P, C.POINTER(KnnOpts), P, P, C.POINTER(KnnInfo)]),
    "srx_knn_points": (C.c_int32, [P, P, C.c_uint64, P, C.c_uint64, C.c_uint64, C.POINTER(KnnOpts), P, P, C.POINTER(KnnInfo)]),
    "srx_neighbors_result": (C.c_int32, [P, C.POINTER(KnnOpts), C.POINTER(KnnInfo), C.POINTER(P)]),
    "srx_neighbors_from_knn": (C.c_int32, [P, P, P, C.c_uint64, C.c_uint32, C.POINTER(P)]),
    "srx_graph_info_get": (C.c_int32, [P, C.POINTER(GraphInfo)]),
    "srx_graph_fetch": (C.c_int32, [P, C.c_int32, P, P, P]),
    "srx_graph_fetch_scales": (C.c_int32, [P, P, P]),
    "srx_graph_free": (None, [P]),
    "srx_louvain": (C.c_int32, [P, C.POINTER(LouvainOpts), P, C.POINTER(LouvainInfo)]),
    "srx_louvain_csr": (C.c_int32, [P, P, P, P, C.c_uint64, C.POINTER(LouvainOpts), P, C.POINTER(LouvainInfo)]),
    "srx_graph_labels_fetch": (C.c_int32, [P, P]),
    "srx_group_moments": (C.c_int32, [P, P, C.c_uint32, P, P, P, P]),
    "srx_rank_genes_groups": (C.c_int32, [P, P, C.c_uint32, C.POINTER(RankGenesOpts), C.POINTER(P)]),
    "srx_rank_genes_groups_graph": (C.c_int32, [P, P, C.POINTER(RankGenesOpts), C.POINTER(P)]),
    "srx_markers_info_get": (C.c_int32, [P, C.POINTER(MarkersInfo)]),
    "srx_markers_fetch_top": (C.c_int32, [P, P, P, P]),
    "srx_markers_fetch_table": (C.c_int32, [P, C.c_int32, P]),
    "srx_markers_fetch_sizes": (C.c_int32, [P, P]),
    "srx_markers_free": (None, [P]),
    "srx_rank_genes_wilcoxon": (C.c_int32, [P, P, C.c_uint32, C.POINTER(WilcoxonOpts), C.POINTER(P)]),
    "srx_rank_genes_wilcoxon_graph": (C.c_int32, [P, P, C.POINTER(WilcoxonOpts), C.POINTER(P)]),
    "srx_markers_fetch_ties": (C.c_int32, [P, P]),
    "srx_markers_wilcoxon_info_get": (C.c_int32, [P, C.POINTER(WilcoxonInfo)]),
    "srx_umap": (C.c_int32, [P, P, C.POINTER(UmapOpts), P, P, C.POINTER(UmapInfo)]),
    "srx_umap_csr": (C.c_int32, [P, P, P, P, C.c_uint64, C.POINTER(UmapOpts), P, P, C.POINTER(UmapInfo)]),
    "srx_graph_embedding_fetch": (C.c_int32, [P, P, C.POINTER(C.c_uint32)]),
    "srx_umap_fit_ab": (C.c_int32, [C.c_double, C.c_double, C.POINTER(C.c_double), C.POINTER(C.c_double)]),
    "srx_diffmap": (C.c_int32, [P, C.POINTER(DiffmapOpts), P, P, C.POINTER(DiffmapInfo)]),
    "srx_diffmap_csr": (C.c_int32, [P, P, P, P, C.c_uint64, C.POINTER(DiffmapOpts), P, P, C.POINTER(DiffmapInfo)]),
    "srx_graph_diffmap_fetch": (C.c_int32, [P, P, P, C.POINTER(C.c_uint32)]),
    "srx_graph_transitions_fetch": (C.c_int32, [P, P]),
    "srx_dpt": (C.c_int32, [P, C.c_uint64, C.c_double, P]),
    "srx_dpt_from": (C.c_int32, [P, P, P, C.c_uint64, C.c_uint32, C.c_uint64, C.c_double, P]),
    "srx_harmony_result": (C.c_int32, [P, P, C.c_uint32, C.POINTER(HarmonyOpts), C.POINTER(P), C.POINTER(HarmonyInfo)]),
    "srx_harmony_points": (C.c_int32, [P, P, C.c_uint64, C.c_uint64, P, C.c_uint32, C.POINTER(HarmonyOpts), C.POINTER(P),
                                       C.POINTER(HarmonyInfo)]),
    "srx_harmony_fetch": (C.c_int32, [P, C.c_int32, P]),
    "srx_harmony_info_get": (C.c_int32, [P, C.POINTER(HarmonyInfo)]),
    "srx_knn_harmony": (C.c_int32, [P, C.POINTER(KnnOpts), P, P, C.POINTER(KnnInfo)]),
    "srx_neighbors_harmony": (C.c_int32, [P, C.POINTER(KnnOpts), C.POINTER(KnnInfo), C.POINTER(P)]),
    "srx_harmony_free": (None, [P]),
    "srx_spmm": (C.c_int32, [P, P, C.c_uint64, P, P, P, P]),
    "srx_pipeline": (C.c_int32, [P, C.c_double, C.c_uint64, C.POINTER(PcaOpts), C.POINTER(PipelineResult)]),
    "srx_result_fetch": (C.c_int32, [P, P, P, P, P, P, P]),
    "srx_backed_create": (C.c_int32, [P, C.c_uint64, C.c_int32, C.POINTER(P)]),
    "srx_backed_destroy": (None, [P]),
    "srx_backed_stats_tile": (C.c_int32, [P, C.POINTER(Csr), C.c_double, C.c_int32, P, P]),
    "srx_backed_moments": (C.c_int32, [P, P, P, P, C.POINTER(C.c_uint64)]),
    "srx_backed_select": (C.c_int32, [P, C.c_uint64, P, C.c_uint64, C.POINTER(PcaOpts), P, C.POINTER(C.c_uint64)]),
    "srx_backed_gram_tile": (C.c_int32, [P, C.POINTER(Csr), C.c_double, C.c_int32]),
    "srx_backed_solve": (C.c_int32, [P, C.POINTER(PcaInfo)]),
    "srx_backed_fetch": (C.c_int32, [P, P, P, P, P, P, P]),
    "srx_prof_enable": (C.c_int32, [P, C.c_uint32]),
    "srx_prof_reset": (C.c_int32, [P]),
    "srx_prof_get": (C.c_int32, [P, C.c_int32, C.POINTER(C.c_double), C.POINTER(C.c_uint64), C.POINTER(C.c_double)]),
    "srx_prof_get_aux": (C.c_int32, [P, C.c_int32, C.POINTER(C.c_double)]),
    # srx_synth.h
    "srx_synth_defaults": (None, [C.POINTER(SynthParams), C.c_uint64, C.c_uint64, C.c_uint64, C.c_double]),
    "srx_synth_indptr": (C.c_int32, [C.POINTER(SynthParams), C.c_uint64, C.c_uint64, P]),
    "srx_synth_fill_host": (C.c_int32, [C.POINTER(SynthParams), C.c_uint64, C.c_uint64, P, P, P]),
    "srx_synth_generate": (C.c_int32, [P, C.POINTER(SynthParams), C.c_uint64, C.c_uint64, C.c_int32, C.c_int32, C.POINTER(P)]),
}
EXPORTS = tuple(_SIGS)

_lib = None


def lib() -> C.CDLL:
    """Load libsrx_hip.so (built in-tree by singlerust_amd.build / __graft_entry__.build)."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise SrxError(E_HIP, f"{LIB_PATH} is missing: run `python -m singlerust_amd.build` "
                                  "(hipcc --offload-arch=gfx950); there is no CPU fallback")
        l = C.CDLL(LIB_PATH)
        for name, (res, args) in _SIGS.items():
            fn = getattr(l, name)
            fn.restype = res
            fn.argtypes = args
        _lib = l
    return _lib


def check(rc: int, ctx=None) -> None:
    if rc != OK:
        msg = lib().srx_last_error(ctx)
        raise SrxError(rc, msg.decode() if msg else "")


def ptr(a):
    """void* of a numpy array (or None)."""
    return None if a is None else C.c_void_p(a.ctypes.data)
