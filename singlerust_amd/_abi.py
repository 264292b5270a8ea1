"""singlerust_amd/_abi.py — GENERATED from include/srx.h and include/srx_synth.h by scripts/gen_ctypes_bindings.py;
do not edit.  The ctypes description of libsrx_hip.so's C ABI: constants, structures, the signature of every function.
To change it, edit the header and run the generator (and scripts/gen_rust_bindings.py).  singlerust_amd/_ffi.py loads
the library and applies SIGNATURES."""
import ctypes as C

P = C.c_void_p

ABI_VERSION = 6
UNIQUE_ID_BYTES = 128
GENE_LISTS_MAX = 4096
KNN_MAX_DIMS = 128
LOUVAIN_MAX_LEVELS = 32
GROUPS_MAX = 4096
UMAP_GROUP = 8
UMAP_MAX_EPOCHS = 1048576
UMAP_TRANSFORM_CHUNK = 64
TSNE_MAX_K = 64
TSNE_MAX_LEVELS = 12
TSNE_GROUP = 8
TSNE_MAX_ITERS = 1048576
FA2_GROUP = 8
FA2_MAX_ITERS = 1048576
DIFFMAP_GROUP = 8
DIFFMAP_MAX_COMPS = 64
DIFFMAP_MAX_NCV = 129
HARMONY_MAX_CLUSTERS = 256
HARMONY_MAX_BATCHES = 256
HARMONY_MAX_ROUNDS = 64
DOUBLET_MAX_K = 64
DOUBLET_MAX_ROUNDS = 10000
DOUBLET_WAVE_ROW = 8192
IT_ALIAS_B = 1
IT_ZERO_WP = 1
IT_Z0 = 1
IT_Z0_IS_SRC = 8
IT_SRC_IS_W = 16
SEL_NO_VECTORS = 1
SEL_COUNTER_UNUSED = 2147483646
SYNTH_MAX_TYPES = 128
OK = 0
E_ARG = -1
E_DTYPE = -2
E_FORMAT = -3
E_BOUNDS = -4
E_HIP = -5
E_RCCL = -6
E_OOM = -7
E_NAN = -8
E_SHAPE = -9
E_NOCONV = -10
I8 = 0
I16 = 1
I32 = 2
U8 = 3
U16 = 4
U32 = 5
F32 = 6
F64 = 7
ROW = 0
COLUMN = 1
STORE_AUTO = 0
STORE_F32 = 1
STORE_F64 = 2
FORMAT_CSR = 0
FORMAT_CSC = 1
FLEX_NONE = 0
FLEX_ABSOLUTE = 1
FLEX_RELATIVE = 2
SOLVER_AUTO = 0
SOLVER_GRAM = 1
SOLVER_SPMM = 2
PEARSON_TOTALS_ALL = 0
PEARSON_TOTALS_SELECTED = 1
GRAPH_DISTANCES = 0
GRAPH_CONNECTIVITIES = 1
SNN_JACCARD = 0
SNN_NUMBER = 1
SNN_PAIRS_SHARED = 0
SNN_PAIRS_KNN = 1
MARKERS_CNT = 0
MARKERS_SUM = 1
MARKERS_SUMSQ = 2
MARKERS_MEAN = 3
MARKERS_VAR = 4
MARKERS_MEAN_REST = 5
MARKERS_VAR_REST = 6
MARKERS_SCORE = 7
MARKERS_LFC = 8
MARKERS_PCT = 9
MARKERS_PCT_REST = 10
MARKERS_RANKSUM2 = 11
UMAP_INIT_GIVEN = 0
UMAP_INIT_RANDOM = 1
UMAP_INIT_PCA = 2
TSNE_INIT_GIVEN = 0
TSNE_INIT_RANDOM = 1
TSNE_INIT_PCA = 2
FA2_INIT_GIVEN = 0
FA2_INIT_RANDOM = 1
HARMONY_CORRECTED = 0
HARMONY_R = 1
HARMONY_CENTROIDS = 2
HARMONY_OBSERVED = 3
HARMONY_EXPECTED = 4
DOUBLETS_SCORES_OBS = 0
DOUBLETS_SCORES_SIM = 1
DOUBLETS_SE_OBS = 2
DOUBLETS_SE_SIM = 3
DOUBLETS_Z = 4
DOUBLETS_PREDICTED = 5
DOUBLETS_POINTS = 6
DOUBLETS_PARENTS = 7
DOUBLETS_KNN = 8
IT_APPLY = 0
IT_GRAM1 = 1
IT_GRAM2 = 2
IT_CHOL = 3
IT_TRSM = 4
IT_EIG = 5
IT_RITZ = 6
IT_CHEB = 7
SEL_HVG = 0
SEL_LIST = 1
BACKED_NORMALIZE = 1
BACKED_LOG1P = 2
K_NORMALIZE = 0
K_MOMENTS = 1
K_COMPACT = 2
K_SPMM_FWD = 3
K_SPMM_T = 4
K_GRAM = 5
K_DENSE = 6
K_ROWSUM = 7
K_ITERATE = 8
K_SELECT = 9
K_BUCKET = 10
K_KNN = 11
K_GRAPH = 12
K_COUNT_ = 13

STATUS_NAMES = {0: "SRX_OK", -1: "SRX_E_ARG", -2: "SRX_E_DTYPE", -3: "SRX_E_FORMAT", -4: "SRX_E_BOUNDS",
                -5: "SRX_E_HIP", -6: "SRX_E_RCCL", -7: "SRX_E_OOM", -8: "SRX_E_NAN", -9: "SRX_E_SHAPE",
                -10: "SRX_E_NOCONV"}


class Csr(C.Structure):      # srx_csr
    _fields_ = [("n_rows", C.c_uint64), ("n_cols", C.c_uint64), ("nnz", C.c_uint64), ("indptr", P), ("indices", P),
                ("values", P), ("dtype", C.c_int32)]


class MatInfo(C.Structure):      # srx_mat_info
    _fields_ = [("n_rows", C.c_uint64), ("n_cols", C.c_uint64), ("nnz", C.c_uint64), ("dtype", C.c_int32),
                ("store", C.c_int32), ("row_offset", C.c_uint64), ("n_rows_global", C.c_uint64)]


class Flex(C.Structure):      # srx_flex
    _fields_ = [("kind", C.c_int32), ("absolute", C.c_uint32), ("relative", C.c_double)]


class PearsonOpts(C.Structure):      # srx_pearson_opts
    _fields_ = [("theta", C.c_double), ("clip", C.c_double)]


class PearsonInfo(C.Structure):      # srx_pearson_info
    _fields_ = [("n_cells", C.c_uint64), ("n_genes", C.c_uint64), ("n_expressed", C.c_uint64),
                ("n_empty_cells", C.c_uint64), ("total", C.c_double), ("theta", C.c_double), ("clip", C.c_double),
                ("sum_quantum", C.c_double), ("sq_quantum", C.c_double), ("ms_dense", C.c_double),
                ("ms_sparse", C.c_double), ("ms_rank", C.c_double)]


class PcaOpts(C.Structure):      # srx_pca_opts
    _fields_ = [("n_components", C.c_int32), ("center", C.c_int32), ("scale", C.c_int32), ("n_threads", C.c_int32),
                ("block", C.c_int32), ("max_iter", C.c_int32), ("solver", C.c_int32), ("tol", C.c_double),
                ("seed", C.c_uint64)]


class PcaInfo(C.Structure):      # srx_pca_info
    _fields_ = [("n_cells_global", C.c_uint64), ("k", C.c_uint32), ("n_pc", C.c_uint32), ("block", C.c_uint32),
                ("n_iter", C.c_uint32), ("residual", C.c_double), ("nnz_selected", C.c_uint64),
                ("solver", C.c_uint32), ("reserved_", C.c_uint32)]


class PearsonPcaOpts(C.Structure):      # srx_pearson_pca_opts
    _fields_ = [("pearson", PearsonOpts), ("totals", C.c_int32), ("center", C.c_int32), ("chunk_cells", C.c_uint64),
                ("pca", PcaOpts)]


class PearsonPcaInfo(C.Structure):      # srx_pearson_pca_info
    _fields_ = [("n_cells", C.c_uint64), ("n_genes", C.c_uint64), ("n_expressed", C.c_uint64),
                ("n_empty_cells", C.c_uint64), ("total", C.c_double), ("theta", C.c_double), ("clip", C.c_double),
                ("pca", PcaInfo), ("ms_gram", C.c_double), ("ms_solve", C.c_double), ("ms_scores", C.c_double),
                ("n_chunks", C.c_uint64), ("chunk_cells", C.c_uint64), ("chunk_bytes", C.c_uint64)]


class RegressOpts(C.Structure):      # srx_regress_opts
    _fields_ = [("scale", C.c_int32), ("reserved", C.c_int32), ("max_value", C.c_double), ("chunk_cells", C.c_uint64),
                ("pca", PcaOpts)]


class RegressInfo(C.Structure):      # srx_regress_info
    _fields_ = [("n_cells", C.c_uint64), ("n_genes", C.c_uint64), ("n_cov", C.c_uint64),
                ("n_constant_genes", C.c_uint64), ("n_clipped", C.c_uint64), ("min_pivot", C.c_double),
                ("ms_fit", C.c_double), ("ms_scale", C.c_double), ("ms_gram", C.c_double), ("ms_solve", C.c_double),
                ("ms_scores", C.c_double), ("n_chunks", C.c_uint64), ("chunk_cells", C.c_uint64),
                ("chunk_bytes", C.c_uint64), ("pca", PcaInfo)]


class GeneListInfo(C.Structure):      # srx_gene_list_info
    _fields_ = [("n_rows", C.c_uint64), ("n_cols", C.c_uint64), ("n_lists", C.c_uint64), ("longest_list", C.c_uint64),
                ("sum_scale_log2", C.c_int32), ("n_walks", C.c_uint32), ("max_abs", C.c_double),
                ("ms_scan", C.c_double), ("ms_walk", C.c_double)]


class ScoreGenesOpts(C.Structure):      # srx_score_genes_opts
    _fields_ = [("ctrl_size", C.c_uint32), ("n_bins", C.c_uint32), ("seed", C.c_uint64), ("ctrl_as_ref", C.c_int32),
                ("reserved", C.c_int32)]


class ScoreGenesInfo(C.Structure):      # srx_score_genes_info
    _fields_ = [("n_rows", C.c_uint64), ("n_cols", C.c_uint64), ("n_sets", C.c_uint64), ("n_pool", C.c_uint64),
                ("n_ctrl_total", C.c_uint64), ("n_items", C.c_uint64), ("longest_list", C.c_uint64),
                ("sum_scale_log2", C.c_int32), ("n_walks", C.c_uint32), ("max_abs", C.c_double),
                ("ms_mean", C.c_double), ("ms_ctrl", C.c_double), ("ms_walk", C.c_double)]


class KnnOpts(C.Structure):      # srx_knn_opts
    _fields_ = [("k", C.c_int32), ("n_dims", C.c_int32), ("include_self", C.c_int32), ("reserved_", C.c_int32)]


class KnnInfo(C.Structure):      # srx_knn_info
    _fields_ = [("n_ref", C.c_uint64), ("n_query", C.c_uint64), ("d", C.c_uint32), ("k", C.c_uint32),
                ("n_candidates", C.c_uint32), ("reserved_", C.c_uint32), ("rows_certified", C.c_uint64),
                ("rows_recomputed", C.c_uint64)]


class GraphInfo(C.Structure):      # srx_graph_info
    _fields_ = [("n", C.c_uint64), ("k", C.c_uint32), ("reserved_", C.c_uint32), ("nnz_distances", C.c_uint64),
                ("nnz_connectivities", C.c_uint64), ("n_mutual", C.c_uint64), ("rows_no_root", C.c_uint64),
                ("rows_clamped", C.c_uint64), ("rows_all_zero", C.c_uint64), ("entries_dropped", C.c_uint64),
                ("max_row_nnz", C.c_uint64)]


class SnnOpts(C.Structure):      # srx_snn_opts
    _fields_ = [("weight", C.c_int32), ("pairs", C.c_int32), ("include_self", C.c_int32), ("reserved_", C.c_int32),
                ("prune", C.c_double)]


class SnnInfo(C.Structure):      # srx_snn_info
    _fields_ = [("n", C.c_uint64), ("k", C.c_uint32), ("set_size", C.c_uint32), ("min_shared", C.c_uint32),
                ("max_shared", C.c_uint32), ("pairs_considered", C.c_uint64), ("pairs_kept", C.c_uint64),
                ("nnz", C.c_uint64), ("max_row_nnz", C.c_uint64), ("max_in_degree", C.c_uint64),
                ("max_candidates", C.c_uint64), ("sum_candidates", C.c_uint64), ("wave_capacity", C.c_uint32),
                ("short_capacity", C.c_uint32), ("rows_wave", C.c_uint64), ("rows_long", C.c_uint64),
                ("rows_empty", C.c_uint64), ("ms", C.c_double), ("ms_lists", C.c_double), ("ms_count", C.c_double),
                ("ms_fill", C.c_double)]


class IvfOpts(C.Structure):      # srx_ivf_opts
    _fields_ = [("n_lists", C.c_int32), ("train_iters", C.c_int32), ("seed", C.c_uint64),
                ("max_train_points", C.c_uint64)]


class IvfInfo(C.Structure):      # srx_ivf_info
    _fields_ = [("n_ref", C.c_uint64), ("n_train", C.c_uint64), ("d", C.c_uint32), ("n_lists", C.c_uint32),
                ("train_iters", C.c_uint32), ("reserved_", C.c_uint32), ("min_list", C.c_uint64),
                ("max_list", C.c_uint64), ("empty_lists", C.c_uint64), ("inertia", C.c_double),
                ("ms_train", C.c_double), ("ms_assign", C.c_double)]


class IvfSearchInfo(C.Structure):      # srx_ivf_search_info
    _fields_ = [("n_query", C.c_uint64), ("k", C.c_uint32), ("n_probe", C.c_uint32), ("n_candidates", C.c_uint32),
                ("reserved_", C.c_uint32), ("rows_certified", C.c_uint64), ("rows_rescanned", C.c_uint64),
                ("rows_exhaustive", C.c_uint64), ("pairs", C.c_uint64), ("points_scanned", C.c_uint64)]


class LouvainOpts(C.Structure):      # srx_louvain_opts
    _fields_ = [("resolution", C.c_double), ("min_gain", C.c_double), ("max_levels", C.c_int32),
                ("max_sweeps", C.c_int32)]


class LouvainInfo(C.Structure):      # srx_louvain_info
    _fields_ = [("n", C.c_uint64), ("n_communities", C.c_uint64), ("n_levels", C.c_uint32), ("reserved_", C.c_uint32),
                ("sweeps", C.c_uint64), ("moves", C.c_uint64), ("modularity", C.c_double), ("ms", C.c_double),
                ("level_communities", C.c_uint64 * 32), ("level_modularity", C.c_double * 32)]


class RankGenesOpts(C.Structure):      # srx_rank_genes_opts
    _fields_ = [("n_top", C.c_int32), ("logged", C.c_int32)]


class MarkersInfo(C.Structure):      # srx_markers_info
    _fields_ = [("n_rows", C.c_uint64), ("n_cols", C.c_uint64), ("n_groups", C.c_uint32), ("n_top", C.c_uint32),
                ("sum_scale_log2", C.c_int32), ("sq_scale_log2", C.c_int32), ("groups_degenerate", C.c_uint32),
                ("reserved_", C.c_uint32), ("max_abs", C.c_double), ("ms", C.c_double)]


class WilcoxonOpts(C.Structure):      # srx_wilcoxon_opts
    _fields_ = [("n_top", C.c_int32), ("logged", C.c_int32), ("tie_correct", C.c_int32), ("reserved_", C.c_int32),
                ("scratch_bytes", C.c_uint64)]


class WilcoxonInfo(C.Structure):      # srx_wilcoxon_info
    _fields_ = [("tie_correct", C.c_int32), ("n_chunks", C.c_uint32), ("scratch_bytes", C.c_uint64),
                ("segment_limit", C.c_uint64), ("segments_short", C.c_uint64), ("segments_long", C.c_uint64),
                ("ms_stage", C.c_double), ("ms_sort", C.c_double), ("ms_ranks", C.c_double)]


class SeuratV3Opts(C.Structure):      # srx_seurat_v3_opts
    _fields_ = [("span", C.c_double), ("paper_order", C.c_int32), ("reserved_", C.c_int32)]


class SeuratV3Tables(C.Structure):      # srx_seurat_v3_tables
    _fields_ = [("means", P), ("variances", P), ("variances_norm", P), ("median", P), ("nbatches", P), ("mean", P),
                ("var", P), ("fitted", P), ("reg_var", P), ("clip", P), ("clip_sum", P), ("clip_sumsq", P), ("nv", P),
                ("rank", P)]


class SeuratV3Info(C.Structure):      # srx_seurat_v3_info
    _fields_ = [("n_cells", C.c_uint64), ("n_genes", C.c_uint64), ("n_batches", C.c_uint32),
                ("sum_scale_log2", C.c_int32), ("sq_scale_log2", C.c_int32), ("reserved_", C.c_uint32),
                ("max_abs", C.c_double), ("min_batch_cells", C.c_uint64), ("span", C.c_double),
                ("ms_moments", C.c_double), ("ms_loess", C.c_double), ("ms_clip", C.c_double), ("ms_rank", C.c_double)]


class UmapOpts(C.Structure):      # srx_umap_opts
    _fields_ = [("a", C.c_double), ("b", C.c_double), ("min_dist", C.c_double), ("spread", C.c_double),
                ("gamma", C.c_double), ("alpha0", C.c_double), ("seed", C.c_uint64), ("n_epochs", C.c_int32),
                ("stop_after", C.c_int32), ("n_components", C.c_int32), ("negative_sample_rate", C.c_int32),
                ("init", C.c_int32), ("reserved_", C.c_int32)]


class UmapInfo(C.Structure):      # srx_umap_info
    _fields_ = [("n", C.c_uint64), ("nnz", C.c_uint64), ("entries_active", C.c_uint64), ("samples", C.c_uint64),
                ("negatives", C.c_uint64), ("negatives_skipped", C.c_uint64), ("n_epochs", C.c_uint32),
                ("epochs_run", C.c_uint32), ("dim", C.c_uint32), ("reserved_", C.c_uint32), ("a", C.c_double),
                ("b", C.c_double), ("w_max", C.c_double), ("ms", C.c_double)]


class UmapTransformOpts(C.Structure):      # srx_umap_transform_opts
    _fields_ = [("a", C.c_double), ("b", C.c_double), ("min_dist", C.c_double), ("spread", C.c_double),
                ("gamma", C.c_double), ("alpha0", C.c_double), ("seed", C.c_uint64), ("n_epochs", C.c_int32),
                ("stop_after", C.c_int32), ("negative_sample_rate", C.c_int32), ("chunk_epochs", C.c_int32)]


class UmapTransformOut(C.Structure):      # srx_umap_transform_out
    _fields_ = [("embedding", P), ("start", P), ("weights", P), ("columns", P), ("sigma", P)]


class UmapTransformInfo(C.Structure):      # srx_umap_transform_info
    _fields_ = [("n_query", C.c_uint64), ("n_ref", C.c_uint64), ("entries_active", C.c_uint64),
                ("samples", C.c_uint64), ("negatives", C.c_uint64), ("rows_no_root", C.c_uint64),
                ("rows_clamped", C.c_uint64), ("rows_all_zero", C.c_uint64), ("rows_start_nearest", C.c_uint64),
                ("kq", C.c_uint32), ("dim", C.c_uint32), ("n_epochs", C.c_uint32), ("epochs_run", C.c_uint32),
                ("a", C.c_double), ("b", C.c_double), ("w_max", C.c_double), ("ms", C.c_double),
                ("membership_ms", C.c_double)]


class TsneInfo(C.Structure):      # srx_tsne_info
    _fields_ = [("n", C.c_uint64), ("nnz", C.c_uint64), ("n_mutual", C.c_uint64), ("rows_no_root", C.c_uint64),
                ("entries_dropped", C.c_uint64), ("k", C.c_uint32), ("reserved_", C.c_uint32),
                ("perplexity", C.c_double)]


class TsneOpts(C.Structure):      # srx_tsne_opts
    _fields_ = [("theta", C.c_double), ("exaggeration", C.c_double), ("learning_rate", C.c_double),
                ("seed", C.c_uint64), ("n_iter", C.c_int32), ("exaggeration_iters", C.c_int32),
                ("stop_after", C.c_int32), ("levels", C.c_int32), ("init", C.c_int32), ("reserved_", C.c_int32)]


class TsneRunInfo(C.Structure):      # srx_tsne_run_info
    _fields_ = [("n", C.c_uint64), ("nnz", C.c_uint64), ("n_iter", C.c_uint32), ("iters_run", C.c_uint32),
                ("levels", C.c_uint32), ("reserved_", C.c_uint32), ("eta", C.c_double), ("Z", C.c_double),
                ("kl", C.c_double), ("side", C.c_double), ("cells_accepted", C.c_uint64), ("cells_exact", C.c_uint64),
                ("pairs_exact", C.c_uint64), ("ms", C.c_double)]


class TsneForceInfo(C.Structure):      # srx_tsne_force_info
    _fields_ = [("levels", C.c_uint32), ("reserved_", C.c_uint32), ("side", C.c_double), ("lo", C.c_double * 2),
                ("cells_accepted", C.c_uint64), ("cells_exact", C.c_uint64), ("pairs_exact", C.c_uint64)]


class Fa2Opts(C.Structure):      # srx_fa2_opts
    _fields_ = [("theta", C.c_double), ("scaling_ratio", C.c_double), ("gravity", C.c_double),
                ("jitter_tolerance", C.c_double), ("seed", C.c_uint64), ("n_iter", C.c_int32),
                ("stop_after", C.c_int32), ("levels", C.c_int32), ("init", C.c_int32), ("strong_gravity", C.c_int32),
                ("linlog", C.c_int32)]


class Fa2Info(C.Structure):      # srx_fa2_info
    _fields_ = [("n", C.c_uint64), ("nnz", C.c_uint64), ("total_mass", C.c_uint64), ("n_iter", C.c_uint32),
                ("iters_run", C.c_uint32), ("levels", C.c_uint32), ("reserved_", C.c_uint32), ("speed", C.c_double),
                ("speed_efficiency", C.c_double), ("swing", C.c_double), ("traction", C.c_double),
                ("side", C.c_double), ("cells_accepted", C.c_uint64), ("cells_exact", C.c_uint64),
                ("pairs_exact", C.c_uint64), ("pairs_coincident", C.c_uint64), ("ms", C.c_double)]


class Fa2ForceInfo(C.Structure):      # srx_fa2_force_info
    _fields_ = [("levels", C.c_uint32), ("reserved_", C.c_uint32), ("side", C.c_double), ("lo", C.c_double * 2),
                ("total_mass", C.c_uint64), ("cells_accepted", C.c_uint64), ("cells_exact", C.c_uint64),
                ("pairs_exact", C.c_uint64), ("pairs_coincident", C.c_uint64)]


class DiffmapOpts(C.Structure):      # srx_diffmap_opts
    _fields_ = [("tol", C.c_double), ("seed", C.c_uint64), ("n_comps", C.c_int32), ("ncv", C.c_int32),
                ("max_matvecs", C.c_int32), ("density_normalize", C.c_int32)]


class DiffmapInfo(C.Structure):      # srx_diffmap_info
    _fields_ = [("n", C.c_uint64), ("nnz", C.c_uint64), ("n_comps", C.c_uint32), ("ncv", C.c_uint32),
                ("matvecs", C.c_uint32), ("restarts", C.c_uint32), ("breakdowns", C.c_uint32),
                ("reserved_", C.c_uint32), ("max_residual", C.c_double), ("max_ortho", C.c_double), ("ms", C.c_double)]


class PagaInfo(C.Structure):      # srx_paga_info
    _fields_ = [("n", C.c_uint64), ("nnz", C.c_uint64), ("n_groups", C.c_uint32), ("groups_empty", C.c_uint32),
                ("edges_inner", C.c_uint64), ("edges_inter", C.c_uint64), ("pairs_connected", C.c_uint64),
                ("pairs_clipped", C.c_uint64), ("tree_edges", C.c_uint32), ("components", C.c_uint32),
                ("ms", C.c_double)]


class PagaTables(C.Structure):      # srx_paga_tables
    _fields_ = [("sizes", P), ("out_edges", P), ("counts", P), ("connectivities", P), ("expected", P), ("tree", P)]


class AutocorrOpts(C.Structure):      # srx_autocorr_opts
    _fields_ = [("rows_per_block", C.c_uint32), ("reserved_", C.c_uint32)]


class AutocorrOut(C.Structure):      # srx_autocorr_out
    _fields_ = [("morans_i", P), ("gearys_c", P), ("z_i", P), ("z_c", P), ("sum", P), ("sumsq", P), ("dsum", P),
                ("dsumsq", P), ("cross", P), ("sum_int", P), ("sumsq_int", P), ("dsum_int", P), ("dsumsq_int", P),
                ("cross_int", P)]


class AutocorrInfo(C.Structure):      # srx_autocorr_info
    _fields_ = [("n", C.c_uint64), ("n_genes", C.c_uint64), ("nnz", C.c_uint64), ("s_sum", C.c_int32),
                ("s_sumsq", C.c_int32), ("s_dsum", C.c_int32), ("s_dsumsq", C.c_int32), ("s_cross", C.c_int32),
                ("s_w", C.c_int32), ("s_1", C.c_int32), ("s_2", C.c_int32), ("max_abs", C.c_double),
                ("max_weight", C.c_double), ("max_degree", C.c_double), ("w_int", C.c_int64), ("s1_int", C.c_int64),
                ("s2_int", C.c_int64), ("w", C.c_double), ("s1", C.c_double), ("s2", C.c_double), ("e_i", C.c_double),
                ("var_i", C.c_double), ("e_c", C.c_double), ("var_c", C.c_double), ("genes_constant", C.c_uint64),
                ("ms", C.c_double), ("ms_graph", C.c_double), ("ms_moments", C.c_double), ("ms_walk", C.c_double),
                ("ms_wmax", C.c_double), ("ms_degrees", C.c_double), ("ms_s2", C.c_double),
                ("ms_sum_sumsq", C.c_double), ("ms_dsum_dsumsq", C.c_double)]


class HarmonyOpts(C.Structure):      # srx_harmony_opts
    _fields_ = [("theta", C.c_double), ("sigma", C.c_double), ("lambda_", C.c_double),
                ("epsilon_cluster", C.c_double), ("epsilon_harmony", C.c_double), ("seed", C.c_uint64),
                ("n_clusters", C.c_int32), ("n_blocks", C.c_int32), ("max_rounds", C.c_int32),
                ("max_cluster_iters", C.c_int32), ("init_iters", C.c_int32), ("n_dims", C.c_int32)]


class HarmonyInfo(C.Structure):      # srx_harmony_info
    _fields_ = [("n", C.c_uint64), ("d", C.c_uint32), ("n_batches", C.c_uint32), ("n_clusters", C.c_uint32),
                ("n_blocks", C.c_uint32), ("rounds", C.c_uint32), ("converged", C.c_uint32),
                ("cluster_iters", C.c_uint64), ("round_iters", C.c_uint32 * 64), ("round_objective", C.c_double * 64),
                ("ms", C.c_double)]


class BbknnOpts(C.Structure):      # srx_bbknn_opts
    _fields_ = [("neighbors_within_batch", C.c_int32), ("n_dims", C.c_int32), ("trim", C.c_int64)]


class TrimInfo(C.Structure):      # srx_trim_info
    _fields_ = [("trim", C.c_uint64), ("rows_over_trim", C.c_uint64), ("nnz_before", C.c_uint64),
                ("nnz_after", C.c_uint64), ("entries_trimmed", C.c_uint64), ("max_row_nnz_before", C.c_uint64),
                ("max_row_nnz_after", C.c_uint64), ("rows_emptied", C.c_uint64), ("wave_capacity", C.c_uint32),
                ("short_capacity", C.c_uint32), ("reserved_", C.c_uint32 * 2), ("rows_wave", C.c_uint64),
                ("rows_short", C.c_uint64), ("rows_long", C.c_uint64)]


class BbknnInfo(C.Structure):      # srx_bbknn_info
    _fields_ = [("n", C.c_uint64), ("n_batches", C.c_uint32), ("neighbors_within_batch", C.c_uint32),
                ("k", C.c_uint32), ("d", C.c_uint32), ("min_batch_cells", C.c_uint64),
                ("max_batch_cells", C.c_uint64), ("n_searches", C.c_uint32), ("reserved_", C.c_uint32),
                ("pairs_searched", C.c_uint64), ("rows_certified", C.c_uint64), ("rows_recomputed", C.c_uint64),
                ("trim", TrimInfo), ("ms", C.c_double), ("ms_sort", C.c_double), ("ms_search", C.c_double),
                ("ms_merge", C.c_double), ("ms_graph", C.c_double), ("ms_trim", C.c_double)]


class DoubletOpts(C.Structure):      # srx_doublet_opts
    _fields_ = [("sim_ratio", C.c_double), ("expected_rate", C.c_double), ("stdev_rate", C.c_double),
                ("target_sum", C.c_double), ("threshold", C.c_double), ("seed", C.c_uint64), ("k", C.c_int32),
                ("n_dims", C.c_int32), ("transform", C.c_int32), ("reserved_", C.c_int32)]


class DoubletInfo(C.Structure):      # srx_doublet_info
    _fields_ = [("n_obs", C.c_uint64), ("n_sim", C.c_uint64), ("nnz_sim", C.c_uint64), ("k", C.c_uint32),
                ("k_adj", C.c_uint32), ("d", C.c_uint32), ("threshold_found", C.c_uint32), ("threshold", C.c_double),
                ("smooth_rounds", C.c_uint32), ("reserved_", C.c_uint32), ("n_predicted", C.c_uint64),
                ("detected_rate", C.c_double), ("detectable_fraction", C.c_double), ("overall_rate", C.c_double),
                ("rows_certified", C.c_uint64), ("rows_recomputed", C.c_uint64), ("ms_simulate", C.c_double),
                ("ms_project", C.c_double), ("ms_knn", C.c_double), ("ms_score", C.c_double)]


class IterateArgs(C.Structure):      # srx_iterate_args
    _fields_ = [("k", C.c_int32), ("n", C.c_int32), ("l_act", C.c_int32), ("n_pc", C.c_int32), ("n_want", C.c_int32),
                ("d", C.c_int32), ("variant", C.c_int32), ("flags", C.c_int32), ("off_tol2", C.c_double), ("c", P),
                ("blk", P * 5), ("sm", P * 2), ("vec", P * 3), ("xi", P), ("out", C.c_double * 8),
                ("status", C.c_int32 * 2), ("tail_touched", C.c_int32), ("reserved", C.c_int32)]


class SelectArgs(C.Structure):      # srx_select_args
    _fields_ = [("G", C.c_uint64), ("take", C.c_uint64), ("n_cells", C.c_uint64), ("op", C.c_int32),
                ("route", C.c_int32), ("center", C.c_int32), ("scale", C.c_int32), ("flags", C.c_int32),
                ("reserved", C.c_int32), ("cnt", P), ("sum", P), ("sq", P), ("genes", P), ("var", P), ("rank", P),
                ("sel_rank", P), ("bits", P), ("prefix", P), ("mu", P), ("sd", P), ("dinv", P), ("trace", C.c_double),
                ("counter", C.c_uint32), ("status", C.c_int32), ("tail_touched", C.c_int32), ("reserved2", C.c_int32)]


class PipelineResult(C.Structure):      # srx_pipeline_result
    _fields_ = [("pca", PcaInfo), ("ms_normalize", C.c_double), ("ms_moments", C.c_double), ("ms_select", C.c_double),
                ("ms_compact", C.c_double), ("ms_pca", C.c_double)]


class SynthParams(C.Structure):      # srx_synth_params
    _fields_ = [("seed", C.c_uint64), ("n_rows_global", C.c_uint64), ("n_cols", C.c_uint64), ("density", C.c_double),
                ("lib_sigma", C.c_double), ("type_decay", C.c_double), ("n_types", C.c_uint32),
                ("marker_genes", C.c_uint32), ("expr_boost", C.c_uint32), ("value_boost", C.c_uint32),
                ("skew", C.c_uint32), ("reserved_", C.c_uint32)]


HOST_ALLREDUCE_FN = C.CFUNCTYPE(C.c_int32, P, C.POINTER(C.c_double), C.c_uint64)      # srx_host_allreduce_fn

SIGNATURES = {
    # name: (restype, argtypes)
    "srx_abi_version": (C.c_int32, []),
    "srx_device_count": (C.c_int32, [P]),
    "srx_ctx_create": (C.c_int32, [C.c_int32, C.POINTER(P)]),
    "srx_ctx_destroy": (None, [P]),
    "srx_ctx_synchronize": (C.c_int32, [P]),
    "srx_last_error": (C.c_char_p, [P]),
    "srx_comm_unique_id": (C.c_int32, [P]),
    "srx_comm_init": (C.c_int32, [P, C.c_int32, C.c_int32, P]),
    "srx_comm_init_host": (C.c_int32, [P, C.c_int32, C.c_int32, P, P]),
    "srx_comm_destroy": (C.c_int32, [P]),
    "srx_comm_info": (C.c_int32, [P, P, P, P, P]),
    "srx_comm_overlap_info": (C.c_int32, [P, P, P]),
    "srx_gram_mode_info": (C.c_int32, [P, P]),
    "srx_gram_exchange_ranges": (C.c_int32, [C.c_uint64, P]),
    "srx_partition_rows": (C.c_int32, [P, C.c_uint64, C.c_int32, P]),
    "srx_matrix_upload": (C.c_int32, [P, C.POINTER(Csr), C.c_int32, C.POINTER(P)]),
    "srx_matrix_upload_csc": (C.c_int32, [P, C.POINTER(Csr), C.c_int32, C.POINTER(P)]),
    "srx_matrix_format": (C.c_int32, [P, P]),
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
    "srx_gene_moments": (C.c_int32, [P, P, P, P]),
    "srx_filter_cells": (C.c_int32, [P, Flex, Flex, C.POINTER(P), P]),
    "srx_filter_genes": (C.c_int32, [P, Flex, Flex, C.POINTER(P), P]),
    "srx_subset": (C.c_int32, [P, P, P, C.POINTER(P)]),
    "srx_matrix_download_pattern": (C.c_int32, [P, P, P]),
    "srx_normalize_total_inplace": (C.c_int32, [P, C.c_double, C.c_int32]),
    "srx_log1p_inplace": (C.c_int32, [P]),
    "srx_normalize_log1p_inplace": (C.c_int32, [P, C.c_double, P]),
    "srx_select_hvg": (C.c_int32, [P, C.c_uint64, P, P]),
    "srx_pearson_gene_variance": (C.c_int32, [P, C.POINTER(PearsonOpts), P, C.POINTER(PearsonInfo)]),
    "srx_select_hvg_pearson": (C.c_int32, [P, C.c_uint64, C.POINTER(PearsonOpts), P, P, P, C.POINTER(PearsonInfo)]),
    "srx_pearson_residuals": (C.c_int32, [P, P, C.c_uint64, C.POINTER(PearsonOpts), P, C.POINTER(PearsonInfo)]),
    "srx_pca": (C.c_int32, [P, P, C.c_uint64, C.POINTER(PcaOpts), P, P, P, P, P, C.POINTER(PcaInfo)]),
    "srx_pca_loadings": (C.c_int32, [P, P, P, C.c_uint64, C.c_uint64, C.c_uint64, P]),
    "srx_pca_pearson": (C.c_int32, [P, P, C.c_uint64, C.POINTER(PearsonPcaOpts), P, P, P, P, C.POINTER(PearsonPcaInfo)]),
    "srx_pearson_gram": (C.c_int32, [P, P, C.c_uint64, C.POINTER(PearsonPcaOpts), P, P, C.POINTER(PearsonPcaInfo)]),
    "srx_regress_fit": (C.c_int32, [P, P, C.c_uint64, P, C.c_uint64, C.POINTER(RegressOpts), P, P, P,
                                    C.POINTER(RegressInfo)]),
    "srx_regress_sums": (C.c_int32, [P, P, C.c_uint64, P, C.c_uint64, C.POINTER(RegressOpts), P, P, P,
                                     C.POINTER(RegressInfo)]),
    "srx_regress_residuals": (C.c_int32, [P, P, C.c_uint64, P, C.c_uint64, C.POINTER(RegressOpts), P,
                                          C.POINTER(RegressInfo)]),
    "srx_regress_gram": (C.c_int32, [P, P, C.c_uint64, P, C.c_uint64, C.POINTER(RegressOpts), P, P,
                                     C.POINTER(RegressInfo)]),
    "srx_pca_regress": (C.c_int32, [P, P, C.c_uint64, P, C.c_uint64, C.POINTER(RegressOpts), P, P, P, P, P,
                                    C.POINTER(RegressInfo)]),
    "srx_gene_list_sums": (C.c_int32, [P, P, P, C.c_uint64, P, P, C.POINTER(GeneListInfo)]),
    "srx_score_genes_controls": (C.c_int32, [P, C.c_uint64, P, C.c_uint64, P, P, C.c_uint64,
                                             C.POINTER(ScoreGenesOpts), P, P, C.c_uint64, P]),
    "srx_score_genes": (C.c_int32, [P, P, P, C.c_uint64, P, C.c_uint64, C.POINTER(ScoreGenesOpts), P, P, P,
                                    C.c_uint64, C.POINTER(ScoreGenesInfo)]),
    "srx_pca_model_from_result": (C.c_int32, [P, C.POINTER(P)]),
    "srx_pca_model_create": (C.c_int32, [P, C.c_uint64, C.c_uint64, P, P, P, P, C.c_int32, C.c_int32, C.POINTER(P)]),
    "srx_pca_model_info": (C.c_int32, [P, P, P, P]),
    "srx_pca_model_free": (None, [P]),
    "srx_pca_transform": (C.c_int32, [P, P, P, C.c_double, C.c_int32, P]),
    "srx_knn_result": (C.c_int32, [P, C.POINTER(KnnOpts), P, P, C.POINTER(KnnInfo)]),
    "srx_knn_points": (C.c_int32, [P, P, C.c_uint64, P, C.c_uint64, C.c_uint64, C.POINTER(KnnOpts), P, P,
                                   C.POINTER(KnnInfo)]),
    "srx_neighbors_result": (C.c_int32, [P, C.POINTER(KnnOpts), C.POINTER(KnnInfo), C.POINTER(P)]),
    "srx_neighbors_from_knn": (C.c_int32, [P, P, P, C.c_uint64, C.c_uint32, C.POINTER(P)]),
    "srx_graph_info_get": (C.c_int32, [P, C.POINTER(GraphInfo)]),
    "srx_graph_fetch": (C.c_int32, [P, C.c_int32, P, P, P]),
    "srx_graph_fetch_scales": (C.c_int32, [P, P, P]),
    "srx_graph_free": (None, [P]),
    "srx_snn_from_knn": (C.c_int32, [P, P, P, C.c_uint64, C.c_uint32, C.POINTER(SnnOpts), C.POINTER(SnnInfo),
                                     C.POINTER(P)]),
    "srx_snn_graph": (C.c_int32, [P, C.POINTER(SnnOpts), C.POINTER(SnnInfo), C.POINTER(P)]),
    "srx_snn_min_shared": (C.c_int32, [C.c_uint32, C.c_int32, C.c_double, P]),
    "srx_knn_index_result": (C.c_int32, [P, C.c_int32, C.POINTER(IvfOpts), C.POINTER(P)]),
    "srx_knn_index_points": (C.c_int32, [P, P, C.c_uint64, C.c_uint64, C.POINTER(IvfOpts), P, C.POINTER(P)]),
    "srx_knn_index_info_get": (C.c_int32, [P, C.POINTER(IvfInfo)]),
    "srx_knn_index_fetch": (C.c_int32, [P, P, P, P]),
    "srx_knn_index_search": (C.c_int32, [P, P, C.c_uint64, C.POINTER(KnnOpts), C.c_int32, P, P,
                                         C.POINTER(IvfSearchInfo)]),
    "srx_neighbors_index": (C.c_int32, [P, C.POINTER(KnnOpts), C.c_int32, C.POINTER(IvfSearchInfo), C.POINTER(P)]),
    "srx_knn_index_free": (None, [P]),
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
    "srx_select_hvg_seurat_v3": (C.c_int32, [P, C.c_uint64, P, C.c_uint32, C.POINTER(SeuratV3Opts), P, P,
                                             C.POINTER(SeuratV3Tables), C.POINTER(SeuratV3Info)]),
    "srx_loess_direct": (C.c_int32, [P, P, P, C.c_uint64, C.c_double, P]),
    "srx_clipped_group_moments": (C.c_int32, [P, P, C.c_uint32, P, P, P, C.POINTER(MarkersInfo)]),
    "srx_umap": (C.c_int32, [P, P, C.POINTER(UmapOpts), P, P, C.POINTER(UmapInfo)]),
    "srx_umap_csr": (C.c_int32, [P, P, P, P, C.c_uint64, C.POINTER(UmapOpts), P, P, C.POINTER(UmapInfo)]),
    "srx_graph_embedding_fetch": (C.c_int32, [P, P, P]),
    "srx_umap_fit_ab": (C.c_int32, [C.c_double, C.c_double, P, P]),
    "srx_umap_transform_knn": (C.c_int32, [P, P, P, C.c_uint64, C.c_uint32, P, C.c_uint64, C.c_uint32,
                                           C.POINTER(UmapTransformOpts), C.POINTER(UmapTransformOut),
                                           C.POINTER(UmapTransformInfo)]),
    "srx_umap_transform_graph": (C.c_int32, [P, P, P, C.c_uint64, C.c_uint32, C.c_uint32,
                                             C.POINTER(UmapTransformOpts), C.POINTER(UmapTransformOut),
                                             C.POINTER(UmapTransformInfo)]),
    "srx_knn_vote": (C.c_int32, [P, P, C.c_uint64, C.c_uint32, P, C.c_uint64, C.c_uint32, P, P]),
    "srx_knn_vote_graph": (C.c_int32, [P, P, C.c_uint64, C.c_uint32, P, P]),
    "srx_tsne_affinities_knn": (C.c_int32, [P, P, P, C.c_uint64, C.c_uint32, C.c_double, C.POINTER(P)]),
    "srx_tsne_affinities_graph": (C.c_int32, [P, C.c_double, C.POINTER(P)]),
    "srx_tsne_info_get": (C.c_int32, [P, C.POINTER(TsneInfo)]),
    "srx_tsne_fetch_affinities": (C.c_int32, [P, P, P, P, P]),
    "srx_tsne_forces": (C.c_int32, [P, P, C.c_double, C.c_int32, P, P, P, C.POINTER(TsneForceInfo)]),
    "srx_tsne_run": (C.c_int32, [P, P, C.POINTER(TsneOpts), P, P, C.POINTER(TsneRunInfo)]),
    "srx_tsne_embedding_fetch": (C.c_int32, [P, P]),
    "srx_tsne_free": (None, [P]),
    "srx_draw_graph": (C.c_int32, [P, C.POINTER(Fa2Opts), P, P, C.POINTER(Fa2Info)]),
    "srx_draw_graph_csr": (C.c_int32, [P, P, P, P, C.c_uint64, C.POINTER(Fa2Opts), P, P, C.POINTER(Fa2Info)]),
    "srx_graph_layout_fetch": (C.c_int32, [P, P]),
    "srx_draw_graph_forces": (C.c_int32, [P, P, P, P, C.c_uint64, P, C.POINTER(Fa2Opts), P, P, P, P,
                                          C.POINTER(Fa2ForceInfo)]),
    "srx_fa2_speed": (C.c_int32, [C.c_uint64, C.c_double, C.c_double, C.c_double, P, P]),
    "srx_diffmap": (C.c_int32, [P, C.POINTER(DiffmapOpts), P, P, C.POINTER(DiffmapInfo)]),
    "srx_diffmap_csr": (C.c_int32, [P, P, P, P, C.c_uint64, C.POINTER(DiffmapOpts), P, P, C.POINTER(DiffmapInfo)]),
    "srx_graph_diffmap_fetch": (C.c_int32, [P, P, P, P]),
    "srx_graph_transitions_fetch": (C.c_int32, [P, P]),
    "srx_dpt": (C.c_int32, [P, C.c_uint64, C.c_double, P]),
    "srx_dpt_from": (C.c_int32, [P, P, P, C.c_uint64, C.c_uint32, C.c_uint64, C.c_double, P]),
    "srx_paga": (C.c_int32, [P, P, C.c_uint32, C.POINTER(PagaTables), C.POINTER(PagaInfo)]),
    "srx_paga_csr": (C.c_int32, [P, P, P, C.c_uint64, P, C.c_uint32, C.POINTER(PagaTables), C.POINTER(PagaInfo)]),
    "srx_paga_from_counts": (C.c_int32, [P, P, C.c_uint32, C.POINTER(PagaTables), C.POINTER(PagaInfo)]),
    "srx_paga_init_positions": (C.c_int32, [P, P, P, C.c_uint64, C.c_uint32, P, P, C.c_uint32, C.c_uint64, P]),
    "srx_autocorr": (C.c_int32, [P, P, C.POINTER(AutocorrOpts), C.POINTER(AutocorrOut), C.POINTER(AutocorrInfo)]),
    "srx_autocorr_csr": (C.c_int32, [P, P, P, P, C.c_uint64, C.POINTER(AutocorrOpts), C.POINTER(AutocorrOut),
                                     C.POINTER(AutocorrInfo)]),
    "srx_autocorr_scales": (C.c_int32, [C.POINTER(AutocorrInfo)]),
    "srx_autocorr_from_tables": (C.c_int32, [P, P, P, P, P, C.c_uint64, C.POINTER(AutocorrInfo),
                                             C.POINTER(AutocorrOut)]),
    "srx_harmony_result": (C.c_int32, [P, P, C.c_uint32, C.POINTER(HarmonyOpts), C.POINTER(P), C.POINTER(HarmonyInfo)]),
    "srx_harmony_points": (C.c_int32, [P, P, C.c_uint64, C.c_uint64, P, C.c_uint32, C.POINTER(HarmonyOpts),
                                       C.POINTER(P), C.POINTER(HarmonyInfo)]),
    "srx_harmony_fetch": (C.c_int32, [P, C.c_int32, P]),
    "srx_harmony_info_get": (C.c_int32, [P, C.POINTER(HarmonyInfo)]),
    "srx_knn_harmony": (C.c_int32, [P, C.POINTER(KnnOpts), P, P, C.POINTER(KnnInfo)]),
    "srx_neighbors_harmony": (C.c_int32, [P, C.POINTER(KnnOpts), C.POINTER(KnnInfo), C.POINTER(P)]),
    "srx_harmony_free": (None, [P]),
    "srx_bbknn_result": (C.c_int32, [P, P, C.c_uint32, C.POINTER(BbknnOpts), C.POINTER(BbknnInfo), C.POINTER(P)]),
    "srx_bbknn_points": (C.c_int32, [P, P, C.c_uint64, C.c_uint64, P, C.c_uint32, C.POINTER(BbknnOpts), P, P,
                                     C.POINTER(BbknnInfo), C.POINTER(P)]),
    "srx_bbknn_harmony": (C.c_int32, [P, P, C.c_uint32, C.POINTER(BbknnOpts), C.POINTER(BbknnInfo), C.POINTER(P)]),
    "srx_graph_trim": (C.c_int32, [P, C.c_int64, C.POINTER(TrimInfo), C.POINTER(P)]),
    "srx_doublets_simulate": (C.c_int32, [P, C.c_uint64, C.c_uint64, P, C.POINTER(P), P]),
    "srx_doublet_scores_knn": (C.c_int32, [P, P, C.c_uint64, C.c_uint64, C.c_uint32, C.c_double, C.c_double, P, P]),
    "srx_doublets_threshold": (C.c_int32, [P, C.c_uint64, P, P, P]),
    "srx_doublets_result": (C.c_int32, [P, P, C.POINTER(DoubletOpts), C.POINTER(P), C.POINTER(DoubletInfo)]),
    "srx_doublets_call": (C.c_int32, [P, C.c_double, C.POINTER(DoubletInfo)]),
    "srx_doublets_fetch": (C.c_int32, [P, C.c_int32, P]),
    "srx_doublets_info_get": (C.c_int32, [P, C.POINTER(DoubletInfo)]),
    "srx_doublets_free": (None, [P]),
    "srx_spmm": (C.c_int32, [P, P, C.c_uint64, P, P, P, P]),
    "srx_iterate_op": (C.c_int32, [P, C.c_int32, C.POINTER(IterateArgs)]),
    "srx_select_op": (C.c_int32, [P, C.POINTER(SelectArgs)]),
    "srx_pipeline": (C.c_int32, [P, C.c_double, C.c_uint64, C.POINTER(PcaOpts), C.POINTER(PipelineResult)]),
    "srx_result_fetch": (C.c_int32, [P, P, P, P, P, P, P]),
    "srx_backed_create": (C.c_int32, [P, C.c_uint64, C.c_int32, C.POINTER(P)]),
    "srx_backed_destroy": (None, [P]),
    "srx_backed_stats_tile": (C.c_int32, [P, C.POINTER(Csr), C.c_double, C.c_int32, P, P]),
    "srx_backed_moments": (C.c_int32, [P, P, P, P, P]),
    "srx_backed_select": (C.c_int32, [P, C.c_uint64, P, C.c_uint64, C.POINTER(PcaOpts), P, P]),
    "srx_backed_gram_tile": (C.c_int32, [P, C.POINTER(Csr), C.c_double, C.c_int32]),
    "srx_backed_solve": (C.c_int32, [P, C.POINTER(PcaInfo)]),
    "srx_backed_fetch": (C.c_int32, [P, P, P, P, P, P, P]),
    "srx_prof_enable": (C.c_int32, [P, C.c_uint32]),
    "srx_prof_reset": (C.c_int32, [P]),
    "srx_prof_get": (C.c_int32, [P, C.c_int32, P, P, P]),
    "srx_prof_get_aux": (C.c_int32, [P, C.c_int32, P]),
    "srx_synth_defaults": (None, [C.POINTER(SynthParams), C.c_uint64, C.c_uint64, C.c_uint64, C.c_double]),
    "srx_synth_indptr": (C.c_int32, [C.POINTER(SynthParams), C.c_uint64, C.c_uint64, P]),
    "srx_synth_fill_host": (C.c_int32, [C.POINTER(SynthParams), C.c_uint64, C.c_uint64, P, P, P]),
    "srx_synth_generate": (C.c_int32, [P, C.POINTER(SynthParams), C.c_uint64, C.c_uint64, C.c_int32, C.c_int32,
                                       C.POINTER(P)]),
}
EXPORTS = tuple(SIGNATURES)
