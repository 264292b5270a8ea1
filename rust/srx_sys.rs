// rust/srx_sys.rs — GENERATED from include/srx.h by scripts/gen_rust_bindings.py; do not edit.
// `extern "C"` declarations of libsrx_hip.so for the shim of INTEGRATION.md (src/gpu/ffi.rs in a SingleRust
// checkout, behind a cargo feature).  Not compile-checked here: the build image has no rustc.  The hand-written
// part of the binding (the `upload` helper and the replaced function bodies) is rust/shim.rs.
#![allow(non_camel_case_types, dead_code)]
use std::os::raw::{c_char, c_void};

pub const SRX_ABI_VERSION: i32 = 6;
pub const SRX_UNIQUE_ID_BYTES: usize = 128;
pub const SRX_GENE_LISTS_MAX: i32 = 4096;
pub const SRX_KNN_MAX_DIMS: i32 = 128;
pub const SRX_LOUVAIN_MAX_LEVELS: i32 = 32;
pub const SRX_GROUPS_MAX: i32 = 4096;
pub const SRX_UMAP_GROUP: i32 = 8;
pub const SRX_UMAP_MAX_EPOCHS: i32 = 1048576;
pub const SRX_UMAP_TRANSFORM_CHUNK: i32 = 64;
pub const SRX_TSNE_MAX_K: i32 = 64;
pub const SRX_TSNE_MAX_LEVELS: i32 = 12;
pub const SRX_TSNE_GROUP: i32 = 8;
pub const SRX_TSNE_MAX_ITERS: i32 = 1048576;
pub const SRX_FA2_GROUP: i32 = 8;
pub const SRX_FA2_MAX_ITERS: i32 = 1048576;
pub const SRX_DIFFMAP_GROUP: i32 = 8;
pub const SRX_DIFFMAP_MAX_COMPS: i32 = 64;
pub const SRX_DIFFMAP_MAX_NCV: i32 = 129;
pub const SRX_HARMONY_MAX_CLUSTERS: i32 = 256;
pub const SRX_HARMONY_MAX_BATCHES: i32 = 256;
pub const SRX_HARMONY_MAX_ROUNDS: i32 = 64;
pub const SRX_DOUBLET_MAX_K: i32 = 64;
pub const SRX_DOUBLET_MAX_ROUNDS: i32 = 10000;
pub const SRX_DOUBLET_WAVE_ROW: i32 = 8192;
pub const SRX_IT_ALIAS_B: i32 = 1;
pub const SRX_IT_ZERO_WP: i32 = 1;
pub const SRX_IT_Z0: i32 = 1;
pub const SRX_IT_Z0_IS_SRC: i32 = 8;
pub const SRX_IT_SRC_IS_W: i32 = 16;
pub const SRX_SEL_NO_VECTORS: i32 = 1;
pub const SRX_SEL_COUNTER_UNUSED: i32 = 2147483646;
pub const SRX_OK: i32 = 0;
pub const SRX_E_ARG: i32 = -1;
pub const SRX_E_DTYPE: i32 = -2;
pub const SRX_E_FORMAT: i32 = -3;
pub const SRX_E_BOUNDS: i32 = -4;
pub const SRX_E_HIP: i32 = -5;
pub const SRX_E_RCCL: i32 = -6;
pub const SRX_E_OOM: i32 = -7;
pub const SRX_E_NAN: i32 = -8;
pub const SRX_E_SHAPE: i32 = -9;
pub const SRX_E_NOCONV: i32 = -10;
pub const SRX_I8: i32 = 0;
pub const SRX_I16: i32 = 1;
pub const SRX_I32: i32 = 2;
pub const SRX_U8: i32 = 3;
pub const SRX_U16: i32 = 4;
pub const SRX_U32: i32 = 5;
pub const SRX_F32: i32 = 6;
pub const SRX_F64: i32 = 7;
pub const SRX_ROW: i32 = 0;
pub const SRX_COLUMN: i32 = 1;
pub const SRX_STORE_AUTO: i32 = 0;
pub const SRX_STORE_F32: i32 = 1;
pub const SRX_STORE_F64: i32 = 2;
pub const SRX_FORMAT_CSR: i32 = 0;
pub const SRX_FORMAT_CSC: i32 = 1;
pub const SRX_FLEX_NONE: i32 = 0;
pub const SRX_FLEX_ABSOLUTE: i32 = 1;
pub const SRX_FLEX_RELATIVE: i32 = 2;
pub const SRX_SOLVER_AUTO: i32 = 0;
pub const SRX_SOLVER_GRAM: i32 = 1;
pub const SRX_SOLVER_SPMM: i32 = 2;
pub const SRX_PEARSON_TOTALS_ALL: i32 = 0;
pub const SRX_PEARSON_TOTALS_SELECTED: i32 = 1;
pub const SRX_GRAPH_DISTANCES: i32 = 0;
pub const SRX_GRAPH_CONNECTIVITIES: i32 = 1;
pub const SRX_SNN_JACCARD: i32 = 0;
pub const SRX_SNN_NUMBER: i32 = 1;
pub const SRX_SNN_PAIRS_SHARED: i32 = 0;
pub const SRX_SNN_PAIRS_KNN: i32 = 1;
pub const SRX_MARKERS_CNT: i32 = 0;
pub const SRX_MARKERS_SUM: i32 = 1;
pub const SRX_MARKERS_SUMSQ: i32 = 2;
pub const SRX_MARKERS_MEAN: i32 = 3;
pub const SRX_MARKERS_VAR: i32 = 4;
pub const SRX_MARKERS_MEAN_REST: i32 = 5;
pub const SRX_MARKERS_VAR_REST: i32 = 6;
pub const SRX_MARKERS_SCORE: i32 = 7;
pub const SRX_MARKERS_LFC: i32 = 8;
pub const SRX_MARKERS_PCT: i32 = 9;
pub const SRX_MARKERS_PCT_REST: i32 = 10;
pub const SRX_MARKERS_RANKSUM2: i32 = 11;
pub const SRX_UMAP_INIT_GIVEN: i32 = 0;
pub const SRX_UMAP_INIT_RANDOM: i32 = 1;
pub const SRX_UMAP_INIT_PCA: i32 = 2;
pub const SRX_TSNE_INIT_GIVEN: i32 = 0;
pub const SRX_TSNE_INIT_RANDOM: i32 = 1;
pub const SRX_TSNE_INIT_PCA: i32 = 2;
pub const SRX_FA2_INIT_GIVEN: i32 = 0;
pub const SRX_FA2_INIT_RANDOM: i32 = 1;
pub const SRX_HARMONY_CORRECTED: i32 = 0;
pub const SRX_HARMONY_R: i32 = 1;
pub const SRX_HARMONY_CENTROIDS: i32 = 2;
pub const SRX_HARMONY_OBSERVED: i32 = 3;
pub const SRX_HARMONY_EXPECTED: i32 = 4;
pub const SRX_DOUBLETS_SCORES_OBS: i32 = 0;
pub const SRX_DOUBLETS_SCORES_SIM: i32 = 1;
pub const SRX_DOUBLETS_SE_OBS: i32 = 2;
pub const SRX_DOUBLETS_SE_SIM: i32 = 3;
pub const SRX_DOUBLETS_Z: i32 = 4;
pub const SRX_DOUBLETS_PREDICTED: i32 = 5;
pub const SRX_DOUBLETS_POINTS: i32 = 6;
pub const SRX_DOUBLETS_PARENTS: i32 = 7;
pub const SRX_DOUBLETS_KNN: i32 = 8;
pub const SRX_IT_APPLY: i32 = 0;
pub const SRX_IT_GRAM1: i32 = 1;
pub const SRX_IT_GRAM2: i32 = 2;
pub const SRX_IT_CHOL: i32 = 3;
pub const SRX_IT_TRSM: i32 = 4;
pub const SRX_IT_EIG: i32 = 5;
pub const SRX_IT_RITZ: i32 = 6;
pub const SRX_IT_CHEB: i32 = 7;
pub const SRX_SEL_HVG: i32 = 0;
pub const SRX_SEL_LIST: i32 = 1;
pub const SRX_BACKED_NORMALIZE: i32 = 1;
pub const SRX_BACKED_LOG1P: i32 = 2;
pub const SRX_K_NORMALIZE: i32 = 0;
pub const SRX_K_MOMENTS: i32 = 1;
pub const SRX_K_COMPACT: i32 = 2;
pub const SRX_K_SPMM_FWD: i32 = 3;
pub const SRX_K_SPMM_T: i32 = 4;
pub const SRX_K_GRAM: i32 = 5;
pub const SRX_K_DENSE: i32 = 6;
pub const SRX_K_ROWSUM: i32 = 7;
pub const SRX_K_ITERATE: i32 = 8;
pub const SRX_K_SELECT: i32 = 9;
pub const SRX_K_BUCKET: i32 = 10;
pub const SRX_K_KNN: i32 = 11;
pub const SRX_K_GRAPH: i32 = 12;
pub const SRX_K_COUNT_: i32 = 13;

#[repr(C)] pub struct SrxCtx { _private: [u8; 0] }      // opaque `srx_ctx`
#[repr(C)] pub struct SrxMat { _private: [u8; 0] }      // opaque `srx_mat`
#[repr(C)] pub struct SrxPcaModel { _private: [u8; 0] }      // opaque `srx_pca_model`
#[repr(C)] pub struct SrxGraph { _private: [u8; 0] }      // opaque `srx_graph`
#[repr(C)] pub struct SrxKnnIndex { _private: [u8; 0] }      // opaque `srx_knn_index`
#[repr(C)] pub struct SrxMarkers { _private: [u8; 0] }      // opaque `srx_markers`
#[repr(C)] pub struct SrxTsne { _private: [u8; 0] }      // opaque `srx_tsne`
#[repr(C)] pub struct SrxHarmony { _private: [u8; 0] }      // opaque `srx_harmony`
#[repr(C)] pub struct SrxDoublets { _private: [u8; 0] }      // opaque `srx_doublets`
#[repr(C)] pub struct SrxBacked { _private: [u8; 0] }      // opaque `srx_backed`

#[repr(C)]
#[derive(Clone, Copy)]
pub struct SrxCsr {      // `srx_csr`
    pub n_rows: u64,
    pub n_cols: u64,
    pub nnz: u64,
    pub indptr: *const u64,
    pub indices: *const u64,
    pub values: *mut c_void,
    pub dtype: i32,
}

#[repr(C)]
#[derive(Clone, Copy)]
pub struct SrxMatInfo {      // `srx_mat_info`
    pub n_rows: u64,
    pub n_cols: u64,
    pub nnz: u64,
    pub dtype: i32,
    pub store: i32,
    pub row_offset: u64,
    pub n_rows_global: u64,
}

#[repr(C)]
#[derive(Clone, Copy)]
pub struct SrxFlex {      // `srx_flex`
    pub kind: i32,
    pub absolute: u32,
    pub relative: f64,
}

#[repr(C)]
#[derive(Clone, Copy)]
pub struct SrxPearsonOpts {      // `srx_pearson_opts`
    pub theta: f64,
    pub clip: f64,
}

#[repr(C)]
#[derive(Clone, Copy)]
pub struct SrxPearsonInfo {      // `srx_pearson_info`
    pub n_cells: u64,
    pub n_genes: u64,
    pub n_expressed: u64,
    pub n_empty_cells: u64,
    pub total: f64,
    pub theta: f64,
    pub clip: f64,
    pub sum_quantum: f64,
    pub sq_quantum: f64,
    pub ms_dense: f64,
    pub ms_sparse: f64,
    pub ms_rank: f64,
}

#[repr(C)]
#[derive(Clone, Copy)]
pub struct SrxPcaOpts {      // `srx_pca_opts`
    pub n_components: i32,
    pub center: i32,
    pub scale: i32,
    pub n_threads: i32,
    pub block: i32,
    pub max_iter: i32,
    pub solver: i32,
    pub tol: f64,
    pub seed: u64,
}

#[repr(C)]
#[derive(Clone, Copy)]
pub struct SrxPcaInfo {      // `srx_pca_info`
    pub n_cells_global: u64,
    pub k: u32,
    pub n_pc: u32,
    pub block: u32,
    pub n_iter: u32,
    pub residual: f64,
    pub nnz_selected: u64,
    pub solver: u32,
    pub reserved: u32,
}

#[repr(C)]
#[derive(Clone, Copy)]
pub struct SrxPearsonPcaOpts {      // `srx_pearson_pca_opts`
    pub pearson: SrxPearsonOpts,
    pub totals: i32,
    pub center: i32,
    pub chunk_cells: u64,
    pub pca: SrxPcaOpts,
}

#[repr(C)]
#[derive(Clone, Copy)]
pub struct SrxPearsonPcaInfo {      // `srx_pearson_pca_info`
    pub n_cells: u64,
    pub n_genes: u64,
    pub n_expressed: u64,
    pub n_empty_cells: u64,
    pub total: f64,
    pub theta: f64,
    pub clip: f64,
    pub pca: SrxPcaInfo,
    pub ms_gram: f64,
    pub ms_solve: f64,
    pub ms_scores: f64,
    pub n_chunks: u64,
    pub chunk_cells: u64,
    pub chunk_bytes: u64,
}

#[repr(C)]
#[derive(Clone, Copy)]
pub struct SrxRegressOpts {      // `srx_regress_opts`
    pub scale: i32,
    pub reserved: i32,
    pub max_value: f64,
    pub chunk_cells: u64,
    pub pca: SrxPcaOpts,
}

#[repr(C)]
#[derive(Clone, Copy)]
pub struct SrxRegressInfo {      // `srx_regress_info`
    pub n_cells: u64,
    pub n_genes: u64,
    pub n_cov: u64,
    pub n_constant_genes: u64,
    pub n_clipped: u64,
    pub min_pivot: f64,
    pub ms_fit: f64,
    pub ms_scale: f64,
    pub ms_gram: f64,
    pub ms_solve: f64,
    pub ms_scores: f64,
    pub n_chunks: u64,
    pub chunk_cells: u64,
    pub chunk_bytes: u64,
    pub pca: SrxPcaInfo,
}

#[repr(C)]
#[derive(Clone, Copy)]
pub struct SrxGeneListInfo {      // `srx_gene_list_info`
    pub n_rows: u64,
    pub n_cols: u64,
    pub n_lists: u64,
    pub longest_list: u64,
    pub sum_scale_log2: i32,
    pub n_walks: u32,
    pub max_abs: f64,
    pub ms_scan: f64,
    pub ms_walk: f64,
}

#[repr(C)]
#[derive(Clone, Copy)]
pub struct SrxScoreGenesOpts {      // `srx_score_genes_opts`
    pub ctrl_size: u32,
    pub n_bins: u32,
    pub seed: u64,
    pub ctrl_as_ref: i32,
    pub reserved: i32,
}

#[repr(C)]
#[derive(Clone, Copy)]
pub struct SrxScoreGenesInfo {      // `srx_score_genes_info`
    pub n_rows: u64,
    pub n_cols: u64,
    pub n_sets: u64,
    pub n_pool: u64,
    pub n_ctrl_total: u64,
    pub n_items: u64,
    pub longest_list: u64,
    pub sum_scale_log2: i32,
    pub n_walks: u32,
    pub max_abs: f64,
    pub ms_mean: f64,
    pub ms_ctrl: f64,
    pub ms_walk: f64,
}

#[repr(C)]
#[derive(Clone, Copy)]
pub struct SrxKnnOpts {      // `srx_knn_opts`
    pub k: i32,
    pub n_dims: i32,
    pub include_self: i32,
    pub reserved: i32,
}

#[repr(C)]
#[derive(Clone, Copy)]
pub struct SrxKnnInfo {      // `srx_knn_info`
    pub n_ref: u64,
    pub n_query: u64,
    pub d: u32,
    pub k: u32,
    pub n_candidates: u32,
    pub reserved: u32,
    pub rows_certified: u64,
    pub rows_recomputed: u64,
}

#[repr(C)]
#[derive(Clone, Copy)]
pub struct SrxGraphInfo {      // `srx_graph_info`
    pub n: u64,
    pub k: u32,
    pub reserved: u32,
    pub nnz_distances: u64,
    pub nnz_connectivities: u64,
    pub n_mutual: u64,
    pub rows_no_root: u64,
    pub rows_clamped: u64,
    pub rows_all_zero: u64,
    pub entries_dropped: u64,
    pub max_row_nnz: u64,
}

#[repr(C)]
#[derive(Clone, Copy)]
pub struct SrxSnnOpts {      // `srx_snn_opts`
    pub weight: i32,
    pub pairs: i32,
    pub include_self: i32,
    pub reserved: i32,
    pub prune: f64,
}

#[repr(C)]
#[derive(Clone, Copy)]
pub struct SrxSnnInfo {      // `srx_snn_info`
    pub n: u64,
    pub k: u32,
    pub set_size: u32,
    pub min_shared: u32,
    pub max_shared: u32,
    pub pairs_considered: u64,
    pub pairs_kept: u64,
    pub nnz: u64,
    pub max_row_nnz: u64,
    pub max_in_degree: u64,
    pub max_candidates: u64,
    pub sum_candidates: u64,
    pub wave_capacity: u32,
    pub short_capacity: u32,
    pub rows_wave: u64,
    pub rows_long: u64,
    pub rows_empty: u64,
    pub ms: f64,
    pub ms_lists: f64,
    pub ms_count: f64,
    pub ms_fill: f64,
}

#[repr(C)]
#[derive(Clone, Copy)]
pub struct SrxIvfOpts {      // `srx_ivf_opts`
    pub n_lists: i32,
    pub train_iters: i32,
    pub seed: u64,
    pub max_train_points: u64,
}

#[repr(C)]
#[derive(Clone, Copy)]
pub struct SrxIvfInfo {      // `srx_ivf_info`
    pub n_ref: u64,
    pub n_train: u64,
    pub d: u32,
    pub n_lists: u32,
    pub train_iters: u32,
    pub reserved: u32,
    pub min_list: u64,
    pub max_list: u64,
    pub empty_lists: u64,
    pub inertia: f64,
    pub ms_train: f64,
    pub ms_assign: f64,
}

#[repr(C)]
#[derive(Clone, Copy)]
pub struct SrxIvfSearchInfo {      // `srx_ivf_search_info`
    pub n_query: u64,
    pub k: u32,
    pub n_probe: u32,
    pub n_candidates: u32,
    pub reserved: u32,
    pub rows_certified: u64,
    pub rows_rescanned: u64,
    pub rows_exhaustive: u64,
    pub pairs: u64,
    pub points_scanned: u64,
}

#[repr(C)]
#[derive(Clone, Copy)]
pub struct SrxLouvainOpts {      // `srx_louvain_opts`
    pub resolution: f64,
    pub min_gain: f64,
    pub max_levels: i32,
    pub max_sweeps: i32,
}

#[repr(C)]
#[derive(Clone, Copy)]
pub struct SrxLouvainInfo {      // `srx_louvain_info`
    pub n: u64,
    pub n_communities: u64,
    pub n_levels: u32,
    pub reserved: u32,
    pub sweeps: u64,
    pub moves: u64,
    pub modularity: f64,
    pub ms: f64,
    pub level_communities: [u64; SRX_LOUVAIN_MAX_LEVELS as usize],
    pub level_modularity: [f64; SRX_LOUVAIN_MAX_LEVELS as usize],
}

#[repr(C)]
#[derive(Clone, Copy)]
pub struct SrxRankGenesOpts {      // `srx_rank_genes_opts`
    pub n_top: i32,
    pub logged: i32,
}

#[repr(C)]
#[derive(Clone, Copy)]
pub struct SrxMarkersInfo {      // `srx_markers_info`
    pub n_rows: u64,
    pub n_cols: u64,
    pub n_groups: u32,
    pub n_top: u32,
    pub sum_scale_log2: i32,
    pub sq_scale_log2: i32,
    pub groups_degenerate: u32,
    pub reserved: u32,
    pub max_abs: f64,
    pub ms: f64,
}

#[repr(C)]
#[derive(Clone, Copy)]
pub struct SrxWilcoxonOpts {      // `srx_wilcoxon_opts`
    pub n_top: i32,
    pub logged: i32,
    pub tie_correct: i32,
    pub reserved: i32,
    pub scratch_bytes: u64,
}

#[repr(C)]
#[derive(Clone, Copy)]
pub struct SrxWilcoxonInfo {      // `srx_wilcoxon_info`
    pub tie_correct: i32,
    pub n_chunks: u32,
    pub scratch_bytes: u64,
    pub segment_limit: u64,
    pub segments_short: u64,
    pub segments_long: u64,
    pub ms_stage: f64,
    pub ms_sort: f64,
    pub ms_ranks: f64,
}

#[repr(C)]
#[derive(Clone, Copy)]
pub struct SrxSeuratV3Opts {      // `srx_seurat_v3_opts`
    pub span: f64,
    pub paper_order: i32,
    pub reserved: i32,
}

#[repr(C)]
#[derive(Clone, Copy)]
pub struct SrxSeuratV3Tables {      // `srx_seurat_v3_tables`
    pub means: *mut f64,
    pub variances: *mut f64,
    pub variances_norm: *mut f64,
    pub median: *mut f64,
    pub nbatches: *mut u32,
    pub mean: *mut f64,
    pub var: *mut f64,
    pub fitted: *mut f64,
    pub reg_var: *mut f64,
    pub clip: *mut f64,
    pub clip_sum: *mut f64,
    pub clip_sumsq: *mut f64,
    pub nv: *mut f64,
    pub rank: *mut u32,
}

#[repr(C)]
#[derive(Clone, Copy)]
pub struct SrxSeuratV3Info {      // `srx_seurat_v3_info`
    pub n_cells: u64,
    pub n_genes: u64,
    pub n_batches: u32,
    pub sum_scale_log2: i32,
    pub sq_scale_log2: i32,
    pub reserved: u32,
    pub max_abs: f64,
    pub min_batch_cells: u64,
    pub span: f64,
    pub ms_moments: f64,
    pub ms_loess: f64,
    pub ms_clip: f64,
    pub ms_rank: f64,
}

#[repr(C)]
#[derive(Clone, Copy)]
pub struct SrxUmapOpts {      // `srx_umap_opts`
    pub a: f64,
    pub b: f64,
    pub min_dist: f64,
    pub spread: f64,
    pub gamma: f64,
    pub alpha0: f64,
    pub seed: u64,
    pub n_epochs: i32,
    pub stop_after: i32,
    pub n_components: i32,
    pub negative_sample_rate: i32,
    pub init: i32,
    pub reserved: i32,
}

#[repr(C)]
#[derive(Clone, Copy)]
pub struct SrxUmapInfo {      // `srx_umap_info`
    pub n: u64,
    pub nnz: u64,
    pub entries_active: u64,
    pub samples: u64,
    pub negatives: u64,
    pub negatives_skipped: u64,
    pub n_epochs: u32,
    pub epochs_run: u32,
    pub dim: u32,
    pub reserved: u32,
    pub a: f64,
    pub b: f64,
    pub w_max: f64,
    pub ms: f64,
}

#[repr(C)]
#[derive(Clone, Copy)]
pub struct SrxUmapTransformOpts {      // `srx_umap_transform_opts`
    pub a: f64,
    pub b: f64,
    pub min_dist: f64,
    pub spread: f64,
    pub gamma: f64,
    pub alpha0: f64,
    pub seed: u64,
    pub n_epochs: i32,
    pub stop_after: i32,
    pub negative_sample_rate: i32,
    pub chunk_epochs: i32,
}

#[repr(C)]
#[derive(Clone, Copy)]
pub struct SrxUmapTransformOut {      // `srx_umap_transform_out`
    pub embedding: *mut f64,
    pub start: *mut f64,
    pub weights: *mut f64,
    pub columns: *mut u32,
    pub sigma: *mut f64,
}

#[repr(C)]
#[derive(Clone, Copy)]
pub struct SrxUmapTransformInfo {      // `srx_umap_transform_info`
    pub n_query: u64,
    pub n_ref: u64,
    pub entries_active: u64,
    pub samples: u64,
    pub negatives: u64,
    pub rows_no_root: u64,
    pub rows_clamped: u64,
    pub rows_all_zero: u64,
    pub rows_start_nearest: u64,
    pub kq: u32,
    pub dim: u32,
    pub n_epochs: u32,
    pub epochs_run: u32,
    pub a: f64,
    pub b: f64,
    pub w_max: f64,
    pub ms: f64,
    pub membership_ms: f64,
}

#[repr(C)]
#[derive(Clone, Copy)]
pub struct SrxTsneInfo {      // `srx_tsne_info`
    pub n: u64,
    pub nnz: u64,
    pub n_mutual: u64,
    pub rows_no_root: u64,
    pub entries_dropped: u64,
    pub k: u32,
    pub reserved: u32,
    pub perplexity: f64,
}

#[repr(C)]
#[derive(Clone, Copy)]
pub struct SrxTsneOpts {      // `srx_tsne_opts`
    pub theta: f64,
    pub exaggeration: f64,
    pub learning_rate: f64,
    pub seed: u64,
    pub n_iter: i32,
    pub exaggeration_iters: i32,
    pub stop_after: i32,
    pub levels: i32,
    pub init: i32,
    pub reserved: i32,
}

#[repr(C)]
#[derive(Clone, Copy)]
pub struct SrxTsneRunInfo {      // `srx_tsne_run_info`
    pub n: u64,
    pub nnz: u64,
    pub n_iter: u32,
    pub iters_run: u32,
    pub levels: u32,
    pub reserved: u32,
    pub eta: f64,
    pub Z: f64,
    pub kl: f64,
    pub side: f64,
    pub cells_accepted: u64,
    pub cells_exact: u64,
    pub pairs_exact: u64,
    pub ms: f64,
}

#[repr(C)]
#[derive(Clone, Copy)]
pub struct SrxTsneForceInfo {      // `srx_tsne_force_info`
    pub levels: u32,
    pub reserved: u32,
    pub side: f64,
    pub lo: [f64; 2 as usize],
    pub cells_accepted: u64,
    pub cells_exact: u64,
    pub pairs_exact: u64,
}

#[repr(C)]
#[derive(Clone, Copy)]
pub struct SrxFa2Opts {      // `srx_fa2_opts`
    pub theta: f64,
    pub scaling_ratio: f64,
    pub gravity: f64,
    pub jitter_tolerance: f64,
    pub seed: u64,
    pub n_iter: i32,
    pub stop_after: i32,
    pub levels: i32,
    pub init: i32,
    pub strong_gravity: i32,
    pub linlog: i32,
}

#[repr(C)]
#[derive(Clone, Copy)]
pub struct SrxFa2Info {      // `srx_fa2_info`
    pub n: u64,
    pub nnz: u64,
    pub total_mass: u64,
    pub n_iter: u32,
    pub iters_run: u32,
    pub levels: u32,
    pub reserved: u32,
    pub speed: f64,
    pub speed_efficiency: f64,
    pub swing: f64,
    pub traction: f64,
    pub side: f64,
    pub cells_accepted: u64,
    pub cells_exact: u64,
    pub pairs_exact: u64,
    pub pairs_coincident: u64,
    pub ms: f64,
}

#[repr(C)]
#[derive(Clone, Copy)]
pub struct SrxFa2ForceInfo {      // `srx_fa2_force_info`
    pub levels: u32,
    pub reserved: u32,
    pub side: f64,
    pub lo: [f64; 2 as usize],
    pub total_mass: u64,
    pub cells_accepted: u64,
    pub cells_exact: u64,
    pub pairs_exact: u64,
    pub pairs_coincident: u64,
}

#[repr(C)]
#[derive(Clone, Copy)]
pub struct SrxDiffmapOpts {      // `srx_diffmap_opts`
    pub tol: f64,
    pub seed: u64,
    pub n_comps: i32,
    pub ncv: i32,
    pub max_matvecs: i32,
    pub density_normalize: i32,
}

#[repr(C)]
#[derive(Clone, Copy)]
pub struct SrxDiffmapInfo {      // `srx_diffmap_info`
    pub n: u64,
    pub nnz: u64,
    pub n_comps: u32,
    pub ncv: u32,
    pub matvecs: u32,
    pub restarts: u32,
    pub breakdowns: u32,
    pub reserved: u32,
    pub max_residual: f64,
    pub max_ortho: f64,
    pub ms: f64,
}

#[repr(C)]
#[derive(Clone, Copy)]
pub struct SrxPagaInfo {      // `srx_paga_info`
    pub n: u64,
    pub nnz: u64,
    pub n_groups: u32,
    pub groups_empty: u32,
    pub edges_inner: u64,
    pub edges_inter: u64,
    pub pairs_connected: u64,
    pub pairs_clipped: u64,
    pub tree_edges: u32,
    pub components: u32,
    pub ms: f64,
}

#[repr(C)]
#[derive(Clone, Copy)]
pub struct SrxPagaTables {      // `srx_paga_tables`
    pub sizes: *mut u64,
    pub out_edges: *mut u64,
    pub counts: *mut u64,
    pub connectivities: *mut f64,
    pub expected: *mut f64,
    pub tree: *mut f64,
}

#[repr(C)]
#[derive(Clone, Copy)]
pub struct SrxAutocorrOpts {      // `srx_autocorr_opts`
    pub rows_per_block: u32,
    pub reserved: u32,
}

#[repr(C)]
#[derive(Clone, Copy)]
pub struct SrxAutocorrOut {      // `srx_autocorr_out`
    pub morans_i: *mut f64,
    pub gearys_c: *mut f64,
    pub z_i: *mut f64,
    pub z_c: *mut f64,
    pub sum: *mut f64,
    pub sumsq: *mut f64,
    pub dsum: *mut f64,
    pub dsumsq: *mut f64,
    pub cross: *mut f64,
    pub sum_int: *mut i64,
    pub sumsq_int: *mut i64,
    pub dsum_int: *mut i64,
    pub dsumsq_int: *mut i64,
    pub cross_int: *mut i64,
}

#[repr(C)]
#[derive(Clone, Copy)]
pub struct SrxAutocorrInfo {      // `srx_autocorr_info`
    pub n: u64,
    pub n_genes: u64,
    pub nnz: u64,
    pub s_sum: i32,
    pub s_sumsq: i32,
    pub s_dsum: i32,
    pub s_dsumsq: i32,
    pub s_cross: i32,
    pub s_w: i32,
    pub s_1: i32,
    pub s_2: i32,
    pub max_abs: f64,
    pub max_weight: f64,
    pub max_degree: f64,
    pub w_int: i64,
    pub s1_int: i64,
    pub s2_int: i64,
    pub w: f64,
    pub s1: f64,
    pub s2: f64,
    pub e_i: f64,
    pub var_i: f64,
    pub e_c: f64,
    pub var_c: f64,
    pub genes_constant: u64,
    pub ms: f64,
    pub ms_graph: f64,
    pub ms_moments: f64,
    pub ms_walk: f64,
    pub ms_wmax: f64,
    pub ms_degrees: f64,
    pub ms_s2: f64,
    pub ms_sum_sumsq: f64,
    pub ms_dsum_dsumsq: f64,
}

#[repr(C)]
#[derive(Clone, Copy)]
pub struct SrxHarmonyOpts {      // `srx_harmony_opts`
    pub theta: f64,
    pub sigma: f64,
    pub lambda: f64,
    pub epsilon_cluster: f64,
    pub epsilon_harmony: f64,
    pub seed: u64,
    pub n_clusters: i32,
    pub n_blocks: i32,
    pub max_rounds: i32,
    pub max_cluster_iters: i32,
    pub init_iters: i32,
    pub n_dims: i32,
}

#[repr(C)]
#[derive(Clone, Copy)]
pub struct SrxHarmonyInfo {      // `srx_harmony_info`
    pub n: u64,
    pub d: u32,
    pub n_batches: u32,
    pub n_clusters: u32,
    pub n_blocks: u32,
    pub rounds: u32,
    pub converged: u32,
    pub cluster_iters: u64,
    pub round_iters: [u32; SRX_HARMONY_MAX_ROUNDS as usize],
    pub round_objective: [f64; SRX_HARMONY_MAX_ROUNDS as usize],
    pub ms: f64,
}

#[repr(C)]
#[derive(Clone, Copy)]
pub struct SrxBbknnOpts {      // `srx_bbknn_opts`
    pub neighbors_within_batch: i32,
    pub n_dims: i32,
    pub trim: i64,
}

#[repr(C)]
#[derive(Clone, Copy)]
pub struct SrxTrimInfo {      // `srx_trim_info`
    pub trim: u64,
    pub rows_over_trim: u64,
    pub nnz_before: u64,
    pub nnz_after: u64,
    pub entries_trimmed: u64,
    pub max_row_nnz_before: u64,
    pub max_row_nnz_after: u64,
    pub rows_emptied: u64,
    pub wave_capacity: u32,
    pub short_capacity: u32,
    pub reserved: [u32; 2 as usize],
    pub rows_wave: u64,
    pub rows_short: u64,
    pub rows_long: u64,
}

#[repr(C)]
#[derive(Clone, Copy)]
pub struct SrxBbknnInfo {      // `srx_bbknn_info`
    pub n: u64,
    pub n_batches: u32,
    pub neighbors_within_batch: u32,
    pub k: u32,
    pub d: u32,
    pub min_batch_cells: u64,
    pub max_batch_cells: u64,
    pub n_searches: u32,
    pub reserved: u32,
    pub pairs_searched: u64,
    pub rows_certified: u64,
    pub rows_recomputed: u64,
    pub trim: SrxTrimInfo,
    pub ms: f64,
    pub ms_sort: f64,
    pub ms_search: f64,
    pub ms_merge: f64,
    pub ms_graph: f64,
    pub ms_trim: f64,
}

#[repr(C)]
#[derive(Clone, Copy)]
pub struct SrxDoubletOpts {      // `srx_doublet_opts`
    pub sim_ratio: f64,
    pub expected_rate: f64,
    pub stdev_rate: f64,
    pub target_sum: f64,
    pub threshold: f64,
    pub seed: u64,
    pub k: i32,
    pub n_dims: i32,
    pub transform: i32,
    pub reserved: i32,
}

#[repr(C)]
#[derive(Clone, Copy)]
pub struct SrxDoubletInfo {      // `srx_doublet_info`
    pub n_obs: u64,
    pub n_sim: u64,
    pub nnz_sim: u64,
    pub k: u32,
    pub k_adj: u32,
    pub d: u32,
    pub threshold_found: u32,
    pub threshold: f64,
    pub smooth_rounds: u32,
    pub reserved: u32,
    pub n_predicted: u64,
    pub detected_rate: f64,
    pub detectable_fraction: f64,
    pub overall_rate: f64,
    pub rows_certified: u64,
    pub rows_recomputed: u64,
    pub ms_simulate: f64,
    pub ms_project: f64,
    pub ms_knn: f64,
    pub ms_score: f64,
}

#[repr(C)]
#[derive(Clone, Copy)]
pub struct SrxIterateArgs {      // `srx_iterate_args`
    pub k: i32,
    pub n: i32,
    pub l_act: i32,
    pub n_pc: i32,
    pub n_want: i32,
    pub d: i32,
    pub variant: i32,
    pub flags: i32,
    pub off_tol2: f64,
    pub c: *mut f64,
    pub blk: [*mut f64; 5 as usize],
    pub sm: [*mut f64; 2 as usize],
    pub vec: [*mut f64; 3 as usize],
    pub xi: *mut f64,
    pub out: [f64; 8 as usize],
    pub status: [i32; 2 as usize],
    pub tail_touched: i32,
    pub reserved: i32,
}

#[repr(C)]
#[derive(Clone, Copy)]
pub struct SrxSelectArgs {      // `srx_select_args`
    pub G: u64,
    pub take: u64,
    pub n_cells: u64,
    pub op: i32,
    pub route: i32,
    pub center: i32,
    pub scale: i32,
    pub flags: i32,
    pub reserved: i32,
    pub cnt: *const u64,
    pub sum: *const f64,
    pub sq: *const f64,
    pub genes: *const u64,
    pub var: *mut f64,
    pub rank: *mut u32,
    pub sel_rank: *mut i32,
    pub bits: *mut u32,
    pub prefix: *mut u32,
    pub mu: *mut f64,
    pub sd: *mut f64,
    pub dinv: *mut f64,
    pub trace: f64,
    pub counter: u32,
    pub status: i32,
    pub tail_touched: i32,
    pub reserved2: i32,
}

#[repr(C)]
#[derive(Clone, Copy)]
pub struct SrxPipelineResult {      // `srx_pipeline_result`
    pub pca: SrxPcaInfo,
    pub ms_normalize: f64,
    pub ms_moments: f64,
    pub ms_select: f64,
    pub ms_compact: f64,
    pub ms_pca: f64,
}

pub type SrxHostAllreduceFn = extern "C" fn(user: *mut c_void, buf: *mut f64, count: u64) -> i32;      // `srx_host_allreduce_fn`

#[link(name = "srx_hip")]
extern "C" {
    pub fn srx_abi_version() -> i32;
    pub fn srx_device_count(n_out: *mut i32) -> i32;
    pub fn srx_ctx_create(device_id: i32, out: *mut *mut SrxCtx) -> i32;
    pub fn srx_ctx_destroy(ctx: *mut SrxCtx);
    pub fn srx_ctx_synchronize(ctx: *mut SrxCtx) -> i32;
    pub fn srx_last_error(ctx: *const SrxCtx) -> *const c_char;
    pub fn srx_comm_unique_id(id_out_128: *mut c_void) -> i32;
    pub fn srx_comm_init(ctx: *mut SrxCtx, n_ranks: i32, rank: i32, id_128: *const c_void) -> i32;
    pub fn srx_comm_init_host(ctx: *mut SrxCtx, n_ranks: i32, rank: i32, fn_: SrxHostAllreduceFn, user: *mut c_void) -> i32;
    pub fn srx_comm_destroy(ctx: *mut SrxCtx) -> i32;
    pub fn srx_comm_info(ctx: *mut SrxCtx, kind_out: *mut i32, n_ranks_out: *mut i32, rccl_version_out: *mut i32,
                         ranks_seen_out: *mut i32) -> i32;
    pub fn srx_comm_overlap_info(ctx: *mut SrxCtx, split_exchanges_out: *mut i32, cu_masked_out: *mut i32) -> i32;
    pub fn srx_gram_mode_info(ctx: *mut SrxCtx, mode_out: *mut i32) -> i32;
    pub fn srx_gram_exchange_ranges(k: u64, offsets_out: *mut u64) -> i32;
    pub fn srx_partition_rows(indptr: *const u64, n_rows: u64, n_ranks: i32, cut_out: *mut u64) -> i32;
    pub fn srx_matrix_upload(ctx: *mut SrxCtx, host: *const SrxCsr, store: i32, out: *mut *mut SrxMat) -> i32;
    pub fn srx_matrix_upload_csc(ctx: *mut SrxCtx, host: *const SrxCsr, store: i32, out: *mut *mut SrxMat) -> i32;
    pub fn srx_matrix_format(m: *const SrxMat, format_out: *mut i32) -> i32;
    pub fn srx_matrix_to_csr(m: *mut SrxMat, out: *mut *mut SrxMat) -> i32;
    pub fn srx_matrix_to_csc(m: *mut SrxMat, out: *mut *mut SrxMat) -> i32;
    pub fn srx_matrix_alloc(ctx: *mut SrxCtx, n_rows: u64, n_cols: u64, nnz: u64, dtype: i32, store: i32,
                            out: *mut *mut SrxMat) -> i32;
    pub fn srx_matrix_device_ptrs(m: *mut SrxMat, indptr: *mut *mut c_void, indices: *mut *mut c_void,
                                  values: *mut *mut c_void) -> i32;
    pub fn srx_matrix_info(m: *const SrxMat, out: *mut SrxMatInfo) -> i32;
    pub fn srx_matrix_set_shard(m: *mut SrxMat, row_offset: u64) -> i32;
    pub fn srx_matrix_download_values(m: *mut SrxMat, values_out: *mut c_void, dtype_out: i32) -> i32;
    pub fn srx_matrix_prepare(m: *mut SrxMat) -> i32;
    pub fn srx_matrix_reserve_results(m: *mut SrxMat, n_selected: u64, n_components: i32) -> i32;
    pub fn srx_matrix_clone(m: *mut SrxMat, out: *mut *mut SrxMat) -> i32;
    pub fn srx_matrix_copy_values(dst: *mut SrxMat, src: *const SrxMat) -> i32;
    pub fn srx_matrix_free(m: *mut SrxMat);
    pub fn srx_compute_number(m: *mut SrxMat, direction: i32, out: *mut u32) -> i32;
    pub fn srx_compute_sum(m: *mut SrxMat, direction: i32, out: *mut f64) -> i32;
    pub fn srx_compute_variance(m: *mut SrxMat, direction: i32, out: *mut f64) -> i32;
    pub fn srx_compute_std_dev(m: *mut SrxMat, direction: i32, out: *mut f64) -> i32;
    pub fn srx_compute_min_max(m: *mut SrxMat, direction: i32, min_out: *mut f64, max_out: *mut f64) -> i32;
    pub fn srx_compute_qc_variables(m: *mut SrxMat, num_per_cell: *mut u32, num_per_gene: *mut u32,
                                    expr_per_gene: *mut f64, expr_per_cell: *mut f64, variance_per_gene: *mut f64,
                                    variance_per_cell: *mut f64, std_dev_per_cell: *mut f64,
                                    std_dev_per_gene: *mut f64) -> i32;
    pub fn srx_gene_moments(m: *mut SrxMat, cnt: *mut u64, sum: *mut f64, sumsq: *mut f64) -> i32;
    pub fn srx_filter_cells(m: *mut SrxMat, lower: SrxFlex, upper: SrxFlex, out: *mut *mut SrxMat, mask_out: *mut u8) -> i32;
    pub fn srx_filter_genes(m: *mut SrxMat, lower: SrxFlex, upper: SrxFlex, out: *mut *mut SrxMat, mask_out: *mut u8) -> i32;
    pub fn srx_subset(m: *mut SrxMat, row_mask: *const u8, col_mask: *const u8, out: *mut *mut SrxMat) -> i32;
    pub fn srx_matrix_download_pattern(m: *mut SrxMat, indptr_out: *mut u64, indices_out: *mut u64) -> i32;
    pub fn srx_normalize_total_inplace(m: *mut SrxMat, target_sum: f64, direction: i32) -> i32;
    pub fn srx_log1p_inplace(m: *mut SrxMat) -> i32;
    pub fn srx_normalize_log1p_inplace(m: *mut SrxMat, target_sum: f64, row_sums_out: *mut f64) -> i32;
    pub fn srx_select_hvg(m: *mut SrxMat, n: u64, idx_out: *mut u64, n_out: *mut u64) -> i32;
    pub fn srx_pearson_gene_variance(m: *mut SrxMat, opts: *const SrxPearsonOpts, var_out: *mut f64,
                                     info: *mut SrxPearsonInfo) -> i32;
    pub fn srx_select_hvg_pearson(m: *mut SrxMat, n: u64, opts: *const SrxPearsonOpts, idx_out: *mut u64,
                                  n_out: *mut u64, var_out: *mut f64, info: *mut SrxPearsonInfo) -> i32;
    pub fn srx_pearson_residuals(m: *mut SrxMat, genes: *const u64, k: u64, opts: *const SrxPearsonOpts,
                                 out: *mut f64, info: *mut SrxPearsonInfo) -> i32;
    pub fn srx_pca(m: *mut SrxMat, sel: *const u64, k: u64, opts: *const SrxPcaOpts, scores: *mut f64,
                   components: *mut f64, evr: *mut f64, mean: *mut f64, std: *mut f64, info: *mut SrxPcaInfo) -> i32;
    pub fn srx_pca_loadings(components: *const f64, std: *const f64, sel: *const u64, k: u64, n_pc: u64,
                            n_vars: u64, out: *mut f64) -> i32;
    pub fn srx_pca_pearson(m: *mut SrxMat, genes: *const u64, k: u64, opts: *const SrxPearsonPcaOpts,
                           scores: *mut f64, components: *mut f64, evr: *mut f64, mean: *mut f64,
                           info: *mut SrxPearsonPcaInfo) -> i32;
    pub fn srx_pearson_gram(m: *mut SrxMat, genes: *const u64, k: u64, opts: *const SrxPearsonPcaOpts,
                            gram_out: *mut f64, colsum_out: *mut f64, info: *mut SrxPearsonPcaInfo) -> i32;
    pub fn srx_regress_fit(m: *mut SrxMat, genes: *const u64, k: u64, cov: *const f64, p: u64,
                           opts: *const SrxRegressOpts, beta_out: *mut f64, xbar_out: *mut f64, sd_out: *mut f64,
                           info: *mut SrxRegressInfo) -> i32;
    pub fn srx_regress_sums(m: *mut SrxMat, genes: *const u64, k: u64, cov: *const f64, p: u64,
                            opts: *const SrxRegressOpts, cbar_out: *mut f64, a_out: *mut f64, w_out: *mut f64,
                            info: *mut SrxRegressInfo) -> i32;
    pub fn srx_regress_residuals(m: *mut SrxMat, genes: *const u64, k: u64, cov: *const f64, p: u64,
                                 opts: *const SrxRegressOpts, out: *mut f64, info: *mut SrxRegressInfo) -> i32;
    pub fn srx_regress_gram(m: *mut SrxMat, genes: *const u64, k: u64, cov: *const f64, p: u64,
                            opts: *const SrxRegressOpts, gram_out: *mut f64, colsum_out: *mut f64,
                            info: *mut SrxRegressInfo) -> i32;
    pub fn srx_pca_regress(m: *mut SrxMat, genes: *const u64, k: u64, cov: *const f64, p: u64,
                           opts: *const SrxRegressOpts, scores: *mut f64, components: *mut f64, evr: *mut f64,
                           mean: *mut f64, sd: *mut f64, info: *mut SrxRegressInfo) -> i32;
    pub fn srx_gene_list_sums(m: *mut SrxMat, list_ptr: *const u64, list_genes: *const u64, n_lists: u64,
                              sum_out: *mut f64, cnt_out: *mut u32, info: *mut SrxGeneListInfo) -> i32;
    pub fn srx_score_genes_controls(gene_mean: *const f64, n_genes: u64, pool: *const u64, n_pool: u64,
                                    set_ptr: *const u64, set_genes: *const u64, n_sets: u64,
                                    opts: *const SrxScoreGenesOpts, ctrl_ptr_out: *mut u64,
                                    ctrl_genes_out: *mut u64, capacity: u64, cut_out: *mut u32) -> i32;
    pub fn srx_score_genes(m: *mut SrxMat, set_ptr: *const u64, set_genes: *const u64, n_sets: u64,
                           pool: *const u64, n_pool: u64, opts: *const SrxScoreGenesOpts, score_out: *mut f64,
                           ctrl_ptr_out: *mut u64, ctrl_genes_out: *mut u64, capacity: u64,
                           info: *mut SrxScoreGenesInfo) -> i32;
    pub fn srx_pca_model_from_result(m: *mut SrxMat, out: *mut *mut SrxPcaModel) -> i32;
    pub fn srx_pca_model_create(ctx: *mut SrxCtx, k: u64, n_pc: u64, components: *const f64, mean: *const f64,
                                std: *const f64, sel: *const u64, center: i32, scale: i32,
                                out: *mut *mut SrxPcaModel) -> i32;
    pub fn srx_pca_model_info(p: *const SrxPcaModel, k_out: *mut u64, n_pc_out: *mut u64, sel_out: *mut u64) -> i32;
    pub fn srx_pca_model_free(p: *mut SrxPcaModel);
    pub fn srx_pca_transform(p: *mut SrxPcaModel, q: *mut SrxMat, feat: *const u64, target_sum: f64,
                             transform: i32, scores_out: *mut f64) -> i32;
    pub fn srx_knn_result(m: *mut SrxMat, opts: *const SrxKnnOpts, indices_out: *mut u32, distances_out: *mut f64,
                          info: *mut SrxKnnInfo) -> i32;
    pub fn srx_knn_points(ctx: *mut SrxCtx, ref_: *const f64, n_ref: u64, query: *const f64, n_query: u64, d: u64,
                          opts: *const SrxKnnOpts, indices_out: *mut u32, distances_out: *mut f64,
                          info: *mut SrxKnnInfo) -> i32;
    pub fn srx_neighbors_result(m: *mut SrxMat, opts: *const SrxKnnOpts, knn_info: *mut SrxKnnInfo,
                                out: *mut *mut SrxGraph) -> i32;
    pub fn srx_neighbors_from_knn(ctx: *mut SrxCtx, indices: *const u32, distances: *const f64, n: u64, k: u32,
                                  out: *mut *mut SrxGraph) -> i32;
    pub fn srx_graph_info_get(g: *const SrxGraph, info: *mut SrxGraphInfo) -> i32;
    pub fn srx_graph_fetch(g: *mut SrxGraph, which: i32, indptr: *mut u64, indices: *mut u32, data: *mut f64) -> i32;
    pub fn srx_graph_fetch_scales(g: *mut SrxGraph, rho: *mut f64, sigma: *mut f64) -> i32;
    pub fn srx_graph_free(g: *mut SrxGraph);
    pub fn srx_snn_from_knn(ctx: *mut SrxCtx, indices: *const u32, distances: *const f64, n: u64, k: u32,
                            opts: *const SrxSnnOpts, info: *mut SrxSnnInfo, out: *mut *mut SrxGraph) -> i32;
    pub fn srx_snn_graph(g: *mut SrxGraph, opts: *const SrxSnnOpts, info: *mut SrxSnnInfo, out: *mut *mut SrxGraph) -> i32;
    pub fn srx_snn_min_shared(k: u32, include_self: i32, prune: f64, out: *mut u32) -> i32;
    pub fn srx_knn_index_result(m: *mut SrxMat, n_dims: i32, opts: *const SrxIvfOpts, out: *mut *mut SrxKnnIndex) -> i32;
    pub fn srx_knn_index_points(ctx: *mut SrxCtx, ref_: *const f64, n_ref: u64, d: u64, opts: *const SrxIvfOpts,
                                centroids: *const f64, out: *mut *mut SrxKnnIndex) -> i32;
    pub fn srx_knn_index_info_get(ix: *const SrxKnnIndex, info: *mut SrxIvfInfo) -> i32;
    pub fn srx_knn_index_fetch(ix: *mut SrxKnnIndex, centroids: *mut f64, list_offsets: *mut u64,
                               list_members: *mut u32) -> i32;
    pub fn srx_knn_index_search(ix: *mut SrxKnnIndex, query: *const f64, n_query: u64, opts: *const SrxKnnOpts,
                                n_probe: i32, indices_out: *mut u32, distances_out: *mut f64,
                                info: *mut SrxIvfSearchInfo) -> i32;
    pub fn srx_neighbors_index(ix: *mut SrxKnnIndex, opts: *const SrxKnnOpts, n_probe: i32,
                               info: *mut SrxIvfSearchInfo, out: *mut *mut SrxGraph) -> i32;
    pub fn srx_knn_index_free(ix: *mut SrxKnnIndex);
    pub fn srx_louvain(g: *mut SrxGraph, opts: *const SrxLouvainOpts, labels_out: *mut u32,
                       info: *mut SrxLouvainInfo) -> i32;
    pub fn srx_louvain_csr(ctx: *mut SrxCtx, indptr: *const u64, indices: *const u32, weights: *const f64, n: u64,
                           opts: *const SrxLouvainOpts, labels_out: *mut u32, info: *mut SrxLouvainInfo) -> i32;
    pub fn srx_graph_labels_fetch(g: *mut SrxGraph, labels_out: *mut u32) -> i32;
    pub fn srx_group_moments(m: *mut SrxMat, labels: *const u32, n_groups: u32, n_cells_out: *mut u64,
                             cnt_out: *mut u64, sum_out: *mut f64, sumsq_out: *mut f64) -> i32;
    pub fn srx_rank_genes_groups(m: *mut SrxMat, labels: *const u32, n_groups: u32, opts: *const SrxRankGenesOpts,
                                 out: *mut *mut SrxMarkers) -> i32;
    pub fn srx_rank_genes_groups_graph(m: *mut SrxMat, g: *mut SrxGraph, opts: *const SrxRankGenesOpts,
                                       out: *mut *mut SrxMarkers) -> i32;
    pub fn srx_markers_info_get(mk: *const SrxMarkers, info: *mut SrxMarkersInfo) -> i32;
    pub fn srx_markers_fetch_top(mk: *mut SrxMarkers, genes_out: *mut u32, scores_out: *mut f64, lfc_out: *mut f64) -> i32;
    pub fn srx_markers_fetch_table(mk: *mut SrxMarkers, which: i32, out: *mut c_void) -> i32;
    pub fn srx_markers_fetch_sizes(mk: *mut SrxMarkers, n_cells_out: *mut u64) -> i32;
    pub fn srx_markers_free(mk: *mut SrxMarkers);
    pub fn srx_rank_genes_wilcoxon(m: *mut SrxMat, labels: *const u32, n_groups: u32, opts: *const SrxWilcoxonOpts,
                                   out: *mut *mut SrxMarkers) -> i32;
    pub fn srx_rank_genes_wilcoxon_graph(m: *mut SrxMat, g: *mut SrxGraph, opts: *const SrxWilcoxonOpts,
                                         out: *mut *mut SrxMarkers) -> i32;
    pub fn srx_markers_fetch_ties(mk: *mut SrxMarkers, out: *mut u64) -> i32;
    pub fn srx_markers_wilcoxon_info_get(mk: *const SrxMarkers, info: *mut SrxWilcoxonInfo) -> i32;
    pub fn srx_select_hvg_seurat_v3(m: *mut SrxMat, n_top: u64, batch: *const u32, n_batches: u32,
                                    opts: *const SrxSeuratV3Opts, idx_out: *mut u64, n_out: *mut u64,
                                    tables: *mut SrxSeuratV3Tables, info: *mut SrxSeuratV3Info) -> i32;
    pub fn srx_loess_direct(ctx: *mut SrxCtx, x: *const f64, y: *const f64, m: u64, span: f64, fitted_out: *mut f64) -> i32;
    pub fn srx_clipped_group_moments(m: *mut SrxMat, labels: *const u32, n_groups: u32, clip: *const f64,
                                     sum_out: *mut f64, sumsq_out: *mut f64, info: *mut SrxMarkersInfo) -> i32;
    pub fn srx_umap(g: *mut SrxGraph, m: *mut SrxMat, opts: *const SrxUmapOpts, init: *const f64,
                    embedding_out: *mut f64, info: *mut SrxUmapInfo) -> i32;
    pub fn srx_umap_csr(ctx: *mut SrxCtx, indptr: *const u64, indices: *const u32, weights: *const f64, n: u64,
                        opts: *const SrxUmapOpts, init: *const f64, embedding_out: *mut f64, info: *mut SrxUmapInfo) -> i32;
    pub fn srx_graph_embedding_fetch(g: *mut SrxGraph, out: *mut f64, dim_out: *mut u32) -> i32;
    pub fn srx_umap_fit_ab(spread: f64, min_dist: f64, a: *mut f64, b: *mut f64) -> i32;
    pub fn srx_umap_transform_knn(ctx: *mut SrxCtx, indices: *const u32, distances: *const f64, n_query: u64,
                                  kq: u32, ref_embedding: *const f64, n_ref: u64, dim: u32,
                                  opts: *const SrxUmapTransformOpts, out: *mut SrxUmapTransformOut,
                                  info: *mut SrxUmapTransformInfo) -> i32;
    pub fn srx_umap_transform_graph(g: *mut SrxGraph, indices: *const u32, distances: *const f64, n_query: u64,
                                    kq: u32, dim: u32, opts: *const SrxUmapTransformOpts,
                                    out: *mut SrxUmapTransformOut, info: *mut SrxUmapTransformInfo) -> i32;
    pub fn srx_knn_vote(ctx: *mut SrxCtx, indices: *const u32, n_query: u64, k: u32, ref_labels: *const u32,
                        n_ref: u64, n_groups: u32, labels_out: *mut u32, counts_out: *mut u32) -> i32;
    pub fn srx_knn_vote_graph(g: *mut SrxGraph, indices: *const u32, n_query: u64, k: u32, labels_out: *mut u32,
                              counts_out: *mut u32) -> i32;
    pub fn srx_tsne_affinities_knn(ctx: *mut SrxCtx, indices: *const u32, distances: *const f64, n: u64, k: u32,
                                   perplexity: f64, out: *mut *mut SrxTsne) -> i32;
    pub fn srx_tsne_affinities_graph(g: *mut SrxGraph, perplexity: f64, out: *mut *mut SrxTsne) -> i32;
    pub fn srx_tsne_info_get(h: *const SrxTsne, info: *mut SrxTsneInfo) -> i32;
    pub fn srx_tsne_fetch_affinities(h: *mut SrxTsne, indptr: *mut u64, indices: *mut u32, data: *mut f64,
                                     beta: *mut f64) -> i32;
    pub fn srx_tsne_forces(h: *mut SrxTsne, Y: *const f64, theta: f64, levels: i32, attr_out: *mut f64,
                           rep_out: *mut f64, z_out: *mut f64, info: *mut SrxTsneForceInfo) -> i32;
    pub fn srx_tsne_run(h: *mut SrxTsne, m: *mut SrxMat, opts: *const SrxTsneOpts, init: *const f64,
                        embedding_out: *mut f64, info: *mut SrxTsneRunInfo) -> i32;
    pub fn srx_tsne_embedding_fetch(h: *mut SrxTsne, out: *mut f64) -> i32;
    pub fn srx_tsne_free(h: *mut SrxTsne);
    pub fn srx_draw_graph(g: *mut SrxGraph, opts: *const SrxFa2Opts, init: *const f64, layout_out: *mut f64,
                          info: *mut SrxFa2Info) -> i32;
    pub fn srx_draw_graph_csr(ctx: *mut SrxCtx, indptr: *const u64, indices: *const u32, weights: *const f64,
                              n: u64, opts: *const SrxFa2Opts, init: *const f64, layout_out: *mut f64,
                              info: *mut SrxFa2Info) -> i32;
    pub fn srx_graph_layout_fetch(g: *mut SrxGraph, out: *mut f64) -> i32;
    pub fn srx_draw_graph_forces(ctx: *mut SrxCtx, indptr: *const u64, indices: *const u32, weights: *const f64,
                                 n: u64, Y: *const f64, opts: *const SrxFa2Opts, rep_out: *mut f64,
                                 grav_out: *mut f64, attr_out: *mut f64, mass_out: *mut u32,
                                 info: *mut SrxFa2ForceInfo) -> i32;
    pub fn srx_fa2_speed(n: u64, S: f64, Tr: f64, jitter_tolerance: f64, speed: *mut f64, eff: *mut f64) -> i32;
    pub fn srx_diffmap(g: *mut SrxGraph, opts: *const SrxDiffmapOpts, evals_out: *mut f64, evecs_out: *mut f64,
                       info: *mut SrxDiffmapInfo) -> i32;
    pub fn srx_diffmap_csr(ctx: *mut SrxCtx, indptr: *const u64, indices: *const u32, weights: *const f64, n: u64,
                           opts: *const SrxDiffmapOpts, evals_out: *mut f64, evecs_out: *mut f64,
                           info: *mut SrxDiffmapInfo) -> i32;
    pub fn srx_graph_diffmap_fetch(g: *mut SrxGraph, evals: *mut f64, evecs: *mut f64, n_comps_out: *mut u32) -> i32;
    pub fn srx_graph_transitions_fetch(g: *mut SrxGraph, data: *mut f64) -> i32;
    pub fn srx_dpt(g: *mut SrxGraph, root: u64, cap: f64, pseudotime_out: *mut f64) -> i32;
    pub fn srx_dpt_from(ctx: *mut SrxCtx, evals: *const f64, evecs: *const f64, n: u64, m: u32, root: u64,
                        cap: f64, pseudotime_out: *mut f64) -> i32;
    pub fn srx_paga(g: *mut SrxGraph, labels: *const u32, n_groups: u32, t: *mut SrxPagaTables,
                    info: *mut SrxPagaInfo) -> i32;
    pub fn srx_paga_csr(ctx: *mut SrxCtx, indptr: *const u64, indices: *const u32, n: u64, labels: *const u32,
                        n_groups: u32, t: *mut SrxPagaTables, info: *mut SrxPagaInfo) -> i32;
    pub fn srx_paga_from_counts(counts: *const u64, sizes: *const u64, n_groups: u32, t: *mut SrxPagaTables,
                                info: *mut SrxPagaInfo) -> i32;
    pub fn srx_paga_init_positions(g: *mut SrxGraph, ctx: *mut SrxCtx, labels: *const u32, n: u64, n_groups: u32,
                                   connectivities: *const f64, pos: *const f64, dim: u32, seed: u64, out: *mut f64) -> i32;
    pub fn srx_autocorr(m: *mut SrxMat, g: *mut SrxGraph, opts: *const SrxAutocorrOpts, out: *mut SrxAutocorrOut,
                        info: *mut SrxAutocorrInfo) -> i32;
    pub fn srx_autocorr_csr(m: *mut SrxMat, indptr: *const u64, indices: *const u32, weights: *const f64, n: u64,
                            opts: *const SrxAutocorrOpts, out: *mut SrxAutocorrOut, info: *mut SrxAutocorrInfo) -> i32;
    pub fn srx_autocorr_scales(info: *mut SrxAutocorrInfo) -> i32;
    pub fn srx_autocorr_from_tables(sum_int: *const i64, sumsq_int: *const i64, dsum_int: *const i64,
                                    dsumsq_int: *const i64, cross_int: *const i64, n_genes: u64,
                                    info: *mut SrxAutocorrInfo, out: *mut SrxAutocorrOut) -> i32;
    pub fn srx_harmony_result(m: *mut SrxMat, batch: *const u32, n_batches: u32, opts: *const SrxHarmonyOpts,
                              out: *mut *mut SrxHarmony, info: *mut SrxHarmonyInfo) -> i32;
    pub fn srx_harmony_points(ctx: *mut SrxCtx, points: *const f64, n: u64, d: u64, batch: *const u32,
                              n_batches: u32, opts: *const SrxHarmonyOpts, out: *mut *mut SrxHarmony,
                              info: *mut SrxHarmonyInfo) -> i32;
    pub fn srx_harmony_fetch(h: *mut SrxHarmony, which: i32, out: *mut f64) -> i32;
    pub fn srx_harmony_info_get(h: *const SrxHarmony, info: *mut SrxHarmonyInfo) -> i32;
    pub fn srx_knn_harmony(h: *mut SrxHarmony, opts: *const SrxKnnOpts, indices_out: *mut u32,
                           distances_out: *mut f64, info: *mut SrxKnnInfo) -> i32;
    pub fn srx_neighbors_harmony(h: *mut SrxHarmony, opts: *const SrxKnnOpts, knn_info: *mut SrxKnnInfo,
                                 out: *mut *mut SrxGraph) -> i32;
    pub fn srx_harmony_free(h: *mut SrxHarmony);
    pub fn srx_bbknn_result(m: *mut SrxMat, batch: *const u32, n_batches: u32, opts: *const SrxBbknnOpts,
                            info: *mut SrxBbknnInfo, out: *mut *mut SrxGraph) -> i32;
    pub fn srx_bbknn_points(ctx: *mut SrxCtx, points: *const f64, n: u64, d: u64, batch: *const u32,
                            n_batches: u32, opts: *const SrxBbknnOpts, indices_out: *mut u32,
                            distances_out: *mut f64, info: *mut SrxBbknnInfo, out: *mut *mut SrxGraph) -> i32;
    pub fn srx_bbknn_harmony(h: *mut SrxHarmony, batch: *const u32, n_batches: u32, opts: *const SrxBbknnOpts,
                             info: *mut SrxBbknnInfo, out: *mut *mut SrxGraph) -> i32;
    pub fn srx_graph_trim(g: *mut SrxGraph, trim: i64, info: *mut SrxTrimInfo, out: *mut *mut SrxGraph) -> i32;
    pub fn srx_doublets_simulate(counts: *mut SrxMat, n_sim: u64, seed: u64, parents: *const u64,
                                 out: *mut *mut SrxMat, parents_out: *mut u64) -> i32;
    pub fn srx_doublet_scores_knn(ctx: *mut SrxCtx, indices: *const u32, n_obs: u64, n_sim: u64, k_adj: u32,
                                  expected_rate: f64, stdev_rate: f64, score_out: *mut f64, se_out: *mut f64) -> i32;
    pub fn srx_doublets_threshold(sim_scores: *const f64, n: u64, threshold_out: *mut f64, found_out: *mut i32,
                                  rounds_out: *mut u32) -> i32;
    pub fn srx_doublets_result(fitted: *mut SrxMat, counts: *mut SrxMat, opts: *const SrxDoubletOpts,
                               out: *mut *mut SrxDoublets, info: *mut SrxDoubletInfo) -> i32;
    pub fn srx_doublets_call(h: *mut SrxDoublets, threshold: f64, info: *mut SrxDoubletInfo) -> i32;
    pub fn srx_doublets_fetch(h: *mut SrxDoublets, which: i32, out: *mut c_void) -> i32;
    pub fn srx_doublets_info_get(h: *const SrxDoublets, info: *mut SrxDoubletInfo) -> i32;
    pub fn srx_doublets_free(h: *mut SrxDoublets);
    pub fn srx_spmm(m: *mut SrxMat, sel: *const u64, k: u64, panel: *const f64, y_out: *mut f64, t_out: *mut f64,
                    gram_out: *mut f64) -> i32;
    pub fn srx_iterate_op(ctx: *mut SrxCtx, op: i32, args: *mut SrxIterateArgs) -> i32;
    pub fn srx_select_op(ctx: *mut SrxCtx, args: *mut SrxSelectArgs) -> i32;
    pub fn srx_pipeline(m: *mut SrxMat, target_sum: f64, n_hvg: u64, opts: *const SrxPcaOpts,
                        res: *mut SrxPipelineResult) -> i32;
    pub fn srx_result_fetch(m: *mut SrxMat, scores: *mut f64, components: *mut f64, evr: *mut f64, mean: *mut f64,
                            std: *mut f64, hvg_idx: *mut u64) -> i32;
    pub fn srx_backed_create(ctx: *mut SrxCtx, n_cols: u64, store: i32, out: *mut *mut SrxBacked) -> i32;
    pub fn srx_backed_destroy(b: *mut SrxBacked);
    pub fn srx_backed_stats_tile(b: *mut SrxBacked, tile: *const SrxCsr, target_sum: f64, transform: i32,
                                 row_number_out: *mut u32, row_sum_out: *mut f64) -> i32;
    pub fn srx_backed_moments(b: *mut SrxBacked, cnt: *mut u64, sum: *mut f64, sumsq: *mut f64,
                              n_rows_global: *mut u64) -> i32;
    pub fn srx_backed_select(b: *mut SrxBacked, n_hvg: u64, sel: *const u64, n_sel: u64, opts: *const SrxPcaOpts,
                             sel_out: *mut u64, n_out: *mut u64) -> i32;
    pub fn srx_backed_gram_tile(b: *mut SrxBacked, tile: *const SrxCsr, target_sum: f64, transform: i32) -> i32;
    pub fn srx_backed_solve(b: *mut SrxBacked, info: *mut SrxPcaInfo) -> i32;
    pub fn srx_backed_fetch(b: *mut SrxBacked, scores: *mut f64, components: *mut f64, evr: *mut f64,
                            mean: *mut f64, std: *mut f64, sel: *mut u64) -> i32;
    pub fn srx_prof_enable(ctx: *mut SrxCtx, class_mask: u32) -> i32;
    pub fn srx_prof_reset(ctx: *mut SrxCtx) -> i32;
    pub fn srx_prof_get(ctx: *mut SrxCtx, kernel_class: i32, total_ms: *mut f64, launches: *mut u64,
                        algorithmic_bytes: *mut f64) -> i32;
    pub fn srx_prof_get_aux(ctx: *mut SrxCtx, kernel_class: i32, aux_bytes: *mut f64) -> i32;
}
