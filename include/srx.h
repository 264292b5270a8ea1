/*
 * srx.h — C ABI of libsrx_hip.so: the MI355X (gfx950) implementation of SingleRust's
 * sparse count-matrix hot path
 *
 *     normalize_total(1e4, Row) -> log1p -> per-gene moments / HVG(n) -> n_pc-component PCA
 *
 * This header IS the drop-in boundary.  The reference (SingleRust/SingleRust @ 2024_10_08,
 * pure Rust) has no FFI of its own; each entry point below replaces the body of one
 * reference function and is what a Rust shim in that function would bind (see
 * INTEGRATION.md for the `extern "C"` block and the shim).  Paths cite the reference as
 * <file>:<lines> relative to the reference repository root.
 *
 * Conventions
 *   - plain C types only; every function returns an srx_status (0 = ok, <0 = error) and
 *     never throws or aborts across the boundary; srx_last_error() gives the message the
 *     shim turns into anyhow!(..).
 *   - the caller owns every host buffer; the library never keeps a host pointer after a
 *     call returns.  An srx_mat owns device memory only.
 *   - one srx_ctx per process and GPU (one process per GPU); a ctx is not thread-safe —
 *     the reference holds the IMArrayElement RwLock for the whole op, the shim does too.
 *   - there is NO CPU fallback: without a usable HIP device every compute call fails with
 *     SRX_E_HIP.
 */
#ifndef SRX_H
#define SRX_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SRX_ABI_VERSION 6      /* 2: srx_matrix_reserve_results, kernel classes 7-9, srx_synth_params.skew; 3: kernel class 10;
                                  4: srx_comm_info, srx_prof_get_aux; 5: srx_comm_overlap_info; 6: srx_gram_mode_info, srx_gram_exchange_ranges.
                                  Purely additive entry points leave the version as it is and are detected by symbol:
                                  srx_pca_model_* / srx_pca_transform (fitted-PCA projection) and srx_knn_result /
                                  srx_knn_points (kernel class 11) came that way at 6, as did srx_neighbors_* / srx_graph_*
                                  (kernel class 12) and srx_louvain / srx_louvain_csr / srx_graph_labels_fetch (no class of
                                  their own: the time is in srx_louvain_info.ms) and srx_group_moments / srx_rank_genes_groups[_graph] /
                                  srx_markers_* (no class either: srx_markers_info.ms) and srx_diffmap[_csr] /
                                  srx_graph_diffmap_fetch / srx_graph_transitions_fetch / srx_dpt[_from] (srx_diffmap_info.ms) and
                                  srx_iterate_op (the dense solver's kernels one at a time: tests and diagnostics) and
                                  srx_select_op (the feature selection on host arrays, every route: tests and diagnostics) */

typedef struct srx_ctx srx_ctx;   /* one GPU + stream + (optional) RCCL communicator      */
typedef struct srx_mat srx_mat;   /* device-resident CSR (the `X` of an IMAnnData)        */

typedef enum srx_status {
    SRX_OK = 0,
    SRX_E_ARG = -1,      /* null pointer / inconsistent sizes                             */
    SRX_E_DTYPE = -2,    /* dtype outside match_dyn_csr_matrix! (src/shared/mod.rs:110-129) */
    SRX_E_FORMAT = -3,   /* "X is not a CSR matrix" (scale/mod.rs:87, transform/mod.rs:58) */
    SRX_E_BOUNDS = -4,   /* column index >= n_cols, selection index out of range          */
    SRX_E_HIP = -5,      /* HIP runtime error / no device                                 */
    SRX_E_RCCL = -6,
    SRX_E_OOM = -7,
    SRX_E_NAN = -8,      /* NaN variance in HVG ranking: partial_cmp().unwrap() panic,
                            dim_red/mod.rs:138                                            */
    SRX_E_SHAPE = -9,    /* pca_inplace needs k >= 2 and N >= 5 (dim_red/mod.rs:38-41)    */
    SRX_E_NOCONV = -10   /* subspace iteration hit max_iter before reaching tol           */
} srx_status;

/* Value dtypes: the set match_dyn_csr_matrix! accepts (src/shared/mod.rs:114-124).  The
 * variants it panics on (I64, U64, Usize, Bool, String) map to SRX_E_DTYPE. */
typedef enum srx_dtype {
    SRX_I8 = 0, SRX_I16 = 1, SRX_I32 = 2, SRX_U8 = 3, SRX_U16 = 4, SRX_U32 = 5,
    SRX_F32 = 6, SRX_F64 = 7
} srx_dtype;

/* src/shared/mod.rs:39-42 */
typedef enum srx_direction { SRX_ROW = 0, SRX_COLUMN = 1 } srx_direction;

/* The reference data model: nalgebra_sparse::CsrMatrix<T> slices as the
 * shim obtains them under the IMArrayElement guard — row_offsets(), col_indices(),
 * values()/values_mut().  usize == uint64_t on x86-64. */
typedef struct srx_csr {
    uint64_t n_rows, n_cols, nnz;
    const uint64_t* indptr;    /* n_rows + 1                                              */
    const uint64_t* indices;   /* nnz; sorted and unique within a row (canonical CSR)     */
    void* values;              /* nnz elements of `dtype`                                  */
    int32_t dtype;             /* srx_dtype                                               */
} srx_csr;

/* Device value storage chosen at upload. AUTO: I8/I16/U8/U16/F32 -> f32 (exact), I32/U32/
 * F64 -> f64 — and the storage then FOLLOWS the reference's variant: where the reference turns X
 * into DynCsrMatrix::F64 (normalize_total on anything, log1p on a non-F32 matrix:
 * scale/mod.rs:74-83, transform/mod.rs:48-55) an AUTO handle held in f32 is widened to f64, under
 * the separate calls and under srx_pipeline alike; srx_matrix_copy_values on an AUTO destination
 * follows the source's storage.  An explicit F32 keeps f32 throughout: half the HBM traffic of
 * every pass, still within the 1e-5 bound; F64 reproduces the reference's f64 arithmetic to ~1e-15. */
typedef enum srx_store { SRX_STORE_AUTO = 0, SRX_STORE_F32 = 1, SRX_STORE_F64 = 2 } srx_store;

/* ---- context ---------------------------------------------------------------------------- */
int32_t srx_abi_version(void);
int32_t srx_device_count(int32_t* n_out);
int32_t srx_ctx_create(int32_t device_id, srx_ctx** out);
void    srx_ctx_destroy(srx_ctx* ctx);
int32_t srx_ctx_synchronize(srx_ctx* ctx);
/* Message of the last failing call on this ctx (or, with ctx == NULL, on this thread). */
const char* srx_last_error(const srx_ctx* ctx);

/* ---- row sharding over the GPUs of one node (new; the reference is single-process) ------
 * One process per GPU.  Rank 0 obtains an id, the host broadcasts the 128 bytes by any
 * means (torch.distributed / MPI / a file), every rank calls srx_comm_init.  Afterwards
 * every per-gene reduction (moments, Z^T Y blocks, Gram matrices, the global cell count)
 * is summed across ranks with ONE ncclAllReduce(f64, sum) each over xGMI; per-cell results
 * stay local to the rank that owns the rows.  Entry points whose answer would be the shard's own
 * rather than the matrix's refuse a sharded context with SRX_E_ARG: srx_filter_cells /
 * srx_filter_genes with a FlexValue::Relative limit (a quantile of all cells' / genes' sums) and
 * srx_compute_min_max(Column); CSC handles are single-rank. */
#define SRX_UNIQUE_ID_BYTES 128
int32_t srx_comm_unique_id(void* id_out_128);
int32_t srx_comm_init(srx_ctx* ctx, int32_t n_ranks, int32_t rank, const void* id_128);
/* Alternative to srx_comm_init for hosts that already own a transport (MPI, sockets): every
 * cross-rank sum of the path (3G+1 doubles of moments, the packed Gram tiles or the k x 64 block,
 * 64 x 64 blocks) is handed to `fn` as a host buffer to be summed over all ranks IN PLACE
 * (return 0 on success).  Collective calls must be made by all ranks in the same order. */
typedef int32_t (*srx_host_allreduce_fn)(void* user, double* buf, uint64_t count);
int32_t srx_comm_init_host(srx_ctx* ctx, int32_t n_ranks, int32_t rank, srx_host_allreduce_fn fn, void* user);
int32_t srx_comm_destroy(srx_ctx* ctx);
/* What the context's cross-rank sums go through: *kind_out = 0 (no communicator), 1 (RCCL), 2 (host transport);
 * *rccl_version_out = ncclGetVersion() (0 when RCCL is not loaded); *ranks_seen_out = a 1.0 summed over the
 * communicator with the same all-reduce the path uses (a COLLECTIVE call when kind != 0: every rank makes it) —
 * equal to n_ranks when every rank really takes part.  Any out pointer may be NULL. */
int32_t srx_comm_info(srx_ctx* ctx, int32_t* kind_out, int32_t* n_ranks_out, int32_t* rccl_version_out,
                      int32_t* ranks_seen_out);
/* How the Gram solver's one exchange has been run on this context so far: *split_exchanges_out = the number of Gram
 * matrices whose packed triangle went round the ranks in three pieces, two of them UNDER the second half of the stripe
 * kernel (the arrangement of a multi-rank RCCL context); *cu_masked_out = 1 when that second half ran on a stream whose
 * CU mask keeps it off the CUs left to the collective (0: the mask could not be set, or no split exchange yet).
 * Introspection for tests and the bench line; either pointer may be NULL. */
int32_t srx_comm_overlap_info(srx_ctx* ctx, int32_t* split_exchanges_out, int32_t* cu_masked_out);
/* Which accumulation mode the LAST sparse Gram launch of this context ran in (the kernel decides on the device, from value
 * statistics of the compacted matrix — summed over the ranks first when the rows are sharded, so that every rank takes the
 * same mode): *mode_out = 0 (no launch yet), 1 (f64 LDS atomics), 2 (fixed-point products, 64-bit integer LDS atomics:
 * non-negative values whose binary exponents lie within 6 of the largest's).  Drains the stream.  Introspection for tests. */
int32_t srx_gram_mode_info(srx_ctx* ctx, int32_t* mode_out);
/* The Gram solver's one exchange when the rows are sharded over RCCL ranks: the packed upper triangle of X_sel^T X_sel
 * (k (k + 1) / 2 doubles, row-major) is summed in THREE all-reduces — offsets_out[0] .. [1] and [2] .. [3] first (under the
 * second half of the stripe kernel), [1] .. [2] after it; offsets_out[3] = k (k + 1) / 2.  The ranges depend on k alone (every
 * rank, with or without rows, issues the same three calls).  Pure host helper, no GPU needed. */
int32_t srx_gram_exchange_ranges(uint64_t k, uint64_t* offsets_out);
/* Contiguous nnz-balanced row ranges: cut[r]..cut[r+1] is rank r's rows (cut has
 * n_ranks+1 entries).  Pure host helper, no GPU needed. */
int32_t srx_partition_rows(const uint64_t* indptr, uint64_t n_rows, int32_t n_ranks,
                           uint64_t* cut_out);

/* ---- matrix ------------------------------------------------------------------------------ */
/* Narrowing upload of a reference-layout CSR (u64 -> i32 column indices on device, i64 row
 * offsets).  Validates sortedness/bounds on device (SRX_E_FORMAT / SRX_E_BOUNDS).
 * The indices are narrowed on the HOST side of the link by the transfer workers (to 16 bits
 * when n_cols <= 65536: 2 of their 8 bytes cross PCIe); the host buffers may be pageable or
 * pinned (hipHostMalloc / hipHostRegister: values of the storage type are then copied by one
 * DMA straight out of them).  The call returns when every host buffer has been read. */
int32_t srx_matrix_upload(srx_ctx* ctx, const srx_csr* host, int32_t store, srx_mat** out);
/* CSC storage (ArrayData::CscMatrix / DynCscMatrix): `host` describes X (n_rows cells x n_cols
 * genes) with indptr = col_offsets[n_cols+1], indices = row_indices[nnz] (sorted per column).
 * Replaces the CSC arms of the reference: src/shared/statistics/helper/csc.rs:15-216,
 * scale_row_csc / scale_col_csc (src/memory/processing/scale/mod.rs:25-57,104-139), log1p on a
 * CSC matrix, convert_to_array_f64_csc[_selected] (src/shared/mod.rs:204-215,261-290) for the PCA.
 * Every entry point that takes an srx_mat accepts the handle and follows the reference's CSC
 * arithmetic (e.g. compute_variance(Column) is the two-pass form with NaN for an empty gene,
 * csc.rs:164-177); srx_matrix_info reports the shape of X; srx_matrix_download_pattern / _values
 * return the CSC arrays.  srx_pca / srx_pipeline transpose on the device first.  Not available
 * on a CSC handle: srx_gene_moments, srx_spmm, multi-rank contexts (shard by cells = CSR rows). */
int32_t srx_matrix_upload_csc(srx_ctx* ctx, const srx_csr* host, int32_t store, srx_mat** out);
enum { SRX_FORMAT_CSR = 0, SRX_FORMAT_CSC = 1 };
int32_t srx_matrix_format(const srx_mat* m, int32_t* format_out);
/* Storage conversion on the device (a copy; the input is left as it is).  The copy keeps the input's dtype and value
 * storage, SRX_STORE_AUTO included: f32 storage of an AUTO matrix still widens to f64 at normalize_total.  The row-ordering
 * pass holds a bitmap of the input's STORED rows in LDS: more than 655,360 of them (cells of a CSR input, genes of a CSC
 * one) are refused with SRX_E_ARG. */
int32_t srx_matrix_to_csr(srx_mat* m, srx_mat** out);
int32_t srx_matrix_to_csc(srx_mat* m, srx_mat** out);
/* Uninitialised device CSR for producers that fill HBM directly (synthetic generator, a
 * host that already holds device buffers). `dtype` is the logical dtype the values are
 * deemed to have (what DynCsrMatrix variant X is). */
int32_t srx_matrix_alloc(srx_ctx* ctx, uint64_t n_rows, uint64_t n_cols, uint64_t nnz,
                         int32_t dtype, int32_t store, srx_mat** out);
/* Device pointers of an srx_mat: indptr = int64[n_rows+1], indices = int32[nnz],
 * values = float[nnz] or double[nnz] (see srx_matrix_info). */
int32_t srx_matrix_device_ptrs(srx_mat* m, void** indptr, void** indices, void** values);
typedef struct srx_mat_info {
    uint64_t n_rows, n_cols, nnz;  /* shape of X (cells x genes), CSR or CSC                  */
    int32_t dtype;        /* current LOGICAL dtype (F64 after normalize_total, ...)       */
    int32_t store;        /* SRX_STORE_F32 or SRX_STORE_F64                               */
    uint64_t row_offset;  /* global index of local row 0 (sharded runs)                   */
    uint64_t n_rows_global;
} srx_mat_info;
int32_t srx_matrix_info(const srx_mat* m, srx_mat_info* out);
/* Tell a shard where it sits in the global matrix (used for deterministic seeds only). */
int32_t srx_matrix_set_shard(srx_mat* m, uint64_t row_offset);
/* D2H of the current values, converted to SRX_F32 or SRX_F64 (what the shim copies back
 * into values_mut(), or into the fresh Vec<f64> when the DynCsrMatrix variant changes). */
int32_t srx_matrix_download_values(srx_mat* m, void* values_out, int32_t dtype_out);
/* Build the pattern-only index structures of the device layout now (the gene-tile cuts of every
 * row used by the per-gene passes) instead of lazily at first use; clones inherit them.  They
 * depend on indptr/indices only, never on the values. */
int32_t srx_matrix_prepare(srx_mat* m);
/* Allocate the handle's result block now (N x n_components f64 scores + the small results of a PCA over
 * n_selected features) instead of inside the first srx_pca / srx_pipeline on it: a pipeline step on a prepared
 * and reserved matrix makes no device allocation.  Clones inherit the reservation (each gets its own block). */
int32_t srx_matrix_reserve_results(srx_mat* m, uint64_t n_selected, int32_t n_components);
/* Deep copy on device (normalize_total / log1p_transform, the copying forms,
 * processing/mod.rs:314-322,329-332, deep_clone X). */
int32_t srx_matrix_clone(srx_mat* m, srx_mat** out);
/* Overwrite dst's values/dtype from src (same sparsity pattern); bench uses it to restore
 * raw counts between steps. */
int32_t srx_matrix_copy_values(srx_mat* dst, const srx_mat* src);
void    srx_matrix_free(srx_mat* m);

/* ---- statistics: memory::statistics::* (src/memory/statistics/mod.rs:10-46) ------------- */
/* compute_number -> csr.rs:16-38.  out: n_rows (Row) or n_cols (Column) u32. */
int32_t srx_compute_number(srx_mat* m, int32_t direction, uint32_t* out);
/* compute_sum -> csr.rs:81-102. f64 accumulate; exact for integer data. */
int32_t srx_compute_sum(srx_mat* m, int32_t direction, double* out);
/* compute_variance -> csr.rs:149-188. Column: variance over the NON-ZERO entries,
 * sumsq/cnt - mean^2, 0.0 when cnt == 0.  Row: two-pass, NaN for an empty row. */
int32_t srx_compute_variance(srx_mat* m, int32_t direction, double* out);
/* compute_std_dev -> csr.rs:225-228. */
int32_t srx_compute_std_dev(srx_mat* m, int32_t direction, double* out);
/* compute_min_max -> csr.rs:194-223 (+inf/-inf for empty). */
int32_t srx_compute_min_max(srx_mat* m, int32_t direction, double* min_out, double* max_out);
/* compute_qc_variables (statistics/mod.rs:48-72): the eight vectors of StatisticsContainer
 * (structs/mod.rs:1-10) from ONE pass over the rows (number, sum, variance per cell; NaN variance
 * for an empty cell, csr.rs:161) and ONE pass over the columns (the cached per-gene moments) — the
 * reference makes ~14 serial passes.  Per-cell outputs have n_rows entries, per-gene outputs n_cols;
 * any pointer may be NULL. */
int32_t srx_compute_qc_variables(srx_mat* m, uint32_t* num_per_cell, uint32_t* num_per_gene, double* expr_per_gene,
                                 double* expr_per_cell, double* variance_per_gene, double* variance_per_cell,
                                 double* std_dev_per_cell, double* std_dev_per_gene);
/* Superset used internally: per-gene (nnz_j, sum x, sum x^2) from ONE pass. Any output may
 * be NULL. */
int32_t srx_gene_moments(srx_mat* m, uint64_t* cnt, double* sum, double* sumsq);

/* ---- QC filters: memory::processing::filter_cells / filter_genes (processing/mod.rs:86-146, :245-299) -------
 * FlexValue (src/shared/mod.rs:62-66): Absolute(u32) thresholds the nnz COUNT of the cell / gene, Relative(p)
 * the linear-interpolated p-quantile of the SUMS (calculate_percentiles, mod.rs:148-174), None = no limit; the
 * nine (lower, upper) combinations of create_filter_mask (mod.rs:33-84).  `*out` receives a NEW matrix holding
 * the kept rows / columns in their original order (the reference's `subset`; the in-place forms swap it in), in the
 * input's format, dtype and value storage (SRX_STORE_AUTO included, as srx_subset);
 * `mask_out` (n_rows resp. n_cols bytes, may be NULL) receives the boolean mask. */
enum { SRX_FLEX_NONE = 0, SRX_FLEX_ABSOLUTE = 1, SRX_FLEX_RELATIVE = 2 };
typedef struct srx_flex {
    int32_t kind;      /* SRX_FLEX_* */
    uint32_t absolute; /* FlexValue::Absolute(u32) */
    double relative;   /* FlexValue::Relative(f64), a quantile in [0, 1] */
} srx_flex;
int32_t srx_filter_cells(srx_mat* m, srx_flex lower, srx_flex upper, srx_mat** out, uint8_t* mask_out);
int32_t srx_filter_genes(srx_mat* m, srx_flex lower, srx_flex upper, srx_mat** out, uint8_t* mask_out);
/* anndata `subset` on X: boolean masks over rows / columns (NULL = keep all), order preserved.  The result keeps the
 * input's format, dtype and value storage; a matrix created with SRX_STORE_AUTO stays AUTO (its f32 storage widens to
 * f64 at normalize_total, like the reference's DynCsrMatrix::F64), as srx_matrix_clone. */
int32_t srx_subset(srx_mat* m, const uint8_t* row_mask, const uint8_t* col_mask, srx_mat** out);
/* Sparsity pattern back to the host in the reference's layout (u64 offsets / indices); either may be NULL. */
int32_t srx_matrix_download_pattern(srx_mat* m, uint64_t* indptr_out, uint64_t* indices_out);

/* ---- normalise / log1p: memory::processing::* ------------------------------------------- */
/* normalize_total_inplace (processing/mod.rs:303-312 -> scale/mod.rs:7-23,59-89;
 * Column: :91-107,141-173).  scale = (sum == 0) ? 0 : target/sum; v *= scale.  The logical
 * dtype becomes F64 whatever it was (scale/mod.rs:74-83). */
int32_t srx_normalize_total_inplace(srx_mat* m, double target_sum, int32_t direction);
/* log1p_transform_inplace (processing/mod.rs:324-326 -> transform/mod.rs:36-57). Logical
 * F32 stays F32 (f32::ln_1p), everything else becomes F64. */
int32_t srx_log1p_inplace(srx_mat* m);
/* Fused fast path of the two calls above with Direction::Row: one read + one write of the
 * values (8 B/nnz at f32 storage).  row_sums_out (host, n_rows f64) may be NULL. */
int32_t srx_normalize_log1p_inplace(srx_mat* m, double target_sum, double* row_sums_out);

/* ---- feature selection: dim_red::select_features, arm HighlyVariable(n)
 * (dim_red/mod.rs:135-140): stable descending sort of the nz-only gene variances, first n
 * gene indices IN RANK ORDER.  idx_out has room for min(n, n_cols) entries. */
int32_t srx_select_hvg(srx_mat* m, uint64_t n, uint64_t* idx_out, uint64_t* n_out);

/* ---- highly variable genes by analytic Pearson residuals (not in the reference) ---------------------------------------------
 * scanpy's experimental.pp.highly_variable_genes(flavor = "pearson_residuals") and normalize_pearson_residuals (Lause,
 * Berens & Kobak 2021) on RAW counts, before srx_normalize_log1p_inplace; additive, detected by symbol, no profiling class of
 * its own (the times are in srx_pearson_info).
 *
 * Definition.  X is n x G with non-negative entries, r_i its row sums (cells), g_j its column sums (genes), T = sum_i r_i (a
 * fixed-order f64 sum).  theta > 0 (+inf: Poisson) and the clip c >= 0 are the options.  For every pair (i, j), in f64, in this
 * order, without contraction and without fast-math:
 *      mu   = (r_i * g_j) / T
 *      s    = sqrt(mu + (mu * mu) / theta)          (theta = +inf: sqrt(mu))
 *      z_ij = min(max((x_ij - mu) / s, -c), c)      (mu == 0: z_ij = 0)
 *   v_j = (sum_i z_ij^2) / n - ((sum_i z_ij) / n)^2: the population variance over ALL n cells, zeros included (np.var).
 *   A gene with g_j = 0 has v_j = 0.0 exactly and is never selected; a cell with r_i = 0 has z = 0 for every gene and counts in
 *   n.  T = 0: every v_j is 0 and nothing is selected; that is no error.
 *   Selection: the first n genes with g_j > 0 by descending v_j, equal variances in ascending gene index, in rank order (the
 *   order of srx_select_hvg for any key array: the same ranking kernel).
 *   Defaults are scanpy's: theta == 0 in the option struct means 100, clip == 0 means sqrt(n_rows); clip = +inf: no clipping.
 * How v_j is summed.  A CSC handle (genes are its stored rows) evaluates z_ij of every pair of a gene as defined, zeros
 *   included, and sums z and z^2 over the cells in one fixed order, in f64 (sum_quantum = sq_quantum = 0).  A CSR handle makes
 *   S1_j = sum_i z_ij and S2_j = sum_i z_ij^2 each as the sum of a DENSE part over all n cells of the residual of a zero
 *   entry, f = -min(mu' / sqrt(mu' (1 + mu' / theta)), c) with mu' = r_i * (g_j / T), f^2 its square (cells in chunks, the
 *   chunks' partial sums added in ascending order), and a SPARSE correction over the stored entries of z - f and z^2 - f^2 (z
 *   as defined above), kept in 64-bit fixed point (integer atomics: exact in any order) with
 *      b = min(c, sqrt(T)),   sum_quantum = 2^(ceil(log2(2 n b)) - 61),   sq_quantum = 2^(ceil(log2(n b b)) - 61)
 *   (|z| <= b for non-negative X: x <= r_i and x <= g_j give mu >= x^2 / T), each no finer than 2^-200; every stored entry adds
 *   at most half a quantum of error to its gene's sum.  No floating-point atomics: results are bit-identical from call to call,
 *   and two identical columns get bit-identical variances wherever they sit.
 * Departures from scanpy: scanpy yields NaN for an empty cell (here 0) and leaves ties to an unstable argsort (here: gene
 *   index); batch_key (median rank over batches) is not built for this flavour (srx_select_hvg_seurat_v3 below has it).
 * All three calls accept CSR and CSC handles at either value storage and any dtype, leave the handle as it was (values,
 *   logical dtype; the moments cache is filled with the moments of the current values if it was empty) and compute on the
 *   device only.  Non-integer values are accepted.
 * Refused with SRX_E_ARG and a message, nothing written: a NULL handle or output (opts, info and the var_out of
 *   srx_select_hvg_pearson may be NULL); theta negative or NaN; clip negative or NaN; a gene index >= n_cols; a negative, NaN
 *   or infinite stored value (found on the device by the pass that reads the values first); a context with more than one rank;
 *   a context with an open backed session (sharded and out-of-core forms are out of scope). */
typedef struct srx_pearson_opts { double theta; double clip; } srx_pearson_opts;          /* NULL = {0, 0} */
typedef struct srx_pearson_info {
    uint64_t n_cells, n_genes, n_expressed /* g_j > 0 */, n_empty_cells;
    double   total, theta, clip;           /* T and the values actually used */
    double   sum_quantum, sq_quantum;      /* 0 unless the sparse sums are kept in fixed point: their resolution */
    double   ms_dense, ms_sparse, ms_rank;
} srx_pearson_info;
/* v_j of every gene (var_out: n_cols f64, host). */
int32_t srx_pearson_gene_variance(srx_mat* m, const srx_pearson_opts* opts, double* var_out /* n_cols */, srx_pearson_info* info);
/* The selection: idx_out has room for min(n, n_cols) entries, *n_out = min(n, n_expressed) of them are written. */
int32_t srx_select_hvg_pearson(srx_mat* m, uint64_t n, const srx_pearson_opts* opts, uint64_t* idx_out, uint64_t* n_out,
                               double* var_out /* n_cols, may be NULL */, srx_pearson_info* info);
/* The clipped residuals z_ij of the listed genes (any order, repeats allowed), all cells, zeros included: scanpy's
 * normalize_pearson_residuals restricted to a gene list.  Made on the device in chunks of rows of at most 1 GiB.  The timing
 * and quantum fields of info are 0. */
int32_t srx_pearson_residuals(srx_mat* m, const uint64_t* genes, uint64_t k, const srx_pearson_opts* opts,
                              double* out /* host, n_rows x k row-major */, srx_pearson_info* info);

/* ---- PCA: dim_red::pca_inplace (dim_red/mod.rs:24-94); arithmetic spec
 * src/shared/processing/pca/mod.rs:74-215.  Computed by randomized block subspace
 * iteration on the implicit standardised matrix Z = (X[:, sel] - 1 mu^T) D^-1 with a
 * CSR x dense-panel SpMM (forward) and its transpose, or — Gram solver — with X_sel^T X_sel
 * accumulated once from the sparse rows; never densifies X.  Between Rayleigh–Ritz steps the
 * block is advanced by Chebyshev filters of C = Z^T Z (plain powers during the warm-up); the
 * whole iteration runs on the device (SRX_NO_GRAPH=1 / SRX_NO_CHEB=1 / SRX_PCA_TRACE=1 in the
 * environment: no hipGraph replay / plain sweeps instead of filters / residual trace on stderr).
 * Hard spectra (a few strong components over a flat bulk) are handled by bounding the filter
 * degree, by deflation rounds of <= 32 components when one round stalls, and by a last-resort
 * mode (CholeskyQR3 after every application of C; SRX_PCA_ROBUST=1 forces it): SRX_E_NOCONV is
 * left for a zero matrix, NaN input or an exhausted max_iter.  n_components beyond the structural
 * rank bound min(k, N - centred) is SRX_E_ARG (k <= 64 excepted: the exact eigen-solver takes any
 * rank); components beyond the NUMERICAL rank of the selected columns (a handful of cells, most
 * selected columns empty) come back with explained variance 0 and a zero vector (k > 64) or an
 * arbitrary unit vector of the null space (k <= 64) — the reference returns whatever its SVD
 * makes of a zero singular value. */
typedef enum srx_pca_solver {
    SRX_SOLVER_AUTO = 0,
    SRX_SOLVER_GRAM = 1,   /* explicit sparse Gram X_sel^T X_sel once, dense k x k iteration  */
    SRX_SOLVER_SPMM = 2    /* matrix-free: forward + transposed SpMM every iteration         */
} srx_pca_solver;

typedef struct srx_pca_opts {
    int32_t n_components;  /* < 0 = None -> 2        (dim_red/mod.rs:52); any value up to k
                              with the Gram solver (beyond 56 the solve runs in deflation
                              rounds of 48), up to 56 with the SpMM solver                */
    int32_t center;        /* < 0 = None -> true     (:55)                                */
    int32_t scale;         /* < 0 = None -> true     (:56)                                */
    int32_t n_threads;     /* accepted, ignored on GPU (:61)                              */
    int32_t block;         /* panel width l; 0 -> default (64)                            */
    int32_t max_iter;      /* bound on the sweeps (one sweep = power applications of C:
                              3 in the Gram solver, 1 in the SpMM solver) after the
                              warm-up; 0 -> default 200 (Gram) / 600 (SpMM)               */
    int32_t solver;        /* srx_pca_solver; 0 = auto (Gram when k <= 16384)             */
    double  tol;           /* relative Ritz-residual tolerance; 0 -> default (1e-7 with
                              f32 storage, 1e-9 with f64 storage)                         */
    uint64_t seed;         /* start panel seed (the reference has no randomness here)     */
} srx_pca_opts;

typedef struct srx_pca_info {
    uint64_t n_cells_global;
    uint32_t k;            /* selected features                                           */
    uint32_t n_pc;
    uint32_t block;
    uint32_t n_iter;       /* sweep equivalents executed (applications of C / power)      */
    double residual;       /* final max relative Ritz residual over the n_pc pairs        */
    uint64_t nnz_selected; /* non-zeros of the HVG-compacted CSR actually walked (local)  */
    uint32_t solver;       /* srx_pca_solver actually used                                */
    uint32_t reserved_;
} srx_pca_info;

/* sel: k feature indices in selection order (NULL = FeatureSelection::None, all genes).
 * Host outputs, each may be NULL:
 *   scores      n_rows x n_pc  row-major  (obsm["X_pca"], dim_red/mod.rs:105-106)
 *   components  k x n_pc       row-major  (V[:, :n_pc], pca/mod.rs:144)
 *   evr         n_pc           explained_variance_ratio (pca/mod.rs:145-149)
 *   mean, std   k              column mean / std (ddof 0) over ALL cells (pca/mod.rs:87-91)
 * Sign convention (the reference has none): each component is flipped so that its
 * largest-|.| entry is positive.  A zero-variance selected column gives NaN in the
 * reference (pca/mod.rs:108); here its std is treated as 1 (documented deviation). */
int32_t srx_pca(srx_mat* m, const uint64_t* sel, uint64_t k, const srx_pca_opts* opts,
                double* scores, double* components, double* evr, double* mean, double* std_,
                srx_pca_info* info);
/* varm["PCA_loadings"] layout (dim_red/mod.rs:108-118): n_vars x n_pc, row sel[i] <-
 * loadings row i = components[i,:] * std[i] (pca/mod.rs:204-215), other rows 0. */
int32_t srx_pca_loadings(const double* components, const double* std_, const uint64_t* sel,
                         uint64_t k, uint64_t n_pc, uint64_t n_vars, double* out);

/* ---- PCA of the Pearson residuals (not in the reference) ----------------------------------------------------------------------
 * scanpy's experimental.pp.normalize_pearson_residuals_pca, the second half of recipe_pearson_residuals: the clipped residuals of
 * a gene list, then their PCA, on RAW counts; additive, detected by symbol, no profiling class of its own (the times are in
 * srx_pearson_pca_info).  The scores stay resident as the handle's PCA result: everything that reads "the resident scores of the
 * handle" (neighbours, Harmony, the graph, clustering, the layouts) follows without a host round trip.  What goes through a
 * fitted MODEL does not: srx_pca_model_from_result, and with it srx_doublets_result, which projects its simulated cells with
 * srx_pca_transform, are refused on such a result (below).
 *
 * Definition.  m holds raw counts (CSR or CSC), genes lists k DISTINCT gene indices.  Z is the n x k matrix of the clipped
 *   residuals z_ij exactly as the section above defines them (the same order of operations, in f64, no contraction; mu == 0
 *   gives 0; an empty cell is a row of zeros, a listed gene with g_j = 0 a column of zeros), with the sums taken per `totals`:
 *      SRX_PEARSON_TOTALS_ALL       r_i, g_j and T of the whole matrix: what srx_pearson_residuals does;
 *      SRX_PEARSON_TOTALS_SELECTED  r_i and T are sums over the listed genes only (g_j is the same either way): what scanpy's
 *                                   normalize_pearson_residuals_pca does, which subsets before it normalises.  r_i is summed
 *                                   over the stored entries of the cell in one fixed order, T over the r_i as above.
 *   The default clip stays sqrt(n_rows) either way.  Then
 *      m_j    = (sum_i z_ij) / n                                       (center false: m = 0)
 *      C      = (Z^T Z - n m m^T) / (n - 1)                            (no scaling)
 *      the n_pc algebraically largest eigenpairs of C are the explained variances and the components V (k x n_pc)
 *      evr_p  = eigenvalue_p / trace(C)
 *      scores = (Z - 1 m^T) V
 *   with the sign rule of srx_pca (the largest-|.| entry of each component is positive) and the components' rows in the
 *   caller's gene order.  The solver works on (n - 1) C and on its trace, like srx_pca: the ratio is the same.
 * How it is computed.  Z is dense and not low-rank once the clip is active: Z^T Z is a product of n x k doubles.  Z is made in
 *   chunks of cells from the definition (chunk_cells rows; 0: what a quarter of the last-level cache holds, 64 MiB), each chunk
 *   read back by an f64 matrix-core product: G += Z_c^T Z_c (upper triangle, 64 x 64 tiles) with the column sums of Z_c, the
 *   Gram solver of srx_pca on C (plans, deflation rounds, robust mode and result block are shared), then the chunks again for
 *   scores = Z_c V - 1 (m^T V).  No floating-point atomics; the chunks, and the slabs a chunk may be cut into, are added in
 *   ascending order: two calls give bit-identical results, and the Gram matrix is symmetric bit for bit.
 * The result block of the handle: mean = m, std = ones, the selection = the list; srx_result_fetch, srx_knn_result and every
 *   other reader of the resident SCORES work as after srx_pca.  srx_pca_model_from_result is refused (SRX_E_ARG):
 *   srx_pca_transform would apply normalise / log1p arithmetic to a residual model, and projecting new cells onto a residual
 *   PCA is out of scope; srx_doublets_result on such a handle is refused for the same reason, with a message that says so.
 * Options: `center` < 0 or 1: true, 0: false (pca.center is not read); pca.n_components, max_iter, tol, seed, solver (AUTO or
 *   GRAM) as for srx_pca; opts == NULL: Pearson defaults, totals ALL, centred, 2 components.
 * Departures from scanpy: scanpy yields NaN for an empty cell (here a row of zeros); the sign rule is this library's; scanpy is
 *   not part of the test environment, nothing is compared with it.  batch_key stays out of scope.
 * Refused, in this order: what the section above refuses without a pass over the matrix (a NULL handle or list, several ranks,
 *   a backed session, theta, clip), an empty list, totals outside {0, 1}, k > 16384, a gene index >= n_cols, a repeated gene,
 *   pca.scale > 0, pca.solver == SRX_SOLVER_SPMM (all SRX_E_ARG); k < 2 or n < 5 (SRX_E_SHAPE, as srx_pca; srx_pca_pearson
 *   only); a negative, NaN or infinite stored value (SRX_E_ARG, found on the device). */
typedef enum srx_pearson_totals {
    SRX_PEARSON_TOTALS_ALL = 0,
    SRX_PEARSON_TOTALS_SELECTED = 1
} srx_pearson_totals;
typedef struct srx_pearson_pca_opts {
    srx_pearson_opts pearson;
    int32_t  totals;        /* srx_pearson_totals                                          */
    int32_t  center;        /* < 0 or 1: true, 0: false                                    */
    uint64_t chunk_cells;   /* cells per chunk of Z; 0: auto                               */
    srx_pca_opts pca;
} srx_pearson_pca_opts;
typedef struct srx_pearson_pca_info {
    uint64_t n_cells, n_genes, n_expressed /* g_j > 0, whole matrix */, n_empty_cells /* r_i == 0 under `totals` */;
    double   total, theta, clip;           /* T under `totals` and the values actually used */
    srx_pca_info pca;                      /* nnz_selected is 0: the residuals are dense   */
    double   ms_gram, ms_solve, ms_scores; /* chunks + SYRK; the eigen-solve; chunks + score product */
    uint64_t n_chunks, chunk_cells, chunk_bytes;   /* chunk_bytes: one chunk of Z as stored (rows padded to 64 columns) */
} srx_pearson_pca_info;
/* Host outputs, each may be NULL: scores n_rows x n_pc, components k x n_pc (rows in the caller's gene order), evr n_pc,
 * mean k (m, the caller's order).  SRX_E_NOCONV as for srx_pca. */
int32_t srx_pca_pearson(srx_mat* m, const uint64_t* genes, uint64_t k, const srx_pearson_pca_opts* opts, double* scores,
                        double* components, double* evr, double* mean, srx_pearson_pca_info* info);
/* Kernel-level entry (as srx_spmm for the sparse kernels): Z^T Z (k x k, both triangles, the caller's gene order) and the
 * column sums of Z, so that the SYRK can be checked alone.  opts->center and opts->pca are not read; one of the two outputs
 * may be NULL; k >= 1 (an empty list is SRX_E_ARG) and any n. */
int32_t srx_pearson_gram(srx_mat* m, const uint64_t* genes, uint64_t k, const srx_pearson_pca_opts* opts,
                         double* gram_out /* k x k, host */, double* colsum_out /* k, host */, srx_pearson_pca_info* info);

/* ---- regress out covariates, scale, clip; PCA of the result (not in the reference) --------------------------------------------
 * scanpy's sc.pp.regress_out(adata, keys) -> sc.pp.scale(adata, max_value) -> sc.tl.pca(adata), Seurat's
 * ScaleData(vars.to.regress = ...) -> RunPCA, for continuous covariates, on a gene list; additive, detected by symbol, no
 * profiling class of its own (the times are in srx_regress_info).  The scores of srx_pca_regress stay resident as the handle's PCA
 * result, exactly as after srx_pca_pearson: the readers of "the resident scores of the handle" follow, the readers of a fitted
 * MODEL (srx_pca_model_from_result, srx_doublets_result) refuse, naming this call.
 *
 * Definition.  m is a CSR or CSC handle with n cells and G genes; its values are read as stored (typically after
 *   srx_normalize_log1p_inplace; f32 storage is read as (double)x).  genes lists k DISTINCT gene indices.  cov is a host array,
 *   n x p row-major f64, 0 <= p <= 16; p = 0 is plain scale + clip.  Everything is f64, in the order written, without
 *   contraction, fast-math or floating-point atomics; every sum over the cells is taken in one fixed order (below).
 *   1. Covariates.  cbar_q = (sum_i c_iq) / n;  ct_iq = c_iq - cbar_q;  A = Ct^T Ct (p x p).  An intercept is always part of the
 *      model: centring the covariates is how it is fitted, and it keeps A from inheriting the scale of a covariate such as a
 *      library size of 1e4.  A is factored as the Cholesky factor of D^-1/2 A D^-1/2, D = diag A.  A covariate with A_qq == 0
 *      (constant) is refused with SRX_E_ARG, naming q; so is one whose pivot (1 - R^2 of that covariate on the earlier ones)
 *      is below 1e-10: there the normal equations have lost ten of sixteen digits.  statsmodels would silently take a
 *      pseudo-inverse: a stated departure.
 *   2. Fit, per listed gene j.  xbar_j = srx_compute_sum(m, Column)[j] / n, the library's own column sum, bit for bit;
 *      w_qj = sum_i ct_iq x_ij;  bt_j solves A bt_j = w_j by that factor (forward and back substitution on the scaled system).
 *   3. Residual.  r_ij = (x_ij - xbar_j) - sum_q ct_iq bt_qj, q ascending, the sum started at ct_i0 bt_0j.  A gene whose n values
 *      are all equal (no non-zero entry at all, or n stored entries of one value; found from srx_compute_number and
 *      srx_compute_min_max) has r_ij = 0 for every cell, as scanpy's regress_out returns zeros there.
 *   4. Scale (`scale`, default on).  v_j = (sum_i r_ij^2) / (n - 1), the sum over the residuals themselves;  s_j = sqrt(v_j),
 *      s_j = 1 where v_j == 0.  The mean of r_.j is zero by construction; scanpy subtracts its rounding error, here it is not
 *      subtracted.  Flag off: s_j = 1.
 *   5. Clip.  z_ij = r_ij / s_j;  with max_value > 0, z_ij = min(max(z_ij, -max_value), max_value) (both sides, as current
 *      scanpy does when it centres);  max_value == 0: no clip.
 *   6. PCA of Z, exactly the second half of the srx_pca_pearson section: m_j = (sum_i z_ij) / n (not zero once the clip is
 *      active), C = (Z^T Z - n m m^T) / (n - 1), the n_pc largest eigenpairs, evr = eigenvalue / trace C,
 *      scores = (Z - 1 m^T) V, the library's sign rule, component rows in the caller's gene order.  In the result block
 *      mean = m, std = s (the caller's order) and the selection is the list.
 * How it is computed.  Z is dense.  It is made in chunks of cells (chunk_cells; 0: as srx_pca_pearson) by ONE pair of chunk
 *   kernels that evaluate one element function in three modes (x, r or z), and is read by four passes over the chunks: W (a
 *   weighted column sum: per column and slab of 64-row groups the rows in ascending order, the slabs, then the chunks, added in
 *   ascending order), sum r^2 (the same kernel with the column's own value as weight), then the Gram + column-sum pass and the
 *   score pass of srx_pca_pearson, the same kernels on the f64 matrix cores.  cbar is summed on the host in ascending cell
 *   order, A by the weighted column-sum kernel over Ct itself; the p x p factor and the k solves run on the host in f64.
 *   n_clipped (the pairs with |r_ij / s_j| > max_value) is an integer count made with the chunks of the Gram pass.  Two calls
 *   give bit-identical results.
 * All calls leave the handle's values and dtype as they were (the moments cache is filled with the
 *   moments of the current values if it was empty); srx_pca_regress replaces the handle's PCA result.
 * Departures from scanpy: scanpy regresses with statsmodels' GLM and scales with a mean subtraction of rounding size; neither
 *   package is part of the test environment and nothing is compared with them.  Out of scope: a categorical regressor
 *   (scanpy's per-category means), zero_center = False, sharded and backed contexts, projecting new cells onto such a PCA
 *   (srx_pca_model_from_result refuses, as for the Pearson result), and the sparse-plus-low-rank Gram that would avoid the dense
 *   product when nothing is clipped.
 * Refused with SRX_E_ARG and a message, nothing written, in this order: (1) a NULL handle or list, or cov == NULL with p > 0
 *   (and a call with no output at all); (2) several ranks; (3) an open backed session; (4) max_value negative or NaN; (5) p > 16;
 *   (6) k == 0, k > 16384, a gene index >= n_cols, a repeated gene; (7) pca.scale > 0 (scaling is this call's own flag) or
 *   pca.solver == SRX_SOLVER_SPMM; then SRX_E_SHAPE: n < p + 2, and for srx_pca_regress k < 2 or n < 5 as srx_pca; then again
 *   SRX_E_ARG: (8) a non-finite covariate; (9) a constant or collinear covariate, as above; (10) a non-finite stored value, found
 *   on the device. */
typedef struct srx_regress_opts {
    int32_t  scale;        /* < 0 or 1: true, 0: false                                     */
    int32_t  reserved;
    double   max_value;    /* 0: no clip                                                   */
    uint64_t chunk_cells;  /* cells per chunk of Z; 0: auto, as srx_pca_pearson            */
    srx_pca_opts pca;      /* n_components, max_iter, tol, seed, solver (AUTO or GRAM)     */
} srx_regress_opts;        /* NULL: scale on, no clip, auto chunks, 2 components           */
typedef struct srx_regress_info {
    uint64_t n_cells, n_genes /* k */, n_cov, n_constant_genes;
    uint64_t n_clipped;                    /* pairs with |r / s| > max_value (0 from srx_regress_fit / _sums) */
    double   min_pivot;                    /* the smallest Cholesky pivot of the scaled A (1 with p = 0) */
    double   ms_fit, ms_scale, ms_gram, ms_solve, ms_scores;   /* covariates + W pass + solves; the r^2 pass; as srx_pearson_pca_info */
    uint64_t n_chunks, chunk_cells, chunk_bytes;
    srx_pca_info pca;
} srx_regress_info;
/* Kernel-level entries, so that each stage can be checked alone (as srx_pearson_residuals and srx_pearson_gram).  Host
 * outputs in the caller's gene order; each output of srx_regress_fit may be NULL (not all), beta_out is p x k row-major. */
int32_t srx_regress_fit(srx_mat* m, const uint64_t* genes, uint64_t k, const double* cov, uint64_t p, const srx_regress_opts* opts,
                        double* beta_out /* p x k */, double* xbar_out /* k */, double* sd_out /* k: s */, srx_regress_info* info);
/* The sums the fit is made of, so that each can be held against its dot-product bound: cbar (p), A (p x p) and W (p x k, the
 * caller's gene order); each output may be NULL (not all).  Needs p >= 1. */
int32_t srx_regress_sums(srx_mat* m, const uint64_t* genes, uint64_t k, const double* cov, uint64_t p, const srx_regress_opts* opts,
                         double* cbar_out /* p */, double* a_out /* p x p */, double* w_out /* p x k */, srx_regress_info* info);
/* z (n x k row-major), made by the chunk kernels the Gram and score passes read. */
int32_t srx_regress_residuals(srx_mat* m, const uint64_t* genes, uint64_t k, const double* cov, uint64_t p,
                              const srx_regress_opts* opts, double* out /* host n x k */, srx_regress_info* info);
/* Z^T Z (k x k, both triangles) and the column sums of Z; one of the two may be NULL. */
int32_t srx_regress_gram(srx_mat* m, const uint64_t* genes, uint64_t k, const double* cov, uint64_t p, const srx_regress_opts* opts,
                         double* gram_out /* k x k */, double* colsum_out /* k */, srx_regress_info* info);
/* Host outputs, each may be NULL: scores n x n_pc, components k x n_pc, evr n_pc, mean k (m), sd k (s).  SRX_E_NOCONV as
 * for srx_pca. */
int32_t srx_pca_regress(srx_mat* m, const uint64_t* genes, uint64_t k, const double* cov, uint64_t p, const srx_regress_opts* opts,
                        double* scores, double* components, double* evr, double* mean, double* sd, srx_regress_info* info);

/* ---- sums over gene lists per cell; the gene-set score built on them (not in the reference) ----------------------------------
 * What sc.tl.score_genes and sc.tl.score_genes_cell_cycle give obs["score"], obs["S_score"], obs["G2M_score"] (the usual
 * covariates of the regress section above), and what calculate_qc_metrics(qc_vars=...) gives per gene subset
 * (total_counts_mt, pct_counts_mt).  Additive, detected by symbol, no profiling class of its own (the times are in the info
 * structs).  The definition here is what is tested.  NOTHING has been compared with scanpy, which is not installed where this
 * was built; the control genes are chosen by a hash where scanpy samples with numpy's or pandas's generator (a stated
 * departure, below), so the scores of one dataset differ from scanpy's by the choice of controls.
 *
 * 1. Sums over gene lists (srx_gene_list_sums).  m is a CSR handle with N cells and G genes, read as stored (f32 storage is
 *   read as (double)x).  List t holds DISTINCT gene indices < G: list_genes[list_ptr[t] .. list_ptr[t + 1]); a gene may be in
 *   any number of lists.  Per (cell i, list t) over the STORED entries of row i whose column is in list t (a stored 0 counts):
 *     c[i][t] = their number,   S[i][t] = their sum,
 *   S accumulated as a 64-bit fixed-point integer round(x 2^sum_scale_log2), ties to even.  The scale rule is that of
 *   srx_group_moments with one change:
 *     max_abs = the largest |x| over ALL stored values (one reduction pass, which also refuses NaN / Inf: SRX_E_NAN),
 *     e = the smallest integer with max_abs < 2^e (0 when max_abs == 0), taken no lower than -30,
 *     L = ceil(log2(max(longest list of the call, 1)))    (not from N: rows are canonical CSR, so a sum has at most as many
 *         terms as its list has genes),
 *     sum_scale_log2 = 62 - e - L.
 *   SUM = f64(S_int) 2^-sum_scale_log2.  Consequences: every |S_int| stays below 2^62; the sums are independent of the order in
 *   which the entries are met and bit-identical from call to call; they are exact (equal to the integer sums) for integer counts
 *   while sum_scale_log2 >= 0; otherwise |S_int 2^-sum_scale_log2 - exact| <= c 2^-(sum_scale_log2 + 1), and SUM, the f64 of an
 *   integer that may exceed 2^53, lies within another half ulp of SUM of that.  The scale belongs to the CALL (its longest
 *   list): the same list summed beside a list of another power-of-two size class may differ within that bound.
 *   How: more than 64 lists are ceil(n_lists / 64) walks over the column indices (the 16-bit mirror where the handle has one,
 *   else the 32-bit indices); each index is tested against a 1-bit "in any list of this walk" bitmap (in LDS up to 524288 genes,
 *   read from global memory above); only a hit loads its value and the gene's 64-bit membership mask from a G x 8 B table and
 *   adds into the per-list integer accumulators of its row's wave in LDS.  No floating-point atomic, no contraction.
 *   The handle is left exactly as it was: values, dtype, version, moments cache, resident PCA result.
 *   Refused with a message, nothing written, in this order.  SRX_E_ARG: (1) a NULL handle, list_ptr or list_genes, or both outputs
 *   NULL; (2) n_lists 0 or above SRX_GENE_LISTS_MAX; (3) a CSC handle; (4) a context with more than one rank; (5) an open backed
 *   session; (6) 2^32 rows or more; (7) a list_ptr that does not start at 0 or that decreases; (8) an empty list; (9) a gene index
 *   >= n_cols; (10) a gene repeated within a list.  Then SRX_E_NAN: a stored value is NaN or Inf.  SRX_E_OOM: the N x n_lists
 *   tables do not fit on the device.
 *
 * 2. Control genes (srx_score_genes_controls): pure host code, no context, no device.  gene_mean holds G means; `pool` lists the
 *   P genes controls may come from (NULL, 0: every gene, P = G).  These are scanpy's lines, restated:
 *     n_items = rint(P / (n_bins - 1)), ties to even (np.round);   rank_j = 1 + the number of pool genes with a strictly smaller
 *     mean (pandas rank(method="min"); -0.0 == 0.0);   cut_j = rank_j / n_items, integer division.
 *   For set s and every distinct cut c among its genes the candidates are the pool genes with cut == c — as they are with
 *   ctrl_as_ref, without the set's own genes otherwise.  More than ctrl_size candidates: the ctrl_size that come first under
 *   (key_j ascending, j ascending) are kept, key_j = mix(seed + 0x9E3779B97F4A7C15 (j + 1)) mod 2^64, mix() being splitmix64's
 *   finaliser as in the UMAP section.  The control list of s is the union over its cuts minus the set's own genes, in ascending
 *   gene order.  Property: the key depends on neither the set nor the cut, so scoring several sets in one call equals scoring
 *   each alone, bit for bit.
 *   Worked example: means [0, 0, 1, 2, 3, 5, 8, 13], n_bins = 5: n_items = 2; ranks 1, 1, 3, 4, 5, 6, 7, 8; cuts 0, 0, 1, 2, 2,
 *   3, 3, 4.  P = 10, n_bins = 5: n_items = rint(2.5) = 2.
 *   Stated departure: scanpy draws the ctrl_size genes of a bin with numpy's / pandas's generator; here the hash decides.
 *   Capacity: set s needs at most ctrl_size * min(|s|, P / n_items + 1) entries of ctrl_genes_out; `capacity` is their sum.
 *   Refused with SRX_E_ARG and a message, nothing written, in this order: (1) a NULL array (gene_mean, set_ptr, set_genes,
 *   ctrl_ptr_out, ctrl_genes_out; pool NULL with n_pool > 0); n_sets == 0; (2) n_bins < 2; (3) a pool gene >= n_genes or repeated;
 *   (4) n_items == 0; (5) a non-finite mean of a pool gene; (6) a set_ptr that does not start at 0 or that decreases, an empty
 *   set; (7) a set gene >= n_genes, repeated within its set, or not in the pool; (8) a set whose control list comes out empty,
 *   naming the set; (9) a capacity smaller than the lists need.
 *
 * 3. The score (srx_score_genes).  gene_mean_j = srx_compute_sum(m, Column)[j] / N, the library's own column sum, bit for bit
 *   (as the regress section); controls from 2.; sums from 1. over 2 n_sets lists — the sets, then their controls — in one call,
 *   so one walk up to 32 sets;  score[i][s] = SUM_set / |set| - SUM_ctrl / |ctrl|, f64, in that order, no contraction, on the
 *   device.  Refusals, in this order: 1.(1)-(6) with n_sets in place of n_lists (1 .. SRX_GENE_LISTS_MAX / 2; score_out may not
 *   be NULL; the control outputs may, both or neither), SRX_E_NAN, then 2.(2)-(9), where `capacity` is only checked when the
 *   control outputs are given.  The moments cache is filled with the moments of the current values if it was empty (that is
 *   srx_compute_sum); everything else about the handle stays.
 * Out of scope: CSC handles, sharded contexts and backed sessions; use_raw and layers (the values are read as stored); scanpy's
 *   random sampling; weighted signatures. */
#define SRX_GENE_LISTS_MAX 4096
typedef struct srx_gene_list_info {
    uint64_t n_rows, n_cols, n_lists, longest_list;
    int32_t  sum_scale_log2;
    uint32_t n_walks;
    double   max_abs;
    double   ms_scan, ms_walk;   /* hipEvent times: the reduction over the values; the walks with their table uploads */
} srx_gene_list_info;
typedef struct srx_score_genes_opts {
    uint32_t ctrl_size;    /* 0: 50                          */
    uint32_t n_bins;       /* 0: 25                          */
    uint64_t seed;
    int32_t  ctrl_as_ref;  /* < 0 or 1: true, 0: false       */
    int32_t  reserved;
} srx_score_genes_opts;    /* NULL: {50, 25, 0, true}        */
typedef struct srx_score_genes_info {
    uint64_t n_rows, n_cols, n_sets, n_pool, n_ctrl_total /* sum of |ctrl| */, n_items, longest_list;
    int32_t  sum_scale_log2;
    uint32_t n_walks;
    double   max_abs;
    double   ms_mean, ms_ctrl, ms_walk;   /* hipEvent times: scan + column means; the control genes (host); walks + score */
} srx_score_genes_info;
/* sum_out (f64), cnt_out (u32): host, n_rows x n_lists row-major; either may be NULL, not both. */
int32_t srx_gene_list_sums(srx_mat* m, const uint64_t* list_ptr /* n_lists + 1 */, const uint64_t* list_genes, uint64_t n_lists,
                           double* sum_out, uint32_t* cnt_out, srx_gene_list_info* info);
/* cut_out: G entries, UINT32_MAX outside the pool; may be NULL. */
int32_t srx_score_genes_controls(const double* gene_mean /* n_genes */, uint64_t n_genes, const uint64_t* pool, uint64_t n_pool,
                                 const uint64_t* set_ptr /* n_sets + 1 */, const uint64_t* set_genes, uint64_t n_sets,
                                 const srx_score_genes_opts* opts, uint64_t* ctrl_ptr_out /* n_sets + 1 */, uint64_t* ctrl_genes_out,
                                 uint64_t capacity, uint32_t* cut_out);
/* score_out: host, n_rows x n_sets row-major. */
int32_t srx_score_genes(srx_mat* m, const uint64_t* set_ptr, const uint64_t* set_genes, uint64_t n_sets, const uint64_t* pool,
                        uint64_t n_pool, const srx_score_genes_opts* opts, double* score_out, uint64_t* ctrl_ptr_out,
                        uint64_t* ctrl_genes_out, uint64_t capacity, srx_score_genes_info* info);

/* ---- a fitted PCA applied to other cells: Pca::transform (src/shared/processing/pca/mod.rs:156-185)
 * A model is k feature rows (V: k x n_pc, mu, sd, flags center / scale) held on the device.  For a query
 * matrix Xq (cells x its own genes) and a feature map feat (k entries: the query column of model row i,
 * UINT64_MAX = the gene is absent from the query):
 *     scores[r, j] = sum_i ((x(r, i) - (center ? mu_i : 0)) / (scale ? sd'_i : 1)) * V[i, j]
 *     x(r, i) = Xq'[r, feat[i]], 0 for an absent gene;  sd'_i = sd_i, or 1 where sd_i == 0 (as srx_pca)
 *     Xq' = Xq, or normalize_total(target_sum, Row) then ln_1p per the SRX_BACKED_NORMALIZE / _LOG1P bits,
 *           applied on the fly (both bits: the rounding of the pipeline's write-back) — the query's values
 *           are never modified.
 * Absent genes still contribute their -mu_i / sd'_i V[i, :] term (every model row enters the constant).
 * No sign flip: the components were sign-fixed by the fit.  The transform is row-local: on a sharded
 * context each rank scores its own rows, no collective.  The same model and query give bit-identical
 * scores on every call, and the query's own resident PCA result is left as it was. */
typedef struct srx_pca_model srx_pca_model;
/* The model the last srx_pca / srx_pipeline on m left in HBM, copied device to device (no host round trip);
 * it owns its copies, so m may be freed or re-fitted afterwards.  SRX_E_ARG when m holds no result. */
int32_t srx_pca_model_from_result(srx_mat* m, srx_pca_model** out);
/* A model fitted elsewhere: components k x n_pc row-major, mean / std k (as srx_pca returns them; mean may be
 * NULL when !center, std NULL when !scale).  sel (k gene ids of the fitted matrix, may be NULL) is only
 * remembered for srx_pca_model_info and for srx_pca_transform with feat == NULL.  SRX_E_ARG for k < 1,
 * n_pc < 1, n_pc > k, NaN in components or mean, a negative or non-finite std. */
int32_t srx_pca_model_create(srx_ctx* ctx, uint64_t k, uint64_t n_pc, const double* components, const double* mean,
                             const double* std_, const uint64_t* sel, int32_t center, int32_t scale, srx_pca_model** out);
/* Shape of a model; sel_out (room for k, may be NULL) receives its sel — SRX_E_ARG if it has none. */
int32_t srx_pca_model_info(const srx_pca_model* p, uint64_t* k_out, uint64_t* n_pc_out, uint64_t* sel_out);
void    srx_pca_model_free(srx_pca_model* p);
/* feat: k query columns aligned with the model's rows (UINT64_MAX = absent; a column named twice is
 * SRX_E_ARG, one >= the query's gene count SRX_E_BOUNDS); NULL = the model's own sel (the query has the fitted
 * matrix's gene axis).  transform: SRX_BACKED_NORMALIZE | SRX_BACKED_LOG1P bits (0 = the values as they are).
 * scores_out: n_rows x n_pc row-major f64 (obsm["X_pca"] layout); a query with 0 rows writes nothing.  A CSC
 * query is transposed on the device first.  Model and query must share the context. */
int32_t srx_pca_transform(srx_pca_model* p, srx_mat* q, const uint64_t* feat, double target_sum, int32_t transform,
                          double* scores_out);

/* Exact k-nearest-neighbour search (Euclidean) on the device: the step that consumes obsm["X_pca"].  Not in the
 * reference; it stands in front of what its commented-out tsne / tsne_inplace (dim_red/mod.rs:159-227) would
 * build from the scores.  The distance of a pair is sqrt(sum_j (q_j - r_j)^2) summed in f64 in this difference
 * form; the result is the exact k nearest under it, every row ascending by (distance, reference index) — ties go
 * to the lower index, at the k-th place too — and bit-identical from call to call.  An f32 matrix-core pass keeps
 * n_candidates = k + 8 candidates per row, f64 re-ranks them and proves the row exact or sends it through a full
 * f64 pass (srx_knn_info counts both).  SRX_E_ARG: k outside 1..64 or above the number of admissible references
 * (n_ref - 1 for a self graph without self), n_dims above the coordinates there are, more than SRX_KNN_MAX_DIMS
 * coordinates in use, NaN / Inf in the points, a context with more than one rank (rows are sharded; neighbours
 * need all cells).  Outputs are n_query x k row-major; either may be NULL, info too.  n_query == 0 writes nothing. */
#define SRX_KNN_MAX_DIMS 128
typedef struct srx_knn_opts {
    int32_t k;             /* neighbours per query row, 1..64                                        */
    int32_t n_dims;        /* use the first n_dims coordinates (leading PCs); 0 = all                */
    int32_t include_self;  /* self graph only: 0 = a row is never its own neighbour (default), 1 = it
                              may be (it then comes first at distance 0 unless an exact duplicate with
                              a lower index ties with it)                                            */
    int32_t reserved_;
} srx_knn_opts;
typedef struct srx_knn_info {
    uint64_t n_ref, n_query;
    uint32_t d, k;
    uint32_t n_candidates;     /* candidates per row kept by the f32 pass                            */
    uint32_t reserved_;
    uint64_t rows_certified;   /* rows whose result was proven exact from the f32 pass + f64 re-rank */
    uint64_t rows_recomputed;  /* rows that went through the full f64 pass; the two sum to n_query   */
} srx_knn_info;
/* Self graph of the cells of m in the space of the scores its last srx_pca / srx_pipeline left in HBM (no host
 * round trip; the result stays as it is).  SRX_E_ARG when m holds no result. */
int32_t srx_knn_result(srx_mat* m, const srx_knn_opts* opts, uint32_t* indices_out, double* distances_out,
                       srx_knn_info* info);
/* The same search on caller-supplied points (row-major f64, n x d): neighbours of every query row among the
 * reference rows.  query == NULL: the self graph of ref (n_query is ignored).  This is how projected cells
 * (srx_pca_transform output) find their neighbours in the fitted data set. */
int32_t srx_knn_points(srx_ctx* ctx, const double* ref, uint64_t n_ref, const double* query, uint64_t n_query,
                       uint64_t d, const srx_knn_opts* opts, uint32_t* indices_out, double* distances_out,
                       srx_knn_info* info);

/* ---- the weighted neighbour graph: obsp["distances"] and obsp["connectivities"] -------------------------------
 * What clustering, UMAP, diffusion maps and PAGA read.  Not in the reference; it is scanpy's pp.neighbors graph, i.e.
 * umap-learn's fuzzy_simplicial_set with local_connectivity = 1 and set_op_mix_ratio = 1, restated for k-NN rows that
 * do NOT carry the cell itself (scanpy's n_neighbors counts the cell: n_neighbors = k + 1 there, hence log2(k + 1) and
 * the k + 1 of the floor below).  The formulas here are what is tested; the output has NOT been compared with
 * umap-learn or scanpy.
 *
 * Input: for every row i, k distinct neighbours j != i with finite Euclidean distances d_ij >= 0; 1 <= k <= 64.
 * T = log2(k + 1).  Per row:
 *   rho_i    = the smallest strictly positive distance of the row; a row without one (k exact duplicates) has
 *              rho_i = sigma_i = 0 and every weight 1 (rows_all_zero; such a row also counts in rows_no_root).
 *   c_i      = neighbours with d_ij <= rho_i;  S_i(s) = c_i + sum over {d_ij > rho_i} exp(-(d_ij - rho_i) / s).
 *   sigma*_i = the root of S_i(s) = T when c_i < T, solved to |S_i - T| <= 1e-9 (umap-learn stops at 1e-5), else 0
 *              (rows_no_root: enough neighbours tie at the minimum).
 *   sigma_i  = max(sigma*_i, 1e-3 * (sum_j d_ij) / (k + 1))      (rows_clamped: the floor is the larger).
 *   a_ij     = 1 when d_ij <= rho_i, else exp(-(d_ij - rho_i) / sigma_i), in f64.
 * Connectivities C = A + A^T - A o A^T: for every pair joined in either direction C[i,j] = fma(-a, b, a + b) with
 * a = a_ij, b = a_ji (0 when absent).  Entries that are exactly 0.0 are not stored (entries_dropped).  Distances D:
 * D[i,j] = d_ij on the k-NN edges, all n k entries stored.  Both are CSR with u64 indptr (n + 1), u32 indices
 * ascending within a row and f64 data.  C is exactly symmetric (C[i,j] and C[j,i] are the same bits), has no
 * diagonal, 0 < C[i,j] <= 1, and the whole result is bit-identical from call to call and independent of the order of
 * the entries within an input row.
 * The formulas are evaluated literally in IEEE f64: a row whose sum_j d_ij overflows has floor = sigma_i = +inf, every
 * weight of that row is 1 and it counts in rows_clamped.  The 1e-9 of sigma*_i holds for distances in the normal range:
 * with subnormal distances sigma*_i is the upper end of the last one-ulp bracket of the root, and on that grid S_i can
 * miss T by more.
 *
 * The handle owns its device buffers (a later k-NN or graph call does not touch them); free it before its context. */
typedef struct srx_graph srx_graph;
typedef struct srx_graph_info {
    uint64_t n;
    uint32_t k, reserved_;
    uint64_t nnz_distances, nnz_connectivities;
    uint64_t n_mutual;         /* unordered pairs present in both directions of the k-NN list            */
    uint64_t rows_no_root, rows_clamped, rows_all_zero;
    uint64_t entries_dropped;  /* exact zeros of A + A^T - A o A^T that are not stored                   */
    uint64_t max_row_nnz;      /* longest row of the connectivities                                      */
} srx_graph_info;
/* srx_knn_result (opts as there, include_self must be 0: else SRX_E_ARG) on the scores the last fit left in HBM, then
 * the graph of that list; indices and distances never leave the device.  knn_info may be NULL. */
int32_t srx_neighbors_result(srx_mat* m, const srx_knn_opts* opts, srx_knn_info* knn_info, srx_graph** out);
/* The graph of a caller-supplied k-NN list (n x k row-major, e.g. what srx_knn_points returned).  SRX_E_ARG: k outside
 * 1..64, k > n - 1, an index >= n, a row naming itself or one neighbour twice, a negative / NaN / Inf distance, a
 * context with more than one rank.  Rows need not be sorted.  n == 0 gives an empty graph. */
int32_t srx_neighbors_from_knn(srx_ctx* ctx, const uint32_t* indices, const double* distances, uint64_t n, uint32_t k,
                               srx_graph** out);
int32_t srx_graph_info_get(const srx_graph* g, srx_graph_info* info);
enum { SRX_GRAPH_DISTANCES = 0, SRX_GRAPH_CONNECTIVITIES = 1 };
/* Copy one of the two matrices to the host; any pointer may be NULL, sizes from srx_graph_info. */
int32_t srx_graph_fetch(srx_graph* g, int32_t which, uint64_t* indptr, uint32_t* indices, double* data);
int32_t srx_graph_fetch_scales(srx_graph* g, double* rho, double* sigma);   /* n each */
void    srx_graph_free(srx_graph* g);

/* ---- the shared-nearest-neighbour (SNN) graph of a k-NN list: Jaccard weights, pruned -----------------------------------
 * What Seurat's FindNeighbors (ComputeSNN), PhenoGraph and scran's buildSNNGraph(type = "jaccard" / "number") cluster.
 * Not in the reference.  The definition below is what is tested; Seurat, PhenoGraph and scran are NOT installed where
 * this was built and the output has NOT been compared with any of them.
 *
 * Input: a k-NN list as srx_neighbors_from_knn takes it: n rows of k distinct neighbours j != i, 1 <= k <= 64,
 *   k <= n - 1; rows need not be sorted; distances play no part in the weights.
 * Neighbour sets: include_self = 1 (the default, Seurat's convention): N(i) = {i} u knn(i), K = k + 1;
 *   include_self = 0: N(i) = knn(i), K = k.  For i != j the shared count is s_ij = |N(i) n N(j)|, an integer in 0 .. K.
 * Pairs considered: SRX_SNN_PAIRS_SHARED (the default, Seurat's ComputeSNN): every pair i != j with s_ij >= 1;
 *   SRX_SNN_PAIRS_KNN (PhenoGraph's restriction): of those, the pairs joined by the list in either direction
 *   (j in knn(i) or i in knn(j)).
 * Value: J_ij = (double)s_ij / (double)(2 K - s_ij), ONE IEEE f64 division of two exactly converted integers.  A
 *   considered pair is stored if and only if J_ij >= prune (Seurat zeroes value < prune: equality keeps the pair).  J rises
 *   with s, so this is s_ij >= min_shared with min_shared = srx_snn_min_shared(k, include_self, prune), the smallest s in
 *   1 .. K whose J >= prune by that same expression (K + 1: none, the graph is empty).  The stored weight is J_ij for
 *   SRX_SNN_JACCARD and (double)s_ij for SRX_SNN_NUMBER.  prune lies in [0, 1]; the default is 1/15; prune = 0 keeps
 *   every considered pair.
 * Result: CSR like the connectivities: u64 indptr (n + 1), u32 indices ascending within a row, f64 data.  It is exactly
 *   symmetric (both entries of a pair are the same bits), has NO diagonal (a stated departure: Seurat stores the
 *   diagonal as 1), does not depend on the order of the entries within an input row, and is bit-identical from call to
 *   call: everything up to the one division is integer arithmetic, and no floating-point atomic takes part.
 * The result is an ordinary srx_graph: its C block (SRX_GRAPH_CONNECTIVITIES) holds the SNN graph, its D block a copy
 *   of the source list in column order with its distances (zeros when none were given); rho, sigma and the directed
 *   weights are zero; srx_graph_info has n, k, nnz_distances, nnz_connectivities and max_row_nnz, the other counters
 *   are 0.  Every call that takes an srx_graph (srx_louvain, srx_umap, srx_paga, srx_diffmap, srx_autocorr, ...) works
 *   on it unchanged.
 * Refusals, each SRX_E_ARG with a message: those of srx_neighbors_from_knn (k outside 1..64, k > n - 1, an index >= n,
 *   a row naming itself or one neighbour twice, a negative / NaN / Inf distance where distances are given, a context
 *   with more than one rank); prune NaN or outside [0, 1]; an unknown weight or pairs.  n == 0 gives an empty graph.
 * Out of scope: scran's type = "rank" weighting (it needs the ranks carried in the reverse lists). */
enum { SRX_SNN_JACCARD = 0, SRX_SNN_NUMBER = 1 };
enum { SRX_SNN_PAIRS_SHARED = 0, SRX_SNN_PAIRS_KNN = 1 };
typedef struct srx_snn_opts {
    int32_t weight;            /* SRX_SNN_JACCARD | SRX_SNN_NUMBER                                         */
    int32_t pairs;             /* SRX_SNN_PAIRS_SHARED | SRX_SNN_PAIRS_KNN                                 */
    int32_t include_self;      /* non-zero: N(i) holds i                                                   */
    int32_t reserved_;
    double  prune;
} srx_snn_opts;                /* NULL = {SRX_SNN_JACCARD, SRX_SNN_PAIRS_SHARED, 1, 0, 1.0 / 15.0}         */
typedef struct srx_snn_info {
    uint64_t n;
    uint32_t k, set_size;      /* set_size = K                                                             */
    uint32_t min_shared;       /* srx_snn_min_shared(k, include_self, prune)                               */
    uint32_t max_shared;       /* the largest s_ij over the considered pairs (0: none)                     */
    uint64_t pairs_considered; /* unordered pairs                                                          */
    uint64_t pairs_kept;       /* ... of them stored: nnz / 2                                              */
    uint64_t nnz;
    uint64_t max_row_nnz;
    uint64_t max_in_degree;    /* the longest reverse list R(m) = {j : m in knn(j)}                        */
    uint64_t max_candidates;   /* the largest c_i = sum over m in N(i) of |{j : m in N(j)}| over the rows  */
    uint64_t sum_candidates;   /* the sum of c_i over the rows: what one pass into a staging would reserve */
    uint32_t wave_capacity;    /* c_i up to here: one wave per row, a hash table in LDS                    */
    uint32_t short_capacity;   /* c_i up to here: one workgroup per row, a hash table in LDS               */
    uint64_t rows_wave;        /* rows on the first route                                                  */
    uint64_t rows_long;        /* rows beyond short_capacity: one workgroup per row over windows of the index range */
    uint64_t rows_empty;       /* rows of the result without an entry                                      */
    double   ms;               /* hipEvent time of the device work                                         */
    double   ms_lists, ms_count, ms_fill;   /* of it: the reverse lists | the count pass | the fill pass   */
} srx_snn_info;
/* The SNN graph of a caller-supplied list (n x k row-major u32; distances n x k f64 or NULL).  opts and info may be NULL. */
int32_t srx_snn_from_knn(srx_ctx* ctx, const uint32_t* indices, const double* distances, uint64_t n, uint32_t k,
                         const srx_snn_opts* opts, srx_snn_info* info, srx_graph** out);
/* The same from the list that a handle holds on the device (its D block), whichever call made the handle
 * (srx_neighbors_result, srx_neighbors_from_knn, srx_neighbors_index, srx_neighbors_harmony, or one of the two calls
 * here): no host round trip.  g stays untouched; *out is a new handle. */
int32_t srx_snn_graph(srx_graph* g, const srx_snn_opts* opts, srx_snn_info* info, srx_graph** out);
/* Host code, no GPU: the smallest s in 1 .. K with (double)s / (double)(2 K - s) >= prune, K + 1 when there is none.
 * SRX_E_ARG: k outside 1..64, prune NaN or outside [0, 1], out == NULL. */
int32_t srx_snn_min_shared(uint32_t k, int32_t include_self, double prune, uint32_t* out);

/* ---- approximate k-NN: an inverted-file (IVF) index over dense points -----------------------------------------------
 * The exact search above costs n^2 products; this one probes a few lists of an index.  Not in the reference; it is the
 * classical IVF-flat scheme, defined here tightly enough to be tested bit for bit.  It has NOT been compared with FAISS,
 * pynndescent or scanpy.
 *
 * Distance, order and ties are those of srx_knn_*: dist2(a, b) = sum_j (a_j - b_j)^2 in f64, in coordinate order.
 *
 * Index over n_ref >= 1 points with d coordinates (1 <= d <= SRX_KNN_MAX_DIMS, all finite).  It holds n_lists centroids
 * (f64, n_lists x d), the assignment of every point to its nearest centroid — ties to the lower centroid index — and the
 * lists: offsets (n_lists + 1) and members, ascending by point index within a list.  The index owns a copy of the
 * points; it depends on no later fit, search or graph call.
 *
 * Centroids.  Supplied by the caller (n_lists x d f64, n_lists >= 1, taken as they are): the whole search is then a pure
 * function of its inputs.  Or trained (centroids == NULL):
 *   n_lists == 0 means round(4 sqrt(n_ref)) clipped to 1..n_ref; max_train_points == 0 means 64 n_lists;
 *   n_train = min(n_ref, max(max_train_points, n_lists)).
 *   h_i = splitmix64(splitmix64(seed) ^ i), splitmix64(x) = mix(x + 0x9E3779B97F4A7C15) with the mix() of the UMAP
 *   section; the sample is the n_train points with the smallest (h_i, i), in that order (a draw without replacement).
 *   The first n_lists sample points are the start.  Then train_iters Lloyd iterations: every sample point is assigned
 *   as above, and every centroid becomes the f64 mean of its sample points, taken in sample order by a fixed summation
 *   tree (no floating-point atomics); a centroid without points keeps its place.  The result is bit-identical from call
 *   to call for one seed.  srx_ivf_opts == NULL means {0, 10, 0, 0}.
 *
 * Search: k in 1..64, n_probe in 1..64 and <= n_lists (0 = min(20, n_lists)), include_self as in srx_knn_opts; n_dims
 * must be 0 or the index's d.  The probe set of a query is its n_probe nearest centroids by (distance, centroid index).
 * The result of a row is the exact k nearest among the admissible members of its probed lists, ascending by (distance,
 * point index), bit-identical from call to call.  A row whose probed lists hold fewer than k admissible points is
 * searched over ALL references instead (rows_exhaustive).  Hence n_probe == n_lists returns what srx_knn_points returns,
 * bit for bit.  In the self form (query == NULL) the list of a point is its first probe, so it is always searched.
 *
 * How: assignments and probe sets are the exact search of srx_knn_points against the centroids.  An f32 matrix-core
 * pass, one workgroup per (list, block of 128 queries probing it), keeps n_candidates = k + 8 candidates per (query,
 * probe); the k + 8 of a row with the lowest f32 scores are re-ranked in f64, which proves the row by the certificate of
 * the exact search (rows_certified: whatever a pair or the row dropped scores at or above the bound) or selects in
 * f64 over the members of the probed lists (rows_rescanned).  The three row counters sum to n_query.  pairs = the
 * number of (query, probed list) pairs, points_scanned = the sum of their list lengths.  Candidates are processed in
 * chunks of queries of at most 1 GiB.  The default of 20 probes is the smallest measured count whose recall@15 on the
 * pipeline scores of 1.3 M cells reaches 0.95 (profiles/knn_ivf.md: 0.965; 16 probes give 0.936).
 *
 * SRX_E_ARG, with a message and nothing written: everything srx_knn_points refuses; n_ref == 0; n_lists outside
 * 0..n_ref, or 0 with supplied centroids; train_iters outside 0..1000; NaN / Inf in the centroids; n_probe outside 0..64
 * or above n_lists; n_dims neither 0 nor d; k above the admissible count; a context with more than one rank. */
typedef struct srx_knn_index srx_knn_index;
typedef struct srx_ivf_opts {
    int32_t  n_lists;           /* 0 = round(4 sqrt(n_ref))                                   */
    int32_t  train_iters;       /* Lloyd iterations, 0..1000                                  */
    uint64_t seed;
    uint64_t max_train_points;  /* 0 = 64 n_lists                                             */
} srx_ivf_opts;
typedef struct srx_ivf_info {
    uint64_t n_ref, n_train;    /* n_train == 0: supplied centroids                           */
    uint32_t d, n_lists, train_iters, reserved_;
    uint64_t min_list, max_list, empty_lists;
    double   inertia;           /* sum over all points of dist2 to the assigned centroid, a fixed-order f64 sum */
    double   ms_train, ms_assign;
} srx_ivf_info;
typedef struct srx_ivf_search_info {
    uint64_t n_query;
    uint32_t k, n_probe, n_candidates, reserved_;
    uint64_t rows_certified, rows_rescanned, rows_exhaustive, pairs, points_scanned;
} srx_ivf_search_info;
/* over the first n_dims (0 = all) coordinates of the scores the last fit left in HBM; trained centroids */
int32_t srx_knn_index_result(srx_mat* m, int32_t n_dims, const srx_ivf_opts* opts, srx_knn_index** out);
/* over caller-supplied points (row-major f64, n_ref x d); centroids NULL: trained */
int32_t srx_knn_index_points(srx_ctx* ctx, const double* ref, uint64_t n_ref, uint64_t d, const srx_ivf_opts* opts,
                             const double* centroids, srx_knn_index** out);
int32_t srx_knn_index_info_get(const srx_knn_index* ix, srx_ivf_info* info);
/* centroids n_lists x d, list_offsets n_lists + 1, list_members n_ref; any may be NULL */
int32_t srx_knn_index_fetch(srx_knn_index* ix, double* centroids, uint64_t* list_offsets, uint32_t* list_members);
/* query NULL: the self form (n_query is ignored).  Outputs n_query x k row-major; either may be NULL, info too. */
int32_t srx_knn_index_search(srx_knn_index* ix, const double* query, uint64_t n_query, const srx_knn_opts* opts,
                             int32_t n_probe, uint32_t* indices_out, double* distances_out, srx_ivf_search_info* info);
/* the self search with include_self == 0 (else SRX_E_ARG), then the graph of that list as srx_neighbors_result builds
 * it: the list never leaves the device, and every consumer of an srx_graph works on it unchanged.  info may be NULL. */
int32_t srx_neighbors_index(srx_knn_index* ix, const srx_knn_opts* opts, int32_t n_probe, srx_ivf_search_info* info,
                            srx_graph** out);
void    srx_knn_index_free(srx_knn_index* ix);

/* ---- Louvain communities of a symmetric weighted graph: what sc.tl.louvain / leiden give obs["louvain"] ----------
 * Not in the reference.  The method is a parallel Louvain with synchronous sweeps, defined here; it is tested against this
 * definition and, for quality, against networkx's louvain_communities.  Leiden's refinement phase is not part of it.
 *
 * Input: a symmetric graph W as CSR (u64 indptr, u32 indices ascending within a row, f64 weights > 0, no diagonal).
 *   k_i = sum_j W_ij (plus the self weight of a coarse vertex),  2m = sum_i k_i,  gamma = resolution.
 * Modularity of a labelling:  Q = sum_c [ in_c / 2m - gamma (tot_c / 2m)^2 ],  in_c = sum of W_ij over the ORDERED pairs
 * inside c (a coarse vertex's self weight counts both directions, as S^T W S does),  tot_c = sum over i in c of k_i.
 * A level starts from singletons and runs sweeps t = 0, 1, ...  In sweep t only the vertices with (i + t) even may move.
 * Against the labelling and the tot_c as they stood BEFORE the sweep a vertex evaluates, for every community c among its
 * neighbours and for its own (there it counts as removed),
 *     g(c) = w_{i->c} - gamma k_i (tot_c - [c = c_i] k_i) / 2m
 * and moves to the best c only if g(c) > g(own) strictly; ties between targets go to the lowest community id; a vertex
 * alone in its community does not move into another singleton community with a LOWER id (no swap oscillation: of two
 * lone neighbours only the lower-numbered one may join the other).  The level ends when two consecutive sweeps (both
 * parities) move nothing, or after max_sweeps (a synchronous scheme can cycle; the labelling the last sweep left is the
 * level's).  Then the communities become
 * vertices: weights are summed, the weight inside a community becomes a self weight that takes part in k and tot but is
 * never a "neighbour community"; levels repeat on the coarse graph.  A level whose labelling does not raise Q above the
 * previous level's (for the first level: above the singletons') by more than min_gain is discarded and ends the run, so
 * level_modularity is strictly increasing; the run also ends when a level moves nothing or at max_levels.
 * Final labels number the communities 0, 1, ... by descending size, ties to the community with the smallest member
 * (scanpy's convention).  Isolated vertices are communities of their own; n = 0 gives an empty result; a graph without
 * edges gives singletons, Q = 0 and n_levels = 0.
 * The result is bit-identical from call to call: every sum that atomics make is 64-bit fixed point at the scale
 * 2^(60 - ceil(log2(2m))) — tot_c, the sums of Q, the weights of a long row per community, the coarse weights — and the run
 * is refused (SRX_E_ARG) if 2m at that scale would reach 2^61.  tot_c and coarse weights therefore carry an absolute
 * error of at most half a unit of 2m 2^-60 per summand; info.modularity agrees with an f64 evaluation of Q on the
 * returned labels to about nnz 2^-53.
 * Where every weight is a multiple of 2^-20 and 2m < 2^32, every k_i, tot_c, w_{i->c} and coarse weight is exact both in
 * f64 and at these scales, and the result (labels, sweeps, moves, the communities of every level) is exactly that of this
 * definition evaluated in f64 with g(c) computed as  w - gamma * k_i * t / 2m  from left to right, as long as no level's
 * Q comes within 1e-9 of its keep-or-discard threshold; this is the condition the exact tests use
 * (tests/test_louvain_exact_gpu.py). */
#define SRX_LOUVAIN_MAX_LEVELS 32
typedef struct srx_louvain_opts {
    double  resolution;   /* gamma; <= 0 or NaN: SRX_E_ARG; NULL opts = {1.0, 0.0, 0, 0}               */
    double  min_gain;     /* a level must raise Q by more than this (default 0)                        */
    int32_t max_levels;   /* 0 = SRX_LOUVAIN_MAX_LEVELS */
    int32_t max_sweeps;   /* per level, 0 = 200 */
} srx_louvain_opts;
typedef struct srx_louvain_info {
    uint64_t n, n_communities;
    uint32_t n_levels, reserved_;
    uint64_t sweeps, moves;                              /* over all kept levels */
    double   modularity;                                 /* of the returned labels, f64 */
    double   ms;                                         /* hipEvent time of the device work */
    uint64_t level_communities[SRX_LOUVAIN_MAX_LEVELS];
    double   level_modularity[SRX_LOUVAIN_MAX_LEVELS];
} srx_louvain_info;
/* The communities of the handle's connectivities, read where they lie (no host round trip; C is left untouched).  The
 * labels stay on the device with the handle (srx_graph_labels_fetch); labels_out (n u32) and info may be NULL. */
int32_t srx_louvain(srx_graph* g, const srx_louvain_opts* opts, uint32_t* labels_out, srx_louvain_info* info);
/* The same on a caller-supplied symmetric graph.  Validated on the device, SRX_E_ARG with a message for: an index >= n, a
 * diagonal entry, a row not strictly ascending, a weight that is <= 0, NaN or Inf, W_ij and W_ji not the same bits or not
 * both present; also for an indptr that does not start at 0 or decreases, and a context with more than one rank. */
int32_t srx_louvain_csr(srx_ctx* ctx, const uint64_t* indptr, const uint32_t* indices, const double* weights, uint64_t n,
                        const srx_louvain_opts* opts, uint32_t* labels_out, srx_louvain_info* info);
/* The last srx_louvain's labels, kept on the device (n u32).  SRX_E_ARG when none has run on the handle. */
int32_t srx_graph_labels_fetch(srx_graph* g, uint32_t* labels_out);

/* ---- marker genes per group: grouped per-gene moments and Welch's t statistic, group against rest ---------------------
 * What sc.tl.rank_genes_groups(method="t-test") gives uns["rank_genes_groups"].  Not in the reference; the definition here is
 * what is tested.  The output has NOT been compared with scanpy (scanpy is not installed where this was built); the scores
 * of the host test reference agree with scipy.stats.ttest_ind(equal_var=False).
 *
 * Input: the current stored values x of a CSR matrix (N = n_rows cells x n_cols genes) and one label < n_groups per cell.
 * Moments.  Group g has n_g cells.  Per (group, gene) over the STORED entries of the group's rows (a stored 0 counts):
 *   c_g = their number,  S_g = sum of x,  Q_g = sum of x * x (the product rounded to f64 first).
 * S and Q are accumulated as 64-bit fixed-point integers round(x 2^sum_scale_log2), round(x x 2^sq_scale_log2), ties to even:
 *   max_abs = the largest |x| over all stored values (found by one reduction pass that also refuses NaN / Inf: SRX_E_NAN),
 *   e = the smallest integer with max_abs < 2^e (0 when max_abs == 0), taken no lower than -30 (the cap: 2^(62 + 60) is the
 *       largest scale formed),  L = ceil(log2(max(N, 1))),
 *   sum_scale_log2 = 62 - e - L,   sq_scale_log2 = 62 - 2 e - L       (no other cap; either may be negative).
 * Every total therefore stays below 2^62, |S_dev - S_exact| <= n_g 2^-(sum_scale_log2 + 1) (likewise Q), the tables are
 * bit-identical from call to call and independent of the order of the rows, and integer-valued data gives exact moments
 * as long as the scales are not negative.  SUM = f64(S_int) 2^-sum_scale_log2, SUMSQ likewise.
 * Totals and rest: S_total = sum over g of S_int (integer), S_rest = S_total - S_g (integer subtraction, THEN converted to
 * f64); c_rest and Q_rest the same way; n_r = N - n_g.
 * Statistics, all f64, no FMA contraction, in exactly this order (group: S, Q, c, n = n_g; rest: the rest values, n = n_r):
 *   mean = S / n                                         (0 when n == 0)
 *   var  = max(0, (Q / n - mean * mean) * (n / (n - 1)))   (a value that is not > 0 gives +0)
 *   d = var_g / n_g + var_r / n_r;   score = (mean_g - mean_r) / sqrt(d) when d > 0, else 0
 *   pct = c / n                                          (0 when n == 0)
 *   lfc = log2((expm1(mean_g) + 1e-9) / (expm1(mean_r) + 1e-9)) when logged, else log2((mean_g + 1e-9) / (mean_r + 1e-9))
 * A group with n_g < 2 or n_r < 2 is degenerate (an empty group and n_groups == 1 included): its variances (both sides) and
 * its scores are 0, its means, pct and lfc are as above; info.groups_degenerate counts such groups.
 * Ranking: per group the genes by (score descending, gene index ascending); the first n_top are kept. */
#define SRX_GROUPS_MAX 4096
typedef struct srx_markers srx_markers;   /* owns its device tables; free it before its context */
typedef struct srx_rank_genes_opts {
    int32_t n_top;     /* genes kept per group; 0 = min(100, n_cols); above n_cols or negative: SRX_E_ARG */
    int32_t logged;    /* the values are ln(1 + x) (lfc through expm1); < 0 = yes.  NULL opts = {0, -1}    */
} srx_rank_genes_opts;
typedef struct srx_markers_info {
    uint64_t n_rows, n_cols;
    uint32_t n_groups, n_top;
    int32_t sum_scale_log2, sq_scale_log2;
    uint32_t groups_degenerate, reserved_;
    double max_abs;
    double ms;             /* hipEvent time of the device work */
} srx_markers_info;
enum { SRX_MARKERS_CNT = 0, SRX_MARKERS_SUM = 1, SRX_MARKERS_SUMSQ = 2, SRX_MARKERS_MEAN = 3, SRX_MARKERS_VAR = 4,
       SRX_MARKERS_MEAN_REST = 5, SRX_MARKERS_VAR_REST = 6, SRX_MARKERS_SCORE = 7, SRX_MARKERS_LFC = 8, SRX_MARKERS_PCT = 9,
       SRX_MARKERS_PCT_REST = 10,
       SRX_MARKERS_RANKSUM2 = 11 /* u64; a handle of srx_rank_genes_wilcoxon only (below) */ };
/* The primitive (pseudobulk sums, dot-plot fractions): labels = n_rows host u32, each < n_groups; n_cells_out n_groups u64;
 * cnt_out (u64), sum_out, sumsq_out (f64) n_groups x n_cols row-major; any output may be NULL.
 * Refusals of this and the two calls below, each with a message.  SRX_E_ARG: n_groups outside 1 .. SRX_GROUPS_MAX, a label
 * >= n_groups (validated on the device), a CSC handle, a context with more than one rank (labels live on one rank; sharding
 * is out of scope), 2^32 rows or more.  SRX_E_NAN: a stored value is NaN or Inf.  SRX_E_OOM: the tables do not fit.
 * m is never modified: its values, version, moments cache and resident PCA result stay as they were (the pattern-only gene
 * tiles of srx_matrix_prepare are built if the handle has none yet). */
int32_t srx_group_moments(srx_mat* m, const uint32_t* labels, uint32_t n_groups, uint64_t* n_cells_out, uint64_t* cnt_out,
                          double* sum_out, double* sumsq_out);
/* Moments, statistics and ranking for host labels.  *out is written on success only. */
int32_t srx_rank_genes_groups(srx_mat* m, const uint32_t* labels, uint32_t n_groups, const srx_rank_genes_opts* opts,
                              srx_markers** out);
/* The same with the labels the last srx_louvain left on g, read on the device (no host round trip); n_groups = the largest
 * label + 1.  SRX_E_ARG also when g holds no labels, g's n differs from m's n_rows, or the two handles' contexts differ. */
int32_t srx_rank_genes_groups_graph(srx_mat* m, srx_graph* g, const srx_rank_genes_opts* opts, srx_markers** out);
int32_t srx_markers_info_get(const srx_markers* mk, srx_markers_info* info);
/* n_groups x n_top row-major each; any pointer may be NULL. */
int32_t srx_markers_fetch_top(srx_markers* mk, uint32_t* genes_out, double* scores_out, double* lfc_out);
/* One full n_groups x n_cols table, row-major: SRX_MARKERS_CNT is u64, every other one f64. */
int32_t srx_markers_fetch_table(srx_markers* mk, int32_t which, void* out);
int32_t srx_markers_fetch_sizes(srx_markers* mk, uint64_t* n_cells_out);   /* n_groups */
void    srx_markers_free(srx_markers* mk);

/* ---- marker genes per group: the Wilcoxon rank-sum statistic, group against rest, from exact grouped rank sums ---------
 * What sc.tl.rank_genes_groups(method="wilcoxon") gives uns["rank_genes_groups"].  Not in the reference; the definition here
 * is what is tested.  The output has NOT been compared with scanpy (scanpy is not installed where this was built); the rank
 * sums of the host test reference equal scipy.stats.rankdata / mannwhitneyu, its tie-corrected scores give scipy's p-value.
 *
 * Input: that of srx_rank_genes_groups.  Per gene j the column holds N values: its c_j stored entries and N - c_j implicit
 * zeros.
 * Ordering.  Values are compared as real numbers, each storage (f32, f64) in its own precision; a stored 0.0 or -0.0 ties
 *   with the implicit zeros; NaN / Inf are refused (SRX_E_NAN).
 * Doubled rank.  A value whose tie run has t members, with b strictly smaller values in the column, has r2 = 2 b + t + 1:
 *   twice the average rank (scipy's rankdata), always an integer.
 * Rank sums.  R2[g][j] = the sum of r2 over the cells of group g (u64); the implicit zeros of group g contribute
 *   (n_g - c_gj) r2_zero, c_gj the stored count of the grouped moments.  The sum over g of R2[g][j] is N (N + 1) for every gene.
 * Tie term.  T[j] = the sum over the column's tie runs of t^3 - t (u64); computed only with tie_correct.
 * Score, all f64, no FMA contraction, in exactly this order (n_r = N - n_g):
 *   num = (double)(int64)(R2 - n_g (N + 1)) * 0.5                     (the subtraction in integers)
 *   tc  = 1.0 - (double)T / (double)(N^3 - N)  with tie_correct and N >= 2 (N^3 - N formed as an integer), else 1.0
 *   d   = (((double)(n_g n_r) * (double)(N + 1)) / 12.0) * tc           (n_g n_r formed as an integer)
 *   score = num / sqrt(d) when d > 0, else 0
 * This is scanpy's z (tie_correct = 0 is scanpy's default); with tie_correct it is the asymptotic Mann-Whitney z without
 * continuity correction.  A group with n_g == 0 or n_r == 0 is degenerate: its scores are 0 and info.groups_degenerate counts
 * it (the t-test's rule, n < 2, still governs VAR / VAR_REST).  Ranking as above: score descending, gene index ascending.
 * Everything is integer arithmetic up to the score, so R2, T, the scores and the top lists are exact, independent of the order
 * of the rows and bit-identical from call to call, whatever the staging order and however the genes were chunked.
 * The other tables (CNT, SUM, SUMSQ, MEAN, VAR, PCT, LFC, the _REST ones) are those of srx_rank_genes_groups for the same
 * input, from the same grouped moments. */
typedef struct srx_wilcoxon_opts {
    int32_t n_top;             /* as srx_rank_genes_opts                                                                */
    int32_t logged;            /* as srx_rank_genes_opts                                                                */
    int32_t tie_correct;       /* non-zero: form T and apply tc                                                         */
    int32_t reserved_;
    uint64_t scratch_bytes;    /* cap of the gene-major staging buffer (both sides of the sort's ping-pong: 12 B per
                                  stored entry at f32 storage, 20 B at f64); the genes are cut into chunks that fit.  0 =
                                  2 GiB.  A cap below the longest single gene is raised to fit that gene and reported in
                                  srx_wilcoxon_info.scratch_bytes, not refused.  (The tile table of the long-segment sort,
                                  about 1 B per entry of a long segment, is not counted.)  The buffer and that table are
                                  allocated by the call and released before it returns: a context keeps neither.
                                  NULL opts = {0, -1, 0, 0, 0}                                                          */
} srx_wilcoxon_opts;
typedef struct srx_wilcoxon_info {
    int32_t tie_correct;
    uint32_t n_chunks;         /* gene chunks the staging was cut into                                                  */
    uint64_t scratch_bytes;    /* staging bytes the largest chunk used                                                  */
    uint64_t segment_limit;    /* the longest stored segment (entries of one gene) the one-workgroup LDS sort takes      */
    uint64_t segments_short;   /* genes with 1 .. segment_limit stored entries                                          */
    uint64_t segments_long;    /* genes with more: the radix route                                                      */
    double ms_stage, ms_sort, ms_ranks;   /* hipEvent times, summed over the chunks; part of srx_markers_info.ms        */
} srx_wilcoxon_info;
/* Refusals as srx_rank_genes_groups[_graph], and SRX_E_ARG for n_rows >= 2^31 (the doubled rank sums must stay below 2^63)
 * and for tie_correct with n_rows > 2^21 (N^3 - N must fit 64 bits).  m is never modified.  The result is an ordinary
 * srx_markers: srx_markers_info_get, _fetch_top, _fetch_table (SRX_MARKERS_SCORE is the score above), _fetch_sizes, _free. */
int32_t srx_rank_genes_wilcoxon(srx_mat* m, const uint32_t* labels, uint32_t n_groups, const srx_wilcoxon_opts* opts,
                                srx_markers** out);
int32_t srx_rank_genes_wilcoxon_graph(srx_mat* m, srx_graph* g, const srx_wilcoxon_opts* opts, srx_markers** out);
/* T, n_cols u64.  SRX_E_ARG unless the handle was made by srx_rank_genes_wilcoxon with tie_correct. */
int32_t srx_markers_fetch_ties(srx_markers* mk, uint64_t* out);
/* SRX_E_ARG on a handle of the t-test. */
int32_t srx_markers_wilcoxon_info_get(const srx_markers* mk, srx_wilcoxon_info* info);

/* ---- highly variable genes as Seurat v3 chooses them, with batches (not in the reference) --------------------------------------
 * scanpy's pp.highly_variable_genes(flavor = "seurat_v3" / "seurat_v3_paper", batch_key = ..) on RAW counts, beside the
 * Pearson-residual selection above; it stands here because it is built on the grouped moments of this section (a batch is
 * a group).  Additive, detected by symbol, no profiling class of its own (the times are in srx_seurat_v3_info).  The
 * definition here is what is tested; the output has NOT been compared with scanpy or skmisc (neither is installed where this
 * was built).
 *
 * Input: the raw counts of a CSR handle (N cells x G genes, non-negative stored values, non-integers accepted) and optionally
 * one batch label < n_batches per cell (NULL: one batch).  Everything below is f64, without FMA contraction, in the order
 * written.
 * Step 1, batch moments.  For batch b with N_b cells: S, Q = the per-gene sum and sum of squares over the batch's stored
 *   entries, in the fixed point of srx_group_moments (its scales: integer counts give exact moments);
 *      mean = S / N_b,     var = (Q / N_b - mean * mean) * (N_b / (N_b - 1))        (not clamped)
 *   a gene is NOT CONSTANT in b when var > 0.
 * Step 2, trend.  Over the m not-constant genes of b: x = log10(mean), y = log10(var), and e_j = the value at x_j of a DIRECT
 *   loess fit: local quadratic, tricube weights, family gaussian, no robustness iterations:
 *      q = min(m, max(1, floor(span * m + 1e-5))),    h = the q-th smallest |x_i - x_j| (the point itself included),
 *      t_i = (x_i - x_j) / h,   u = |t_i|,   w_i = (1 - (u * u) * u)^3 formed as c = 1 - (u * u) * u, w = (c * c) * c,
 *      for the points with |x_i - x_j| < h (every other point has weight 0);  h == 0: the points with x_i == x_j, t = 0, w = 1.
 *   Moments over the weighted points: M_k = sum w t^k (k = 0 .. 4, each term formed as ((w t) t) ..), B_k = sum ((w t^k) y)
 *   (k = 0 .. 2).  The fitted value is the intercept of the weighted least-squares polynomial in t, by Cramer's rule:
 *      c00 = M2 M4 - M3 M3,  c01 = M1 M4 - M2 M3,  c02 = M1 M3 - M2 M2,  det = (M0 c00 - M1 c01) + M2 c02,  d2 = M0 M2 - M1 M1
 *      det > 2^-33 ((M0 M2) M4):  e = ((B0 c00 - M1 (B1 M4 - B2 M3)) + M2 (B1 M3 - B2 M2)) / det        (degree 2)
 *      else d2 > 2^-33 (M0 M2):   e = (B0 M2 - B1 M1) / d2                                              (degree 1)
 *      else                       e = B0 / M0                                                           (degree 0)
 *   This is the degree rule: fewer than three distinct weighted abscissae make det vanish, fewer than two make d2 vanish
 *   (one abscissa, h == 0 included, gives M1 = M2 = 0 exactly); each is bounded by the product it is compared with, so
 *   rounding leaves it some 2^-50 of that product and the test at 2^-33 decides the degree from the weighted moments alone,
 *   without a sort.  A window whose three abscissae are that close to two is fitted as a line.  The test reference
 *   (tests/hvg_seurat_ref.py) states the same rule.
 *   The moment sums run over the weighted points in one fixed order that depends on the value x_j alone (sorted by (x, gene
 *   index); lane l of a wave takes the points first + l, first + l + 64, ..; one butterfly), so two genes with bit-identical
 *   (mean, var) get bit-identical e wherever they sit, and results are bit-identical from call to call.  A constant gene has
 *   e = 0.
 * Step 3, clip and normalised variance.  reg_var = 10^e (pow: the one operation here that is not correctly rounded; clip and
 *   nv are formed from the value the tables report as reg_var), reg_std = sqrt(reg_var), clip = reg_std * sqrt(N_b) + mean;
 *   S_c, Q_c = the per-gene sums of min(x, clip) and of its square over the batch's stored entries, in the same fixed point
 *   and at the same two scales as step 1 (round(c 2^sum_scale_log2), round((c * c) 2^sq_scale_log2) with c = min(x, clip),
 *   ties to even, integer atomics, order-free);
 *      nv = ((N_b * (mean * mean) + Q_c) - (2 * S_c) * mean) / ((N_b - 1) * reg_var)
 * Step 4, ranks.  rank_b(j) = the number of genes before j under (nv descending, gene index ascending); nbatches_j = the number
 *   of batches with rank_b(j) < min(n_top, G); median_j = the median of those ranks (the mean of the two middle ones for an
 *   even count; NaN when nbatches_j == 0).
 * Step 5, selection.  The first min(n_top, G) genes, in rank order, under (median ascending with NaN last, nbatches
 *   descending, gene index ascending) — scanpy's "seurat_v3" — or with paper_order != 0 under (nbatches descending, median
 *   ascending, gene index ascending) — its "seurat_v3_paper".
 * Per gene: means and variances over ALL cells from the integer totals over the batches by the formulas of step 1;
 *   variances_norm = the mean of nv over the batches (added in ascending batch order, divided by n_batches).
 * Departures from scanpy: the loess surface is skmisc's "direct" — scanpy calls it with the default "interpolate" (a kd-tree
 *   and blending between its vertices), which is NOT restated; ties are broken by gene index where scanpy leaves them to an
 *   unstable argsort; ranks are kept as integers where scanpy keeps them as float32.
 * The handle is left as it was (values, dtype, moments cache, resident result), as srx_group_moments promises.
 * Refused with a message, nothing written.  SRX_E_ARG: a NULL handle, idx_out or n_out; n_top == 0; span NaN or outside (0, 1];
 *   n_batches outside 1 .. SRX_GROUPS_MAX; NULL labels with n_batches != 1; a label >= n_batches (found on the device); a batch
 *   with fewer than 2 cells; a negative stored value; a CSC handle; a context with more than one rank; an open backed session.
 *   SRX_E_NAN: a stored value is NaN or Inf. */
typedef struct srx_seurat_v3_opts {
    double  span;          /* 0 = 0.3 */
    int32_t paper_order;   /* != 0: the order of "seurat_v3_paper" */
    int32_t reserved_;
} srx_seurat_v3_opts;      /* NULL = {0, 0, 0} */
/* Host buffers, each may be NULL.  The first five hold one entry per gene, the others n_batches x G, row-major. */
typedef struct srx_seurat_v3_tables {
    double*   means;
    double*   variances;
    double*   variances_norm;
    double*   median;
    uint32_t* nbatches;
    double*   mean;
    double*   var;
    double*   fitted;      /* e */
    double*   reg_var;     /* 10^e as the device's pow gave it: the one operation that is not correctly rounded */
    double*   clip;
    double*   clip_sum;    /* S_c as f64(integer) 2^-sum_scale_log2 */
    double*   clip_sumsq;
    double*   nv;
    uint32_t* rank;
} srx_seurat_v3_tables;
typedef struct srx_seurat_v3_info {
    uint64_t n_cells, n_genes;
    uint32_t n_batches;
    int32_t  sum_scale_log2, sq_scale_log2;
    uint32_t reserved_;
    double   max_abs;
    uint64_t min_batch_cells;     /* the smallest N_b */
    double   span;                /* the value used */
    double   ms_moments, ms_loess, ms_clip, ms_rank;      /* hipEvent times of the four stages */
} srx_seurat_v3_info;
/* idx_out has room for min(n_top, n_cols) entries; *n_out = that many are written. */
int32_t srx_select_hvg_seurat_v3(srx_mat* m, uint64_t n_top, const uint32_t* batch /* n_rows, NULL: one batch */, uint32_t n_batches,
                                 const srx_seurat_v3_opts* opts, uint64_t* idx_out, uint64_t* n_out, srx_seurat_v3_tables* tables,
                                 srx_seurat_v3_info* info);
/* Step 2 alone on host arrays (x, y, fitted_out: m f64; x in any order): how the kernel is tested on its own; no stability
 * promise beyond the definition.  SRX_E_ARG: a NULL context or array, span NaN or outside (0, 1]; SRX_E_NAN: a point that is
 * NaN or Inf.  m == 0 writes nothing. */
int32_t srx_loess_direct(srx_ctx* ctx, const double* x, const double* y, uint64_t m, double span, double* fitted_out);
/* Step 3's pass alone for any clip table (clip: n_groups x n_cols f64 on the host, every entry >= 0, +inf allowed): the sums
 * of min(x, clip) and of its square per (group, gene), as srx_group_moments gives SUM and SUMSQ, with its refusals and its
 * scales (info; may be NULL) — with every clip +inf the tables equal srx_group_moments's bit for bit.  Also SRX_E_ARG: a NULL
 * clip table, a clip that is negative or NaN, an open backed session. */
int32_t srx_clipped_group_moments(srx_mat* m, const uint32_t* labels, uint32_t n_groups, const double* clip, double* sum_out,
                                  double* sumsq_out, srx_markers_info* info);

/* ---- UMAP layout of a symmetric weighted graph in 2 or 3 dimensions: what sc.tl.umap gives obsm["X_umap"] -----------------
 * Not in the reference (it stops at plot_pca and a commented-out tsne).  This is umap-learn's optimize_layout_euclidean
 * RESTATED as a synchronous, vertex-owned iteration so that the result is bit-identical from call to call (the original
 * lets threads add into positions that other threads are reading).  The definition here is what is tested; the output has
 * NOT been compared with umap-learn, which is not installed where this was built.
 *
 * Input: a symmetric graph W as CSR with exactly the contract of srx_louvain_csr (u64 indptr, u32 indices strictly
 *   ascending within a row, f64 weights > 0, no diagonal, W_ij and W_ji the same bits); nnz stored entries, entry e is its
 *   position in that CSR; n < 2^32; dim = n_components (2 or 3); E = n_epochs; curve parameters a, b > 0; gamma (repulsion
 *   strength); R = negative_sample_rate (0..32); alpha0; a 64-bit seed; start positions Y^0 (n x dim f64, finite).
 * Schedule (stateless).  w_max = the largest stored weight, r_e = w_e / w_max (one f64 division), c_e(t) = floor(t * r_e)
 *   in f64 (t converted to f64, one multiplication).  Entry e is SAMPLED in epoch t (t = 1..E) iff c_e(t) > c_e(t - 1).  An
 *   entry with c_e(E) = 0 never acts (umap-learn's pruning of weights below max / n_epochs); info.entries_active counts the
 *   entries with c_e(E) > 0.
 * Negative samples.  mix(z) is splitmix64's finaliser: z ^= z >> 30; z *= 0xBF58476D1CE4E5B9; z ^= z >> 27;
 *   z *= 0x94D049BB133111EB; z ^= z >> 31 (all mod 2^64).  For a sampled entry e in epoch t and p = 0..R-1:
 *   z = mix(seed + 0x9E3779B97F4A7C15 * (1 + (t * nnz + e) * R + p))  (mod 2^64),  target k = ((z >> 32) * n) >> 32.
 * Epoch t.  Every vertex i reads only Y^{t-1}.  alpha_t = alpha0 * (1 - (t - 1) / E).  All arithmetic is f64, every operation
 *   rounded once (no FMA contraction), d2 summed over the coordinates in ascending order.
 *   For every sampled entry (i, j) of row i:
 *     attraction: d2 = |y_i - y_j|^2;  q = ((-2 a b) * d2^(b-1)) / (a * d2^b + 1) if d2 > 0, else 0;
 *                 g = clip(q * (y_i - y_j), -4, 4) per coordinate;  delta_i += (2 alpha_t) * g.
 *       The factor 2 is the head move of (i, j) plus the tail move of (j, i): the same vector, because W is bit-symmetric,
 *       both entries carry the same schedule, and both ends are read as they stood before the epoch.
 *     repulsion, for each of its R targets k:  k == i is skipped and counted in info.negatives_skipped; otherwise
 *       d2 = |y_i - y_k|^2; if d2 > 0: q = (2 gamma b) / ((0.001 + d2) * (a * d2^b + 1)), g = clip(q * (y_i - y_k), -4, 4),
 *       delta_i += alpha_t * g; if d2 == 0 nothing is added.
 *   Then Y^t = Y^{t-1} + delta.  The sum of a row's terms may be taken in any order that is fixed by (n, indptr) alone: here
 *   SRX_UMAP_GROUP lanes own a vertex, lane s sums the terms of the entries lo + s, lo + s + SRX_UMAP_GROUP, ... of its row
 *   in that order (an entry's attraction, then its targets p = 0..R-1), and the lanes' sums meet in a butterfly.  The result
 *   is bit-identical from call to call.  x^y is the device library's pow(double, double) (ocml, documented to 1 ulp; not
 *   -ffast-math, no native_ / half_ variant).
 * stop_after = s (0 = E) runs only epochs 1..s of the E-epoch schedule.
 * Counters, exact integers: samples = the sampled (entry, epoch) pairs of the epochs run; negatives_skipped;
 *   negatives = samples * R - negatives_skipped; entries_active.
 * Starts.  SRX_UMAP_INIT_GIVEN: `init`, a host pointer to n x dim f64.  SRX_UMAP_INIT_RANDOM: coordinate c = i * dim + j is
 *   -10 + 20 * ((mix(seed + 0x9E3779B97F4A7C15 * (c + 1)) >> 11) * 2^-53).  SRX_UMAP_INIT_PCA: the first dim columns of the
 *   scores the last fit left on the matrix handle, each times s = 10 / max |score| over those columns (s one f64 division);
 *   read on the device, deterministic.
 * Curve.  srx_umap_fit_ab(spread, min_dist) is host only: the least-squares fit of 1 / (1 + a x^(2b)) to y(x) = 1 for
 *   x < min_dist and exp(-(x - min_dist) / spread) otherwise, on 300 equally spaced x in [0, 3 spread], by a two-parameter
 *   Levenberg-Marquardt from (1, 1).  opts.a == opts.b == 0 means "fit from min_dist, spread".
 * Defaults (NULL opts): min_dist 0.5, spread 1.0 (scanpy's), gamma 1, alpha0 1, R 5, dim 2, seed 0, the PCA start;
 *   n_epochs == 0 means 500 for n <= 10 000, else 200.
 * Out of scope: spectral initialisation, densMAP, supervised and non-Euclidean outputs (new points: the next section).
 * Refused with SRX_E_ARG and a message, nothing written: dim not 2 or 3; R outside 0..32; a, b (unless both 0), gamma,
 *   alpha0 or spread not finite or <= 0; min_dist < 0 or > spread (or NaN); n_epochs < 0 or > 2^20; stop_after < 0 or
 *   > n_epochs; an unknown start; a NaN or Inf start; the PCA start without a usable result (none, or fewer than dim
 *   components), with m's n_rows != n, or with m on another context; SRX_UMAP_INIT_GIVEN with init == NULL; a context with
 *   more than one rank; for srx_umap_csr also everything srx_louvain_csr refuses, and the PCA start (there is no matrix).
 * n = 0 gives an empty result; a graph without entries returns the start unchanged with samples = 0. */
#define SRX_UMAP_GROUP 8         /* lanes that own one vertex */
#define SRX_UMAP_MAX_EPOCHS 1048576
enum { SRX_UMAP_INIT_GIVEN = 0, SRX_UMAP_INIT_RANDOM = 1, SRX_UMAP_INIT_PCA = 2 };
typedef struct srx_umap_opts {
    double   a, b;                  /* both 0: fitted from min_dist, spread */
    double   min_dist, spread, gamma, alpha0;
    uint64_t seed;
    int32_t  n_epochs;              /* 0 = 500 for n <= 10 000, else 200 */
    int32_t  stop_after;            /* 0 = n_epochs */
    int32_t  n_components, negative_sample_rate, init, reserved_;
} srx_umap_opts;
typedef struct srx_umap_info {
    uint64_t n, nnz, entries_active, samples, negatives, negatives_skipped;
    uint32_t n_epochs, epochs_run, dim, reserved_;
    double   a, b, w_max;
    double   ms;                    /* hipEvent time of the device work */
} srx_umap_info;
/* The layout of the handle's connectivities, read where they lie (C and the labels are left untouched).  The embedding stays
 * on the device with the handle (srx_graph_embedding_fetch).  m: the matrix whose scores start the layout, NULL unless
 * init = SRX_UMAP_INIT_PCA; init: NULL unless SRX_UMAP_INIT_GIVEN; embedding_out (n x dim f64, row-major) and info may be NULL. */
int32_t srx_umap(srx_graph* g, srx_mat* m, const srx_umap_opts* opts, const double* init, double* embedding_out,
                 srx_umap_info* info);
/* The same on a caller-supplied symmetric graph, validated on the device as srx_louvain_csr validates its input. */
int32_t srx_umap_csr(srx_ctx* ctx, const uint64_t* indptr, const uint32_t* indices, const double* weights, uint64_t n,
                     const srx_umap_opts* opts, const double* init, double* embedding_out, srx_umap_info* info);
/* The last srx_umap's embedding, kept on the device (n x dim f64; dim_out may be NULL).  SRX_E_ARG when none has run. */
int32_t srx_graph_embedding_fetch(srx_graph* g, double* out, uint32_t* dim_out);
/* Host only.  SRX_E_ARG: spread or min_dist not finite, spread <= 0, min_dist < 0 or > spread, a null output. */
int32_t srx_umap_fit_ab(double spread, double min_dist, double* a, double* b);

/* ---- new cells on a fitted data set: the label vote and the UMAP transform; what sc.tl.ingest gives obs[...] and
 * obsm["X_umap"] of the query ------------------------------------------------------------------------------------------------
 * Not in the reference.  The transform is umap-learn's UMAP.transform RESTATED so that the result is bit-identical from call
 * to call; the vote is pandas' mode as scanpy's ingest.map_labels takes it.  The definition here is what is tested.
 * NOT compared: umap-learn, scanpy (not installed).  Projecting the new cells (srx_pca_transform) and finding their
 * neighbours among the fitted ones (srx_knn_points / srx_knn_index_search) are the sections above.
 *
 * Input: a k-NN list of n_query rows x kq entries, u32 indices into n_ref reference points and f64 distances, finite and
 *   >= 0; 3 <= kq <= 64, kq <= n_ref < 2^32; a row never names one reference twice; rows need not be sorted.  Reference
 *   positions Yref: n_ref x dim f64, finite, dim 2 or 3.  Everything below is stated on the row in ASCENDING REFERENCE INDEX
 *   order, slot s = 0..kq-1 (the order k_graph_rows makes), so the result does not depend on the order of the entries
 *   within an input row; j_s and d_s are the index and distance of slot s.
 * Membership of row i (umap-learn's smooth_knn_dist with rho_i = 0).  The row's NEAREST entry, the minimum by (distance,
 *   index), is left out of the sum S and still gets a weight: smooth_knn_dist starts at column 1 in a transform as in a fit,
 *   where column 0 is the point itself.  Over the other m = kq - 1 entries, with T = log2(kq):
 *   c_i      = those with d = 0;   S_i(s) = c_i + sum over {d > 0} of exp(-d / s).
 *   sigma*_i = the root of S_i(s) = T when c_i < T, solved to |S_i - T| <= 1e-9 by the rule of the graph section's kernel:
 *              from lo = hi = the largest d, double hi while S(hi) < T (or halve lo while S(lo) >= T), then halve the bracket
 *              — mid = lo + 0.5 (hi - lo); S(mid) < T moves lo, else hi — until it is one ulp wide or |S(mid) - T| <= 1e-13;
 *              sigma* is the upper end.  Else 0 (rows_no_root).
 *   sigma_i  = max(sigma*_i, 1e-3 * (sum_s d_s) / kq), the sum over all kq entries (rows_clamped: the floor is the larger).
 *              A departure: umap-learn's floor uses the mean distance of the whole batch; the row's own mean keeps a row's
 *              weights independent of which other cells are mapped with it.
 *   A row whose kq distances are all 0 has sigma_i = 0 and every weight 1 (rows_all_zero; it counts in rows_no_root too).
 *   w_is     = 1 when d_s = 0, else exp(-d_s / sigma_i), in f64, for all kq slots.
 *   As in the graph section the formulas are evaluated literally: a row whose sum_s d_s overflows has floor = sigma_i = +inf,
 *   every weight 1, and counts in rows_clamped (unless the doubling of hi overflowed as well: then sigma* = +inf itself and
 *   the floor is not the larger); the 1e-9 holds for distances in the normal range.
 * Start.  W_i = sum_s w_is;  y_i^0 = sum_s (w_is / W_i) * Yref[j_s] per coordinate (one division, one product per term).
 *   Both sums are the 64-lane butterfly over the slots: v_s for s < kq, 0 for s = kq..63, then for off = 32, 16, 8, 4, 2, 1
 *   every v_s becomes v_s + v_(s xor off).  W_i == 0: y_i^0 = the position of the nearest entry (rows_start_nearest).
 * Schedule, negatives, epoch: srx_umap's rules on the bipartite entries e = i * kq + s, nnz = n_query * kq.  w_max = the
 *   largest weight of the whole call; r_e, c_e(t), the sampling rule and entries_active as there.  The hash as there with
 *   target = ((z >> 32) * n_ref) >> 32: a target is a reference point, so NO target is skipped.  Epoch t reads y_i^{t-1} and
 *   Yref only; alpha_t = alpha0 * (1 - (t - 1) / E).  Attraction of a sampled entry (i, j_s): q and g as there with
 *   y_j = Yref[j_s], delta_i += alpha_t * g (the head move alone, factor 1: the reference does not move).  Repulsion from
 *   each of its R targets as there.  d2 == 0 adds nothing.  y_i^t = y_i^{t-1} + delta_i.  Lane u of the SRX_UMAP_GROUP lanes
 *   of a query sums the entries u, u + SRX_UMAP_GROUP, ... of its row in that order (an entry's attraction, then its targets
 *   p = 0..R-1), and the lanes meet in srx_umap's butterfly.  f64, no FMA contraction, ocml's pow.  Query rows do not
 *   interact: a row's result does not depend on the other rows except through w_max and, through e and nnz, its place.
 * Defaults (NULL opts; umap-learn's): alpha0 0.25 (a quarter of the fit's 1), n_epochs == 0 means 100 for n_query <= 10 000,
 *   else 30 (a third of the fit's, rounded as umap-learn does); gamma 1, R 5, seed 0, min_dist 0.5, spread 1.0; a = b = 0
 *   means fitted by srx_umap_fit_ab.  stop_after = s (0 = E) runs epochs 1..s of the E-epoch schedule.
 * How: one launch holds up to chunk_epochs (0 = SRX_UMAP_TRANSFORM_CHUNK, else 1..that) epochs, a query's position staying
 *   in registers between them; the launches run back to back on the context's stream and hand on the positions alone, so
 *   the result is the same bits for every chunk length.
 * Label vote.  A k-NN list n_query x k (1 <= k <= 64 and k <= n_ref, no reference twice in a row; distances are not read)
 *   and ref_labels[n_ref] < n_groups.  label_i = the label that occurs most often among the row's k references, ties to the
 *   LOWEST label; count_i = its number of occurrences (count / k is the confidence the Python layer reports).  Integers.
 * Refused with SRX_E_ARG and a message, nothing written: kq outside 3..64 or > n_ref; k outside 1..64 or > n_ref (vote); an
 *   index >= n_ref; a reference twice in a row; a negative, NaN or Inf distance; a NaN or Inf reference position; dim
 *   not 2 or 3, or not the resident embedding's (_graph transform); a label >= n_groups; R outside 0..32; a, b (unless both 0), gamma, alpha0 or spread not finite or <= 0;
 *   min_dist outside 0..spread; n_epochs < 0 or > SRX_UMAP_MAX_EPOCHS; stop_after outside 0..n_epochs; chunk_epochs outside
 *   0..SRX_UMAP_TRANSFORM_CHUNK; a graph handle without an embedding (_graph transform) or without labels (_graph vote);
 *   n_ref >= 2^32; a NULL list, position or label array where one is needed; a context with more than one rank.
 * n_query == 0 writes nothing but info and succeeds. */
#define SRX_UMAP_TRANSFORM_CHUNK 64   /* epochs per launch at the most: a launch stays short whatever n_epochs is */
typedef struct srx_umap_transform_opts {
    double   a, b;                  /* both 0: fitted from min_dist, spread */
    double   min_dist, spread, gamma, alpha0;
    uint64_t seed;
    int32_t  n_epochs;              /* 0 = 100 for n_query <= 10 000, else 30 */
    int32_t  stop_after;            /* 0 = n_epochs */
    int32_t  negative_sample_rate;
    int32_t  chunk_epochs;          /* 0 = SRX_UMAP_TRANSFORM_CHUNK */
} srx_umap_transform_opts;
typedef struct srx_umap_transform_out {   /* host buffers, each may be NULL */
    double*   embedding;            /* n_query x dim: y after the epochs run                 */
    double*   start;                /* n_query x dim: y^0                                    */
    double*   weights;              /* n_query x kq, in slot order                           */
    uint32_t* columns;              /* n_query x kq: the row's indices ascending (the slots) */
    double*   sigma;                /* n_query                                               */
} srx_umap_transform_out;
typedef struct srx_umap_transform_info {
    uint64_t n_query, n_ref, entries_active, samples, negatives;
    uint64_t rows_no_root, rows_clamped, rows_all_zero, rows_start_nearest;
    uint32_t kq, dim, n_epochs, epochs_run;
    double   a, b, w_max;
    double   ms;                    /* hipEvent time of the device work: membership_ms + the epochs */
    double   membership_ms;         /* the membership and start kernel alone                        */
} srx_umap_transform_info;
/* Everything from host pointers: indices / distances n_query x kq row-major, ref_embedding n_ref x dim row-major.  opts, out,
 * any pointer of out, and info may be NULL. */
int32_t srx_umap_transform_knn(srx_ctx* ctx, const uint32_t* indices, const double* distances, uint64_t n_query, uint32_t kq,
                               const double* ref_embedding, uint64_t n_ref, uint32_t dim, const srx_umap_transform_opts* opts,
                               srx_umap_transform_out* out, srx_umap_transform_info* info);
/* The same against the embedding the last srx_umap left on the handle, read where it lies (n_ref = the graph's n); the handle
 * is left as it was.  dim: what the caller's buffers are sized for; SRX_E_ARG unless it is the embedding's. */
int32_t srx_umap_transform_graph(srx_graph* g, const uint32_t* indices, const double* distances, uint64_t n_query, uint32_t kq,
                                 uint32_t dim, const srx_umap_transform_opts* opts, srx_umap_transform_out* out,
                                 srx_umap_transform_info* info);
/* The label vote; labels_out and counts_out (n_query u32 each) may be NULL. */
int32_t srx_knn_vote(srx_ctx* ctx, const uint32_t* indices, uint64_t n_query, uint32_t k, const uint32_t* ref_labels,
                     uint64_t n_ref, uint32_t n_groups, uint32_t* labels_out, uint32_t* counts_out);
/* The same under the labels the last srx_louvain left on the handle, read where they lie (n_ref = the graph's n). */
int32_t srx_knn_vote_graph(srx_graph* g, const uint32_t* indices, uint64_t n_query, uint32_t k, uint32_t* labels_out,
                           uint32_t* counts_out);

/* ---- t-SNE in 2 dimensions: perplexity affinities of a k-NN list and a Barnes-Hut layout; what sc.tl.tsne gives
 * obsm["X_tsne"] -------------------------------------------------------------------------------------------------------------
 * The reference's commented-out tsne / tsne_inplace (dim_red/mod.rs:159-227: linfa's Barnes-Hut t-SNE on top of a PCA).  The
 * method is RESTATED here so that the result is bit-identical from call to call; this definition is what is tested.  P is
 * compared with scikit-learn's binary search, and the quality of a layout (KL, label purity) with scikit-learn's exact t-SNE
 * (tests/golden/make_tsne_golden.py); the layouts themselves are NOT compared with scikit-learn point for point.
 * All arithmetic is IEEE f64, every operation rounded once: no FMA contraction, no -ffast-math, no floating-point atomics.
 * exp and log are the device library's (ocml).  mix() and G = 0x9E3779B97F4A7C15 are those of the UMAP section.
 *
 * 1. Affinities.  Input as for srx_neighbors_from_knn: every row i names k distinct neighbours j != i with finite distances
 *   d_ij >= 0; 2 <= k <= SRX_TSNE_MAX_K.  Perplexity u with 1 < u < k; u == 0 means min(30, k / 3) (refused if that is <= 1).
 *   Per row: D_j = d_ij * d_ij, m_i = min_j D_j, c_i = the number of neighbours with D_j == m_i.  H_i(beta) is the entropy, in
 *   nats, of p_j = exp(-beta (D_j - m_i)) / sum_l exp(-beta (D_l - m_i)), evaluated as log S + beta * (sum_j x_j e_j) / S with
 *   x_j = D_j - m_i, e_j = exp(-(beta * x_j)), S = sum_j e_j; it falls from log k at beta = 0 to log c_i.  If c_i >= u there is
 *   no root (info.rows_no_root): p_j = 1 / c_i on the tied neighbours, 0 elsewhere, beta_i = +inf.  Otherwise beta_i is the
 *   root of H_i(beta) = log u, solved to |H_i - log u| <= 1e-9: a bracket by factors of two from beta = 1, then bisection.  The
 *   row is put in column order first and every sum over it is a butterfly over the 64 lanes, so p does not depend on the
 *   order within an input row.  Directed entries that are exactly 0.0 stay in the pattern.
 * 2. Joint P.  For every pair joined in either direction P_ij = (p_{j|i} + p_{i|j}) / (2 n) (one addition, one division by
 *   the f64 2 n; an absent direction counts as 0).  CSR: u64 indptr, u32 indices strictly ascending in a row, f64 data, no
 *   diagonal; P_ij and P_ji are the same bits; entries equal to 0.0 are dropped and counted in info.entries_dropped (both
 *   entries of a pair count); info.n_mutual counts the pairs joined in both directions.  Bit-identical from call to call.
 * 3. Repulsion by a uniform pyramid, for positions Y (n x 2).  lo_c = min_i y_ic; ext = max_c (max_i y_ic - lo_c);
 *   side = ext * (1 + 2^-20), or 1 when ext == 0.  U_ic = min(floor(((y_ic - lo_c) / side) * 2^32), 2^32 - 1) as a u32.  Level l
 *   (1 <= l <= L) has 2^l x 2^l cells of side s_l = side * 2^-l; point i lies in cell (U_i0 >> (32 - l), U_i1 >> (32 - l)).  A cell
 *   holds the count m and the u64 integer sums SX, SY of the U of its points (order-free, exact); its centre of mass is
 *   com_c = lo_c + (f64(S_c) / f64(m)) * (side * 2^-32).  levels == 0 means L = the smallest integer with 4^(L+1) >= n, clamped
 *   to 1 .. SRX_TSNE_MAX_LEVELS.
 *   Walk, per point i, from the four level-1 cells.  An empty cell is skipped.  Otherwise d = y_i - com, d2 = d_0 d_0 + d_1 d_1:
 *     if s_l * s_l < (theta * theta) * d2 the cell is ACCEPTED (cells_accepted): q = 1 / (1 + d2), rep_i += (m * q * q) * d,
 *       z_i += m * q;
 *     otherwise, if l == L, it is OPENED EXACTLY (cells_exact): for each member j != i in ascending j, with
 *       q = 1 / (1 + |y_i - y_j|^2): rep_i += (q * q) * (y_i - y_j), z_i += q, and pairs_exact += 1;
 *     otherwise its four children are visited.
 *   theta = 0 never accepts a cell: the exact O(n^2) sum.  The terms of a point may be summed in any order fixed by (n, the
 *   cell of every point) alone: here in the order of the walk, children by ascending code 2 * ybit + xbit.  Z = sum_i z_i in an
 *   order fixed in the same way (the points ordered by finest cell, then index; workgroups of 256 such points summed by
 *   butterflies, the workgroup sums by one workgroup).
 * 4. Iteration t = 1..T, everything read from Y^{t-1}.  alpha = exaggeration and mu = 0.5 while t <= exaggeration_iters;
 *   after that alpha = 1 and mu = 0.8.  attr_i = sum over row i of P of (P_ij * q_ij) * (y_i - y_j), q_ij = 1 / (1 + |y_i - y_j|^2)
 *   (SRX_TSNE_GROUP lanes own a vertex: lane s sums the entries lo + s, lo + s + SRX_TSNE_GROUP, ... in that order, and the
 *   lanes' sums meet in a butterfly).  grad = 4 * (alpha * attr - rep / Z) per coordinate.  gain = gain + 0.2 if
 *   (grad > 0) != (vel > 0), else gain * 0.8; then gain = max(gain, 0.01); gain starts at 1 and vel at 0.
 *   vel = mu * vel - (eta * gain) * grad; y = y + vel.  learning_rate == 0 means eta = max(n / 48, 50) (scikit-learn's "auto"
 *   for this form of the gradient).  n_iter == 0 means T = 1000; stop_after = s (0 = T) runs only iterations 1..s.  After
 *   the last iteration one more pass over that Y gives info.Z and info.kl = sum_e P_e * ((log P_e - log q_e) + log Z), a
 *   row's entries summed as attr is, the rows as Z is (in index order).
 * 5. Starts.  SRX_TSNE_INIT_PCA (the default): the first two columns of the scores the last fit left on the matrix handle
 *   times s = 1e-4 / max |score| over those columns (s one f64 division).  SRX_TSNE_INIT_RANDOM: coordinate c = 2 i + j is
 *   (((mix(seed + G * (c + 1)) >> 11) * 2^-53) - 0.5) * 2e-4.  SRX_TSNE_INIT_GIVEN: `init`, n x 2 f64, finite.
 * Defaults (NULL opts, and 0 in a field that says so): theta 0.5 (taken literally in a given opts), exaggeration 12 (0),
 *   learning_rate auto (0), seed 0, n_iter 1000 (0), exaggeration_iters 250 (taken literally in a given opts: 0 = none), levels
 *   auto (0), the PCA start.
 * Refused with SRX_E_ARG and a message, nothing written (*out is left untouched): perplexity outside (1, k) or NaN; k outside
 *   2 .. SRX_TSNE_MAX_K; theta < 0, NaN or Inf; levels outside 0 .. SRX_TSNE_MAX_LEVELS; exaggeration or learning_rate
 *   negative, NaN or Inf; n_iter or exaggeration_iters negative or above SRX_TSNE_MAX_ITERS, stop_after < 0 or > T;
 *   an unknown start, a NaN or Inf start, SRX_TSNE_INIT_GIVEN without init; the PCA start without a usable result of >= 2
 *   components, with another n, or on another context; everything srx_neighbors_from_knn refuses about a list; a context
 *   with more than one rank; a null handle.  n == 0 gives an empty result; n == 1 an empty P, and the start is returned.
 * Out of scope: 3-D output and FFT-interpolated repulsion; an adaptive tree (dense clumps cost pairs_exact); more than 64
 *   neighbours (scanpy's default perplexity 30 would take 90; what the cut at 64 costs has not been measured); transforming
 *   new points; a Harmony entry point (go through srx_neighbors_harmony and srx_tsne_affinities_graph). */
#define SRX_TSNE_MAX_K 64
#define SRX_TSNE_MAX_LEVELS 12
#define SRX_TSNE_GROUP 8          /* lanes that own one vertex in the attraction */
#define SRX_TSNE_MAX_ITERS 1048576
enum { SRX_TSNE_INIT_GIVEN = 0, SRX_TSNE_INIT_RANDOM = 1, SRX_TSNE_INIT_PCA = 2 };
typedef struct srx_tsne srx_tsne;         /* owns P, beta and the last embedding on the device; free it before its context */
typedef struct srx_tsne_info {
    uint64_t n, nnz, n_mutual, rows_no_root, entries_dropped;
    uint32_t k, reserved_;
    double   perplexity;
} srx_tsne_info;
typedef struct srx_tsne_opts {
    double   theta;                 /* taken literally: 0 is the exact sum */
    double   exaggeration;          /* 0 = 12 */
    double   learning_rate;         /* 0 = max(n / 48, 50) */
    uint64_t seed;
    int32_t  n_iter;                /* 0 = 1000 */
    int32_t  exaggeration_iters;    /* taken literally: 0 = none (NULL opts: 250) */
    int32_t  stop_after;            /* 0 = n_iter */
    int32_t  levels;                /* 0 = from n */
    int32_t  init, reserved_;
} srx_tsne_opts;
typedef struct srx_tsne_run_info {
    uint64_t n, nnz;
    uint32_t n_iter, iters_run, levels, reserved_;
    double   eta, Z, kl, side;      /* Z, kl and side: of the pass over the final Y */
    uint64_t cells_accepted, cells_exact, pairs_exact;   /* the walk of the last iteration */
    double   ms;                    /* hipEvent time of the device work */
} srx_tsne_run_info;
typedef struct srx_tsne_force_info {
    uint32_t levels, reserved_;
    double   side, lo[2];
    uint64_t cells_accepted, cells_exact, pairs_exact;
} srx_tsne_force_info;
/* The affinities of a caller's list (indices n x k u32, distances n x k f64, host).  *out is written on success only. */
int32_t srx_tsne_affinities_knn(srx_ctx* ctx, const uint32_t* indices, const double* distances, uint64_t n, uint32_t k,
                                double perplexity, srx_tsne** out);
/* The same from the distances D a graph handle holds, read where they lie; the graph is left untouched. */
int32_t srx_tsne_affinities_graph(srx_graph* g, double perplexity, srx_tsne** out);
int32_t srx_tsne_info_get(const srx_tsne* h, srx_tsne_info* info);
/* P as CSR (indptr n + 1, indices and data nnz) and beta (n); any pointer may be NULL. */
int32_t srx_tsne_fetch_affinities(srx_tsne* h, uint64_t* indptr, uint32_t* indices, double* data, double* beta);
/* A diagnostic: sections 3 and 4's attr (n x 2), rep (n x 2) and z (n) at the given Y (n x 2 f64, host, finite), once, with
 * the kernels the run uses.  levels as in the options; any output may be NULL. */
int32_t srx_tsne_forces(srx_tsne* h, const double* Y, double theta, int32_t levels, double* attr_out, double* rep_out,
                        double* z_out, srx_tsne_force_info* info);
/* The layout.  m: the matrix whose scores start it, NULL unless init = SRX_TSNE_INIT_PCA; init: NULL unless
 * SRX_TSNE_INIT_GIVEN; embedding_out (n x 2 f64, row-major) and info may be NULL.  The embedding stays with the handle. */
int32_t srx_tsne_run(srx_tsne* h, srx_mat* m, const srx_tsne_opts* opts, const double* init, double* embedding_out,
                     srx_tsne_run_info* info);
/* The last srx_tsne_run's embedding (n x 2 f64).  SRX_E_ARG when none has run. */
int32_t srx_tsne_embedding_fetch(srx_tsne* h, double* out);
void    srx_tsne_free(srx_tsne* h);

/* ---- ForceAtlas2 layout of a symmetric weighted graph in 2 dimensions: what sc.tl.draw_graph(layout="fa") gives
 * obsm["X_draw_graph_fa"] ----------------------------------------------------------------------------------------------------
 * Not in the reference.  ForceAtlas2 is Jacomy, Venturini, Heymann, Bastian 2014 (PLoS ONE 9(6) e98679) with the defaults
 * scanpy passes to the fa2 package, RESTATED here so that the result is bit-identical from call to call; this definition is
 * what is tested.  The three force expressions are compared with networkx.forceatlas2_layout's (3.4.2) through the dense
 * expressions of the tests; networkx's speed control differs (it accumulates swing over the iterations and measures it against
 * positions), so its layouts are NOT compared point for point, only the quality of a layout (label purity,
 * tests/golden/make_draw_graph_golden.py).  The fa2 package, Gephi and scanpy are NOT compared: none of them is installed
 * where the tests are made.  All arithmetic is IEEE f64, every operation rounded once: no FMA contraction, no -ffast-math, no
 * floating-point atomics.  sqrt is correctly rounded; log1p is the device library's (ocml).  mix() and G are those of the
 * UMAP section.
 *
 * 1. Input.  A symmetric graph W with exactly the contract of srx_louvain_csr (u64 indptr, u32 indices strictly ascending in a
 *   row, positive finite weights, no diagonal, W_ij and W_ji the same bits) and positions Y (n x 2 f64).  Only 2-D.
 * 2. Masses.  m_i = 1 + (the number of stored entries of row i), an integer.  M_tot = n + nnz (info.total_mass) must be below
 *   2^32 (refused otherwise): the pyramid's u64 sums of m_i U_i cannot wrap then.
 * 3. Pyramid.  t-SNE's (section 3 above) with masses: lo, side, U, the levels, the cell of a point and the default L are the
 *   same.  A cell holds the integer mass M = sum m_i and the u64 sums SX = sum m_i U_i0, SY = sum m_i U_i1 over its points
 *   (order-free, exact); com_c = lo_c + (f64(S_c) / f64(M)) * (side * 2^-32).
 * 4. Repulsion of point i, kr = scaling_ratio.  The walk of t-SNE's section 3: from the four level-1 cells, children by
 *   ascending code 2 * ybit + xbit, a cell without points skipped.  For a visited cell d = y_i - com, d2 = d_0 d_0 + d_1 d_1:
 *     if s_l * s_l < (theta * theta) * d2 the cell is ACCEPTED (cells_accepted; d2 > 0 follows):
 *       rep_i += ((kr * (f64(m_i) * f64(M))) / d2) * d;
 *     otherwise, if l == L, it is OPENED EXACTLY (cells_exact): for each member j != i in ascending j, e = y_i - y_j,
 *       e2 = e_0 e_0 + e_1 e_1: if e2 > 0, rep_i += ((kr * (f64(m_i) * f64(m_j))) / e2) * e, else pairs_coincident += 1;
 *       pairs_exact counts both kinds;
 *     otherwise its four children are visited.
 *   theta = 0 never accepts a cell: the exact O(n^2) sum.  The terms of a point are added one by one in exactly this
 *   depth-first order, which depends on (n, the cell of every point) alone and not on which points share a wave or a workgroup.
 * 5. Gravity, g = gravity.  r = sqrt(y_i0 y_i0 + y_i1 y_i1); if r == 0 the term is 0.  Linear: grav_i = -(((g * f64(m_i)) / r)
 *   * y_i).  strong_gravity: grav_i = -((g * f64(m_i)) * y_i), Gephi's and networkx's form; the fa2 package multiplies by the
 *   scaling ratio once more, which is NOT done here.
 * 6. Attraction.  attr_i = -(sum over row i of f_ij * (y_i - y_j)) with f_ij = W_ij, or with linlog f_ij = W_ij * (log1p(d) / d)
 *   for d = sqrt(|y_i - y_j|^2) > 0, else 0.  SRX_FA2_GROUP lanes own a vertex: lane s sums the entries lo + s,
 *   lo + s + SRX_FA2_GROUP, ... of the row in that order (each term (f_ij * e_0, f_ij * e_1) added to the lane's sum) and
 *   the lanes' sums meet in a butterfly (offsets SRX_FA2_GROUP / 2, ..., 1); the sum is negated once.
 *   F_i = (rep_i + grav_i) + attr_i.
 * 7. Iteration t = 1..T, everything read from Y^{t-1}.  Start state: Fprev = 0, speed = 1, eff = 1.
 *   swing_i = |Fprev_i - F_i|, tract_i = 0.5 * |Fprev_i + F_i| (|v| = sqrt(v_0 v_0 + v_1 v_1)).  S = sum_i f64(m_i) * swing_i,
 *   Tr = sum_i f64(m_i) * tract_i, the rows in index order: a workgroup of 256 lanes holds 256 / SRX_FA2_GROUP consecutive
 *   rows (the lanes that do not own a row hold 0) and sums its lanes by butterflies, the wave sums left to right; one
 *   workgroup adds the workgroup sums: thread u chains the sums u, u + 256, ..., then the same workgroup sum.
 *   The speed rule (Gephi's, fa2's, networkx's estimate_factor), in this order of operations, jtol = jitter_tolerance:
 *     opt = 0.05 * sqrt(f64(n));  jt = jtol * max(sqrt(opt), min(10, (opt * Tr) / (f64(n) * f64(n))));
 *     if Tr > 0 and S / Tr > 2: if eff > 0.05, eff = eff * 0.5; then jt = max(jt, jtol);
 *     target = +inf if S == 0, else ((jt * eff) * Tr) / S;
 *     if S > jt * Tr: if eff > 0.05, eff = eff * 0.7; else if speed < 1000: eff = eff * 1.3;
 *     speed = speed + min(target - speed, 0.5 * speed).
 *   It runs on the device, as one thread of the kernel that finishes the sums; srx_fa2_speed is the same statement on the host.
 *   Then y_i = y_i + F_i * (speed / (1 + sqrt(speed * (f64(m_i) * swing_i)))) and Fprev = F.
 *   n_iter == 0 means T = 500; stop_after = s (0 = T) runs only iterations 1..s.
 * 8. Starts.  SRX_FA2_INIT_GIVEN: `init`, n x 2 f64, finite (what srx_paga_init_positions makes, for scanpy's
 *   init_pos="paga").  SRX_FA2_INIT_RANDOM: coordinate c = 2 i + j is (mix(seed + G * (c + 1)) >> 11) * 2^-53, in [0, 1): scanpy's
 *   np.random.random((n, 2)) with this hash in the place of numpy's generator.
 * Defaults of a NULL opts: theta 1.2, scaling_ratio 2, gravity 1, jitter_tolerance 1, seed 0, n_iter 500, levels auto, the
 *   hashed start, no flags.  In a given opts the four f64 parameters are taken literally (theta = 0 is the exact sum,
 *   gravity = 0 none); n_iter = 0 means 500 and levels = 0 auto.
 * Refused with SRX_E_ARG and a message, nothing written: theta, scaling_ratio, gravity or jitter_tolerance negative, NaN or
 *   Inf; levels outside 0 .. SRX_TSNE_MAX_LEVELS; n_iter negative or above SRX_FA2_MAX_ITERS, stop_after < 0 or > T; an unknown
 *   start, a NaN or Inf start, SRX_FA2_INIT_GIVEN without init; M_tot >= 2^32; everything srx_louvain_csr refuses about a
 *   graph; a context with more than one rank; a null handle.  n == 0 gives an empty result; n == 1 runs (gravity alone).
 * Out of scope: 3-D; outboundAttractionDistribution; adjustSizes; edgeWeightInfluence other than 1; an adaptive tree (dense
 *   clumps cost pairs_exact); the other igraph layouts of draw_graph (fr, drl, kk, ...); multi-rank. */
#define SRX_FA2_GROUP 8           /* lanes that own one vertex in the attraction */
#define SRX_FA2_MAX_ITERS 1048576
enum { SRX_FA2_INIT_GIVEN = 0, SRX_FA2_INIT_RANDOM = 1 };
typedef struct srx_fa2_opts {
    double   theta;                 /* taken literally: 0 is the exact sum */
    double   scaling_ratio, gravity, jitter_tolerance;
    uint64_t seed;
    int32_t  n_iter;                /* 0 = 500 */
    int32_t  stop_after;            /* 0 = n_iter */
    int32_t  levels;                /* 0 = from n */
    int32_t  init;
    int32_t  strong_gravity, linlog;   /* flags: 0 or 1 */
} srx_fa2_opts;
typedef struct srx_fa2_info {
    uint64_t n, nnz, total_mass;
    uint32_t n_iter, iters_run, levels, reserved_;
    double   speed, speed_efficiency, swing, traction;   /* after / of the last iteration */
    double   side;                                       /* of the last iteration's pyramid */
    uint64_t cells_accepted, cells_exact, pairs_exact, pairs_coincident;   /* the walk of the last iteration */
    double   ms;                    /* hipEvent time of the device work */
} srx_fa2_info;
typedef struct srx_fa2_force_info {
    uint32_t levels, reserved_;
    double   side, lo[2];
    uint64_t total_mass, cells_accepted, cells_exact, pairs_exact, pairs_coincident;
} srx_fa2_force_info;
/* The layout of the connectivities C of a graph handle, read where they lie.  init: NULL unless SRX_FA2_INIT_GIVEN;
 * layout_out (n x 2 f64, row-major) and info may be NULL.  The layout stays with the handle, in a slot of its own: labels,
 * UMAP embedding and diffusion map of the handle are left untouched. */
int32_t srx_draw_graph(srx_graph* g, const srx_fa2_opts* opts, const double* init, double* layout_out, srx_fa2_info* info);
/* The same for any symmetric graph in host CSR form, validated on the device as srx_louvain_csr validates. */
int32_t srx_draw_graph_csr(srx_ctx* ctx, const uint64_t* indptr, const uint32_t* indices, const double* weights, uint64_t n,
                           const srx_fa2_opts* opts, const double* init, double* layout_out, srx_fa2_info* info);
/* The last srx_draw_graph's layout (n x 2 f64).  SRX_E_ARG when none has run on the handle. */
int32_t srx_graph_layout_fetch(srx_graph* g, double* out);
/* A diagnostic: sections 4 to 6's rep, grav and attr (n x 2 each) and the masses (n u32) at the given Y (n x 2 f64, host,
 * finite), once, with the kernels the run uses.  Of opts (NULL: the defaults) theta, scaling_ratio, gravity, levels and the two
 * flags are read.  Any output may be NULL. */
int32_t srx_draw_graph_forces(srx_ctx* ctx, const uint64_t* indptr, const uint32_t* indices, const double* weights, uint64_t n,
                              const double* Y, const srx_fa2_opts* opts, double* rep_out, double* grav_out, double* attr_out,
                              uint32_t* mass_out, srx_fa2_force_info* info);
/* Section 7's speed rule on the host (no GPU): *speed and *eff are read and updated.  Refused: n == 0, S, Tr or
 * jitter_tolerance negative, NaN or Inf, a speed or eff that is negative or NaN, a null pointer. */
int32_t srx_fa2_speed(uint64_t n, double S, double Tr, double jitter_tolerance, double* speed, double* eff);

/* ---- Diffusion maps and pseudotime: what sc.tl.diffmap gives obsm["X_diffmap"], uns["diffmap_evals"], and sc.tl.dpt
 * (without branchings) gives obs["dpt_pseudotime"] ---------------------------------------------------------------------------
 * Not in the reference.  This is scanpy's compute_transitions with its _transitions_sym, compute_eigen and
 * DPT._set_pseudotime RESTATED below; the definition here is what is tested, and the output has NOT been compared with
 * scanpy, which is not installed where this was built.
 *
 * Input: a symmetric graph C as CSR with exactly the contract of srx_louvain_csr (u64 indptr, u32 indices strictly ascending
 *   within a row, f64 weights > 0, no diagonal, C_ij and C_ji the same bits), and every row holds an entry; 2 <= n < 2^32.
 * Transition operator.  With density_normalize: q_i = sum_j C_ij, K_ij = C_ij / (q_i * q_j); without: K = C.  Then
 *   z_i = sum_j K_ij and T_ij = K_ij / (sqrt(z_i) * sqrt(z_j)).  All f64, every operation rounded once (no FMA contraction),
 *   each product formed before its division, so T_ij and T_ji are the same bits.  A row sum is taken in an order fixed by
 *   (n, indptr) alone: SRX_DIFFMAP_GROUP lanes own a row, lane s adds the entries lo + s, lo + s + SRX_DIFFMAP_GROUP, ... in
 *   that order and the lanes' sums meet in a butterfly.  T shares C's indptr and indices; srx_graph_transitions_fetch
 *   returns its nnz values in C's order.  T is symmetric with spectrum in [-1, 1] and largest eigenvalue 1 (once per
 *   connected component).
 * Eigenpairs.  The n_comps ALGEBRAICALLY largest eigenvalues of T, descending, with orthonormal eigenvectors (n x n_comps,
 *   row-major).  n_comps is clamped to n - 1 as scanpy clamps it; info.n_comps is the value used.  scanpy asks ARPACK for the
 *   eigenvalues largest in MAGNITUDE: the two agree whenever |lambda_min| < lambda_{n_comps}, which holds on k-NN graphs
 *   (lambda_min about -0.4 .. -0.5) and fails on, e.g., an odd ring (lambda_min close to -1).  scanpy also reverses ARPACK's
 *   ascending order, as is done here.
 *   Contract, whatever the algorithm: the returned block is re-orthonormalised once, then
 *     lambda_l = v_l . (T v_l),  max_residual = max_l |T v_l - lambda_l v_l|_2,  max_ortho = max |V^T V - I|
 *   are evaluated on the device from the block as returned (sums in a fixed order) and reported.  The call succeeds only if
 *   max_residual <= tol; otherwise SRX_E_NOCONV, with info filled (max_residual is then the residual estimate of the last
 *   restart, Inf when there was none, unless the final evaluation itself failed the test) and nothing else written; the
 *   handle then holds no eigenpairs.  For symmetric T every returned lambda_l lies within max_residual of an eigenvalue.
 *   Sign: the component of largest magnitude of each vector is positive, the lowest index winning ties.
 *   Determinism: the whole result, and every field of info except ms, is bit-identical from call to call: no floating-point
 *   atomics, dot products through fixed per-workgroup slots added in a fixed order.
 * Algorithm (diffmap.hip): thick-restart Lanczos with full reorthogonalisation (classical Gram-Schmidt twice)
 *   on a resident basis of ncv columns, the projected problem solved on the host by a cyclic Jacobi once per restart.  The
 *   start vector is u_i = (mix(seed + 0x9E3779B97F4A7C15 * (i + 1)) >> 11) * 2^-53 - 0.5 with UMAP's mix(); the s-th fresh
 *   vector after it (a breakdown, beta <= 2^-40; or the start of a completeness check) uses i + 1 + s * n.  A Krylov space of
 *   one vector holds one vector per eigenspace, so after the block has converged it is locked and the iteration runs again
 *   in its orthogonal complement until that run's largest pair has converged: a value above the block's smallest (by more
 *   than tol) replaces it and the check repeats.  info.matvecs counts the products y = T x of all these runs (not the n_comps
 *   products of the final evaluation) and never exceeds max_matvecs; info.restarts the thick restarts; info.breakdowns the
 *   breakdowns (at least one whenever the basis reaches n columns).
 * Pseudotime.  Given lambda_l, V (n x m), a root r and a cap c: w_l = lambda_l / (1 - lambda_l) if lambda_l < c, else 1;
 *   d_i = sqrt(sum_{l = 0 .. m-1} (w_l * (V[r, l] - V[i, l]))^2), summed with l ascending, f64, every operation rounded once;
 *   pseudotime_i = d_i / max_j d_j over the finite d_j, and all zeros when that maximum is 0.  (scanpy: DPT._compute_Dchosen_row
 *   and _set_pseudotime; 0.9994 is its allowance for float32 eigenvalues.)
 * Defaults (NULL opts): n_comps 15, ncv max(2 n_comps + 1, 20) (clamped to n, at most 129), tol 1e-10, max_matvecs 10000,
 *   seed 0, density_normalize on.  In a given opts a zero tol, n_comps, ncv or max_matvecs means its default, and
 *   density_normalize is taken as it stands (0 = off).
 * Out of scope: DPT branchings, PAGA, an f32 operator, a spectral start inside srx_umap (pass the fetched components as
 *   SRX_UMAP_INIT_GIVEN).
 * Refused with SRX_E_ARG and a message, nothing written: n_comps outside 1..64; a non-zero ncv below n_comps + 2 or above
 *   129; a negative or NaN tol; a negative max_matvecs; n < 2; a row without entries (q = 0; srx_diffmap_csr only: a built
 *   graph has none); a context with more than one rank; srx_dpt before a successful srx_diffmap on the handle; root >= n; cap
 *   outside (0, 1] (0 = 0.9994); for srx_dpt_from m outside 1..64 or a null pointer; for srx_diffmap_csr also everything
 *   srx_louvain_csr refuses. */
#ifndef SRX_DIFFMAP_GROUP
#define SRX_DIFFMAP_GROUP 8      /* lanes that own one row */
#endif
#define SRX_DIFFMAP_MAX_COMPS 64    /* the largest n_comps (and the largest m of srx_dpt_from) */
#define SRX_DIFFMAP_MAX_NCV 129     /* the largest ncv */
typedef struct srx_diffmap_opts {
    double   tol;                   /* 0 = 1e-10 */
    uint64_t seed;
    int32_t  n_comps;               /* 0 = 15 */
    int32_t  ncv;                   /* 0 = max(2 n_comps + 1, 20) */
    int32_t  max_matvecs;           /* 0 = 10000 */
    int32_t  density_normalize;     /* NULL opts: on */
} srx_diffmap_opts;
typedef struct srx_diffmap_info {
    uint64_t n, nnz;
    uint32_t n_comps, ncv, matvecs, restarts, breakdowns, reserved_;
    double   max_residual, max_ortho;
    double   ms;                    /* hipEvent time of the solve (T is built before it) */
} srx_diffmap_info;
/* The eigenpairs of the handle's connectivities, read where they lie (C, the labels and the embedding are left untouched).  T
 * and the eigenpairs stay on the device with the handle.  evals_out (n_comps f64; room for the requested n_comps suffices),
 * evecs_out (n x n_comps f64, row-major, n_comps = the value used) and info may be NULL. */
int32_t srx_diffmap(srx_graph* g, const srx_diffmap_opts* opts, double* evals_out, double* evecs_out, srx_diffmap_info* info);
/* The same on a caller-supplied symmetric graph, validated on the device as srx_louvain_csr validates its input. */
int32_t srx_diffmap_csr(srx_ctx* ctx, const uint64_t* indptr, const uint32_t* indices, const double* weights, uint64_t n,
                        const srx_diffmap_opts* opts, double* evals_out, double* evecs_out, srx_diffmap_info* info);
/* The last successful srx_diffmap's eigenpairs (any pointer may be NULL).  SRX_E_ARG when there is none. */
int32_t srx_graph_diffmap_fetch(srx_graph* g, double* evals, double* evecs, uint32_t* n_comps_out);
/* T's values, nnz_connectivities f64 in C's order (srx_graph_fetch has indptr and indices).  SRX_E_ARG before an srx_diffmap. */
int32_t srx_graph_transitions_fetch(srx_graph* g, double* data);
/* Pseudotime from the eigenpairs the handle holds: n f64. */
int32_t srx_dpt(srx_graph* g, uint64_t root, double cap, double* pseudotime_out);
/* The same from eigenpairs on the host (evals m f64, evecs n x m row-major), e.g. what srx_diffmap_csr returned. */
int32_t srx_dpt_from(srx_ctx* ctx, const double* evals, const double* evecs, uint64_t n, uint32_t m, uint64_t root, double cap,
                     double* pseudotime_out);

/* ---- PAGA: the neighbour graph coarse-grained over the groups; what sc.tl.paga gives uns["paga"] -----------------------------
 * Not in the reference.  This is scanpy's model="v1.2" (_compute_connectivities_v1_2, _get_connectivities_tree_v1_2) RESTATED
 * below so that the result is exact and bit-identical from call to call.  The definition here is what is tested.  The output
 * has NOT been compared with scanpy (scanpy is not installed where this was built).
 *
 * Input: a directed pattern P as CSR (u64 indptr of n + 1, u32 indices, n < 2^32) and one label < n_groups per row,
 *   1 <= n_groups <= SRX_GROUPS_MAX.  For a handle P is D: n k entries, no diagonal.  Every stored entry (i, j) counts once,
 *   whatever its value and however often the pair is stored; a diagonal entry is an edge inside its group; rows need not be
 *   sorted.  A row holds fewer than 2^22 entries (a workgroup counts its rows' targets in 32-bit counters).
 * Counts, all integers in u64:
 *   n_g = the number of rows with label g,  N = n;
 *   E[g][h] = the number of stored entries with label_i = g and label_j = h, the diagonal g = h included;
 *   es_g = sum over h of E[g][h];   V[g][h] = E[g][h] + E[h][g] for g != h,  V[g][g] = 0.
 * Null model and connectivity, only where V[g][h] > 0 (every other entry of both tables is +0.0):
 *   num = es_g n_h + es_h n_g, formed exactly as an integer (128 bits: it can need 73);
 *   expected[g][h] = (double)num / (double)(N - 1)          (one rounding per conversion, one for the quotient)
 *   r = (double)V[g][h] / expected[g][h];   conn[g][h] = r > 1 ? 1.0 : r.
 *   Both tables are symmetric in the same bits.  V > 0 implies two non-empty groups, hence N >= 2.
 * Tree: the spanning forest that Kruskal's algorithm builds from the unordered pairs g < h with conn > 0, taken in the order
 *   (conn descending, g ascending, h ascending).  tree[g][h] = conn[g][h] for the chosen pairs, stored at g < h only; every
 *   other entry is 0.  (Clipping makes conn == 1.0 common, so the tie rule decides much of the tree.)
 * n == 0 gives all-zero tables with components = n_groups.
 * Start positions (scanpy's get_init_pos_from_paga with a hash in place of numpy's generator).  pos is n_groups x dim f64, the
 * caller's coarse layout, dim 2 or 3.  Per group g: nb(g) = the h with the largest conn[g][h] > 0, ties to the lowest h;
 *   dist_c = pos[g][c] - pos[nb][c].  For cell i of group g and coordinate c:
 *   u = (mix(seed + 0x9E3779B97F4A7C15 * (i * dim + c + 1)) >> 11) * 2^-53          (mix: the UMAP section's)
 *   y = (pos[g][c] - 0.5 * dist_c) + (u - 0.5) * dist_c        (f64, every operation rounded once, no FMA contraction)
 *   A group without a neighbour puts its cells exactly on pos[g].  The result is what srx_umap takes as SRX_UMAP_INIT_GIVEN.
 * Refusals, each SRX_E_ARG with a message and nothing written: a NULL handle or context where one is needed; n_groups outside
 *   1 .. SRX_GROUPS_MAX; a label >= n_groups (found on the device); labels == NULL on a handle that holds none; an index >= n;
 *   an indptr that does not start at 0 or that decreases; a row of 2^22 entries or more; n >= 2^32; a context with more than
 *   one rank; for srx_paga_from_counts NULL counts or sizes, or a non-zero count in a row or column of a group of size 0; for
 *   srx_paga_init_positions dim not 2 or 3, a NaN or Inf in pos or connectivities, NULL out with n > 0, n other than the
 *   handle's.
 * Out of scope: model="v1.0", RNA-velocity transitions, the coarse layout itself (scanpy's pl.paga), sharded contexts. */
typedef struct srx_paga_info {
    uint64_t n, nnz;
    uint32_t n_groups, groups_empty;
    uint64_t edges_inner, edges_inter;      /* the sum of E's diagonal, and the rest: the two sum to nnz               */
    uint64_t pairs_connected;               /* unordered pairs g < h with V > 0                                        */
    uint64_t pairs_clipped;                 /* ... of them, those with r > 1                                           */
    uint32_t tree_edges;
    uint32_t components;                    /* of the graph conn > 0 over all n_groups vertices: an empty group is one of
                                               its own; tree_edges = n_groups - components                             */
    double   ms;                            /* hipEvent time of the device work (0 from srx_paga_from_counts)          */
} srx_paga_info;
typedef struct srx_paga_tables {   /* host buffers, each may be NULL */
    uint64_t* sizes;          /* n_groups                 */
    uint64_t* out_edges;      /* n_groups: es             */
    uint64_t* counts;         /* n_groups x n_groups: E   */
    double*   connectivities; /* n_groups x n_groups, row-major, like the two below */
    double*   expected;
    double*   tree;
} srx_paga_tables;
/* The handle's D, read where it lies: the handle, its C, labels, embedding and diffusion map stay untouched.  labels == NULL:
 * the labels the last srx_louvain left on g, read on the device (n_groups is then srx_louvain_info.n_communities or more);
 * else n host u32, uploaded and checked on the device.  t and info may be NULL. */
int32_t srx_paga(srx_graph* g, const uint32_t* labels, uint32_t n_groups, srx_paga_tables* t, srx_paga_info* info);
/* The same on any pattern. */
int32_t srx_paga_csr(srx_ctx* ctx, const uint64_t* indptr, const uint32_t* indices, uint64_t n, const uint32_t* labels,
                     uint32_t n_groups, srx_paga_tables* t, srx_paga_info* info);
/* Everything after the counts, from E (n_groups x n_groups) and the sizes: out_edges, the three f64 tables, the tree and the
 * counters; n is the sum of the sizes and nnz the sum of counts.  Host only: it needs no GPU, and the two calls above end in
 * it.  t->sizes and t->counts receive copies of the input. */
int32_t srx_paga_from_counts(const uint64_t* counts, const uint64_t* sizes, uint32_t n_groups, srx_paga_tables* t,
                             srx_paga_info* info);
/* The start positions (n x dim f64, row-major, host).  g != NULL && labels == NULL: the handle's labels; ctx may be NULL with a
 * handle (its context is used).  connectivities: n_groups x n_groups as srx_paga gives them. */
int32_t srx_paga_init_positions(srx_graph* g, srx_ctx* ctx, const uint32_t* labels, uint64_t n, uint32_t n_groups,
                                const double* connectivities, const double* pos, uint32_t dim, uint64_t seed, double* out);

/* ---- spatial autocorrelation per gene on a neighbour graph: Moran's I and Geary's C ------------------------------------------
 * What sc.metrics.morans_i / sc.metrics.gearys_c give over obsp["connectivities"], and squidpy's gr.spatial_autocorr over a
 * spatial graph with symmetric weights, with the z-scores PySAL's esda reports under the normality assumption.  Not in the
 * reference; the definition here is what is tested.  NOT compared: scanpy, squidpy, esda (not installed where this was built).
 *
 * Input: the current stored values x of a CSR matrix (N = n_rows cells x G = n_cols genes, f32 or f64 storage) and a symmetric
 *   weighted graph w on the same N cells with zero diagonal: the connectivities C of a graph handle, read where they lie, or
 *   a caller-supplied CSR with exactly the contract of srx_louvain_csr.  nnz = the stored entries of the graph.
 * Five integer tables per gene g, all over STORED entries only (the implicit zeros enter by arithmetic, below); rint is
 *   round-to-nearest-even, every product is rounded to f64 once, in the order the brackets give, no FMA contraction:
 *   S_g = sum_i rint(x_ig 2^s_S)                 Q_g = sum_i rint((x_ig x_ig) 2^s_Q)       (srx_group_moments with one group,
 *                                                                                           bit for bit)
 *   dq_i = sum_j rint(w_ij 2^s_w), an integer;   W = sum_i dq_i;   d_i = f64(dq_i) 2^-s_w  (converted once)
 *   A_g = sum_i rint((d_i x_ig) 2^s_A)           B_g = sum_i rint((d_i (x_ig x_ig)) 2^s_B)
 *   P_g = sum over the stored entries (i, j) of the graph with j > i, both cells storing gene g, of
 *         rint((w_ij (x_ig x_jg)) 2^s_P)         (the strict upper triangle: a pair is visited once; the full double sum is 2 P)
 *   and from the graph alone  S1 = sum_ij rint((w_ij w_ij) 2^s_1),  S2 = sum_i rint((d_i d_i) 2^s_2).
 * Scales.  e(v) = the smallest integer with v < 2^e (0 for v = 0), taken no lower than -30, as for srx_group_moments;
 *   e_x = e(max |x|), e_w = e(max w), e_d = e(max d_i);  L_N = ceil(log2 N), L_E = ceil(log2 nnz):
 *   s_S = 62 - e_x - L_N          s_Q = 62 - 2 e_x - L_N          s_w = 62 - e_w - L_E          s_1 = 62 - 2 e_w - L_E
 *   s_A = 62 - e_d - e_x - L_N    s_B = 62 - e_d - 2 e_x - L_N    s_P = 62 - e_w - 2 e_x - L_E  s_2 = 62 - 2 e_d - L_N
 *   Every term is at most 2^(62 - L) in magnitude and there are at most 2^L of them, so no total can pass 2^62 and every sum
 *   fits a signed 64-bit integer; the tables do not depend on the order of the rows or of the edges and are bit-identical
 *   from call to call; integer counts with dyadic weights give exact tables while the scales are not negative; otherwise
 *   |table - exact| <= (number of terms) 2^-(scale + 1) (for A and B: relative to the d_i above, which are themselves within
 *   (row length) 2^-(s_w + 1) of the exact row sums).  A scale may be negative; none is capped.  Admitted range: max |x|,
 *   max w and max d_i below 2^255 (refused beyond: x x, d (x x) and w (x x) must stay finite and every 2^scale a normal
 *   double; the smallest scale is then about -830).
 * Statistics: host code on the tables, in x87 extended precision (long double, 64-bit significand: every table converts
 *   exactly).  With S, Q, A, B, P, W the tables times 2^-scale (exact), N as a long double, every operation rounded once in
 *   the order written:
 *   den: in integers.  a = N Q_int and b = S_int^2 are formed exactly in 128 bits; sh = 2 s_S - s_Q = 62 - L_N;
 *        D = a - (b >> sh) (exact), r = b mod 2^sh.  N den 2^(2 s_S) = D 2^sh - r exactly, so den > 0 exactly when D >= 1.
 *        den = ((ld(D) 2^sh - ld(r)) 2^(-2 s_S)) / N                                  relative error at most 2^-61
 *   A gene whose den is not > 0 is constant (all-zero genes included): its I, C and both z are NaN, as in scanpy, and it is
 *   counted in info.genes_constant.  (The decision is exact where the tables are; a constant gene of values whose squares
 *   are not representable can land either side of 0.)
 *   t1 = 2 P;  t2 = (2 (S A)) / N;  t3 = (((S S) W) / N) / N;  num_I = (t1 - t2) + t3
 *   I = ((N num_I) / W) / den                  |I - I(tables)| <= 2^-52 |I| + 2^-60 (N / (W den)) (|t1| + |t2| + |t3|)
 *   num_C = B - 2 P;  C = (((N - 1) num_C) / W) / den                                 |C - C(tables)| <= 2^-52 |C|
 *   (num_I cancels heavily when I is near 0: its bound is absolute in the terms; everything else is relative.)
 *   These are the textbook double sums with z = x - m over ALL cells, m = S / N, the implicit zeros included:
 *   sum_ij w_ij z_i z_j = 2P - 2 m A + m^2 W,   sum_ij w_ij (x_i - x_j)^2 = 2B - 4P,   sum_i z_i^2 = Q - N m^2 = den,
 *   I = (N / W) sum_ij w_ij z_i z_j / den,      C = (N - 1) sum_ij w_ij (x_i - x_j)^2 / (2 W den).
 * z-scores under normality (Cliff & Ord; esda's formulas).  s0 = W, s1 = 2 S1 2^-s_1, s2 = 4 S2 2^-s_2 (exact in long double):
 *   E[I] = -1 / (N - 1)         Var[I] = (N^2 s1 - N s2 + 3 s0^2) / ((N^2 - 1) s0^2) - E[I]^2
 *   E[C] = 1                    Var[C] = ((2 s1 + s2)(N - 1) - 4 s0^2) / (2 (N + 1) s0^2)
 *   z = (stat - E) / sqrt(Var), from the long double stat; NaN where Var is not > 0.
 * Refusals, each with a message.  SRX_E_ARG: a NULL handle, a CSC handle, more than one rank, 2^32 - 1 rows or more, a graph
 *   whose n differs from n_rows, handles of different contexts, N < 2, a graph without stored entries (W = 0), max |x|, max w
 *   or max d_i not below 2^255, everything srx_louvain_csr refuses.  SRX_E_NAN: a stored value is NaN or Inf.  SRX_E_OOM: the
 *   tables do not fit.  m is never modified: its values, version, moments cache and resident PCA result stay as they were
 *   (the pattern-only gene tiles of srx_matrix_prepare are built if the handle has none yet); the graph handle is only read.
 * Out of scope: row-standardised or otherwise asymmetric weights (squidpy's default transformation; the directed distances D
 *   are not accepted either), dense values such as obsm columns, permutation p-values, multiple-testing correction, sharded
 *   contexts. */
typedef struct srx_autocorr_opts {
    uint32_t rows_per_block;   /* rows a workgroup of the walk takes; 0 = chosen from N and the gene tiles.  The tables do not
                                  depend on it.  NULL opts = {0}                                                            */
    uint32_t reserved_;
} srx_autocorr_opts;
typedef struct srx_autocorr_out {   /* host buffers of n_cols entries, each may be NULL */
    double*  morans_i;
    double*  gearys_c;
    double*  z_i;
    double*  z_c;
    double*  sum;          /* f64(table) 2^-scale: S, Q, A, B, P */
    double*  sumsq;
    double*  dsum;
    double*  dsumsq;
    double*  cross;
    int64_t* sum_int;      /* the tables themselves */
    int64_t* sumsq_int;
    int64_t* dsum_int;
    int64_t* dsumsq_int;
    int64_t* cross_int;
} srx_autocorr_out;
typedef struct srx_autocorr_info {
    uint64_t n, n_genes, nnz;                 /* N, G, stored entries of the graph                                        */
    int32_t  s_sum, s_sumsq, s_dsum, s_dsumsq, s_cross, s_w, s_1, s_2;     /* the scales s_S, s_Q, s_A, s_B, s_P, s_w, s_1, s_2 */
    double   max_abs, max_weight, max_degree; /* max |x|, max w, max d_i                                                  */
    int64_t  w_int, s1_int, s2_int;           /* W, S1, S2 as integers                                                    */
    double   w, s1, s2;                       /* s0 = W, s1, s2 rounded to f64                                            */
    double   e_i, var_i, e_c, var_c;
    uint64_t genes_constant;
    double   ms;                              /* hipEvent time of the device work: the three parts below                  */
    double   ms_graph, ms_moments, ms_walk;   /* the graph sums with their read-backs | S, Q, A, B | the walk for P       */
    double   ms_wmax, ms_degrees, ms_s2;      /* per kernel, within ms_graph: k_ac_wmax, k_ac_degrees, k_ac_s2            */
    double   ms_sum_sumsq, ms_dsum_dsumsq;    /* per kernel, within ms_moments: the {S, Q} launch, the {A, B} launch      */
} srx_autocorr_info;
/* The handle's C, read where it lies.  opts, out and info may be NULL. */
int32_t srx_autocorr(srx_mat* m, srx_graph* g, const srx_autocorr_opts* opts, srx_autocorr_out* out, srx_autocorr_info* info);
/* The same on a caller-supplied symmetric graph of n vertices, validated on the device as srx_louvain_csr validates its input. */
int32_t srx_autocorr_csr(srx_mat* m, const uint64_t* indptr, const uint32_t* indices, const double* weights, uint64_t n,
                         const srx_autocorr_opts* opts, srx_autocorr_out* out, srx_autocorr_info* info);
/* The scale rule alone, host code: info goes in with n, nnz, max_abs, max_weight and max_degree set and comes back with the
 * eight scales; the device calls use exactly this.  SRX_E_ARG: NULL, n < 2 or n >= 2^32 - 1, nnz == 0, a maximum that is
 * negative, NaN or not below 2^255. */
int32_t srx_autocorr_scales(srx_autocorr_info* info);
/* The statistics from five tables of n_genes integers each: host code, no GPU; the two calls above end in it.  info goes in
 * with n, the eight scales and w_int, s1_int, s2_int set, and comes back with n_genes, w, s1, s2, both E and Var and
 * genes_constant filled as well; every other field is left as it was.  out: its *_int pointers are ignored, the f64 tables
 * are written from the input.  SRX_E_ARG: a NULL table or info, n < 2 or n >= 2^32 - 1, w_int <= 0, 2 s_sum - s_sumsq outside
 * 0 .. 62. */
int32_t srx_autocorr_from_tables(const int64_t* sum_int, const int64_t* sumsq_int, const int64_t* dsum_int, const int64_t* dsumsq_int,
                                 const int64_t* cross_int, uint64_t n_genes, srx_autocorr_info* info, srx_autocorr_out* out);

/* ---- Harmony: batch integration of the PCA scores, what sc.external.pp.harmony_integrate gives obsm["X_pca_harmony"] --------
 * Not in the reference.  This is Harmony (Korsunsky et al. 2019) as harmonypy runs it for ONE batch covariate, RESTATED below
 * with its random choices replaced by hashes so that the result is bit-identical from call to call.  The definition here is
 * what is tested; the output has NOT been compared with harmonypy or the R package, neither of which is installed where this
 * was built.
 *
 * All arithmetic is f64.
 * Input.  Z, n x d with finite entries (the leading n_dims coordinates of the points); batch labels b_i < B; a batch may be
 *   empty.  N_b = the batch's cell count, P_b = N_b / n.  K clusters, K <= n.
 * Hashes.  mix() is the splitmix64 finaliser of the UMAP section, G = 0x9E3779B97F4A7C15,
 *   H(a, i) = mix(seed + G * (1 + a * 2^32 + i))  (mod 2^64).
 * Cosine rows.  Zhat_i = X_i / |X_i|, |X_i|^2 summed in ascending coordinate order; a row of norm 0 gives Zhat_i = 0.
 * Start.  The K start cells are those with the smallest (H(0, i), i); their Zhat rows are Y_0 .. Y_{K-1} in that order.  Then
 *   init_iters rounds of spherical k-means: c_i = argmax_k Zhat_i . Y_k (ties to the lowest k), Y_k = s_k / |s_k| with
 *   s_k = sum_{c_i = k} Zhat_i.  A cluster without a member, or whose s_k is 0, keeps its Y_k; this rule holds wherever a
 *   centroid is normalised.  Then dist_ik = 2 (1 - Zhat_i . Y_k), R_i = softmax_k(-dist_ik / sigma) (the row maximum is
 *   subtracted before exp), O_kb = sum_{i in b} R_ik, E_kb = (sum_i R_ik) P_b.
 * Objective.  o = sum R_ik dist_ik + sigma sum R_ik log R_ik + sigma theta sum_ik R_ik log((O_{k b_i} + 1) / (E_{k b_i} + 1)),
 *   with 0 log 0 = 0.
 * Round r = 1 .. max_rounds.  t counts the cluster iterations of the whole run from 0.  Iteration j = 1 .. max_cluster_iters:
 *   1. Y_k = normalise(sum_i R_ik Zhat_i).
 *   2. dist from Zhat and Y.
 *   3. Cell i is in block q_i = H(1 + t, i) mod n_blocks.  For q = 0 .. n_blocks - 1 in order (an empty block changes nothing):
 *      the block's rows are taken out, O_kb -= sum_{i in q, b} R_ik and E_kb -= (sum_{i in q} R_ik) P_b; for the block's cells
 *      R_i = softmax_k(-dist_ik / sigma + theta log((E_{k b_i} + 1) / (O_{k b_i} + 1))); the new rows are added back.
 *   4. t += 1; o_j = the objective.
 *   5. With epsilon_cluster > 0 the round stops when j >= 6 and (old - new) / |old| < epsilon_cluster, old = o_{j-5} + o_{j-4}
 *      + o_{j-3}, new = o_{j-2} + o_{j-1} + o_j.
 *   h_r (info.round_objective[r - 1]) is the last o_j of the round.
 * Correction, always from the original Z: the closed form of harmonypy's moe_correct_ridge for a one-hot design with an
 *   unpenalised intercept (it agrees with a dense solve of the (B + 1) x (B + 1) system to rounding):
 *   m_kb = sum_{i in b} R_ik;  S_kb = sum_{i in b} R_ik Z_i;  s_k = sum_b lambda m_kb / (m_kb + lambda);
 *   w0_k = (sum_b lambda S_kb / (m_kb + lambda)) / s_k;  W_kb = (S_kb - m_kb w0_k) / (m_kb + lambda), W_k = 0 when s_k == 0;
 *   Z_corr_i = Z_i - sum_k R_ik W_{k b_i}.  Then Zhat = the cosine rows of Z_corr; Y, R, O and E stay as they are.
 * Stopping.  With epsilon_harmony > 0 the run stops after round r >= 2 when (h_{r-1} - h_r) / |h_{r-1}| < epsilon_harmony and
 *   sets info.converged; it also stops at max_rounds.  An epsilon of 0 never stops early.
 * Order of summation.  A sum over cells is a chain over the cells of a contiguous chunk in ascending order followed by chains
 *   over the chunks (runs of consecutive chunks, then the runs; for S_kb the chunks hold the cells of batch b in ascending
 *   order); chunk and run sizes depend on (n, d, K, B) alone.  The
 *   sums over k of one cell (softmax, objective) are a per-lane chain over k = l, l + 64, .. and a butterfly over the 64 lanes.
 *   No floating-point atomics: every table, and every field of info except ms, is bit-identical from call to call.  The
 *   running O and E differ from sums re-derived from the final R by rounding only.
 * Defaults (NULL opts): theta 2, sigma 0.1, lambda 1, epsilon_cluster 1e-5, epsilon_harmony 1e-4, seed 0.  In a given opts
 *   the five doubles are taken literally; a zero n_clusters means max(1, min((n + 15) / 30, 100)) (integer division: n / 30
 *   rounded, halves up), a zero n_blocks 20, max_rounds 10, max_cluster_iters 20, init_iters 10 (-1 = none), n_dims all.
 * Out of scope: per-batch theta, lambda and sigma; several covariates; the tau discount; lambda estimation; reference mapping.
 * Refused with SRX_E_ARG and a message, nothing written (*out is left untouched): a null handle pointer, null labels or
 *   points with n > 0; theta < 0, sigma <= 0, lambda <= 0, a negative epsilon, any of them NaN or Inf; n_clusters outside
 *   0 .. SRX_HARMONY_MAX_CLUSTERS or above n; n_batches outside 1 .. SRX_HARMONY_MAX_BATCHES; n_blocks outside 0 .. 65536;
 *   max_rounds outside 0 .. SRX_HARMONY_MAX_ROUNDS; max_cluster_iters or init_iters above 65536 (or below 0, -1); a label
 *   >= n_batches; NaN or Inf in the points; n_dims above the points' coordinates, or a coordinate count outside
 *   1 .. SRX_KNN_MAX_DIMS; no PCA result on m; n >= 2^32 - 1; a context with more than one rank.  SRX_E_OOM when device memory
 *   cannot be had.  n == 0 gives an empty handle (its fetches write nothing). */
#define SRX_HARMONY_MAX_CLUSTERS 256
#define SRX_HARMONY_MAX_BATCHES  256
#define SRX_HARMONY_MAX_ROUNDS   64
typedef struct srx_harmony srx_harmony;   /* owns Z_corr, R, Y, O, E on the device; free it before its context */
typedef struct srx_harmony_opts {
    double   theta, sigma, lambda;
    double   epsilon_cluster, epsilon_harmony;
    uint64_t seed;
    int32_t  n_clusters;            /* 0 = max(1, min((n + 15) / 30, 100)) */
    int32_t  n_blocks;              /* 0 = 20 */
    int32_t  max_rounds;            /* 0 = 10 */
    int32_t  max_cluster_iters;     /* 0 = 20 */
    int32_t  init_iters;            /* -1 = none, 0 = 10 */
    int32_t  n_dims;                /* leading coordinates used, 0 = all */
} srx_harmony_opts;
typedef struct srx_harmony_info {
    uint64_t n;
    uint32_t d, n_batches, n_clusters, n_blocks, rounds, converged;
    uint64_t cluster_iters;         /* over all rounds */
    uint32_t round_iters[SRX_HARMONY_MAX_ROUNDS];
    double   round_objective[SRX_HARMONY_MAX_ROUNDS];
    double   ms;                    /* hipEvent time of the device work */
} srx_harmony_info;
enum { SRX_HARMONY_CORRECTED = 0 /* n x d */, SRX_HARMONY_R = 1 /* n x K */, SRX_HARMONY_CENTROIDS = 2 /* K x d */,
       SRX_HARMONY_OBSERVED = 3 /* K x B */, SRX_HARMONY_EXPECTED = 4 /* K x B */ };
/* The scores the last fit left on m, read where they lie with their leading dimension and left untouched (the cells are the
 * column axis of a CSC handle, as for srx_knn_result); batch: n host labels.  *out is written on success only; info may be NULL. */
int32_t srx_harmony_result(srx_mat* m, const uint32_t* batch, uint32_t n_batches, const srx_harmony_opts* opts, srx_harmony** out,
                           srx_harmony_info* info);
/* The same for caller-supplied points (n x d f64, row-major, host). */
int32_t srx_harmony_points(srx_ctx* ctx, const double* points, uint64_t n, uint64_t d, const uint32_t* batch, uint32_t n_batches,
                           const srx_harmony_opts* opts, srx_harmony** out, srx_harmony_info* info);
/* One table, row-major f64. */
int32_t srx_harmony_fetch(srx_harmony* h, int32_t which, double* out);
int32_t srx_harmony_info_get(const srx_harmony* h, srx_harmony_info* info);
/* srx_knn_result / srx_neighbors_result over the handle's corrected block, read where it lies: the same search, the same
 * refusals, an ordinary srx_graph (Louvain, UMAP, diffusion maps and the _graph marker entries take it unchanged). */
int32_t srx_knn_harmony(srx_harmony* h, const srx_knn_opts* opts, uint32_t* indices_out, double* distances_out, srx_knn_info* info);
int32_t srx_neighbors_harmony(srx_harmony* h, const srx_knn_opts* opts, srx_knn_info* knn_info, srx_graph** out);
void    srx_harmony_free(srx_harmony* h);

/* ---- BBKNN: batch-balanced neighbours, their graph, and the trimming of a graph's connectivities -----------------------------
 * What bbknn (Polanski et al. 2020; sc.external.pp.bbknn) gives obsp["distances"] / obsp["connectivities"]: the scores stay as
 * they are, and every cell takes its neighbours from EACH batch, so that Louvain, UMAP, PAGA, diffusion maps, the t-SNE
 * affinities and the SNN graph run unchanged on a batch-balanced graph.  Not in the reference.  The definition below is what
 * is tested; the bbknn package, scanpy and umap-learn are NOT installed where this was built and the output has NOT been
 * compared with any of them.
 *
 * Input: n points with d coordinates as srx_knn_* takes them (f64, row-major, finite, 1 <= d <= SRX_KNN_MAX_DIMS, the first
 *   n_dims used); one batch label < B per point, batch b has n_b points; k_within = neighbors_within_batch (default 3).
 * Distance, order, ties: exactly those of srx_knn_*: dist2 summed in f64 in difference form, in coordinate order; the
 *   reported distance is its sqrt; the order is (distance, index of the ORIGINAL point), ties to the lower index.
 * The list: row i holds K = k_within B - 1 entries: from every batch b != batch(i) the k_within nearest points of b, from its
 *   own batch the k_within - 1 nearest points other than i itself; indices are those of the caller's points; the row is
 *   ascending by (distance, index), the distance being the reported one (each batch's points are chosen by dist2, as
 *   srx_knn_* chooses them; two dist2 one ulp apart can share their sqrt).  This is bbknn's list with the cell taken out: bbknn queries every batch for k_within
 *   neighbours and finds the cell itself in its own batch, its n_neighbors = k_within B counts the cell, and umap-learn
 *   then skips column 0.  This library's graph convention is "rows without self, T = log2(k + 1)", so the two agree with
 *   k = K.  Stated departure: bbknn leaves "the cell is its own nearest neighbour" to the index; here self is excluded by
 *   identity, so exact duplicates with lower indices cannot displace it.
 * Graph: srx_neighbors_from_knn's graph of that list, unchanged: rho, sigma and A as there, C = A + A^T - A o A^T, D holds
 *   the list (bbknn's set_op_mix_ratio = 1 and local_connectivity = 1 are its defaults and the only values built).
 * Trimming of a symmetric graph C with an integer trim >= 1 (bbknn's `trimming`): for each row i let L_i be its stored
 *   length; t_i = 0 when L_i <= trim, otherwise t_i is the trim-th largest stored value of row i, counted with multiplicity.
 *   An entry (i, j) is kept if and only if C_ij >= t_i and C_ij >= t_j.  Values at a threshold are kept, so a trimmed row may
 *   stay longer than trim.  The comparison is of the f64 values; C_ij and C_ji are the same bits, so the result is exactly
 *   symmetric, has no diagonal and is bit-identical from call to call.  (bbknn computes the thresholds once and runs two
 *   passes of "zero the row entries below the row's threshold, transpose": that loop equals the closed form.)
 *   opts.trim < 0: the default 10 k_within B (bbknn's 10 * knn_distances.shape[1]); 0: no trimming; > 0: that value.
 *   D, rho, sigma and the directed weights are never trimmed, as in bbknn.
 * Refusals, each SRX_E_ARG with a message, nothing written: K outside 1 .. 64, i.e. k_within B <= 65, the limit every
 *   consumer of a list has (3 neighbours per batch allow 21 batches); k_within < 1; B outside 1 .. 65; NULL labels with
 *   B != 1; a label >= B (found on the device); a batch with fewer than k_within points, an empty batch included (bbknn
 *   raises here too); those of srx_knn_points (NaN / Inf, d, n_dims, more than one rank, n >= 2^32 - 1).  There is no
 *   include_self option.  n == 0 gives an empty graph.
 * Not built: an approximate per-batch search (annoy / pynndescent / the IVF index above), other metrics, set_op_mix_ratio /
 *   local_connectivity other than 1, sharded contexts.
 * The result is an ordinary srx_graph with info.k = K: srx_louvain, srx_umap, srx_draw_graph, srx_paga, srx_diffmap,
 *   srx_snn_graph, srx_tsne_affinities_graph and srx_autocorr read it unchanged. */
typedef struct srx_bbknn_opts {
    int32_t neighbors_within_batch;   /* 0 = 3 */
    int32_t n_dims;                   /* 0 = all */
    int64_t trim;                     /* < 0: 10 * k_within * B; 0: none; > 0: that many */
} srx_bbknn_opts;                     /* NULL = {0, 0, -1} */
typedef struct srx_trim_info {
    uint64_t trim;                    /* value used; 0: none */
    uint64_t rows_over_trim;          /* rows with L_i > trim */
    uint64_t nnz_before, nnz_after, entries_trimmed;   /* stored (directed) entries; the difference is even */
    uint64_t max_row_nnz_before, max_row_nnz_after, rows_emptied;
    uint32_t wave_capacity, short_capacity;  /* longest row each selection route takes (as srx_snn_info) */
    uint32_t reserved_[2];
    uint64_t rows_wave, rows_short, rows_long;   /* rows over trim by selection route; they sum to rows_over_trim */
} srx_trim_info;
typedef struct srx_bbknn_info {
    uint64_t n;
    uint32_t n_batches, neighbors_within_batch, k /* K */, d;
    uint64_t min_batch_cells, max_batch_cells;
    uint32_t n_searches, reserved_;
    uint64_t pairs_searched;          /* sum of n_query * n_ref over the searches */
    uint64_t rows_certified, rows_recomputed;      /* summed over the searches */
    srx_trim_info trim;
    double ms, ms_sort, ms_search, ms_merge, ms_graph, ms_trim;   /* hipEvent times */
} srx_bbknn_info;
/* On the scores the last fit left on m, read where they lie (no host round trip, like srx_neighbors_result); batch: n host
 * labels (NULL allowed when n_batches == 1).  opts and info may be NULL. */
int32_t srx_bbknn_result(srx_mat* m, const uint32_t* batch, uint32_t n_batches, const srx_bbknn_opts* opts, srx_bbknn_info* info,
                         srx_graph** out);
/* On caller-supplied points (n x d f64, row-major, host).  indices_out / distances_out: n x K, either may be NULL, receive
 * the list as defined; out may be NULL when only the list is wanted. */
int32_t srx_bbknn_points(srx_ctx* ctx, const double* points, uint64_t n, uint64_t d, const uint32_t* batch, uint32_t n_batches,
                         const srx_bbknn_opts* opts, uint32_t* indices_out, double* distances_out, srx_bbknn_info* info,
                         srx_graph** out);
/* On the corrected block of a Harmony handle, read where it lies. */
int32_t srx_bbknn_harmony(srx_harmony* h, const uint32_t* batch, uint32_t n_batches, const srx_bbknn_opts* opts,
                          srx_bbknn_info* info, srx_graph** out);
/* The trimming alone, on the C block of ANY graph handle (neighbours, index, SNN, BBKNN), trim > 0.  g is untouched; *out is
 * a new handle with a copy of g's D block, scales and directed weights and the trimmed C; its srx_graph_info is g's with
 * nnz_connectivities and max_row_nnz updated.  info may be NULL. */
int32_t srx_graph_trim(srx_graph* g, int64_t trim, srx_trim_info* info, srx_graph** out);

/* ---- Doublet detection: simulate, project, score; what sc.pp.scrublet gives obs["doublet_score"], obs["predicted_doublet"] ---
 * Not in the reference.  This is Scrublet (Wolock et al. 2019) RESTATED below, with its random parent pairs replaced by a hash
 * so that the result is bit-identical from call to call and its embedding replaced by this library's pipeline.  The definition
 * here is what is tested; the output has NOT been compared with the `scrublet` package, scanpy or scikit-image, none of which
 * is installed where this was built.  n = the observed cells; mix() and G = 0x9E3779B97F4A7C15 are those of the UMAP section.
 *
 * 1. Simulation.  n_sim = round(sim_ratio * n), r = n_sim / n as a double; round(x) = floor(x + 0.5) here and in section 3.  The
 *    parents of synthetic row s are
 *      p(s, c) = ((mix(seed + G * (1 + 2 s + c)) >> 32) * n) >> 32,   c = 0, 1   (mod 2^64; with replacement, p(s, 0) == p(s, 1)
 *    allowed as in Scrublet), or the 2 n_sim parents the caller gives.  Row s of the synthetic matrix is
 *    counts[p(s, 0), :] + counts[p(s, 1), :]: the union of the two patterns, columns ascending and unique; a column of both
 *    parents holds a + b rounded once in the storage type (exact for counts below 2^24 at f32 storage, 2^53 at f64), a column
 *    of one parent that value.  A stored entry stays stored when its sum is 0.0.  The result is an ordinary srx_mat in the
 *    parent's value storage, logical dtype F32 at f32 storage and F64 at f64 storage (a u8 parent does not wrap at 255 + 255),
 *    with the parent's n_cols; every entry point that takes an srx_mat accepts it.  It is bit-identical from call to call: no
 *    atomics, every output position is computed on its own.
 * 2. Embedding.  `fitted` holds a PCA result for the same n cells and the same gene axis (in practice a clone of the counts after
 *    srx_pipeline).  Rows [0, n) of the point block are its resident scores, copied device to device bit for bit; rows
 *    [n, n + n_sim) are what srx_pca_transform gives for the synthetic matrix under srx_pca_model_from_result(fitted),
 *    feat == NULL and the caller's target_sum and transform bits (the caller names what was applied to `fitted`; both bits =
 *    the pipeline's write-back rounding, as documented there), written straight into the block.
 * 3. Neighbours.  k_adj = round(k * (1 + r)); k == 0 means round(0.5 * sqrt(n)).  The exact self search of srx_knn_result over
 *    all n + n_sim points, include_self = 0, the first n_dims coordinates, that section's tie rule.  k_adj outside
 *    1 .. SRX_DOUBLET_MAX_K is SRX_E_ARG: at r = 2 this allows k <= 21, and scanpy's default k exceeds that for more than
 *    about 1 800 cells — the caller then chooses k, or a smaller sim_ratio (t-SNE carries the same 64-neighbour limit).
 * 4. Scores.  For each of the n + n_sim rows, k_d = its neighbours with index >= n, rho = expected_rate, se_rho = stdev_rate:
 *      q     = (k_d + 1) / (k_adj + 2)
 *      D     = 1 - rho - q * (1 - rho - rho / r)
 *      Ld    = q * rho / r / D
 *      se_q  = sqrt(q * (1 - q) / (k_adj + 3))
 *      se_Ld = q * rho / r / (D * D) * sqrt((se_q / q * (1 - rho))^2 + (se_rho / rho * (1 - q))^2)
 *    in f64, in the order written (products and quotients left to right), no contraction, no fast-math.  Ld of rows [0, n) are
 *    the observed scores, those of [n, n + n_sim) the simulated ones.
 * 5. Threshold (host code): scikit-image's threshold_minimum, which Scrublet's call_doublets applies to the simulated scores.
 *    Histogram: 256 equal bins over [min, max], the bin of x is min(255, floor((x - min) / (max - min) * 256)), the centre of
 *    bin b is min + (b + 0.5) * (max - min) / 256, counts held as doubles.  A smoothing round is
 *    s'[i] = (s[i-1] + s[i] + s[i+1]) / 3 summed left to right with s[-1] = s[0], s[256] = s[255].  After each round the maxima:
 *    walk i = 0 .. 254 with a direction that starts as rising; while rising, s[i+1] < s[i] records a maximum at i and turns to
 *    falling; while falling, s[i+1] > s[i] turns to rising.  Stop at the first round with fewer than three maxima (at least
 *    one round is made; the limit is SRX_DOUBLET_MAX_ROUNDS).  Exactly two maxima m0 < m1 below the limit: the threshold is the
 *    centre of the first minimum of s on [m0, m1], found = 1.  Otherwise (fewer than two maxima, the limit reached, fewer than
 *    2 scores, max == min, a non-finite score): threshold NaN, found = 0, nothing is predicted and the rates are NaN; this is
 *    not an error status.  A caller's threshold > 0 replaces all of this (threshold_found and smooth_rounds are then 0).
 *    With a threshold t: predicted[i] = Ld_obs[i] > t, z[i] = (Ld_obs[i] - t) / se_obs[i], detected_rate = mean(Ld_obs > t),
 *    detectable_fraction = mean(Ld_sim > t), overall_rate = detected_rate / detectable_fraction.
 * Not done: UMI subsampling of the synthetic rows (synthetic_doublet_umi_subsampling < 1); Scrublet's own gene filter and
 *    z-scoring (the embedding is this library's pipeline); more than SRX_DOUBLET_MAX_K neighbours.
 * The simulation's count and fill passes give a wave to a synthetic row whose parents hold up to SRX_DOUBLET_WAVE_ROW entries
 *    together and a workgroup to a longer one; the result does not depend on which.
 * Refused with SRX_E_ARG and a message, nothing launched (*out is left untouched): a NULL argument (info, parents and
 *    parents_out may be NULL); counts in CSC storage (convert with srx_matrix_to_csr); a context with more than one rank; fitted
 *    without a PCA result, or with the PCA of a dense residual matrix (srx_pca_pearson, srx_pca_regress: no model to project with); cell or gene counts of the two matrices that differ; n == 0; n_sim == 0 in srx_doublets_result;
 *    n + n_sim >= 2^32; sim_ratio negative or non-finite; expected_rate outside (0, 1); stdev_rate negative or NaN; bad
 *    transform bits; k negative; k_adj outside 1 .. SRX_DOUBLET_MAX_K or above n + n_sim - 1; n_dims above the scores'
 *    components; in the list form k_adj == 0, n_obs == 0 or an index >= n_obs + n_sim.  SRX_E_BOUNDS: a given parent >= n.
 *    srx_doublets_simulate with n_sim == 0 gives an empty matrix of n_cols columns. */
#define SRX_DOUBLET_MAX_K 64
#define SRX_DOUBLET_MAX_ROUNDS 10000
#define SRX_DOUBLET_WAVE_ROW 8192
typedef struct srx_doublets srx_doublets;   /* owns the point block, the list, the parents and the scores; free it before its context */
typedef struct srx_doublet_opts {
    double   sim_ratio;             /* 0 = 2.0 */
    double   expected_rate;         /* 0 = 0.05 */
    double   stdev_rate;            /* 0 = 0.02 */
    double   target_sum;            /* of the transform applied to `fitted` (SRX_BACKED_NORMALIZE) */
    double   threshold;             /* 0 = automatic */
    uint64_t seed;
    int32_t  k;                     /* 0 = round(0.5 * sqrt(n)) */
    int32_t  n_dims;                /* leading components used by the search, 0 = all */
    int32_t  transform;             /* SRX_BACKED_NORMALIZE | SRX_BACKED_LOG1P: what was applied to `fitted` before its fit */
    int32_t  reserved_;
} srx_doublet_opts;
typedef struct srx_doublet_info {
    uint64_t n_obs, n_sim, nnz_sim;
    uint32_t k, k_adj, d;           /* d: coordinates used by the search */
    uint32_t threshold_found;       /* 1: the automatic threshold exists and is in use */
    double   threshold;             /* in use: automatic, the caller's, or NaN */
    uint32_t smooth_rounds;         /* smoothing rounds of the automatic threshold */
    uint32_t reserved_;
    uint64_t n_predicted;
    double   detected_rate, detectable_fraction, overall_rate;
    uint64_t rows_certified, rows_recomputed;             /* of the k-NN search (srx_knn_info) */
    double   ms_simulate, ms_project, ms_knn, ms_score;   /* hipEvent times of the stages */
} srx_doublet_info;
enum { SRX_DOUBLETS_SCORES_OBS = 0 /* n f64 */, SRX_DOUBLETS_SCORES_SIM = 1 /* n_sim f64 */, SRX_DOUBLETS_SE_OBS = 2,
       SRX_DOUBLETS_SE_SIM = 3, SRX_DOUBLETS_Z = 4 /* n f64 */, SRX_DOUBLETS_PREDICTED = 5 /* n u8 */,
       SRX_DOUBLETS_POINTS = 6 /* (n + n_sim) x d f64 row-major: the coordinates the search used */,
       SRX_DOUBLETS_PARENTS = 7 /* 2 n_sim u64 */, SRX_DOUBLETS_KNN = 8 /* (n + n_sim) x k_adj u32 */ };
/* Section 1 alone.  counts: CSR; parents: 2 n_sim host entries (row s: parents[2 s], parents[2 s + 1]) or NULL = hashed from
 * seed; parents_out (room for 2 n_sim, may be NULL) receives the parents used.  *out is an srx_mat the caller frees. */
int32_t srx_doublets_simulate(srx_mat* counts, uint64_t n_sim, uint64_t seed, const uint64_t* parents, srx_mat** out,
                              uint64_t* parents_out);
/* Section 4 alone, on a caller's neighbour list (host, (n_obs + n_sim) x k_adj row-major; any k_adj >= 1): the scoring kernel
 * applied to it.  score_out / se_out: n_obs + n_sim f64 each, either may be NULL. */
int32_t srx_doublet_scores_knn(srx_ctx* ctx, const uint32_t* indices, uint64_t n_obs, uint64_t n_sim, uint32_t k_adj,
                               double expected_rate, double stdev_rate, double* score_out, double* se_out);
/* Section 5's automatic threshold alone: pure host code, no context, no device.  Any output may be NULL. */
int32_t srx_doublets_threshold(const double* sim_scores, uint64_t n, double* threshold_out, int32_t* found_out,
                               uint32_t* rounds_out);
/* The whole chain with every intermediate in HBM; only the simulated scores come to the host, for the threshold.  opts NULL =
 * all defaults (no transform).  The synthetic matrix is freed before the call returns.  *out is written on success only. */
int32_t srx_doublets_result(srx_mat* fitted, srx_mat* counts, const srx_doublet_opts* opts, srx_doublets** out,
                            srx_doublet_info* info);
/* Scrublet's call_doublets(threshold = ...) on the resident scores: threshold 0 = the automatic one again.  Negative or NaN:
 * SRX_E_ARG. */
int32_t srx_doublets_call(srx_doublets* h, double threshold, srx_doublet_info* info);
/* One table (the enum above names each one's type and shape). */
int32_t srx_doublets_fetch(srx_doublets* h, int32_t which, void* out);
int32_t srx_doublets_info_get(const srx_doublets* h, srx_doublet_info* info);
void    srx_doublets_free(srx_doublets* h);

/* The raw operators the PCA is built from, for a caller-supplied 64-column panel (k x 64
 * row-major): y_out (n_rows x 64) = X[:, sel] * panel, t_out (k x 64) = X[:, sel]^T * y, and
 * gram_out (k x k) = X[:, sel]^T X[:, sel] (panel not needed).  `sel` must be strictly
 * ascending; any output may be NULL. */
int32_t srx_spmm(srx_mat* m, const uint64_t* sel, uint64_t k, const double* panel, double* y_out,
                 double* t_out, double* gram_out);

/* ONE operation of the dense k x 64 subspace iteration on caller-supplied host arrays (f64, row-major): a test and diagnostics
 * entry with NO stability promise (additive: detected by symbol, the ABI version stays).  The arrays are uploaded into fresh
 * device buffers of exactly their sizes, the kernel(s) are launched as the solver launches them, the stream is drained and the
 * buffers come back into the same arrays.  Every k x 64 block is allocated with 8 more rows that hold a sentinel; `tail_touched`
 * says whether any of them changed.  Slots an operation does not name may be NULL.
 *
 *   op       variant                            reads                                        writes
 *   APPLY    -                                  c (k x k), blk[0] = W, blk[1] = Wp           blk[1] (Wp += C^T W)
 *   GRAM1    -                                  blk[0] = A, blk[1] = B, sm[0] = H            sm[0] (H += A^T B)
 *   GRAM2    -                                  blk[0] = A, blk[1] = B                       sm[0] = A^T B, sm[1] = B^T B
 *   CHOL     0 plain, 1 shifted, 2 mfma         sm[0] = G, n                                 sm[1] = R, vec[0] = dinv, xi (mfma), sm[0], status[0]
 *   TRSM     0 rows, 1 mfma                     blk[0] = source, sm[1] = R, vec[0] / xi      blk[1] = W, blk[2..4] = z0..z2
 *   EIG      -                                  sm[0] = H, n, off_tol2, n_want               sm[1] = U, vec[0] = theta, sm[0], status[0..1]
 *   RITZ     -                                  blk[0] = W, blk[1] = Wp, sm[1] = U, vec[0]   blk[2] = A1, blk[3] = A2, blk[1], vec[1] = rho,
 *                                               = theta, n_pc, l_act                         vec[2] = colmax, out[0..5]
 *   CHEB     0 first  (blk: A1, A2)             vec[0] = theta, l_act, d (scale)             the blocks
 *            1 first2 (blk: Z, W, cur, prev)
 *            2 step   (blk: Z, cur, prev)
 *            3 scale  (blk: Y)
 * With SRX_IT_ALIAS_B, GRAM1 / GRAM2 pass the device copy of blk[0] as B too.  TRSM passes z_i when SRX_IT_Z0 << i is set (blk[2 + i]
 * is then uploaded and comes back), the SOURCE itself as z0 with SRX_IT_Z0_IS_SRC, and the source as the destination with
 * SRX_IT_SRC_IS_W (the result still comes back in blk[1]).  RITZ passes zero_wp = 1 with SRX_IT_ZERO_WP.
 * SRX_E_ARG (the context stays usable): a null context, argument block or named slot, k < 1, n or l_act outside 1..64, n_pc outside
 * 1..l_act, an unknown op or variant. */
typedef enum srx_iterate_opcode {
    SRX_IT_APPLY = 0, SRX_IT_GRAM1 = 1, SRX_IT_GRAM2 = 2, SRX_IT_CHOL = 3, SRX_IT_TRSM = 4, SRX_IT_EIG = 5, SRX_IT_RITZ = 6,
    SRX_IT_CHEB = 7
} srx_iterate_opcode;
#define SRX_IT_ALIAS_B 1
#define SRX_IT_ZERO_WP 1
#define SRX_IT_Z0 1             /* SRX_IT_Z0 << i: pass z_i, i = 0 .. 2 */
#define SRX_IT_Z0_IS_SRC 8
#define SRX_IT_SRC_IS_W 16
typedef struct srx_iterate_args {
    int32_t k, n, l_act, n_pc, n_want, d, variant, flags;
    double off_tol2;
    double* c;              /* k x k */
    double* blk[5];         /* k x 64 each */
    double* sm[2];          /* 64 x 64 each */
    double* vec[3];         /* 64 each */
    double* xi;             /* 4 x 16 x 16 */
    double out[8];          /* RITZ: k_resid_final's scalars */
    int32_t status[2];      /* the solver's status word and the eigen-solve's sweep count, as the kernels left them */
    int32_t tail_touched;   /* 1: a sentinel row behind a k x 64 block was written */
    int32_t reserved;
} srx_iterate_args;
int32_t srx_iterate_op(srx_ctx* ctx, int32_t op, srx_iterate_args* args);

/* The feature selection of the PCA on caller-supplied host arrays: a test and diagnostics entry with NO stability promise
 * (additive: detected by symbol, the ABI version stays).  The arrays are uploaded into fresh device buffers of exactly their
 * sizes, each followed by 8 sentinel elements; the kernels are launched by the function the pipeline launches them through
 * (select.hip: k_gene_var, k_hvg_candidates, k_rank_selected / k_hvg_rank, k_sel_finish), the stream is drained and everything
 * comes back.  k = min(take, G) genes are selected; n_words = ceil(G / 32).
 *
 *   op    reads                                                         writes
 *   HVG   cnt, sum, sq (G each: the per-gene nonzero count, sum and     var[G], rank[G] (as k_sel_finish reads it), counter,
 *         sum of squares), n_cells, center, scale, route                sel_rank[k], bits[n_words], prefix[n_words], mu[k],
 *                                                                       sd[k], dinv[k], trace, status
 *   LIST  genes (take distinct indices below G, the caller's order),    rank[G] (the position of every gene in the list),
 *         sum, sq, n_cells, center, scale                               sel_rank .. status as above; var and counter are not
 *
 * route (HVG): 0 as the pipeline decides (the candidate route from G = 512), 1 every gene ranked, 2 the threshold nothing
 * reaches (the decision on the device falls back to the full ranking).  counter: the number of candidates M, 0xffffffff where
 * the device fell back, SRX_SEL_COUNTER_UNUSED where the full ranking was launched directly (route 1, G < 512) or op is LIST.
 * LIST with SRX_SEL_NO_VECTORS: the selection alone; sum and sq are not read and may be NULL, mu / sd / dinv / trace come back
 * as they went in.  There is no NaN test on an explicit list: status stays 0.
 * tail_touched: bit i set when a sentinel behind buffer i changed, i = 0 cnt, 1 sum, 2 sq, 3 var, 4 rank, 5 candidate list,
 * 6 counter, 7 sel_rank, 8 bits, 9 prefix, 10 mu, 11 sd, 12 dinv, 13 trace, 14 status.
 * SRX_E_ARG (the context stays usable, no output is written): a null context, argument block or named array (outputs mu, sd,
 * dinv may be NULL with SRX_SEL_NO_VECTORS); G == 0 or take == 0; an unknown op or route; HVG outside the device ranking's
 * envelope (G > 65536, min(take, G) > 8192); LIST with G >= 2^31 or a repeated index.  SRX_E_BOUNDS: LIST with an index >= G. */
typedef enum srx_select_opcode { SRX_SEL_HVG = 0, SRX_SEL_LIST = 1 } srx_select_opcode;
#define SRX_SEL_NO_VECTORS 1
#define SRX_SEL_COUNTER_UNUSED 2147483646 /* 0x7ffffffe: no candidate count (at most 65536) reaches it, and it fits an int */
typedef struct srx_select_args {
    uint64_t G, take, n_cells;
    int32_t op, route, center, scale, flags, reserved;
    const uint64_t* cnt;    /* G */
    const double* sum;      /* G */
    const double* sq;       /* G */
    const uint64_t* genes;  /* LIST: take */
    double* var;            /* G (HVG) */
    uint32_t* rank;         /* G */
    int32_t* sel_rank;      /* k */
    uint32_t* bits;         /* n_words */
    uint32_t* prefix;       /* n_words */
    double* mu;             /* k */
    double* sd;             /* k */
    double* dinv;           /* k */
    double trace;
    uint32_t counter;
    int32_t status;         /* k_sel_finish's status word: bit 0 = a NaN variance */
    int32_t tail_touched;
    int32_t reserved2;
} srx_select_args;
int32_t srx_select_op(srx_ctx* ctx, srx_select_args* args);

/* ---- fused pipeline: normalize_total_inplace(target, Row) -> log1p_transform_inplace ->
 * pca_inplace(n_pc, center, scale, .., HighlyVariable(n_hvg)) with every intermediate
 * resident in HBM.  Results stay on the device until fetched. */
typedef struct srx_pipeline_result {
    srx_pca_info pca;
    double ms_normalize, ms_moments, ms_select, ms_compact, ms_pca; /* hipEvent stage times */
} srx_pipeline_result;
int32_t srx_pipeline(srx_mat* m, double target_sum, uint64_t n_hvg, const srx_pca_opts* opts,
                     srx_pipeline_result* res);
/* Fetch what the last srx_pca / srx_pipeline on `m` left in HBM (any pointer may be NULL;
 * hvg_idx has room for `k` entries). */
int32_t srx_result_fetch(srx_mat* m, double* scores, double* components, double* evr,
                         double* mean, double* std_, uint64_t* hvg_idx);

/* ---- backed (out-of-core) mode: the matrix is visited as consecutive ROW TILES ---------------
 * Replaces src/backed/statistics/mod.rs:5-45 (compute_number / compute_sum with
 * ComputationMode::Chunked(size); chunk loops src/shared/statistics/mod.rs:17-41,59-83,
 * csr.rs:48-74,112-143) and carries the whole path for matrices larger than HBM: two sweeps over
 * the row tiles, only the per-gene moments, the k x k Gram tiles and the HVG-compacted rows stay
 * on the device.  Unlike the reference's Direction::Row chunk loop (csr.rs:126 drops the chunk's
 * row offset), per-row outputs of a tile are written by the caller at the tile's global offset.
 *
 * A tile is an srx_csr whose `indptr` may be a WINDOW of the matrix's row_offsets (n_rows+1
 * entries, indptr[0] != 0 allowed) with `indices` / `values` pointing at the tile's first entry.
 * The upload of a tile overlaps the kernels of the previous one (own stream + staging buffers).
 * Multi-GPU: every rank runs its own session over its own row range; srx_backed_select and
 * srx_backed_solve are collective (one all-reduce each).
 *
 *   sweep 1  srx_backed_stats_tile  per tile: [normalize_total(Row)] [log1p] -> (cnt,sum,sumsq) +=
 *            srx_backed_moments     column statistics so far (compute_number / compute_sum, Column)
 *   select   srx_backed_select      FeatureSelection::HighlyVariable(n) | explicit list | all
 *   sweep 2  srx_backed_gram_tile   per tile, same transform: compaction + Gram tiles +=
 *   solve    srx_backed_solve       PCA (Gram solver) + scores of every tile; srx_backed_fetch  */
typedef struct srx_backed srx_backed;
enum { SRX_BACKED_NORMALIZE = 1, SRX_BACKED_LOG1P = 2 };   /* `transform` bits                    */
int32_t srx_backed_create(srx_ctx* ctx, uint64_t n_cols, int32_t store, srx_backed** out);
void    srx_backed_destroy(srx_backed* b);
/* row_number_out / row_sum_out (NULL or tile->n_rows entries): compute_number / compute_sum in
 * Direction::Row of the tile's RAW values. */
int32_t srx_backed_stats_tile(srx_backed* b, const srx_csr* tile, double target_sum, int32_t transform,
                              uint32_t* row_number_out, double* row_sum_out);
/* per-gene count / sum / sum of squares of the (transformed) values over all tiles so far, summed
 * over ranks; any pointer may be NULL. */
int32_t srx_backed_moments(srx_backed* b, uint64_t* cnt, double* sum, double* sumsq, uint64_t* n_rows_global);
/* n_hvg > 0: HighlyVariable(n_hvg); else `sel` (n_sel indices) or, with sel == NULL, all features
 * (at most 8192 selected).  opts as for srx_pca (solver 2 is refused).  sel_out (room for
 * min(n_hvg, n_cols) or n_sel entries) receives the selection in the reference's order. */
int32_t srx_backed_select(srx_backed* b, uint64_t n_hvg, const uint64_t* sel, uint64_t n_sel,
                          const srx_pca_opts* opts, uint64_t* sel_out, uint64_t* n_out);
int32_t srx_backed_gram_tile(srx_backed* b, const srx_csr* tile, double target_sum, int32_t transform);
int32_t srx_backed_solve(srx_backed* b, srx_pca_info* info);
/* as srx_result_fetch; scores = (rows of this rank, in tile order) x n_pc */
int32_t srx_backed_fetch(srx_backed* b, double* scores, double* components, double* evr, double* mean,
                         double* std_, uint64_t* sel);

/* ---- measurement hooks --------------------------------------------------------------------
 * When enabled, every launch of a kernel class is bracketed by hipEvents on the ctx stream.
 * srx_prof_get returns accumulated device time, launch count and the ALGORITHMIC bytes
 *  the launches moved. */
typedef enum srx_kernel_class {
    SRX_K_NORMALIZE = 0,   /* fused row-sum + scale + log1p                               */
    SRX_K_MOMENTS = 1,     /* gene-tiled (cnt, sum, sumsq)                                */
    SRX_K_COMPACT = 2,     /* HVG compaction                                              */
    SRX_K_SPMM_FWD = 3,    /* Y = X_sel P - 1 c^T                                         */
    SRX_K_SPMM_T = 4,      /* T = X_sel^T Y                                               */
    SRX_K_GRAM = 5,        /* G = X_sel^T X_sel (sparse outer products into LDS tiles)     */
    SRX_K_DENSE = 6,       /* dense k x k times k x 64 products of the Gram solver        */
    SRX_K_ROWSUM = 7,      /* per-cell sums of the raw values (first pass of srx_pipeline)  */
    SRX_K_ITERATE = 8,     /* the k x 64 subspace iteration as a whole (graph replays + the
                              launches between them); contains the SRX_K_DENSE launches     */
    SRX_K_SELECT = 9,      /* device-side HighlyVariable(n): variances, ranks, selection    */
    SRX_K_BUCKET = 10,     /* the Gram kernel's owner records: counts, their read-back, bucket pass;
                              SRX_K_GRAM is the stripe kernel alone                         */
    SRX_K_KNN = 11,        /* srx_knn_*: centre, f32 copy, candidate pass, f64 re-rank and recompute  */
    SRX_K_GRAPH = 12,      /* srx_neighbors_*: scales and weights, reverse lookup, in-only lists, merge           */
    SRX_K_COUNT_ = 13
} srx_kernel_class;
int32_t srx_prof_enable(srx_ctx* ctx, uint32_t class_mask);
int32_t srx_prof_reset(srx_ctx* ctx);
int32_t srx_prof_get(srx_ctx* ctx, int32_t kernel_class, double* total_ms, uint64_t* launches,
                     double* algorithmic_bytes);
/* Bytes of AUXILIARY structures the launches of a class read or wrote besides their algorithmic bytes (the Gram
 * kernel's owner records and block offsets): this implementation's own, never part of a roofline figure. */
int32_t srx_prof_get_aux(srx_ctx* ctx, int32_t kernel_class, double* aux_bytes);

#ifdef __cplusplus
}
#endif
#endif /* SRX_H */
