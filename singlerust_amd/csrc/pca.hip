// pca.hip — dim_red::pca_inplace (src/memory/processing/dim_red/mod.rs:24-94) on the GPU.
//
// The reference densifies X[:, sel] to an N x k f64 matrix (src/shared/mod.rs:230-259) and
// runs a full SVD of the standardised copy (spec: src/shared/processing/pca/mod.rs:74-154).
// Here the standardised matrix  Z = (X[:, sel] - c 1 mu^T) D   (c = center, D = diag(1/std)
// when scale) is never formed.  The top eigenpairs of C = Z^T Z are found by block subspace
// iteration with a Rayleigh–Ritz step on a k x 64 block W; two ways of applying C:
//
//  GRAM solver (default up to k = 16384)
//     G = A^T A is accumulated ONCE, exactly, in f64 (gram.inl): every kept entry times the suffix of its row, one f64 LDS
//     atomic per product, G's rows owned in stripes by the workgroups (12-byte owner records made by a bucket pass).
//     C = D (G - c N mu mu^T) D is then a dense k x k matrix and every iteration is a dense (k x k)(k x 64) product on the
//     f64 matrix cores (iterate.inl).  Across row shards: ONE all-reduce of G's packed upper triangle, half of it under the
//     kernel.  The whole iteration (CholeskyQR, Jacobi eigen-solve of the projected matrix — jacobi.inl —, Chebyshev filter,
//     residuals) runs on the device, replayed from hipGraphs; the host reads one residual per Rayleigh–Ritz step.
//  SPMM solver (matrix-free, any k)
//     forward     Y  = Z W   = A (D W) - 1 (mu^T D W)        sparse x dense panel, panel in LDS        (spmm.inl)
//     transposed  W' = Z^T Y = D (A^T Y - c mu (1^T Y))      scatter form, LDS f64 atomics
//     N m 64 lane-atomics PER ITERATION; across shards one all-reduce of the k x 64 block each.
//
// Either way the scores are one forward SpMM  Z V  (transform, pca/mod.rs:156-185).
// A is the HVG-COMPACTED matrix (compact.inl): row-major (column, value) records — what the Gram kernel and the forward
// product read — and, for the matrix-free solver, a tile-major view; everything of size k x 64 is replicated per rank and
// kept in f64.  Three translation units share pca_internal.hpp: pca_form.hip (compaction, owner records, G = A^T A and its
// exchange across row shards), pca_solve.hip (the sparse products, the k x 64 iteration (struct Iteration), the operators and the solver driver
// run_pca, srx_spmm; the schedule of a solve as plain host functions: pca_schedule.hpp) and this file: feature selection plumbing, the per-matrix driver pca_device, the host copies of the results, the
// out-of-core sessions (backed.inl) and the C entry points srx_pca / srx_pipeline / srx_result_fetch.
//
// Measured on MI355X (profiles/r01_*): LDS f32 float atomics (ds_add_f32) run ~10x slower than
// ds_add_f64, so every LDS accumulation here is f64; pure-f32 accumulation also stalls at ~2e-5
// eigenvector error on close eigenvalue pairs, f64 accumulation reaches ~3e-6 with f32 values.
//
// Algorithmic bytes per launch, s_v = bytes per stored value:
//   forward     nnz_w*(4+s_v) + (n_t N+1)*8 + N*64*4 (write Y) + k*64*4 (panel)
//   transposed  nnz_w*(4+s_v) + (n_t N+1)*8 + N*64*4 (read Y)  + k*64*8 (result)
#include "pca_internal.hpp"

namespace srx {

// Everything up to and including the scores, left in m->pca (device scores + small host vectors).
// Either `hvg_n` > 0: FeatureSelection::HighlyVariable(hvg_n) ranked on the device (the pipeline's route: no host round trip
// between the moments pass and the compaction; only inside hvg_on_device's envelope), or the list `sel` (nullptr = all
// features, FeatureSelection::None).
static int32_t pca_device(srx_mat* m, const uint64_t* sel, uint64_t k64, const srx_pca_opts* opts, uint64_t hvg_n = 0) {
    srx_ctx* ctx = m->ctx;
    SRX_HIP(ctx, hipSetDevice(ctx->device));
    // compaction, Gram and SpMM walk cells: solve on the CSR of X (device transpose, csc.hip) and hand the result to the CSC
    // handle (convert_to_array_f64_csc_selected, src/shared/mod.rs:261-290, builds the same dense matrix from either storage)
    if (m->csc) return on_cells_csr(m, true, [&](srx_mat* t) { return pca_device(t, sel, k64, opts, hvg_n); });
    srx_pca_state& st = m->pca;
    st.valid = false;
    const uint64_t G = m->n_cols;
    if (hvg_n > 0 && (sel || !hvg_on_device(hvg_n, G)))
        return fail(ctx, SRX_E_ARG, "pca: HighlyVariable(%llu) of %llu features is not ranked on the device", (unsigned long long)hvg_n,
                    (unsigned long long)G);
    if (!sel && hvg_n == 0) k64 = G;                                           // FeatureSelection::None, :154
    const int k = (int)(hvg_n > 0 ? std::min(hvg_n, G) : k64);
    SRX_TRY(ensure_moments(m));                                                // for the selection below; also fixes n_rows_global
    const uint64_t Ng = m->n_rows_global;
    Resolved o;
    int l_act = 0;
    SRX_TRY(resolve_opts(ctx, opts, k, Ng, is_f32(m), o, l_act));
    st.center = o.center;
    st.scale = o.scale;
    SelDev sd;
    if (hvg_n > 0) {
        Range r_("srx:select_hvg");
        ProfScope ps_sel(ctx, SRX_K_SELECT, (double)G * 24.0);
        SRX_TRY(select_hvg_device(m, hvg_n, o.center, o.scale, sd));
    } else {
        SRX_TRY(select_list(m, sel, k64, o.center, o.scale, sd));
    }

    // X[:, sel] as row-major records; the 256-tiled view of them only where something reads it (the matrix-free solver)
    Tiled t256;
    RowMajor rm;
    Range r_compact("srx:compact");
    const bool need_t256 = o.solver == 2;
    SRX_TRY(compact_selection(m, sd.d_bits, sd.n_words, k, rm, RowXf{}, o.solver == 1));      // (the stored values)
    if (need_t256) SRX_TRY(retile(m, rm, t256));
    return solve_and_stash(ctx, is_f32(m), &rm, 1, need_t256 ? &t256 : nullptr, nullptr, o, sd, l_act, Ng, rm.nnz, st);
}

// Host copies of the last solve: components (k x n_pc, rows in SELECTION order, sign-fixed), explained variance
// ratio = theta / trace(Z^T Z) (pca/mod.rs:131-133: eigenvalues s^2/(N-1) over ALL components), mean / std per
// selected feature, the selection itself.  One D2H of the matrix's result block.
static int32_t pca_materialize(srx_mat* m) {
    srx_pca_state& st = m->pca;
    if (!st.valid || !st.host_pending) return SRX_OK;
    srx_ctx* ctx = m->ctx;
    const int k = (int)st.k, n_pc = (int)st.n_pc;
    const PcaResultLayout lay = result_block(st);
    std::vector<double> blk(lay.total_doubles());
    SRX_TRY(d2h(ctx, blk.data(), st.d_small, blk.size() * 8));
    const double *mu = blk.data() + lay.mu(), *sd = blk.data() + lay.sd(), trace = blk[lay.trace()];
    const int32_t* hsel = reinterpret_cast<const int32_t*>(blk.data() + lay.sel_rank());
    st.sel.assign(hsel, hsel + k);
    // slot (ascending gene order) of every selected feature
    std::vector<int> order(k), slot_of_sel(k);
    std::iota(order.begin(), order.end(), 0);
    std::sort(order.begin(), order.end(), [&](int a, int b) { return st.sel[a] < st.sel[b]; });
    for (int sI = 0; sI < k; ++sI) slot_of_sel[order[sI]] = sI;
    st.components.assign((size_t)k * n_pc, 0.0);
    st.mean.resize(k);
    st.std_.resize(k);
    for (int i = 0; i < k; ++i) {
        const int sl = slot_of_sel[i];
        for (int p = 0; p < n_pc; ++p) st.components[(size_t)i * n_pc + p] = blk[(size_t)sl * L + lay.col_offset(p)] * blk[lay.sgn_offset(p)];
        st.mean[i] = mu[sl];
        st.std_[i] = sd[sl];
    }
    st.evr.resize(n_pc);
    for (int p = 0; p < n_pc; ++p) st.evr[p] = trace > 0 ? blk[lay.theta_offset(p)] / trace : 0.0;
    st.host_pending = false;
    return SRX_OK;
}

}  // namespace srx

using namespace srx;

#include "backed.inl"

extern "C" {

int32_t srx_result_fetch(srx_mat* m, double* scores, double* components, double* evr, double* mean, double* std_,
                         uint64_t* hvg_idx) {
    if (!m) return fail(nullptr, SRX_E_ARG, "null matrix");
    srx_ctx* ctx = m->ctx;
    if (!m->pca.valid) return fail(ctx, SRX_E_ARG, "no PCA result on this matrix");
    SRX_HIP(ctx, hipSetDevice(ctx->device));
    if (components || evr || mean || std_ || hvg_idx) SRX_TRY(pca_materialize(m));
    const srx_pca_state& st = m->pca;
    if (scores) SRX_TRY(d2h_rows(ctx, scores, st.d_scores, m->csc ? m->n_cols : m->n_rows, (size_t)st.n_pc * 8, (size_t)scores_ld((int)st.n_pc) * 8));
    if (components) memcpy(components, st.components.data(), st.components.size() * 8);
    if (evr) memcpy(evr, st.evr.data(), st.evr.size() * 8);
    if (mean) memcpy(mean, st.mean.data(), st.mean.size() * 8);
    if (std_) memcpy(std_, st.std_.data(), st.std_.size() * 8);
    if (hvg_idx) memcpy(hvg_idx, st.sel.data(), st.sel.size() * 8);
    return SRX_OK;
}

int32_t srx_matrix_reserve_results(srx_mat* m, uint64_t n_selected, int32_t n_components) {
    if (!m) return fail(nullptr, SRX_E_ARG, "null matrix");
    srx_ctx* ctx = m->ctx;
    if (n_components < 1 || n_selected < 1) return fail(ctx, SRX_E_ARG, "reserve_results: need n_selected >= 1 and n_components >= 1");
    SRX_HIP(ctx, hipSetDevice(ctx->device));
    const uint64_t n_cells = m->csc ? m->n_cols : m->n_rows, n_genes = m->csc ? m->n_rows : m->n_cols;
    const int k = (int)std::min<uint64_t>(n_selected, n_genes);
    const int n_pc = std::min(n_components, k);
    size_t score_bytes, small_doubles;
    // dim = k bounds the number of rounds from above (fewer dimensions never take more rounds)
    result_layout(n_cells, k, n_pc, k, score_bytes, small_doubles);
    SRX_TRY(ensure_result_capacity(ctx, m->pca, score_bytes + small_doubles * 8));
    // the per-cell sums of the pipeline's first pass belong to the same promise: no device allocation inside a step
    if (!m->csc && !m->d_row_sum) SRX_HIP(ctx, hipMalloc((void**)&m->d_row_sum, (m->n_rows ? m->n_rows : 1) * sizeof(double)));
    return SRX_OK;
}

int32_t srx_pca(srx_mat* m, const uint64_t* sel, uint64_t k, const srx_pca_opts* opts, double* scores,
                double* components, double* evr, double* mean, double* std_, srx_pca_info* info) {
    if (!m) return fail(nullptr, SRX_E_ARG, "null matrix");
    int32_t rc = pca_device(m, sel, k, opts);
    if (rc != SRX_OK && rc != SRX_E_NOCONV) return rc;
    if (info) *info = m->pca.info;
    int32_t rc2 = srx_result_fetch(m, scores, components, evr, mean, std_, nullptr);
    return rc2 != SRX_OK ? rc2 : rc;
}

int32_t srx_pca_loadings(const double* components, const double* std_, const uint64_t* sel, uint64_t k,
                         uint64_t n_pc, uint64_t n_vars, double* out) {
    if (!components || !std_ || !sel || !out) return fail(nullptr, SRX_E_ARG, "null argument");
    // dim_red/mod.rs:111-116: zeros(n_vars x n_pc); row sel[i] <- loadings row i;
    // loadings = components^T * std (pca/mod.rs:204-215) i.e. component[i][p] * std[i]
    for (uint64_t t = 0; t < n_vars * n_pc; ++t) out[t] = 0.0;
    for (uint64_t i = 0; i < k; ++i) {
        if (sel[i] >= n_vars) return fail(nullptr, SRX_E_BOUNDS, "feature index out of bounds");
        for (uint64_t p = 0; p < n_pc; ++p) out[sel[i] * n_pc + p] = components[i * n_pc + p] * std_[i];
    }
    return SRX_OK;
}

int32_t srx_pipeline(srx_mat* m, double target_sum, uint64_t n_hvg, const srx_pca_opts* opts,
                     srx_pipeline_result* res) {
    if (!m) return fail(nullptr, SRX_E_ARG, "null matrix");
    srx_ctx* ctx = m->ctx;
    SRX_HIP(ctx, hipSetDevice(ctx->device));
    hipEvent_t ev[5] = {nullptr, nullptr, nullptr, nullptr, nullptr};
    auto cleanup = [&]() { for (auto& e : ev) if (e) (void)hipEventDestroy(e); };
    for (auto& e : ev)
        if (hipEventCreate(&e) != hipSuccess) {
            cleanup();
            return fail(ctx, SRX_E_HIP, "srx_pipeline: hipEventCreate failed");
        }
    int32_t rc = SRX_OK;
    // SRX_STORE_AUTO: the storage follows the reference's variant (scale/mod.rs:74-83: X becomes DynCsrMatrix::F64 at
    // normalize_total) exactly as under the three separate calls — the raw values widen to f64 first and the whole path runs at
    // f64 storage.  The f32 fast path (X ends as f32(ln_1p(f64(v) * scale))) is for handles created with SRX_STORE_F32.
    if (!m->csc) rc = promote_to_f64(m);
    if (rc != SRX_OK) {
        cleanup();
        return rc;
    }
    (void)hipEventRecord(ev[0], ctx->stream);
    // normalize_total_inplace(target, Row) + log1p_transform_inplace.  CSR: the row sums, then the moments pass reads the RAW
    // matrix, forms y = ln_1p(v * scale_row) on the fly in f64 (RowXf) — so the per-gene moments behind HighlyVariable(n) are
    // those of the reference's f64 values whatever the storage type — and stores y in place at the storage precision: every
    // pass behind it reads the stored values.  CSC (cells are columns): the two calls, then the stored values.
    bool stored = m->csc;       // the transform is no longer owed: the CSC route's own calls, or the moments pass once it is in the stream
    {
    Range r_("srx:normalize");
    rc = m->csc ? srx_normalize_log1p_inplace(m, target_sum, nullptr) : launch_row_sums(m);
    }
    (void)hipEventRecord(ev[1], ctx->stream);
    // per-gene moments of the transformed values (one pass, all-reduced across shards), adopted for pca_device's selection
    if (rc == SRX_OK && !m->csc) {
        Range r_("srx:gene_moments");
        rc = ensure_moments_xf(m, RowXf{m->d_row_sum, target_sum, true}, &stored);
        if (rc == SRX_OK) moments_adopt(m);
    }
    (void)hipEventRecord(ev[2], ctx->stream);
    // FeatureSelection::HighlyVariable(n_hvg): on the device, inside pca_device (the selection is fetched with the
    // other results once the solve is over); ranked here for the shapes outside the device ranking's envelope (hvg_on_device)
    // and for CSC, and passed on as a list
    std::vector<uint64_t> sel;
    const bool on_device = !m->csc && hvg_on_device(n_hvg, m->n_cols);
    if (rc == SRX_OK && !on_device) rc = hvg_list_host(m, n_hvg, sel);      // (CSC: with the CSC variance, csc.rs:164-177)
    (void)hipEventRecord(ev[3], ctx->stream);
    if (rc == SRX_OK) {
        Range r_("srx:pca");
        rc = on_device ? pca_device(m, nullptr, 0, opts, n_hvg) : pca_device(m, sel.data(), sel.size(), opts);
    }
    if (!stored) {
        // whatever happened above, X ends up normalised and log1p'd (the two in-place calls come first in the reference): an
        // error before the moments pass was in the stream — in place from the row sums in m->d_row_sum
        const int32_t rc_wb = launch_row_apply(m, target_sum, ctx->stream);
        if (rc == SRX_OK) rc = rc_wb;
    } else if (!m->csc) {
        // the moments cached on the matrix are those of the f64 transform, not of the values as stored: retired (a later
        // compute_variance sees what X holds)
        moments_retire(m);
    }
    (void)hipEventRecord(ev[4], ctx->stream);
    (void)hipStreamSynchronize(ctx->stream);
    if (res) {
        memset(res, 0, sizeof *res);
        res->pca = m->pca.info;
        float ms = 0;
        if (hipEventElapsedTime(&ms, ev[0], ev[1]) == hipSuccess) res->ms_normalize = ms;
        if (hipEventElapsedTime(&ms, ev[1], ev[2]) == hipSuccess) res->ms_moments = ms;
        if (hipEventElapsedTime(&ms, ev[2], ev[3]) == hipSuccess) res->ms_select = ms;
        if (hipEventElapsedTime(&ms, ev[3], ev[4]) == hipSuccess) res->ms_pca = ms;
        res->ms_compact = 0.0;
    }
    cleanup();
    return rc;
}

}  // extern "C"
