// pearson_pca.hip — PCA of the clipped Pearson residuals of listed genes (srx.h: srx_pca_pearson, srx_pearson_gram): scanpy's
// experimental.pp.normalize_pearson_residuals_pca on the device.
//
// The residual matrix Z (n x k) is dense and is never held as a whole: this is a caller of the dense route (dense_pca.hip,
// dense_pca_internal.hpp), which makes Z a chunk of cells at a time, forms Z^T Z and the scores on the f64 matrix cores and runs
// the Gram solver in between.  What is Pearson's is here: the element of Z from the definition (pearson_internal.hpp: pr_resid),
// the per-cell sums over the listed genes, the refusals and the two entry points.
// No atomics: every sum of this file has one owner.
#include "pearson_internal.hpp"
#include "dense_pca_internal.hpp"

// the chunk kernels evaluate the definition and the sums of this file are stated in one order
#pragma clang fp contract(off)

namespace srx {

// The element of Z: the residual of cell `row` and the gene of column `slot`
struct PpElem {
    const double* cell_sum;          // r_i
    const double* gsum;              // g_j of the listed genes in slot order
    PrArgs a;
    __device__ __forceinline__ double at(double x, uint64_t row, uint32_t slot, bool* clipped) const {
        *clipped = false;
        return pr_resid(x, cell_sum[row], gsum[slot], a);
    }
};

// ---- per-cell sums over the listed genes (totals = SELECTED): one pass over the stored entries ------------------------------------
// A wave per row; lane l adds the entries l, l + 64, .. in that order, the 64 partial sums meet in a butterfly.
template <typename T>
__global__ __launch_bounds__(256) void k_pp_row_sums(const int64_t* __restrict__ indptr, const int32_t* __restrict__ idx,
                                                     const T* __restrict__ vals, uint64_t n_rows, const int32_t* __restrict__ slot_of,
                                                     double* __restrict__ out) {
    const uint64_t r = global_wave_id();
    if (r >= n_rows) return;
    const int lane = lane_id();
    const int64_t hi = indptr[r + 1];
    double s = 0.0;
    for (int64_t e = indptr[r] + lane; e < hi; e += kWave)
        if (slot_of[idx[e]] >= 0) s += (double)vals[e];
    s = wave_sum(s);
    if (lane == 0) out[r] = s;
}

// the sums of the listed genes in slot order: what both chunk kernels index by the column of Z
__global__ __launch_bounds__(256) void k_pp_gene_sums(const double* __restrict__ gene_sum, const int32_t* __restrict__ slot_of, uint64_t G,
                                                      double* __restrict__ gsum) {
    const uint64_t j = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (j < G && slot_of[j] >= 0) gsum[slot_of[j]] = gene_sum[j];
}

// ---- host side ---------------------------------------------------------------------------------------------------------------------------
namespace {

struct PpRun {                       // everything between the arguments and the two products
    PrPrep p;
    DenseSlots s;                    // slot s of the solver is the s-th smallest listed gene
    DenseChunks g;                   // the chunk geometry and the chunk buffer
    PpElem el{};
};

// `m` is a CSR handle.  The preparation of every Pearson call, the slot table, the sums over the listed genes where asked, the
// element of Z, the chunk size and the chunk buffer.
int32_t pp_setup(srx_mat* m, const uint64_t* genes, uint64_t k64, const srx_pearson_opts* popts, int totals, uint64_t chunk_cells,
                 const char* who, PpRun& R) {
    srx_ctx* ctx = m->ctx;
    SRX_TRY(pr_prepare(m, popts, who, R.p));
    const uint64_t n = R.p.n, G = R.p.G;
    SRX_TRY(dense_slots_setup(ctx, genes, k64, G, R.s));
    if (totals == SRX_PEARSON_TOTALS_SELECTED) {
        double* d_rsel;
        SRX_TRY(scratch(ctx, "pp_rows_sel", at_least_one(n) * sizeof(double), (void**)&d_rsel));
        const unsigned grid = (unsigned)((at_least_one(n) + 3) / 4);
        if (is_f32(m))
            hipLaunchKernelGGL(k_pp_row_sums<float>, dim3(grid), dim3(256), 0, ctx->stream, m->d_indptr, m->d_indices, (const float*)m->d_values,
                               n, (const int32_t*)R.s.d_slot_of, d_rsel);
        else
            hipLaunchKernelGGL(k_pp_row_sums<double>, dim3(grid), dim3(256), 0, ctx->stream, m->d_indptr, m->d_indices, (const double*)m->d_values,
                               n, (const int32_t*)R.s.d_slot_of, d_rsel);
        SRX_HIP(ctx, hipGetLastError());
        R.p.d_cell = d_rsel;
        SRX_TRY(pr_totals(ctx, d_rsel, n, R.p.d_gene, G, &R.p.a.total, &R.p.n_empty));
    }
    double* d_gsum;
    SRX_TRY(scratch(ctx, "pp_gene_sums", k64 * sizeof(double), (void**)&d_gsum));
    hipLaunchKernelGGL(k_pp_gene_sums, dim3(grid256(G)), dim3(256), 0, ctx->stream, R.p.d_gene, (const int32_t*)R.s.d_slot_of, G, d_gsum);
    SRX_HIP(ctx, hipGetLastError());
    R.el = PpElem{R.p.d_cell, d_gsum, R.p.a};
    SRX_TRY(dense_chunks_setup(ctx, n, k64, chunk_cells, R.g));
    return SRX_OK;
}

void pp_info(const PpRun& R, srx_pearson_pca_info* info) {
    memset(info, 0, sizeof *info);
    info->n_cells = R.p.n;
    info->n_genes = R.p.G;
    info->n_expressed = R.p.n_expressed;
    info->n_empty_cells = R.p.n_empty;
    info->total = R.p.a.total;
    info->theta = R.p.a.theta;
    info->clip = R.p.a.clip;
    info->n_chunks = R.g.n_chunks;
    info->chunk_cells = R.g.chunk;
    info->chunk_bytes = R.g.chunk * (uint64_t)R.g.ldz * sizeof(double);
}

int32_t pp_check_common(srx_mat* m, const uint64_t* genes, uint64_t k, const srx_pearson_pca_opts* opts, const char* who) {
    srx_ctx* ctx = m->ctx;
    // the refusals of the Pearson section first (pr_prepare repeats them where it runs), then those of this one
    PrArgs unused;
    SRX_TRY(pr_check_args(m, opts ? &opts->pearson : nullptr, who, unused, m->csc ? m->n_cols : m->n_rows));
    if (k == 0) return fail(ctx, SRX_E_ARG, "%s: an empty gene list (k >= 1)", who);
    if (opts && opts->totals != SRX_PEARSON_TOTALS_ALL && opts->totals != SRX_PEARSON_TOTALS_SELECTED)
        return fail(ctx, SRX_E_ARG, "%s: totals = %d (0: the whole matrix, 1: the listed genes)", who, opts->totals);
    return dense_check_list(ctx, who, genes, k, m->csc ? m->n_rows : m->n_cols);
}

// `m` is a CSR handle of the cells' rows, here and in pp_pca
int32_t pp_gram(srx_mat* m, const uint64_t* genes, uint64_t k, const srx_pearson_pca_opts* opts, double* gram_out, double* colsum_out,
                srx_pearson_pca_info* info) {
    srx_ctx* ctx = m->ctx;
    PpRun R;
    SRX_TRY(pp_setup(m, genes, k, opts ? &opts->pearson : nullptr, opts ? opts->totals : 0, opts ? opts->chunk_cells : 0, "pearson_gram", R));
    const DenseChunkFn make = [&](uint64_t row0, uint64_t rows, double* Z) { return dense_make_chunk<PpElem, false>(m, R.s, R.g, R.el, row0, rows, Z); };
    srx_pearson_pca_info inf;
    pp_info(R, &inf);
    double *Gp, *colsum;
    SRX_TRY(dense_gram_pass(ctx, R.g, make, &Gp, &colsum, &inf.ms_gram));
    SRX_TRY(dense_gram_fetch(ctx, R.s, Gp, colsum, gram_out, colsum_out));
    if (info) *info = inf;
    return SRX_OK;
}

int32_t pp_pca(srx_mat* m, const uint64_t* genes, uint64_t k64, const srx_pearson_pca_opts* opts, srx_pearson_pca_info* info) {
    srx_ctx* ctx = m->ctx;
    m->pca.valid = false;
    // the solver's options: no scaling, the centring flag of this call
    srx_pca_opts po{};
    if (opts) po = opts->pca;
    else po.n_components = -1;
    po.scale = 0;
    po.center = (!opts || opts->center != 0) ? 1 : 0;
    Resolved o;
    int l_act = 0;
    SRX_TRY(resolve_opts(ctx, &po, (int)k64, m->n_rows, false, o, l_act));
    PpRun R;
    SRX_TRY(pp_setup(m, genes, k64, opts ? &opts->pearson : nullptr, opts ? opts->totals : 0, opts ? opts->chunk_cells : 0, "pca_pearson", R));
    const DenseChunkFn make = [&](uint64_t row0, uint64_t rows, double* Z) { return dense_make_chunk<PpElem, false>(m, R.s, R.g, R.el, row0, rows, Z); };
    srx_pearson_pca_info inf;
    pp_info(R, &inf);
    DenseSolved sv;
    const int32_t rc = dense_pca_solve(m, o, l_act, genes, R.g, make, make, kResidualPearson, o.center, nullptr, sv);
    if (!sv.solved) return rc;
    inf.ms_gram = sv.ms_gram;
    inf.ms_solve = sv.ms_solve;
    inf.ms_scores = sv.ms_scores;
    inf.pca = sv.pca;
    if (info) *info = inf;
    return rc;
}

}  // namespace

}  // namespace srx

using namespace srx;

extern "C" {

int32_t srx_pearson_gram(srx_mat* m, const uint64_t* genes, uint64_t k, const srx_pearson_pca_opts* opts, double* gram_out,
                         double* colsum_out, srx_pearson_pca_info* info) {
    if (!m || !genes || (!gram_out && !colsum_out)) return fail(m ? m->ctx : nullptr, SRX_E_ARG, "pearson_gram: null argument");
    SRX_TRY(pp_check_common(m, genes, k, opts, "pearson_gram"));
    SRX_HIP(m->ctx, hipSetDevice(m->ctx->device));
    return on_cells_csr(m, false, [&](srx_mat* x) { return pp_gram(x, genes, k, opts, gram_out, colsum_out, info); });
}

int32_t srx_pca_pearson(srx_mat* m, const uint64_t* genes, uint64_t k, const srx_pearson_pca_opts* opts, double* scores, double* components,
                        double* evr, double* mean, srx_pearson_pca_info* info) {
    if (!m || !genes) return fail(m ? m->ctx : nullptr, SRX_E_ARG, "pca_pearson: null argument");
    srx_ctx* ctx = m->ctx;
    SRX_TRY(pp_check_common(m, genes, k, opts, "pca_pearson"));
    if (opts && opts->pca.scale > 0) return fail(ctx, SRX_E_ARG, "pca_pearson: pca.scale is set (the residuals are not scaled)");
    if (opts && opts->pca.solver == SRX_SOLVER_SPMM)
        return fail(ctx, SRX_E_ARG, "pca_pearson: the matrix-free solver walks sparse rows; the residuals are dense (solver 0 or 1)");
    SRX_HIP(ctx, hipSetDevice(ctx->device));
    const int32_t rc = on_cells_csr(m, true, [&](srx_mat* x) { return pp_pca(x, genes, k, opts, info); });
    if (rc != SRX_OK && rc != SRX_E_NOCONV) return rc;
    const int32_t rc2 = srx_result_fetch(m, scores, components, evr, mean, nullptr, nullptr);
    return rc2 != SRX_OK ? rc2 : rc;
}

}  // extern "C"
