// regress.hip — covariates regressed out of listed genes, the residuals scaled and clipped, and the PCA of the result (srx.h:
// srx_regress_fit, srx_regress_residuals, srx_regress_gram, srx_pca_regress): scanpy's regress_out -> scale -> pca on the device.
//
// Z (n x k) is dense and is never held as a whole: this is a caller of the dense route (dense_pca.hip, dense_pca_internal.hpp),
// which makes Z a CHUNK of cells at a time from ONE element function (rg_value).  A mode says what the chunk holds: the stored x
// (for W = Ct^T X), the residual r (for sum r^2), or z = clip(r / s) (for the products and the block).  Four passes over the chunks:
//   W       a weighted column sum (k_rg_wsum): per column and slab the rows in ascending order, up to 16 weight vectors at once;
//   sum r^2 the same kernel with the column's own value as weight;
//   Gram    Z^T Z and the column sums   } the dense route's products on the f64 matrix cores, handed this file's element
//   scores  Z P - 1 c^T                 } function.
// The p x p factor (p <= 16) and the k solves run on the host in f64.
// No floating-point atomics: a partial sum has one owner, slabs and chunks are added in ascending order.  The only atomics count
// clipped pairs in the chunk kernels (integers: exact in any order).
#include "dense_pca_internal.hpp"

// the chunk kernels evaluate the definition and the sums of this file are stated in one order (host code included)
#pragma clang fp contract(off)

namespace srx {

enum { kRgRaw = 0, kRgResid = 1, kRgZ = 2 };    // what a chunk holds
constexpr int kRgMaxCov = 16;
constexpr int kRgMaxSlabs = 64;                 // slabs of a chunk (k_dense_colsum's bound)
constexpr int kRgCovSlabs = 1024;               // slabs of the covariate matrix, which is summed as one chunk of n rows
constexpr double kRgMinPivot = 1e-10;

struct RgArgs {
    const double* ct;      // n x p centred covariates, row-major
    const double* beta;    // p x k, slot order
    const double* xbar;    // k
    const double* s;       // k
    const uint8_t* cst;    // k: 1 where the gene's n values are all equal
    double max_value;      // 0: no clip
    uint32_t k;
    int p, mode;
    __device__ __forceinline__ double at(double x, uint64_t row, uint32_t slot, bool* clipped) const;   // the dense route's element: rg_value
};

// The element (i, j) of the chunk for the stored value x, in the order srx.h states.  *clipped: |r / s| > max_value.
__device__ __forceinline__ double rg_value(double x, uint64_t i, uint32_t j, const RgArgs& a, bool* clipped) {
#pragma clang fp contract(off)
    *clipped = false;
    if (a.mode == kRgRaw) return x;
    if (a.cst[j]) return 0.0;
    double r = x - a.xbar[j];
    if (a.p > 0) {
        const double* c = a.ct + i * (uint64_t)a.p;
        double f = c[0] * a.beta[j];
        for (int q = 1; q < a.p; ++q) f += c[q] * a.beta[(size_t)q * a.k + j];
        r = r - f;
    }
    if (a.mode == kRgResid) return r;
    const double z = r / a.s[j];
    if (!(a.max_value > 0.0)) return z;
    *clipped = fabs(z) > a.max_value;
    return fmin(fmax(z, -a.max_value), a.max_value);
}

__device__ __forceinline__ double RgArgs::at(double x, uint64_t row, uint32_t slot, bool* clipped) const {
    return rg_value(x, row, slot, *this, clipped);
}

// ---- weighted column sums of a chunk ---------------------------------------------------------------------------------------------------
// A thread per column and slab walks the slab's rows in ascending order (k_dense_colsum's scheme) and adds w[r][q] * Z[r][c] for the
// nw <= 16 weight vectors q at once (w: row r of the chunk at w + r * ldw); sq: one sum, the weight is Z[r][c] itself.
// part[(slab * nw + q) * k + c].
__global__ __launch_bounds__(256) void k_rg_wsum(const double* __restrict__ Z, uint32_t ldz, uint32_t rows, uint32_t slab_rows, uint32_t k,
                                                 const double* __restrict__ w, uint32_t ldw, int nw, int sq, double* __restrict__ part) {
    const uint32_t c = blockIdx.x * 256 + threadIdx.x;
    if (c >= k) return;
    const uint32_t r_beg = blockIdx.y * slab_rows;
    const uint32_t r_end = r_beg + slab_rows < rows ? r_beg + slab_rows : rows;
    double acc[kRgMaxCov];
#pragma unroll
    for (int q = 0; q < kRgMaxCov; ++q) acc[q] = 0.0;
    for (uint32_t r = r_beg; r < r_end; ++r) {
        const double z = Z[(size_t)r * ldz + c];
        if (sq) {
            acc[0] += z * z;
        } else {
            const double* wr = w + (size_t)r * ldw;
#pragma unroll
            for (int q = 0; q < kRgMaxCov; ++q)
                if (q < nw) acc[q] += wr[q] * z;
        }
    }
#pragma unroll
    for (int q = 0; q < kRgMaxCov; ++q)
        if (q < nw) part[((size_t)blockIdx.y * nw + q) * k + c] = acc[q];
}
// out[q * k + c] += the slabs' partial sums in ascending order
__global__ __launch_bounds__(256) void k_rg_wsum_reduce(const double* __restrict__ part, uint32_t n_slabs, int nw, uint32_t k,
                                                        double* __restrict__ out) {
    const uint64_t o = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (o >= (uint64_t)nw * k) return;
    const uint32_t q = (uint32_t)(o / k), c = (uint32_t)(o - (uint64_t)q * k);
    double s = 0.0;
    for (uint32_t sl = 0; sl < n_slabs; ++sl) s += part[((size_t)sl * nw + q) * k + c];
    out[o] += s;
}

// ---- host side --------------------------------------------------------------------------------------------------------------------------
namespace {

enum { kStageFit = 0, kStageBlock = 1, kStageGram = 2, kStagePca = 3, kStageSums = 4 };

struct RgOut {                       // the host outputs of the four calls
    double *beta = nullptr, *xbar = nullptr, *sd = nullptr;   // fit
    double *cbar = nullptr, *A = nullptr, *W = nullptr;       // sums
    double* block = nullptr;                                 // residuals
    double *gram = nullptr, *colsum = nullptr;               // gram
};

struct RgPrep {                      // what is made before the rows are walked: from the arguments and the handle as given
    uint64_t n = 0, G = 0;
    int k = 0, p = 0;
    int scale = 1;
    double max_value = 0.0;
    std::vector<double> ct;          // n x p centred covariates
    std::vector<double> cbar, A;     // p, p x p
    std::vector<double> dsq, Lf;     // sqrt(diag A) and the Cholesky factor of the scaled A (p x p, lower)
    double min_pivot = 1.0;
    double ms_cov = 0.0;
    std::vector<double> xbar;        // caller's order
    std::vector<uint8_t> cst;        // caller's order
    uint64_t n_const = 0;
};

struct RgRun {
    DenseChunks g;
    DenseSlots sl;                   // slots: ascending gene, as the solver and the chunk's columns are ordered
    double *d_ct = nullptr, *d_beta = nullptr, *d_xbar = nullptr, *d_s = nullptr;
    uint8_t* d_cst = nullptr;
    unsigned long long* d_cnt = nullptr;
    std::vector<double> beta, s;     // slot order
};

int32_t rg_wsum(srx_ctx* ctx, const double* Z, uint32_t ldz, uint64_t rows, uint32_t k, const double* w, uint32_t ldw, int nw, int sq,
                int slabs_max, double* part, double* out) {
    const uint64_t gr = (rows + 63) / 64;
    const uint32_t n = (uint32_t)std::min<uint64_t>(gr, (uint64_t)slabs_max);
    const uint32_t slab_rows = (uint32_t)((gr + n - 1) / n * 64);
    const uint32_t ns = (uint32_t)((rows + slab_rows - 1) / slab_rows);
    hipLaunchKernelGGL(k_rg_wsum, dim3(grid256(k), ns), dim3(256), 0, ctx->stream, Z, ldz, (uint32_t)rows, slab_rows, k, w, ldw, nw, sq, part);
    hipLaunchKernelGGL(k_rg_wsum_reduce, dim3(grid256((uint64_t)nw * k)), dim3(256), 0, ctx->stream, (const double*)part, ns, nw, k, out);
    SRX_HIP(ctx, hipGetLastError());
    return SRX_OK;
}

// refusals (1) to (7) of srx.h and the shape
int32_t rg_check(srx_mat* m, const uint64_t* genes, uint64_t k, const double* cov, uint64_t p, const srx_regress_opts* opts, const char* who,
                 bool pca) {
    srx_ctx* ctx = m->ctx;
    const uint64_t n = m->csc ? m->n_cols : m->n_rows, G = m->csc ? m->n_rows : m->n_cols;
    if (ctx->n_ranks > 1) return fail(ctx, SRX_E_ARG, "%s: a context with more than one rank (the sharded form is out of scope)", who);
    if (ctx->pool_on > 0) return fail(ctx, SRX_E_ARG, "%s: a backed session is open on this context (the out-of-core form is out of scope)", who);
    const double mv = opts ? opts->max_value : 0.0;
    if (!(mv >= 0.0)) return fail(ctx, SRX_E_ARG, "%s: max_value = %g (negative or NaN)", who, mv);
    if (p > (uint64_t)kRgMaxCov) return fail(ctx, SRX_E_ARG, "%s: %llu covariates (at most %d)", who, (unsigned long long)p, kRgMaxCov);
    if (k == 0) return fail(ctx, SRX_E_ARG, "%s: an empty gene list (k >= 1)", who);
    SRX_TRY(dense_check_list(ctx, who, genes, k, G));
    if (opts && opts->pca.scale > 0) return fail(ctx, SRX_E_ARG, "%s: pca.scale is set (scaling is the `scale` flag of this call)", who);
    if (opts && opts->pca.solver == SRX_SOLVER_SPMM)
        return fail(ctx, SRX_E_ARG, "%s: the matrix-free solver walks sparse rows; the regressed values are dense (solver 0 or 1)", who);
    if (n < p + 2) return fail(ctx, SRX_E_SHAPE, "%s: %llu cells for %llu covariates and the intercept (n >= p + 2)", who, (unsigned long long)n,
                               (unsigned long long)p);
    if (pca && (k < 2 || n < 5)) return fail(ctx, SRX_E_SHAPE, "%s: %llu cells x %llu genes (a PCA needs n >= 5 and k >= 2)", who,
                                             (unsigned long long)n, (unsigned long long)k);
    return SRX_OK;
}

// refusals (8) to (10), and everything that is read from the handle as the caller gave it (a CSC handle is transposed afterwards)
int32_t rg_prepare(srx_mat* m, const uint64_t* genes, uint64_t k, const double* cov, uint64_t p64, const srx_regress_opts* opts,
                   const char* who, RgPrep& P) {
    srx_ctx* ctx = m->ctx;
    SRX_HIP(ctx, hipSetDevice(ctx->device));
    const uint64_t n = m->csc ? m->n_cols : m->n_rows, G = m->csc ? m->n_rows : m->n_cols;
    const int p = (int)p64;
    P.n = n;
    P.G = G;
    P.k = (int)k;
    P.p = p;
    P.scale = (!opts || opts->scale != 0) ? 1 : 0;
    P.max_value = opts ? opts->max_value : 0.0;
    for (uint64_t e = 0; e < n * p64; ++e)
        if (!is_finite(cov[e]))
            return fail(ctx, SRX_E_ARG, "%s: covariate %llu of cell %llu is not finite", who, (unsigned long long)(e % p64), (unsigned long long)(e / p64));
    // cbar in ascending cell order, Ct, then A = Ct^T Ct by the weighted column sum over Ct itself (one chunk of n rows)
    P.ct.assign((size_t)n * p, 0.0);
    std::vector<double>& A = P.A;
    A.assign((size_t)p * p, 0.0);
    P.cbar.assign(p, 0.0);
    if (p > 0) {
        for (int q = 0; q < p; ++q) {
            double sum = 0.0;
            for (uint64_t i = 0; i < n; ++i) sum += cov[i * p64 + q];
            const double cbar = P.cbar[q] = sum / (double)n;
            for (uint64_t i = 0; i < n; ++i) P.ct[i * p64 + q] = cov[i * p64 + q] - cbar;
        }
        double *d_ct, *d_part, *d_A;
        SRX_TRY(scratch(ctx, "rg_ct", (size_t)n * p * sizeof(double), (void**)&d_ct));
        SRX_TRY(scratch(ctx, "rg_cov_part", (size_t)kRgCovSlabs * p * p * sizeof(double), (void**)&d_part));
        SRX_TRY(scratch(ctx, "rg_A", (size_t)p * p * sizeof(double), (void**)&d_A));
        SRX_TRY(h2d(ctx, d_ct, P.ct.data(), (size_t)n * p * sizeof(double)));
        StreamTimer timer(ctx, ctx->stream);
        SRX_TRY(timer.start());
        SRX_HIP(ctx, hipMemsetAsync(d_A, 0, (size_t)p * p * sizeof(double), ctx->stream));
        SRX_TRY(rg_wsum(ctx, d_ct, (uint32_t)p, n, (uint32_t)p, d_ct, (uint32_t)p, p, 0, kRgCovSlabs, d_part, d_A));
        SRX_TRY(timer.stop(&P.ms_cov));
        SRX_TRY(d2h(ctx, A.data(), d_A, A.size() * sizeof(double)));
    }
    // the Cholesky factor of D^-1/2 A D^-1/2; a pivot is 1 - R^2 of the covariate on the earlier ones
    P.dsq.assign(p, 1.0);
    P.Lf.assign((size_t)p * p, 0.0);
    P.min_pivot = 1.0;
    for (int q = 0; q < p; ++q) {
        if (!(A[(size_t)q * p + q] > 0.0)) return fail(ctx, SRX_E_ARG, "%s: covariate %d is constant (A_qq = 0)", who, q);
        P.dsq[q] = std::sqrt(A[(size_t)q * p + q]);
    }
    for (int j = 0; j < p; ++j) {
        double* L = P.Lf.data();
        double piv = (A[(size_t)j * p + j] / P.dsq[j]) / P.dsq[j];
        for (int t = 0; t < j; ++t) piv -= L[j * p + t] * L[j * p + t];
        P.min_pivot = std::min(P.min_pivot, piv);
        if (!(piv >= kRgMinPivot))
            return fail(ctx, SRX_E_ARG, "%s: covariate %d is collinear with the earlier ones (pivot %.3e < %.0e)", who, j, piv, kRgMinPivot);
        L[j * p + j] = std::sqrt(piv);
        for (int i = j + 1; i < p; ++i) {
            double v = (A[(size_t)i * p + j] / P.dsq[i]) / P.dsq[j];
            for (int t = 0; t < j; ++t) v -= L[i * p + t] * L[j * p + t];
            L[i * p + j] = v / L[j * p + j];
        }
    }
    // the stored values
    if (m->nnz) {
        unsigned long long* d_small;
        SRX_TRY(scratch(ctx, "rg_small", 256, (void**)&d_small));
        SRX_HIP(ctx, hipMemsetAsync(d_small, 0, 256, ctx->stream));
        value_scan(m, d_small);
        SRX_HIP(ctx, hipGetLastError());
        unsigned long long flags = 0;
        SRX_TRY(d2h(ctx, &flags, d_small + VS_FLAGS, sizeof flags));
        if (flags & kValNonFinite) return fail(ctx, SRX_E_ARG, "%s: the matrix holds a NaN or infinite value", who);
    }
    // xbar from the library's own column sums; the genes whose n values are all equal from its counts and extremes
    std::vector<double> sum(at_least_one(G)), mn(at_least_one(G)), mx(at_least_one(G));
    std::vector<uint32_t> cnt(at_least_one(G));
    SRX_TRY(srx_compute_sum(m, SRX_COLUMN, sum.data()));
    SRX_TRY(srx_compute_number(m, SRX_COLUMN, cnt.data()));
    SRX_TRY(srx_compute_min_max(m, SRX_COLUMN, mn.data(), mx.data()));
    P.xbar.resize(k);
    P.cst.resize(k);
    P.n_const = 0;
    for (uint64_t a = 0; a < k; ++a) {
        const uint64_t j = genes[a];
        P.xbar[a] = sum[j] / (double)n;
        const bool all_zero = cnt[j] == 0 || (mn[j] == 0.0 && mx[j] == 0.0);
        const bool one_value = (uint64_t)cnt[j] == n && mn[j] == mx[j];
        P.cst[a] = (all_zero || one_value) ? 1 : 0;
        P.n_const += P.cst[a];
    }
    return SRX_OK;
}

// what makes rows [row0, row0 + rows) of the chunk in `mode`; COUNT: the clipped pairs are counted into R.d_cnt
template <bool COUNT>
DenseChunkFn rg_maker(srx_mat* m, const RgRun& R, const RgPrep& P, int mode) {
    const RgArgs a{R.d_ct, R.d_beta, R.d_xbar, R.d_s, R.d_cst, P.max_value, (uint32_t)P.k, P.p, mode};
    return [m, &R, a](uint64_t row0, uint64_t rows, double* Z) { return dense_make_chunk<RgArgs, COUNT>(m, R.sl, R.g, a, row0, rows, Z, R.d_cnt); };
}

int32_t rg_clipped(srx_ctx* ctx, const RgRun& R, uint64_t* n_clipped) {
    unsigned long long c[3];
    SRX_TRY(d2h(ctx, c, R.d_cnt, sizeof c));
    *n_clipped = (uint64_t)(c[0] + c[1] - c[2]);
    return SRX_OK;
}

// `m` is a CSR handle of the cells' rows.  The fit, the scale, then what `stage` asks for.
int32_t rg_run(srx_mat* m, const uint64_t* genes, const srx_regress_opts* opts, const RgPrep& P, int stage, const RgOut& out,
               srx_regress_info* info) {
    srx_ctx* ctx = m->ctx;
    const uint64_t n = P.n, G = P.G;
    const int k = P.k, p = P.p;
    srx_regress_info inf;
    memset(&inf, 0, sizeof inf);
    inf.n_cells = n;
    inf.n_genes = (uint64_t)k;
    inf.n_cov = (uint64_t)p;
    inf.n_constant_genes = P.n_const;
    inf.min_pivot = P.min_pivot;

    RgRun R;
    SRX_TRY(dense_slots_setup(ctx, genes, (uint64_t)k, G, R.sl));
    const std::vector<int>& slot_of_pos = R.sl.slot_of_pos;
    std::vector<double> xbar(k);
    std::vector<uint8_t> cst(k);
    for (int a = 0; a < k; ++a) {
        xbar[slot_of_pos[a]] = P.xbar[a];
        cst[slot_of_pos[a]] = P.cst[a];
    }
    R.beta.assign((size_t)std::max(p, 1) * k, 0.0);
    R.s.assign(k, 1.0);
    const size_t beta_bytes = (size_t)std::max(p, 1) * k * sizeof(double);
    SRX_TRY(scratch(ctx, "rg_ct", at_least_one((uint64_t)n * p) * sizeof(double), (void**)&R.d_ct));
    SRX_TRY(scratch(ctx, "rg_beta", beta_bytes, (void**)&R.d_beta));
    SRX_TRY(scratch(ctx, "rg_xbar", (size_t)k * sizeof(double), (void**)&R.d_xbar));
    SRX_TRY(scratch(ctx, "rg_s", (size_t)k * sizeof(double), (void**)&R.d_s));
    SRX_TRY(scratch(ctx, "rg_cst", (size_t)k, (void**)&R.d_cst));
    SRX_TRY(scratch(ctx, "rg_cnt", 256, (void**)&R.d_cnt));
    if (p > 0) SRX_TRY(h2d(ctx, R.d_ct, P.ct.data(), (size_t)n * p * sizeof(double)));      // (a CSC call: the transpose ran in between)
    SRX_TRY(h2d(ctx, R.d_beta, R.beta.data(), beta_bytes));
    SRX_TRY(h2d(ctx, R.d_xbar, xbar.data(), (size_t)k * sizeof(double)));
    SRX_TRY(h2d(ctx, R.d_s, R.s.data(), (size_t)k * sizeof(double)));
    SRX_TRY(h2d(ctx, R.d_cst, cst.data(), (size_t)k));
    SRX_HIP(ctx, hipMemsetAsync(R.d_cnt, 0, 256, ctx->stream));
    SRX_TRY(dense_chunks_setup(ctx, n, (uint64_t)k, opts ? opts->chunk_cells : 0, R.g));
    inf.n_chunks = R.g.n_chunks;
    inf.chunk_cells = R.g.chunk;
    inf.chunk_bytes = R.g.chunk * (uint64_t)R.g.ldz * sizeof(double);

    const int nw_max = std::max(p, 1);
    const int slabs_max = (int)std::min<uint64_t>((R.g.chunk + 63) / 64, kRgMaxSlabs);
    double *d_part, *d_sums;
    SRX_TRY(scratch(ctx, "rg_part", (size_t)slabs_max * nw_max * k * sizeof(double), (void**)&d_part));
    SRX_TRY(scratch(ctx, "rg_sums", (size_t)nw_max * k * sizeof(double), (void**)&d_sums));

    // pass 1: W = Ct^T X over chunks of the stored values, then the k solves
    inf.ms_fit = P.ms_cov;
    if (p > 0) {
        StreamTimer timer(ctx, ctx->stream);
        SRX_TRY(timer.start());
        SRX_HIP(ctx, hipMemsetAsync(d_sums, 0, (size_t)p * k * sizeof(double), ctx->stream));
        const DenseChunkFn make_x = rg_maker<false>(m, R, P, kRgRaw);
        for (uint64_t row0 = 0; row0 < n; row0 += R.g.chunk) {
            const uint64_t rows = std::min(R.g.chunk, n - row0);
            SRX_TRY(make_x(row0, rows, R.g.d_Z));
            SRX_TRY(rg_wsum(ctx, R.g.d_Z, R.g.ldz, rows, (uint32_t)k, R.d_ct + row0 * (size_t)p, (uint32_t)p, p, 0, slabs_max, d_part, d_sums));
        }
        double ms = 0.0;
        SRX_TRY(timer.stop(&ms));
        inf.ms_fit += ms;
        std::vector<double> W((size_t)p * k);
        SRX_TRY(d2h(ctx, W.data(), d_sums, W.size() * sizeof(double)));
        if (stage == kStageSums) {
            for (int q = 0; q < p; ++q) {
                if (out.cbar) out.cbar[q] = P.cbar[q];
                for (int t = 0; out.A && t < p; ++t) out.A[(size_t)q * p + t] = P.A[(size_t)q * p + t];
                for (int a = 0; out.W && a < k; ++a) out.W[(size_t)q * k + a] = W[(size_t)q * k + slot_of_pos[a]];
            }
            if (info) *info = inf;
            return SRX_OK;
        }
        const double* L = P.Lf.data();
        double u[kRgMaxCov];
        for (int j = 0; j < k; ++j) {
            for (int q = 0; q < p; ++q) {                      // L u = D^-1/2 w
                double v = W[(size_t)q * k + j] / P.dsq[q];
                for (int t = 0; t < q; ++t) v -= L[q * p + t] * u[t];
                u[q] = v / L[q * p + q];
            }
            for (int q = p - 1; q >= 0; --q) {                 // L^T v = u
                double v = u[q];
                for (int t = q + 1; t < p; ++t) v -= L[t * p + q] * u[t];
                u[q] = v / L[q * p + q];
            }
            for (int q = 0; q < p; ++q) R.beta[(size_t)q * k + j] = u[q] / P.dsq[q];
        }
        SRX_TRY(h2d(ctx, R.d_beta, R.beta.data(), beta_bytes));
    }

    // pass 2: sum r^2 over chunks of the residuals
    if (P.scale) {
        StreamTimer timer(ctx, ctx->stream);
        SRX_TRY(timer.start());
        SRX_HIP(ctx, hipMemsetAsync(d_sums, 0, (size_t)k * sizeof(double), ctx->stream));
        const DenseChunkFn make_r = rg_maker<false>(m, R, P, kRgResid);
        for (uint64_t row0 = 0; row0 < n; row0 += R.g.chunk) {
            const uint64_t rows = std::min(R.g.chunk, n - row0);
            SRX_TRY(make_r(row0, rows, R.g.d_Z));
            SRX_TRY(rg_wsum(ctx, R.g.d_Z, R.g.ldz, rows, (uint32_t)k, nullptr, 0, 1, 1, slabs_max, d_part, d_sums));
        }
        SRX_TRY(timer.stop(&inf.ms_scale));
        std::vector<double> ss(k);
        SRX_TRY(d2h(ctx, ss.data(), d_sums, ss.size() * sizeof(double)));
        for (int j = 0; j < k; ++j) {
            const double v = ss[j] / (double)(n - 1);
            R.s[j] = v == 0.0 ? 1.0 : std::sqrt(v);
        }
        SRX_TRY(h2d(ctx, R.d_s, R.s.data(), (size_t)k * sizeof(double)));
    }

    const DenseChunkFn make_z = rg_maker<false>(m, R, P, kRgZ), make_z_counted = rg_maker<true>(m, R, P, kRgZ);

    if (stage == kStageFit) {
        for (int a = 0; a < k; ++a) {
            const int s = slot_of_pos[a];
            if (out.xbar) out.xbar[a] = P.xbar[a];
            if (out.sd) out.sd[a] = R.s[s];
            for (int q = 0; out.beta && q < p; ++q) out.beta[(size_t)q * k + a] = R.beta[(size_t)q * k + s];
        }
    } else if (stage == kStageBlock) {
        std::vector<double> h((size_t)R.g.chunk * R.g.ldz);
        for (uint64_t row0 = 0; row0 < n; row0 += R.g.chunk) {
            const uint64_t rows = std::min(R.g.chunk, n - row0);
            SRX_TRY(make_z_counted(row0, rows, R.g.d_Z));
            SRX_TRY(d2h(ctx, h.data(), R.g.d_Z, (size_t)rows * R.g.ldz * sizeof(double)));
            for (uint64_t i = 0; i < rows; ++i)
                for (int a = 0; a < k; ++a) out.block[(row0 + i) * (uint64_t)k + a] = h[i * R.g.ldz + slot_of_pos[a]];
        }
        SRX_TRY(rg_clipped(ctx, R, &inf.n_clipped));
    } else if (stage == kStageGram) {
        double *Gp, *colsum;
        SRX_TRY(dense_gram_pass(ctx, R.g, make_z_counted, &Gp, &colsum, &inf.ms_gram));
        SRX_TRY(dense_gram_fetch(ctx, R.sl, Gp, colsum, out.gram, out.colsum));
        SRX_TRY(rg_clipped(ctx, R, &inf.n_clipped));
    } else {
        m->pca.valid = false;
        srx_pca_opts po{};
        if (opts) po = opts->pca;
        else po.n_components = -1;
        po.scale = 0;
        po.center = 1;
        Resolved o;
        int l_act = 0;
        SRX_TRY(resolve_opts(ctx, &po, k, m->n_rows, false, o, l_act));
        // clips are counted in the Gram pass only; Z is scaled where it is made, so the result block's std is s
        DenseSolved sv;
        const int32_t rc = dense_pca_solve(m, o, l_act, genes, R.g, make_z_counted, make_z, kResidualRegress, 1, R.d_s, sv);
        if (!sv.solved) return rc;
        SRX_TRY(rg_clipped(ctx, R, &inf.n_clipped));
        inf.ms_gram = sv.ms_gram;
        inf.ms_solve = sv.ms_solve;
        inf.ms_scores = sv.ms_scores;
        inf.pca = sv.pca;
        if (info) *info = inf;
        return rc;
    }
    if (info) *info = inf;
    return SRX_OK;
}

int32_t rg_entry(srx_mat* m, const uint64_t* genes, uint64_t k, const double* cov, uint64_t p, const srx_regress_opts* opts, const char* who,
                 int stage, const RgOut& out, srx_regress_info* info) {
    SRX_TRY(rg_check(m, genes, k, cov, p, opts, who, stage == kStagePca));
    RgPrep P;
    SRX_TRY(rg_prepare(m, genes, k, cov, p, opts, who, P));
    // the chunks are made from the cells' rows
    return on_cells_csr(m, stage == kStagePca, [&](srx_mat* x) { return rg_run(x, genes, opts, P, stage, out, info); });
}

}  // namespace

}  // namespace srx

using namespace srx;

extern "C" {

int32_t srx_regress_fit(srx_mat* m, const uint64_t* genes, uint64_t k, const double* cov, uint64_t p, const srx_regress_opts* opts,
                        double* beta_out, double* xbar_out, double* sd_out, srx_regress_info* info) {
    if (!m || !genes || (!cov && p) || (!beta_out && !xbar_out && !sd_out))
        return fail(m ? m->ctx : nullptr, SRX_E_ARG, "regress_fit: null argument");
    RgOut out;
    out.beta = beta_out;
    out.xbar = xbar_out;
    out.sd = sd_out;
    return rg_entry(m, genes, k, cov, p, opts, "regress_fit", kStageFit, out, info);
}

int32_t srx_regress_sums(srx_mat* m, const uint64_t* genes, uint64_t k, const double* cov, uint64_t p, const srx_regress_opts* opts,
                         double* cbar_out, double* a_out, double* w_out, srx_regress_info* info) {
    if (!m || !genes || !cov || (!cbar_out && !a_out && !w_out)) return fail(m ? m->ctx : nullptr, SRX_E_ARG, "regress_sums: null argument");
    if (p == 0) return fail(m->ctx, SRX_E_ARG, "regress_sums: no covariate (p >= 1)");
    RgOut out;
    out.cbar = cbar_out;
    out.A = a_out;
    out.W = w_out;
    return rg_entry(m, genes, k, cov, p, opts, "regress_sums", kStageSums, out, info);
}

int32_t srx_regress_residuals(srx_mat* m, const uint64_t* genes, uint64_t k, const double* cov, uint64_t p, const srx_regress_opts* opts,
                              double* block, srx_regress_info* info) {
    if (!m || !genes || (!cov && p) || !block) return fail(m ? m->ctx : nullptr, SRX_E_ARG, "regress_residuals: null argument");
    RgOut out;
    out.block = block;
    return rg_entry(m, genes, k, cov, p, opts, "regress_residuals", kStageBlock, out, info);
}

int32_t srx_regress_gram(srx_mat* m, const uint64_t* genes, uint64_t k, const double* cov, uint64_t p, const srx_regress_opts* opts,
                         double* gram_out, double* colsum_out, srx_regress_info* info) {
    if (!m || !genes || (!cov && p) || (!gram_out && !colsum_out)) return fail(m ? m->ctx : nullptr, SRX_E_ARG, "regress_gram: null argument");
    RgOut out;
    out.gram = gram_out;
    out.colsum = colsum_out;
    return rg_entry(m, genes, k, cov, p, opts, "regress_gram", kStageGram, out, info);
}

int32_t srx_pca_regress(srx_mat* m, const uint64_t* genes, uint64_t k, const double* cov, uint64_t p, const srx_regress_opts* opts,
                        double* scores, double* components, double* evr, double* mean, double* sd, srx_regress_info* info) {
    if (!m || !genes || (!cov && p)) return fail(m ? m->ctx : nullptr, SRX_E_ARG, "pca_regress: null argument");
    const int32_t rc = rg_entry(m, genes, k, cov, p, opts, "pca_regress", kStagePca, RgOut{}, info);
    if (rc != SRX_OK && rc != SRX_E_NOCONV) return rc;
    const int32_t rc2 = srx_result_fetch(m, scores, components, evr, mean, sd, nullptr);
    return rc2 != SRX_OK ? rc2 : rc;
}

}  // extern "C"
