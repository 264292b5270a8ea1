// pca_solve.hip — the solver half of dim_red::pca_inplace on the GPU (pca.hip has the overview): the sparse products with a
// k x 64 panel (spmm.inl), the k x 64 subspace iteration on the device (iterate.inl, jacobi.inl: dense apply on the f64 matrix
// cores, CholeskyQR, Jacobi eigen-solve, Chebyshev filter, residuals; replayed from hipGraphs: struct Iteration), the operators and the
// solver driver (run_pca: deflation rounds, plans A / B, the transform; every host decision: pca_schedule.hpp), srx_spmm (the raw operators, for kernel-level parity tests) and the PCA model
// of srx_pca_transform (pca_model.inl).
#include "pca_internal.hpp"
#include "hash.hpp"

namespace srx {

#include "spmm.inl"

#include "iterate.inl"

// ---- launches ---------------------------------------------------------------------------------
template <typename VT, typename PT>
static int32_t launch_fwd(srx_ctx* ctx, const Tiled& c, const PT* P, const PT* cvec, PT* Y, double* scores = nullptr,
                          int n_pc = 0, int ld = 0) {
    // the output is either the N x 64 panel product (SpMM solver) or, for the transform, the N x n_pc f64 scores
    const double out_bytes = scores ? (double)c.n_rows * n_pc * 8.0 : (double)c.n_rows * L * sizeof(PT);
    const double bytes = (double)c.nnz * (4.0 + sizeof(VT)) + (double)((uint64_t)c.nt * c.n_rows + 1) * 8.0 + out_bytes +
                         (double)c.k * L * sizeof(PT);
    const size_t lds = (size_t)KT * L * sizeof(PT);
    constexpr int kRowsPerWg = (kFwdThreads / 16) * FwdCfg<PT>::kRows;
    const uint64_t n_blocks = (c.n_rows + kRowsPerWg - 1) / kRowsPerWg;
    const int per_cu = sizeof(PT) == 4 ? 2 : 1;                 // 64 KiB vs 128 KiB of LDS per workgroup
    uint64_t grid = (uint64_t)ctx->n_cus * per_cu;
    if (grid > n_blocks) grid = n_blocks;
    if (grid < 1) grid = 1;
    ProfScope ps(ctx, SRX_K_SPMM_FWD, bytes);
    SRX_HIP(ctx, hipFuncSetAttribute((const void*)k_spmm_fwd<VT, PT>, hipFuncAttributeMaxDynamicSharedMemorySize,
                                     (int)lds));
    hipLaunchKernelGGL((k_spmm_fwd<VT, PT>), dim3((unsigned)grid), dim3(kFwdThreads), lds, ctx->stream, c.tptr,
                       (const GramPk<VT>*)c.tpk, c.n_rows, c.nt, c.k, P, cvec, Y, scores, n_pc, ld ? ld : n_pc);
    SRX_HIP(ctx, hipGetLastError());
    return SRX_OK;
}

// Lanes per row of the row-major forward kernel (k_spmm_rows): the widest panel slice (4 Q columns of all k genes) that fits
// the LDS; 0 when even one lane's four columns do not (launch_fwd_rows then walks the genes in ranges).
template <typename PT>
static int fwd_rows_q(int k) {
    const size_t budget = 163840 - 64;
    for (int q = sizeof(PT) == 4 ? 4 : 2; q >= 1; q >>= 1)
        if ((size_t)k * 4 * q * sizeof(PT) <= budget) return q;
    return 0;
}

template <typename VT, typename PT>
static int32_t launch_fwd_rows(srx_ctx* ctx, const RowMajor& r, const PT* P, const PT* cvec, int n_cols, double* scores, PT* Y,
                               int ld) {
    const int Qr = fwd_rows_q<PT>(r.k);
    auto go = [&](auto qtag, auto rtag, auto cltag, int k_lo, int k_hi, int accumulate) -> int32_t {
        constexpr int Q = decltype(qtag)::value;
        constexpr bool RANGE = decltype(rtag)::value;
        constexpr int CL = decltype(cltag)::value;
        constexpr int C = CL * Q;
        const int n_slices = (n_cols + C - 1) / C;
        // (a gene's 16 f32 columns are 64 bytes, so every 16-byte read of a wave's 16 cells starts in bank 0 or 16: half of
        //  the LDS pipe's time goes to bank conflicts, profiles/r03_pmc_spmm.md.  A padded stride of 80 bytes was measured:
        //  0.746 against 0.745 ms — the multiplication is hidden behind the kernel's reads and stores either way)
        const int ldp = C;
        const size_t lds = (size_t)(k_hi - k_lo) * ldp * sizeof(PT);
        const uint64_t groups = kFwdRowsThreads / Q;
        uint64_t n_wg = (r.n_rows + groups - 1) / groups;
        // one workgroup per CU at a time (the panel slice fills the LDS), eight in a row: shorter workgroups even out the CUs
        // (c3, f32: 1 / 2 / 4 / 8 / 16 / 32 per CU: 0.73 / 0.71 / 0.70 / 0.69 / 0.68 / 0.77 ms; f64 panels 1.37 -> 1.30 at 8)
        uint64_t cap = std::max<uint64_t>(1, (uint64_t)ctx->n_cus * 8 / n_slices);
        if (cap > 8) cap &= ~(uint64_t)7;           // (whole rounds of the 8 XCDs: the slices of a row range share an L2)
        if (n_wg > cap) n_wg = cap;
        if (n_wg < 1) n_wg = 1;
        const double out_bytes = scores ? (double)r.n_rows * n_cols * 8.0 : (double)r.n_rows * L * sizeof(PT);
        ProfScope ps(ctx, SRX_K_SPMM_FWD, (double)r.nnz * sizeof(GramPk<VT>) + (double)(r.n_rows + 1) * 8.0 + out_bytes +
                                              (double)(k_hi - k_lo) * L * sizeof(PT) + (r.perm ? (double)r.n_rows * 4.0 : 0.0));
        SRX_HIP(ctx, hipFuncSetAttribute((const void*)k_spmm_rows<VT, PT, Q, RANGE, CL>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        hipLaunchKernelGGL((k_spmm_rows<VT, PT, Q, RANGE, CL>), dim3((unsigned)(n_wg * n_slices)), dim3(kFwdRowsThreads), lds, ctx->stream,
                           r.ptr, (const GramPk<VT>*)r.pk, (const uint32_t*)r.perm, r.n_rows, r.k, P, cvec, n_cols, scores, Y, ld, ldp,
                           k_lo, k_hi, accumulate, 0);
        SRX_HIP(ctx, hipGetLastError());
        return SRX_OK;
    };
    using No = std::false_type;
    using Yes = std::true_type;
    using C4 = std::integral_constant<int, 4>;
    using C5 = std::integral_constant<int, 5>;
    // five columns per lane where the wider slice fits the LDS, saves a pass over the matrix (n_pc = 50: 3 slices of 20 instead
    // of 4 of 16; 5 of 10 instead of 7 of 8 with f64 panels) and stays inside the panel's 64 columns
    constexpr int Qmax = sizeof(PT) == 4 ? 4 : 2;
    const int wide_slices = (n_cols + 5 * Qmax - 1) / (5 * Qmax), narrow_slices = (n_cols + 4 * Qmax - 1) / (4 * Qmax);
    // (f32 panels: 3 slices of 20 columns measured the same 0.64-0.70 ms as 4 of 16 — the launch is not bound by its passes, DESIGN.md 3c —
    //  with the LDS pipe 66 % busy instead of 51 (the 80-byte gene stride conflicts more) and 1.8 GB fetched instead of 1.2:
    //  the wide form is for f64 panels, 1.85 -> 1.35 ms)
    const bool wide = Qr == Qmax && (size_t)r.k * 5 * Qmax * sizeof(PT) <= (size_t)163840 && wide_slices < narrow_slices &&
                      wide_slices * 5 * Qmax <= L && sizeof(PT) == 8;
    if (wide) return go(std::integral_constant<int, Qmax>{}, No{}, C5{}, 0, r.k, 0);
    if (Qr == 4) {
        if constexpr (sizeof(PT) == 4) return go(std::integral_constant<int, 4>{}, No{}, C4{}, 0, r.k, 0);
        else return SRX_E_ARG;
    }
    if (Qr == 2) return go(std::integral_constant<int, 2>{}, No{}, C4{}, 0, r.k, 0);
    if (Qr == 1) return go(std::integral_constant<int, 1>{}, No{}, C4{}, 0, r.k, 0);
    // wider than one slice of four columns: gene ranges of the widest slice, one launch each, the later ones accumulating
    const int per = (int)((163840 - 64) / (4 * sizeof(PT)));
    for (int k_lo = 0, i = 0; k_lo < r.k; k_lo += per, ++i)
        SRX_TRY(go(std::integral_constant<int, 1>{}, Yes{}, C4{}, k_lo, std::min(r.k, k_lo + per), i > 0 ? 1 : 0));
    return SRX_OK;
}

// rows ordered by their number of kept entries (k_spmm_rows); r.ptr must be complete
int32_t build_row_order(srx_ctx* ctx, RowMajor& r) {
    uint32_t* hist;
    SRX_TRY(scratch(ctx, "pca_rm_lenhist", kLenBins * sizeof(uint32_t), (void**)&hist));
    SRX_TRY(scratch(ctx, "pca_rm_perm", (r.n_rows ? r.n_rows : 1) * sizeof(uint32_t), (void**)&r.perm));
    SRX_HIP(ctx, hipMemsetAsync(hist, 0, kLenBins * sizeof(uint32_t), ctx->stream));
    const unsigned g = (unsigned)((r.n_rows + kLenRowsPerWg - 1) / kLenRowsPerWg + (r.n_rows ? 0 : 1));
    hipLaunchKernelGGL(k_len_hist, dim3(g), dim3(256), 0, ctx->stream, r.ptr, r.n_rows, hist);
    hipLaunchKernelGGL(k_len_scan, dim3(1), dim3(kLenBins), 0, ctx->stream, hist);
    hipLaunchKernelGGL(k_len_scatter, dim3(g), dim3(256), 0, ctx->stream, r.ptr, r.n_rows, hist, r.perm);
    SRX_HIP(ctx, hipGetLastError());
    return SRX_OK;
}

template <typename VT, typename YT>
static int32_t launch_t(srx_ctx* ctx, const Tiled& c, const YT* Y, double* T /* k*L + L */) {
    uint64_t want = (uint64_t)(2 * ctx->n_cus) / (uint64_t)c.nt;
    if (want < 1) want = 1;
    uint64_t by_rows = (c.n_rows + 255) / 256;
    if (by_rows < 1) by_rows = 1;
    const uint64_t n_rb = want < by_rows ? want : by_rows;
    const uint64_t rpb = (c.n_rows + n_rb - 1) / n_rb > 0 ? (c.n_rows + n_rb - 1) / n_rb : 1;
    double *part, *part_s;
    SRX_TRY(scratch(ctx, "pca_tpart", n_rb * (size_t)c.k * L * sizeof(double), (void**)&part));
    SRX_TRY(scratch(ctx, "pca_tpart_s", n_rb * L * sizeof(double), (void**)&part_s));
    const size_t lds = (size_t)KT * L * sizeof(double);
    const double bytes = (double)c.nnz * (4.0 + sizeof(VT)) + (double)((uint64_t)c.nt * c.n_rows + 1) * 8.0 +
                         (double)c.n_rows * L * sizeof(YT) + (double)c.k * L * 8.0;
    {
        ProfScope ps(ctx, SRX_K_SPMM_T, bytes);
        SRX_HIP(ctx, hipFuncSetAttribute((const void*)k_spmm_t<VT, YT, double>,
                                         hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        hipLaunchKernelGGL((k_spmm_t<VT, YT, double>), dim3((unsigned)(n_rb * c.nt)), dim3(kTThreads), lds, ctx->stream,
                           c.tptr, (const GramPk<VT>*)c.tpk, c.n_rows, c.k, c.nt, rpb, Y, part, part_s);
        uint64_t tot = (uint64_t)c.k * L + L;
        hipLaunchKernelGGL((k_t_reduce<double>), dim3((unsigned)((tot + 255) / 256)), dim3(256), 0, ctx->stream, part,
                           part_s, c.k, n_rb, T);
    }
    SRX_HIP(ctx, hipGetLastError());
    return SRX_OK;
}

struct Work {                   // k x 64 f64 state, replicated per rank
    double *W, *Wp, *T, *A1, *A2, *small, *mu, *d, *gpart;
    double *dHG, *dM, *dM2, *dTheta, *dRho, *dColmax, *dSgn, *dDinv, *dXi;
};

static int32_t alloc_work(srx_ctx* ctx, int k, Work& w) {
    const size_t kl = (size_t)k * L;
    SRX_TRY(scratch(ctx, "pca_W", kl * 8, (void**)&w.W));
    SRX_TRY(scratch(ctx, "pca_Wp", kl * 8, (void**)&w.Wp));
    SRX_TRY(scratch(ctx, "pca_T", (kl + L) * 8, (void**)&w.T));
    SRX_TRY(scratch(ctx, "pca_A1", kl * 8, (void**)&w.A1));
    SRX_TRY(scratch(ctx, "pca_A2", kl * 8, (void**)&w.A2));
    SRX_TRY(scratch(ctx, "pca_small", (6 * L * L + 8 * L + 4 * 16 * 16) * 8, (void**)&w.small));
    SRX_TRY(scratch(ctx, "pca_mu", (size_t)k * 8, (void**)&w.mu));
    SRX_TRY(scratch(ctx, "pca_d", (size_t)k * 8, (void**)&w.d));
    SRX_TRY(scratch(ctx, "pca_g2part", (size_t)kGram2Blocks * 2 * L * L * 8, (void**)&w.gpart));
    w.dHG = w.small;                    // H then G, contiguous 2 x L x L
    w.dM = w.small + 2 * L * L;
    w.dM2 = w.small + 3 * L * L;
    w.dTheta = w.small + 4 * L * L;
    w.dRho = w.dTheta + L;
    w.dColmax = w.dRho + L;
    w.dSgn = w.dColmax + L;
    w.dDinv = w.dSgn + L;
    w.dXi = w.small + 6 * L * L + 8 * L;       // the CholeskyQR's inverted 16 x 16 diagonal blocks of R
    return SRX_OK;
}

static int32_t gram2(srx_ctx* ctx, const Work& w, const double* A, const double* B, int k) {
    int nb = (k + 31) / 32;                    // one 32-row slab per workgroup where the block count allows
    if (nb > kGram2Blocks) nb = kGram2Blocks;
    if (nb < 1) nb = 1;
    hipLaunchKernelGGL(k_gram2_part, dim3(nb), dim3(1024), 0, ctx->stream, A, B, k, w.gpart);
    hipLaunchKernelGGL(k_gram2_reduce, dim3((2 * L * L + 255) / 256), dim3(256), 0, ctx->stream, w.gpart, nb, w.dHG);
    SRX_HIP(ctx, hipGetLastError());
    return SRX_OK;
}

// The launch of every kernel of the iteration: grid, block, dynamic LDS.  Iteration's segments and srx_iterate_op (the
// kernel-level entry) both go through these, so that what the tests launch is what the solver launches.  They only enqueue
// on ctx->stream: the caller reads hipGetLastError.
static int32_t attr_dense_apply(srx_ctx* ctx) {
    SRX_HIP(ctx, hipFuncSetAttribute((const void*)k_dense_apply, hipFuncAttributeMaxDynamicSharedMemorySize, (int)kDenseLds));
    return SRX_OK;
}
static int32_t attr_jacobi(srx_ctx* ctx) {
    SRX_HIP(ctx, hipFuncSetAttribute((const void*)k_jacobi_eig2, hipFuncAttributeMaxDynamicSharedMemorySize, (int)sizeof(J2Lds)));
    return SRX_OK;
}
static void launch_dense_apply(srx_ctx* ctx, const double* C, const double* Win, int k, double* Wout) {
    hipLaunchKernelGGL(k_dense_apply, dim3((k + 31) / 32, kDenseSplit), dim3(kDenseWaves * 64), kDenseLds, ctx->stream, C, Win, k, Wout);
}
static void launch_gram1(srx_ctx* ctx, const double* A, const double* B, int k, double* H) {
    int nb = (k + 31) / 32;
    if (nb > kGram1Blocks) nb = kGram1Blocks;
    hipLaunchKernelGGL(k_gram1_part, dim3(nb), dim3(1024), 0, ctx->stream, A, B, k, H);
}
static void launch_chol(srx_ctx* ctx, const double* G, int n, double* R, double* dinv, int* status, int shifted) {
    hipLaunchKernelGGL(k_chol_factor, dim3(1), dim3(1024), 0, ctx->stream, G, n, R, dinv, status, shifted);
}
static void launch_chol_mfma(srx_ctx* ctx, double* G, int n, double* R, double* dinv, double* Xi, int* status) {
    hipLaunchKernelGGL(k_chol_factor_mfma, dim3(1), dim3(1024), 0, ctx->stream, G, n, R, dinv, Xi, status);
}
static void launch_trsm_rows(srx_ctx* ctx, const double* src, const double* R, const double* dinv, int k, double* W, double* z0,
                             double* z1, double* z2) {
    hipLaunchKernelGGL(k_trsm_rows, dim3((k + 63) / 64), dim3(64), 0, ctx->stream, src, R, dinv, k, W, z0, z1, z2);
}
static void launch_trsm_mfma(srx_ctx* ctx, const double* src, const double* R, const double* Xi, int k, double* W, double* z0,
                             double* z1, double* z2) {
    hipLaunchKernelGGL(k_trsm_mfma, dim3((k + 16 * kTrsmTiles - 1) / (16 * kTrsmTiles)), dim3(kTrsmTiles * 64), 0, ctx->stream, src,
                       R, Xi, k, W, z0, z1, z2);
}
static void launch_jacobi(srx_ctx* ctx, double* H, int n, double* U, double* theta, int* status, double off_tol2, int n_want) {
    hipLaunchKernelGGL(k_jacobi_eig2, dim3(1), dim3(kJ2Threads), sizeof(J2Lds), ctx->stream, H, n, U, theta, status, off_tol2, n_want);
}
static void launch_ritz_post(srx_ctx* ctx, const double* W, double* Wp, const double* U, const double* theta, int k, double* A1,
                             double* A2, double* part, int zero_wp) {
    hipLaunchKernelGGL(k_ritz_post, dim3(kRitzBlocks), dim3(256), 0, ctx->stream, W, Wp, U, theta, k, A1, A2, part, zero_wp);
}
static void launch_resid_final(srx_ctx* ctx, const double* part, const double* theta, int n_pc, int l_act, const int* status,
                               const int* status_sel, double* rho, double* colmax, double* out) {
    hipLaunchKernelGGL(k_resid_final, dim3(1), dim3(1024), 0, ctx->stream, part, kRitzBlocks, theta, n_pc, l_act, status, status_sel,
                       rho, colmax, out);
}
static unsigned cheb_grid_of(size_t kl) { return (unsigned)((kl + 255) / 256); }
static void launch_cheb_first(srx_ctx* ctx, double* A1, const double* A2, const double* theta, int l_act, size_t kl) {
    hipLaunchKernelGGL(k_cheb_first, dim3(cheb_grid_of(kl)), dim3(256), 0, ctx->stream, A1, A2, theta, l_act, kl);
}
static void launch_cheb_first2(srx_ctx* ctx, double* Z, const double* W, double* cur, double* prev, const double* theta, int l_act,
                               size_t kl) {
    hipLaunchKernelGGL(k_cheb_first2, dim3(cheb_grid_of(kl)), dim3(256), 0, ctx->stream, Z, W, cur, prev, theta, l_act, kl);
}
static void launch_cheb_step(srx_ctx* ctx, double* Z, const double* cur, double* prev, const double* theta, int l_act, size_t kl) {
    hipLaunchKernelGGL(k_cheb_step, dim3(cheb_grid_of(kl)), dim3(256), 0, ctx->stream, Z, cur, prev, theta, l_act, kl);
}
static void launch_cheb_scale(srx_ctx* ctx, double* Y, const double* theta, int l_act, int d, size_t kl) {
    hipLaunchKernelGGL(k_cheb_scale, dim3(cheb_grid_of(kl)), dim3(256), 0, ctx->stream, Y, theta, l_act, d, kl);
}

// Run `enqueue` (kernel launches / async memsets and copies on ctx->stream, no host synchronisation, no
// allocation) through a cached hipGraph: captured the first time a key is seen, one hipGraphLaunch afterwards.
// The key must name everything the launches depend on (shapes, schedule, device pointers).  Any failure of the
// graph machinery switches the context back to plain launches for good.
template <typename Fn>
static int32_t graphed(srx_ctx* ctx, bool enable, const std::string& key, Fn&& enqueue) {
    if (!enable || ctx->graphs_off) return enqueue();
    auto it = ctx->graphs.find(key);
    if (it == ctx->graphs.end()) {
        if (ctx->graphs.size() >= 32) {                     // stale keys (scratch regrown): start over
            for (auto& kv : ctx->graphs) (void)hipGraphExecDestroy(kv.second);
            ctx->graphs.clear();
        }
        if (hipStreamBeginCapture(ctx->stream, hipStreamCaptureModeRelaxed) != hipSuccess) {
            (void)hipGetLastError();
            ctx->graphs_off = true;
            return enqueue();
        }
        ctx->capturing = true;
        const int32_t rc = enqueue();
        ctx->capturing = false;
        hipGraph_t g = nullptr;
        const hipError_t e = hipStreamEndCapture(ctx->stream, &g);
        hipGraphExec_t ex = nullptr;
        if (rc == SRX_OK && e == hipSuccess && g && hipGraphInstantiate(&ex, g, nullptr, nullptr, 0) == hipSuccess) {
            (void)hipGraphDestroy(g);
            it = ctx->graphs.emplace(key, ex).first;
        } else {
            if (g) (void)hipGraphDestroy(g);
            (void)hipGetLastError();
            ctx->graphs_off = true;
            return rc != SRX_OK ? rc : enqueue();
        }
    }
    SRX_HIP(ctx, hipGraphLaunch(it->second, ctx->stream));
    return SRX_OK;
}

// The switches of a solve, read from the environment once.
struct SolveEnv {
    const bool trace = getenv("SRX_PCA_TRACE"), no_graph = getenv("SRX_NO_GRAPH"), robust = getenv("SRX_PCA_ROBUST");
};
struct IterResult {
    double resid = INFINITY;
    int iters = 0;                      // sweeps after the warm-up
    bool converged = false;
    bool bailed_first = false;          // left at the first Ritz step for its flat tail, the block and the queued first filter step intact
};

// Block subspace iteration with Rayleigh–Ritz on span(W); `op.apply(W, Wp, zeroed)` computes Wp = C W.  After run(), w.A2 = W U
// holds the Ritz vectors (k x 64, leading n_pc columns meaningful), theta their Ritz values, w.dColmax the largest-|.| entry
// of each Ritz vector.
// Every member but run(), collect() and trace_step() only ENQUEUES work: the l x l factorisations run on the device, and the
// one number the host needs per Rayleigh–Ritz step (the residual) comes back through a pinned slot and an event, read one step
// late so that the stream never drains.  run() is the host loop: collect, decide (pca_schedule.hpp), enqueue the named segment
// through `graphed`, read back.
// An operator that ACCUMULATES (the Gram solver) adds into a zeroed destination and leaves w.T free.  The applications of a
// sweep then rotate through three scratch blocks (Wp, A1, T), and the kernels that are the last to read a block leave it zeroed
// (the CholeskyQR's substitution: all three; the Ritz tail: Wp; the filter step: its Z) — the eight memset launches a solve
// used to queue in front of its applications are gone (~40 us of a 1 ms iteration).  INVARIANTS: after `orth` Wp, A1 and T
// are zero; after a Ritz step Wp and T are zero, A1 = (C W) U, A2 = W U.
template <typename Op>
struct Iteration {
    static constexpr int kSlots = srx_ctx::kAsyncSlots, kSlotDoubles = 8;
    // the status words and, behind them, the ONE 64 x 64 matrix the partial products of a block pair are summed into (k_gram1_part:
    // global f64 atomics; its single consumer — the Cholesky factorisation or the eigen-solve — reads it once and leaves it zeroed;
    // the memset that clears the status words at the start of a solve clears it too)
    static constexpr size_t kStatusBytes = 256, kStatusAndH1 = kStatusBytes + (size_t)L * L * sizeof(double);
    static constexpr bool acc = Op::accumulates;
    srx_ctx* const ctx;
    const Work& w;
    const int k, l_act;
    const Resolved& o;                 // the round's options
    Op& op;
    const int* const d_status_sel;
    const SolveEnv& env;
    const size_t kl = (size_t)k * L;
    const bool use_graph = Op::graphable && !env.no_graph;
    int* d_status = nullptr;
    double *d_h1 = nullptr, *d_res = nullptr, *d_ritz = nullptr;
    std::string key_base;              // what a captured segment depends on besides its own schedule: shapes, options, every buffer it touches
    double spread = 1.0;               // theta_1 / theta_l of the last collected Ritz step

    int32_t prepare() {
        if (!ctx->pin_async) {
            SRX_HIP(ctx, hipHostMalloc((void**)&ctx->pin_async, kSlots * kSlotDoubles * sizeof(double), hipHostMallocDefault));
            for (auto& e : ctx->async_ev) SRX_HIP(ctx, hipEventCreateWithFlags(&e, hipEventDisableTiming));
        }
        SRX_TRY(scratch(ctx, "pca_status", kStatusAndH1, (void**)&d_status));
        d_h1 = reinterpret_cast<double*>(reinterpret_cast<char*>(d_status) + kStatusBytes);
        SRX_TRY(scratch(ctx, "pca_res", kSlots * kSlotDoubles * sizeof(double), (void**)&d_res));
        SRX_TRY(scratch(ctx, "pca_ritzpart", (size_t)kRitzBlocks * 3 * L * sizeof(double), (void**)&d_ritz));
        SRX_TRY(attr_jacobi(ctx));
        char key0[320];
        snprintf(key0, sizeof key0, "k%d l%d p%d w%d r%d n%d s%llu t%a|%p %p %p %p %p %p %p %p %p %p", k, l_act, o.power, o.warm,
                 (o.robust ? 1 : 0) + (o.direct ? 2 : 0) + (acc ? 4 : 0), o.n_pc,
                 (unsigned long long)o.seed, o.tol, op.key(), (void*)w.W, (void*)w.Wp, (void*)w.A1, (void*)w.A2, (void*)w.small,
                 (void*)w.gpart, (void*)d_status, (void*)d_status_sel, (void*)w.T);       // (d_ritz, d_res: allocated with d_status, never regrown)
        key_base = key0;
        return SRX_OK;
    }
    template <typename Fn>
    int32_t segment(const char* name, Fn&& enqueue) { return graphed(ctx, use_graph, key_base + name, enqueue); }

    // orthonormalise src -> W  (CholeskyQR: G = src^T src = R^T R, W = src R^-1; src == W is fine: every
    // thread of the substitution owns one row); the substitution leaves an accumulating operator's three blocks zeroed
    // (the matrix-free solver's apply overwrites its destination and uses T itself)
    int32_t orth(const double* src) {
        double *const zWp = acc ? w.Wp : nullptr, *const zA1 = acc ? w.A1 : nullptr, *const zT = acc ? w.T : nullptr;
        if (!o.robust) {
            launch_gram1(ctx, src, src, k, d_h1);           // src^T src summed into d_h1 (zero between uses)
            launch_chol_mfma(ctx, d_h1, l_act, w.dM, w.dDinv, w.dXi, d_status);
            launch_trsm_mfma(ctx, src, w.dM, w.dXi, k, w.W, zWp, zA1, zT);
        } else {                                // shifted CholeskyQR, G in dHG + L*L, and a second pass: the first one may have run on a shifted Gram matrix
            SRX_TRY(gram2(ctx, w, src, src, k));
            launch_chol(ctx, w.dHG + L * L, l_act, w.dM, w.dDinv, d_status, 1);
            launch_trsm_rows(ctx, src, w.dM, w.dDinv, k, w.W, zWp, zA1, zT);
            SRX_HIP(ctx, hipGetLastError());
            SRX_TRY(gram2(ctx, w, w.W, w.W, k));
            launch_chol(ctx, w.dHG + L * L, l_act, w.dM, w.dDinv, d_status, 1);
            launch_trsm_rows(ctx, w.W, w.dM, w.dDinv, k, w.W, nullptr, nullptr, nullptr);
        }
        SRX_HIP(ctx, hipGetLastError());
        return SRX_OK;
    }
    // `n` applications of C starting from `src`, ping-ponging between Wp and A1 (no copies); returns where
    // the result is
    // (`after_orth`: Wp, A1 and T are zero; otherwise — after a Ritz step — Wp and T are)
    int32_t apply_n(const double* src, int n, bool after_orth, const double** out) {
        const double* cur = src;
        double* const cand[3] = {w.Wp, w.A1, acc ? w.T : nullptr};
        bool zero[3] = {acc, acc && after_orth, acc};
        for (int t = 0; t < n; ++t) {
            int pick = -1;
            for (int c = 0; c < 3 && pick < 0; ++c)
                if (cand[c] && cand[c] != cur && zero[c]) pick = c;
            for (int c = 0; c < 3 && pick < 0; ++c)
                if (cand[c] && cand[c] != cur) pick = c;
            SRX_TRY(op.apply(cur, cand[pick], zero[pick]));
            zero[pick] = false;
            cur = cand[pick];
        }
        *out = cur;
        return SRX_OK;
    }
    // one Rayleigh–Ritz step on span(W): Wp = C W, H = W^T Wp = U diag(theta) U^T, Ritz vectors
    // A2 = W U, residuals || C v_i - theta_i v_i || in f64; slot <- (residual, status)
    // `loose`: the step after the warm-up.  Its residuals are O(1e-2) whatever the eigen-solver does (it only feeds the
    // filter's bounds and the rotated start), and the tail of the 64-column block holds clustered Ritz values that cost
    // the cyclic Jacobi two slow sweeps: it may stop at an off-diagonal norm of 1e-5 of the diagonal (7 -> 5 sweeps).  The
    // residuals are measured on the vectors actually formed, so a loosely rotated basis is judged as what it is: at the
    // default tolerances (1e-7 / 1e-9) such a step is never accepted as converged — the next, exact one decides.
    int32_t ritz_kernels(int slot, bool loose = false, bool wp_zero = false) {
        SRX_TRY(op.apply(w.W, w.Wp, wp_zero || acc));          // (Gram solver: Wp is zero after every CholeskyQR / filter step)
        // H = W^T (C W) as partial sums -> eigen-solve (adds them on load) -> Ritz vectors, C x Ritz vectors, residual and
        // largest-entry partials in one pass -> the step's scalars: 4 launches (9 on the old route)
        launch_gram1(ctx, w.W, w.Wp, k, d_h1);
        launch_jacobi(ctx, d_h1, l_act, w.dM2, w.dTheta, d_status, jacobi_tol2(loose, o.tol), wanted_pairs(o.direct, l_act, o.n_pc));
        launch_ritz_post(ctx, w.W, w.Wp, w.dM2, w.dTheta, k, w.A1, w.A2, d_ritz, acc ? 1 : 0);
        return resid_final(slot);
    }
    int32_t resid_final(int slot) {             // the step's scalars for this round's n_pc
        launch_resid_final(ctx, d_ritz, w.dTheta, o.n_pc, l_act, d_status, d_status_sel, w.dRho, w.dColmax, d_res + kSlotDoubles * slot);
        SRX_HIP(ctx, hipGetLastError());
        return SRX_OK;
    }
    // the read-back of a Ritz step (pinned slot + event): always a plain stream operation, never captured
    int32_t ritz_readback(int slot) {
        SRX_HIP(ctx, hipMemcpyAsync(ctx->pin_async + kSlotDoubles * slot, d_res + kSlotDoubles * slot,
                                    kSlotDoubles * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
        SRX_HIP(ctx, hipEventRecord(ctx->async_ev[slot], ctx->stream));
        return SRX_OK;
    }
    int32_t collect(int slot, double& r, double& ratio) {
        SRX_HIP(ctx, hipEventSynchronize(ctx->async_ev[slot]));
        const double* const pin = ctx->pin_async + kSlotDoubles * slot;
        r = pin[0];
        const int st = (int)pin[1];
        ratio = pin[2];
        spread = pin[4];
        if ((int)pin[3] & 1) return fail(ctx, SRX_E_NAN, "%s", kNanVarianceMsg);
        if (st & kStatChol) return fail(ctx, SRX_E_NOCONV, "pca: block lost rank (Cholesky pivot <= 0)");
        if (st & kStatEig) return fail(ctx, SRX_E_NOCONV, "pca: l x l eigen-solver did not converge");
        if (r != r) return fail(ctx, SRX_E_NOCONV, "pca: NaN in the Ritz residual");
        return SRX_OK;
    }
    void trace_step(int sweep, int n_ritz, int slot, double r, double ratio) {
        const int n_jacobi = (int)ctx->pin_async[kSlotDoubles * slot + 5];
        fprintf(stderr, "[srx pca] sweep %d (ritz step %d): residual %.3e, theta_l/theta_npc %.3e, %d Jacobi sweeps\n", sweep, n_ritz, r,
                ratio, n_jacobi);
        // the eigen-solve's off-diagonal norm (wanted pairs) over the diagonal's at every sweep's measurement (a drain: trace only)
        int st[64];
        if (d2h(ctx, st, d_status, sizeof st) != SRX_OK) return;
        fprintf(stderr, "[srx pca]   Jacobi off / diag per sweep:");
        for (int q = 0; q <= n_jacobi && q < 32; ++q) {
            float f;
            memcpy(&f, &st[16 + q], 4);
            fprintf(stderr, " %.2e", (double)f);
        }
        fprintf(stderr, "\n");
    }
    // the extra applications of C between two Rayleigh–Ritz steps (cheap dense products only; the
    // block stays well conditioned: kappa ~ (theta_1/theta_l)^power) and the next CholeskyQR
    int32_t advance() {
        // continue from the ROTATED block A1 = (C W) U (same span): its columns are close to eigenvectors,
        // so the next projected matrix is close to diagonal and its Jacobi solve takes 2-3 sweeps, not 8
        const double* res;
        SRX_TRY(apply_n(w.A1, o.power - 1, false, &res));
        return orth(res);
    }
    // one sweep WITHOUT a Rayleigh–Ritz step: `power` applications of C, then CholeskyQR
    int32_t plain_sweep() {
        const double* res;
        SRX_TRY(apply_n(w.W, o.power, true, &res));
        return orth(res);
    }
    // segment "start": random block, CholeskyQR2, warm-up sweeps (the first Ritz residuals are O(1) whatever
    // happens — no Rayleigh–Ritz step to learn that), first Ritz step
    int32_t seg_start() {
        if (o.direct) {                    // W = I (k x k, k = l_act): H = C itself, Ritz pairs = eigenpairs whatever the rank
            SRX_HIP(ctx, hipMemsetAsync(d_status, 0, kStatusAndH1, ctx->stream));
            hipLaunchKernelGGL(k_identity_block, dim3((unsigned)((kl + 255) / 256)), dim3(256), 0, ctx->stream, k, w.W);
            SRX_HIP(ctx, hipGetLastError());
            if (acc) SRX_HIP(ctx, hipMemsetAsync(w.Wp, 0, kl * 8, ctx->stream));      // (no start block, no CholeskyQR: nothing has zeroed it)
            return ritz_kernels(0, false);
        }
        // With a warm-up sweep the random block goes straight into C^power: the CholeskyQR that ends the sweep is the first
        // orthonormalisation the block needs (the conditioning of C^power W is that of the operator's spectrum whether or not
        // the Gaussian W — kappa ~ 1.4 at k = 2000, l = 64 — was orthonormalised first).  Without one (matrix-free solver,
        // robust mode) the Rayleigh-Ritz step needs an orthonormal block: CholeskyQR2 on the random start.
        const bool start_orth = o.robust || o.warm < 1;
        // (Gram solver: the start block goes into W and the three scratch blocks start zeroed; with start_orth the block goes
        //  into Wp, and the CholeskyQR that follows leaves the three zeroed)
        // (the status words and the 64 x 64 projected matrix behind them start from zero: the start block's kernel does it)
        hipLaunchKernelGGL(k_init_block, dim3((unsigned)((kl + 255) / 256)), dim3(256), 0, ctx->stream, o.seed, k, l_act,
                           start_orth ? w.Wp : w.W, acc && !start_orth ? w.Wp : (double*)nullptr,
                           acc ? w.A1 : (double*)nullptr, acc ? w.T : (double*)nullptr, reinterpret_cast<uint32_t*>(d_status),
                           (int)(kStatusAndH1 / 4));
        if (start_orth) {
            SRX_TRY(orth(w.Wp));
            SRX_TRY(orth(w.W));
        }
        for (int sweep = 0; sweep < o.warm; ++sweep) SRX_TRY(plain_sweep());
        return ritz_kernels(0, true);
    }
    // Chebyshev filter after the first Ritz step (Gram solver: w.T is free and `apply` has no collective).
    // Speculative part: Y1 and Z = C Y1 (needed whatever the degree turns out to be, d >= 2).
    int32_t cheb_spec() {
        launch_cheb_first(ctx, w.A1, w.A2, w.dTheta, l_act, kl);
        SRX_HIP(ctx, hipGetLastError());
        return op.apply(w.A1, w.Wp, acc);          // (Gram solver: the Ritz tail left Wp zeroed)
    }
    // the rest of a degree-d filter (Z = C Y1 is in Wp, cur = A1, prev = A2) and the CholeskyQR behind it
    int32_t cheb_filter(int d) {
        double *cur = w.A1, *prev = w.A2;
        for (int j = 1; j < d; ++j) {
            if (j > 1) SRX_TRY(op.apply(cur, w.Wp, true));          // (the step before left Wp zeroed)
            launch_cheb_step(ctx, w.Wp, cur, prev, w.dTheta, l_act, kl);
            std::swap(cur, prev);
        }
        launch_cheb_scale(ctx, cur, w.dTheta, l_act, d, kl);
        SRX_HIP(ctx, hipGetLastError());
        return orth(cur);
    }
    // ... then, where ONE filter of the degree the block can take will not reach the tolerance anyway (flat tails: theta_l / theta_npc
    // = 0.97 gains 10x per degree-10 filter), a SECOND filter straight behind the CholeskyQR — C W, Y1 = a C W - W, C Y1, the
    // recurrence, the CholeskyQR — and only then the Ritz step: the projected Gram product, the eigen-solve, the Ritz tail and a
    // host decision less per pair of filters.  The bounds and the column scales are the last Ritz step's (the block still is that
    // step's Ritz vectors, filtered and re-orthonormalised); the CholeskyQR between the two takes the leading directions out of
    // the guard columns as a Ritz step would.
    int32_t cheb_rest(int d, int d2, int slot) {
        SRX_TRY(cheb_filter(d));
        if (d2 > 0) {
            SRX_TRY(op.apply(w.W, w.Wp, acc));                // (Gram solver: the CholeskyQR left Wp, A1, T zeroed)
            launch_cheb_first2(ctx, w.Wp, w.W, w.A1, w.A2, w.dTheta, l_act, kl);
            SRX_HIP(ctx, hipGetLastError());
            SRX_TRY(op.apply(w.A1, w.Wp, true));
            SRX_TRY(cheb_filter(d2));
        }
        return ritz_kernels(slot, false, true);          // (Wp: zeroed by the last filter step, untouched by the CholeskyQR)
    }
    // segment "next": [advance] + (m - 1) plain sweeps + a Ritz step into `slot`
    int32_t seg_next(bool with_advance, int m, int slot) {
        if (with_advance) SRX_TRY(advance());
        for (int sI = 1; sI < m; ++sI) SRX_TRY(plain_sweep());
        return ritz_kernels(slot);
    }

    // `resume`: the block is the one a one-round plan just left at its FIRST Ritz step (flat tail: bailed_first), with the
    // speculative first filter step already queued behind it — W, A2 = Ritz vectors, theta, A1 = Y1, Wp = C Y1, the Ritz tail's
    // partial sums: everything this round's own start segment (start block, warm-up sweeps, first Ritz step: ~0.45 ms at k =
    // 1000) would recompute, for the same 64-column block.  Only the step's scalars are re-made for this round's n_pc.
    int32_t run(bool resume, IterResult& res) {
        const bool cheb = l_act > o.n_pc && !o.robust && !o.direct;      // both solvers: the filter only needs `apply`
        res = IterResult{};
        int n_ritz = 0, slot = 0;
        int q_applied = o.warm * o.power + 1;          // applications of C the block has seen (warm-up + first Ritz step)
        double r_last = INFINITY, rate_meas = 0.0;
        int sweeps_since = 0;
        if (resume) SRX_TRY(resid_final(slot));
        else SRX_TRY(segment("|start", [&] { return seg_start(); }));
        SRX_TRY(ritz_readback(slot));
        for (;;) {
            ++res.iters;
            const bool first = ++n_ritz == 1;
            if (cheb && first) {
                if (!resume) SRX_TRY(segment("|cheb0", [&] { return cheb_spec(); }));   // speculative: Y1, C Y1 (resume: already there)
            } else if (first && !o.direct) SRX_TRY(segment("|adv", [&] { return advance(); }));   // speculative: completes this sweep
            double r, ratio;
            SRX_TRY(collect(slot, r, ratio));
            res.resid = r;
            if (env.trace) trace_step(res.iters + o.warm, n_ritz, slot, r, ratio);
            if (r <= o.tol) {
                res.converged = true;
                break;
            }
            if (res.iters >= o.max_iter) break;
            if (step_bails(first, o.bail_ratio, ratio)) {
                if (env.trace) fprintf(stderr, "[srx pca] flat tail (theta_l / theta_npc = %.3f): leaving the round to the safe plan\n", ratio);
                res.bailed_first = cheb;           // (the block and the queued first filter step are the next plan's to continue from)
                break;                             // converged stays false
            }
            char kn[64];
            if (cheb) {
                const ChebDegrees c = cheb_degrees(r, o.tol, ratio, spread, q_applied);
                count_filter(c.d, c.d2, o.power, q_applied, res.iters);
                slot = (slot + 1) % kSlots;
                snprintf(kn, sizeof kn, "|cheb f%d d%d e%d s%d", first ? 1 : 0, c.d, c.d2, slot);
                SRX_TRY(segment(kn, [&]() -> int32_t {
                    if (!first) SRX_TRY(cheb_spec());      // later rounds: nothing was queued speculatively
                    return cheb_rest(c.d, c.d2, slot);
                }));
                SRX_TRY(ritz_readback(slot));
                if (env.trace && c.d2)
                    fprintf(stderr, "[srx pca] Chebyshev filters of degree %d and %d, a CholeskyQR between them (t_a = %.3f)\n", c.d, c.d2, c.ta);
                else if (env.trace) fprintf(stderr, "[srx pca] Chebyshev filter of degree %d (t_a = %.3f)\n", c.d, c.ta);
                r_last = INFINITY;                 // the filter's gain says nothing about the rate of plain sweeps
                sweeps_since = 0;
                continue;
            }
            if (const double rm = measured_rate(r, r_last, sweeps_since); rm >= 0.0) rate_meas = rm;
            const int m = plain_sweeps(r, o.tol, ratio, o.power, rate_meas, res.iters, o.max_iter);
            res.iters += m - 1;
            slot = (slot + 1) % kSlots;
            const bool with_adv = !first;          // the first step's half-sweep was queued speculatively
            snprintf(kn, sizeof kn, "|next a%d m%d s%d", with_adv ? 1 : 0, m, slot);
            SRX_TRY(segment(kn, [&] { return seg_next(with_adv, m, slot); }));
            SRX_TRY(ritz_readback(slot));
            r_last = r;
            sweeps_since = m;
        }
        return SRX_OK;
    }
};

// M (64 x 64, row-major) <- diag(s) M: row r scaled by s[r]
__global__ void k_scale_rows(double* __restrict__ M, const double* __restrict__ s) {
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e < L * L) M[e] *= s[e / L];
}
__global__ void k_sub_inplace(double* __restrict__ a, const double* __restrict__ b, size_t n) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) a[i] -= b[i];
}
// columns [at, at + n) of the locked block <- the leading n Ritz vectors / values of a finished round
__global__ void k_lock_columns(double* __restrict__ Vl, double* __restrict__ thl, const double* __restrict__ V,
                               const double* __restrict__ theta, int k, int at, int n) {
    const size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= (size_t)k * n) return;
    const int i = (int)(e / n), c = (int)(e % n);
    Vl[(size_t)i * L + at + c] = V[(size_t)i * L + c];
    if (i == 0) thl[at + c] = theta[c];
}

// C -= V diag(theta) V^T over the first n columns of V (k x 64): the resolved eigenpairs leave the operator.
// theta_c * (v_ic * v_jc) is symmetric in (i, j) to the last bit, so C stays exactly symmetric.
__global__ void k_deflate(double* __restrict__ C, int k, const double* __restrict__ V, const double* __restrict__ theta, int n) {
    const uint64_t e = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= (uint64_t)k * k) return;
    const int i = (int)(e / k), j = (int)(e % k);
    const double* vi = V + (size_t)i * L;
    const double* vj = V + (size_t)j * L;
    double s = 0.0;
    for (int c = 0; c < n; ++c) s += theta[c] * (vi[c] * vj[c]);
    C[e] -= s;
}

// Size of a matrix's result allocation: the N x n_pc f64 scores followed by the block of small results
// (PcaResultLayout) for the most rounds either plan can take.
// Row stride (in doubles) of the score matrix IN HBM: n_pc rounded up to a whole number of 128-byte pieces (16 doubles), so
// that the 16-column piece a panel-slice workgroup of the forward SpMM writes for a cell is its own two aligned 64-byte lines
// — with the reference's N x n_pc layout (400-byte rows at n_pc = 50) every piece straddled lines shared with another
// slice's workgroup.  srx_result_fetch hands out the dense N x n_pc matrix (obsm["X_pca"], dim_red/mod.rs:105-106) whatever
// the stride in HBM is.
int scores_ld(int n_pc) {
    return (n_pc + 15) / 16 * 16;            // (c3, n_pc = 50: the forward SpMM 0.640 -> 0.616 ms against the dense layout)
}
void result_layout(uint64_t n_rows, int k, int n_pc, int dim, size_t& score_bytes, size_t& small_doubles, PcaPlans* plans_out) {
    const PcaPlans plans = pca_plans(dim, n_pc, L);
    score_bytes = (n_rows ? n_rows : 1) * (size_t)scores_ld(n_pc) * 8;
    small_doubles = PcaResultLayout(k, L, plans.max_rounds()).total_doubles();
    if (plans_out) *plans_out = plans;
}
int32_t ensure_result_capacity(srx_ctx* ctx, srx_pca_state& st, size_t need) {
    if (st.scores_cap < need) {
        if (st.d_scores) SRX_HIP(ctx, hipFree(st.d_scores));
        st.d_scores = nullptr;
        st.scores_cap = 0;
        SRX_HIP(ctx, hipMalloc((void**)&st.d_scores, need));
        st.scores_cap = need;
    }
    return SRX_OK;
}

// ---- the operator C of the iteration ------------------------------------------------------------------
// reset() restores the undeflated operator, apply(Win, Wout, out_zeroed) enqueues Wout = C Win, deflate(n_r) removes the
// eigenpairs a round has resolved (w.A2 / w.dTheta, leading n_r columns); key() names the operator in the graph cache.

// explicit Gram: G = A^T A once (all-reduced, the packed triangle Pk), C = D (G - c N mu mu^T) D dense
struct GramOperator {
    static constexpr bool graphable = true;
    static constexpr bool accumulates = true;       // the dense application accumulates into a zeroed block; w.T is free
    srx_ctx* ctx;
    const Work& w;                                  // (w.d, w.mu: the scaling and centring vectors)
    int k, center;
    double n_cells;
    const double* Pk;
    double* C;
    const void* key() const { return C; }
    int32_t reset() {
        hipLaunchKernelGGL(k_gram_expand, dim3((unsigned)(((size_t)k * k + 255) / 256)), dim3(256), 0, ctx->stream, Pk,
                           k, (const double*)w.d, (const double*)w.mu, center, n_cells, C);
        SRX_HIP(ctx, hipGetLastError());
        return SRX_OK;
    }
    int32_t apply(const double* Win, double* Wout, bool out_zeroed) {
        ProfScope ps(ctx, SRX_K_DENSE, (double)k * k * 8.0 + 2.0 * k * L * 8.0);
        if (!out_zeroed) SRX_HIP(ctx, hipMemsetAsync(Wout, 0, (size_t)k * L * 8, ctx->stream));
        launch_dense_apply(ctx, C, Win, k, Wout);
        SRX_HIP(ctx, hipGetLastError());
        return SRX_OK;
    }
    int32_t deflate(int n_r) {                      // C -= V diag(theta) V^T
        hipLaunchKernelGGL(k_deflate, dim3((unsigned)(((size_t)k * k + 255) / 256)), dim3(256), 0, ctx->stream, C, k,
                           (const double*)w.A2, (const double*)w.dTheta, n_r);
        SRX_HIP(ctx, hipGetLastError());
        return SRX_OK;
    }
};

// matrix-free: Z^T (Z W) by a forward and a transposed SpMM; resolved eigenpairs are deflated IMPLICITLY,
// W' -= V_lock (theta_lock * (V_lock^T W)) with the locked vectors in a k x 64 block (plan B locks <= 48)
template <typename VT, typename PT>
struct MatrixFreeOperator {
    static constexpr bool graphable = false;        // (the exchange of apply is a collective)
    static constexpr bool accumulates = false;      // apply overwrites its destination and uses w.T itself
    srx_ctx* ctx;
    const Work& w;
    int k, center;
    const Tiled& t256;
    const RowMajor& rows;
    PT *P, *cvec, *Y;
    double *v_lock, *th_lock;
    int n_lock = 0;
    const void* key() const { return nullptr; }
    int32_t reset() {
        n_lock = 0;
        SRX_HIP(ctx, hipMemsetAsync(v_lock, 0, ((size_t)k * L + L) * 8, ctx->stream));
        return SRX_OK;
    }
    int32_t apply(const double* Win, double* Wout, bool) {
        const size_t kl = (size_t)k * L;
        hipLaunchKernelGGL((k_make_panel<PT>), dim3(1), dim3(1024), 0, ctx->stream, Win, w.d, w.mu,
                           (const double*)nullptr, k, center, P, cvec);
        SRX_HIP(ctx, hipGetLastError());
        // forward product: the row-major batch-stream kernel where its widest slice (8 f64 columns of all k genes: k <= 2559)
        // fits the LDS — 8 passes over the records, 1.48 against 2.45 ms per application at c3 for the tile-major kernel,
        // which reads the matrix once whatever k is and stays the route beyond (narrower slices mean 16+ passes)
        if (rows.pk && fwd_rows_q<PT>(k) >= 2)
            SRX_TRY((launch_fwd_rows<VT, PT>(ctx, rows, P, cvec, L, (double*)nullptr, Y, L)));
        else SRX_TRY((launch_fwd<VT, PT>(ctx, t256, P, cvec, Y)));
        SRX_TRY((launch_t<VT, PT>(ctx, t256, Y, w.T)));
        SRX_TRY(allreduce_f64(ctx, w.T, kl + L));             // the one exchange per iteration
        hipLaunchKernelGGL(k_finish_t, dim3((unsigned)((kl + 255) / 256)), dim3(256), 0, ctx->stream, w.T, w.d, w.mu,
                           k, center, Wout);
        SRX_HIP(ctx, hipGetLastError());
        if (n_lock > 0) {
            SRX_TRY(gram2(ctx, w, v_lock, Win, k));                               // dHG <- V_lock^T W (64 x 64)
            hipLaunchKernelGGL(k_scale_rows, dim3((L * L + 255) / 256), dim3(256), 0, ctx->stream, w.dHG, (const double*)th_lock);
            hipLaunchKernelGGL(k_right_mul, dim3(128), dim3(256), 0, ctx->stream, (const double*)v_lock, (const double*)w.dHG, k, w.T);
            hipLaunchKernelGGL(k_sub_inplace, dim3((unsigned)((kl + 255) / 256)), dim3(256), 0, ctx->stream, Wout, (const double*)w.T, kl);
            SRX_HIP(ctx, hipGetLastError());
        }
        return SRX_OK;
    }
    int32_t deflate(int n_r) {                      // the round's vectors join the locked block
        if (n_lock + n_r > L) return fail(ctx, SRX_E_ARG, "pca: more than %d locked vectors in the matrix-free solver", L);
        hipLaunchKernelGGL(k_lock_columns, dim3((unsigned)(((size_t)k * n_r + 255) / 256)), dim3(256), 0, ctx->stream, v_lock,
                           th_lock, (const double*)w.A2, (const double*)w.dTheta, k, n_lock, n_r);
        SRX_HIP(ctx, hipGetLastError());
        n_lock += n_r;
        return SRX_OK;
    }
};

// ---- the solver driver: DEFLATION ROUNDS.  A round resolves the next eigenpairs with the 64-column block, writes their scores,
// and removes them from the operator, so that the next round's dominant subspace is the one after them.
struct Solve {                              // what the rounds of a solve share, and its running result
    srx_ctx* ctx;
    const Work& w;
    int k, l_act, dim;                      // dim: dimension of the operator's range
    const Resolved& o;
    const int* d_status_sel;
    srx_pca_state& st;
    const SolveEnv env{};
    double resid = INFINITY;
    int iters = 0;
    bool converged = false;
    bool bailed_first = false;              // the last plan was left at its first Ritz step (flat tail) with its block intact
};

// Runs a plan of deflation rounds on the operator.  SRX_E_NOCONV (breakdown) or converged == false (budget spent) leave the
// decision to the caller.
template <typename Op, typename Finish>
static int32_t run_plan(Solve& s, Op& op, const Finish& finish_round, const std::vector<int>& plan, int budget, bool robust,
                        double bail = 0.0, bool resume = false) {
    if (!resume) SRX_TRY(op.reset());     // (resume: nothing was deflated, C is as expanded)
    s.st.round_counts = plan;             // the layout of the result block, for finish_round and every reader
    s.resid = 0.0;
    s.converged = true;
    s.iters = 0;
    int done = 0;
    const int rounds = (int)plan.size();
    for (int r = 0; r < rounds; ++r) {
        const Resolved o_r = round_options(s.o, plan[r], r, budget, bail, robust);
        const int l_r = round_width(rounds, s.l_act, L, s.dim, done);
        IterResult res;
        s.bailed_first = false;
        {
            ProfScope ps_it(s.ctx, SRX_K_ITERATE, (double)s.k * s.k * 8.0);
            Iteration<Op> it{s.ctx, s.w, s.k, l_r, o_r, op, s.d_status_sel, s.env};
            SRX_TRY(it.prepare());
            SRX_TRY(it.run(resume && r == 0 && l_r == s.l_act, res));
        }
        s.bailed_first = res.bailed_first;
        s.resid = std::max(s.resid, res.resid);
        s.iters += res.iters + s.o.warm;
        if (!res.converged) {
            s.converged = false;
            return SRX_OK;
        }
        SRX_TRY(finish_round(r, done, o_r.n_pc));
        if (r + 1 < rounds) SRX_TRY(op.deflate(o_r.n_pc));
        done += o_r.n_pc;
    }
    return SRX_OK;
}

// plan A, then plan B if it stalled or broke down, then robust mode (the policy: PcaPlans, pca_schedule.hpp)
template <typename Op, typename Finish>
static int32_t solve(Solve& s, Op& op, const Finish& finish_round, const PcaPlans& plans) {
    const Resolved& o = s.o;
    if (s.env.robust) {                                           // test switch: the last-resort mode from the start
        SRX_TRY(run_plan(s, op, finish_round, plans.safest(), o.max_iter, true));
        s.iters -= o.warm;
        return SRX_OK;
    }
    int32_t rc = run_plan(s, op, finish_round, plans.a, plans.budget_a(o.max_iter), false, plans.bail_a());
    if (plans.have_b() && (rc == SRX_E_NOCONV || (rc == SRX_OK && !s.converged))) {
        if (s.env.trace)
            fprintf(stderr, "[srx pca] plan A (%zu round(s)) %s at residual %.3e: rounds of <= %d components instead\n",
                    plans.a.size(), rc == SRX_OK ? "stalled" : "broke down", s.resid, plans.b[0]);
        const int spent = s.iters;
        // (left at the first Ritz step for its flat tail: the safe plan's first round continues from that block — the same 64
        //  columns, the same warm-up and Ritz step it would redo from a new random start)
        const bool resume = rc == SRX_OK && s.bailed_first && plans.a.size() == 1;
        rc = run_plan(s, op, finish_round, plans.b, o.max_iter, false, 0.0, resume);
        s.iters += resume ? 0 : spent;
    }
    if (rc == SRX_E_NOCONV) {
        // last resort: a block whose spectrum spans more than ~1e8 between two CholeskyQRs (small exact-rank
        // problems: k = 10 features of 6 cells have theta_1 / theta_5 ~ 1e3 and a sweep is three applications)
        if (s.env.trace) fprintf(stderr, "[srx pca] breakdown again: robust mode (CholeskyQR3 after every application)\n");
        const int spent = s.iters;
        rc = run_plan(s, op, finish_round, plans.safest(), o.max_iter, true);
        s.iters += spent;
    }
    SRX_TRY(rc);
    s.iters -= o.warm;                                            // st.info adds it back once
    return SRX_OK;
}

// The solve of one matrix at the precisions <VT, PT> of its records and panels: work blocks, plans and the result allocation,
// the operator of o.solver, the plans' rounds, st.info.
template <typename VT, typename PT>
static int32_t run_pca(srx_ctx* ctx, const RowMajor* parts, int n_parts, const Tiled* t256p, double* gram_packed,
                       const Resolved& o, const SelDev& sel, int l_act, double n_cells, srx_pca_state& st, const DenseSource* dense) {
    const RowMajor* rmp = n_parts == 1 ? &parts[0] : nullptr;
    const int k = dense ? dense->k : parts[0].k;
    struct { uint64_t n_rows, max_rows; } cc{dense ? dense->n_rows : 0, 0};
    for (int i = 0; i < n_parts; ++i) {
        cc.n_rows += parts[i].n_rows;
        cc.max_rows = std::max(cc.max_rows, parts[i].n_rows);
    }
    const size_t kl = (size_t)k * L;
    Work w;
    st.d_small = nullptr;
    SRX_TRY(alloc_work(ctx, k, w));
    // the centring / scaling vectors of the selection are read in place (they are only ever read; two device copies per step
    // were 9 us on the critical path)
    if (o.center) w.mu = sel.d_mu;
    else SRX_HIP(ctx, hipMemsetAsync(w.mu, 0, (size_t)k * 8, ctx->stream));
    w.d = sel.d_dinv;
    PT *P, *cvec, *Y;
    SRX_TRY(scratch(ctx, "pca_P", (kl + L) * sizeof(PT), (void**)&P));
    cvec = P + kl;
    SRX_TRY(scratch(ctx, "pca_Y", (cc.max_rows ? cc.max_rows : 1) * (size_t)L * sizeof(PT), (void**)&Y));

    // dimension of the operator's range: min(k, N - 1) (N when not centred); a block as wide as that is exact
    const int dim = o.direct ? k : (int)std::min<double>((double)k, n_cells - (o.center ? 1.0 : 0.0));
    PcaPlans plans;
    size_t score_bytes, small_doubles;
    result_layout(cc.n_rows, k, o.n_pc, dim, score_bytes, small_doubles, &plans);
    // one allocation: the scores, then the block of small results (srx_matrix_reserve_results makes it ahead of time)
    SRX_TRY(ensure_result_capacity(ctx, st, score_bytes + small_doubles * 8));
    double* const d_small = st.d_scores + score_bytes / 8;
    // The end of round r, which resolved components [col0, col0 + n_r).  A2 = W U are the Ritz vectors (ascending-gene row order);
    // sign: largest-|.| entry positive.  scores = Z V (transform, pca/mod.rs:156-185): one forward SpMM per row tile with the panel
    // D V, the f64 scores written by the SpMM itself.  The Ritz vectors, values and signs move out of the (per-context) scratch
    // into the matrix's own block; their host copies are made by the first fetch (pca_materialize).
    const auto finish_round = [&](int r, int col0, int n_r) -> int32_t {
        // signs, panel, centring partials and the copy of (Ritz vectors, values, signs) into the result block: one pass
        const PcaResultLayout lay(k, L, st.round_counts);
        hipLaunchKernelGGL((k_make_panel_mb<PT>), dim3(kPanelBlocks), dim3(1024), 0, ctx->stream, (const double*)w.A2, (const double*)w.d,
                           (const double*)w.mu, (const double*)w.dColmax, (const double*)w.dTheta, k, P, w.gpart, w.dSgn, d_small + lay.V(r),
                           d_small + lay.theta(r), d_small + lay.sgn(r));
        hipLaunchKernelGGL((k_cvec_reduce<PT>), dim3(1), dim3(L), 0, ctx->stream, (const double*)w.gpart, kPanelBlocks, o.center, cvec);
        SRX_HIP(ctx, hipGetLastError());
        // scores = Z V: the transform from the row-major records, one launch per row tile (the tile-major kernel — 1.22 ms
        // at c3 against 0.84 — when its view was made: the matrix-free solver)
        uint64_t row0 = 0;
        const int ld_s = scores_ld(o.n_pc);
        if (dense) {                            // the dense source writes its own scores from the panel
            if constexpr (std::is_same_v<PT, double>) SRX_TRY(dense->write_scores(P, cvec, col0, n_r, st.d_scores, ld_s));
            else return fail(ctx, SRX_E_ARG, "pca: a dense source is solved in f64");
        } else if (t256p) {
            SRX_TRY((launch_fwd<VT, PT>(ctx, *t256p, P, cvec, Y, st.d_scores + col0, n_r, ld_s)));
        } else {
            for (int i = 0; i < n_parts; ++i) {
                SRX_TRY((launch_fwd_rows<VT, PT>(ctx, parts[i], P, cvec, n_r, st.d_scores + row0 * (size_t)ld_s + col0, (PT*)nullptr, ld_s)));
                row0 += parts[i].n_rows;
            }
        }
        return SRX_OK;
    };
    Solve s{ctx, w, k, l_act, dim, o, sel.d_status, st};
    if (o.solver == 1) {
        double* C;
        SRX_TRY(scratch(ctx, "pca_C", (size_t)k * k * 8, (void**)&C));
        double* Pk = gram_packed;
        const size_t n_packed = gram_packed_count(k);
        if (!Pk) {
            Range r_("srx:gram");
            SRX_TRY(scratch(ctx, "pca_gpacked", n_packed * sizeof(double), (void**)&Pk));
            bool reduced = false;
            SRX_TRY(launch_gram<VT>(ctx, *rmp, Pk, &reduced, true));  // (a fresh sum: zeroed on the way; sharded rows: the exchange overlaps the second half)
            if (!reduced) SRX_TRY(allreduce_f64(ctx, Pk, n_packed));
        } else if (!dense) {
            SRX_TRY(allreduce_f64(ctx, Pk, n_packed));            // the one exchange of this solver: the packed upper triangle
        }
        GramOperator op{ctx, w, k, o.center, n_cells, Pk, C};
        Range r_("srx:iterate");
        SRX_TRY(attr_dense_apply(ctx));
        SRX_TRY(solve(s, op, finish_round, plans));
    } else {
        if (dense) return fail(ctx, SRX_E_ARG, "pca: a dense source needs the Gram solver");
        if (n_parts != 1 || !t256p) return fail(ctx, SRX_E_ARG, "pca: the SpMM solver needs the matrix resident in one piece");
        double* v_lock;
        SRX_TRY(scratch(ctx, "pca_lock", (kl + L) * 8, (void**)&v_lock));
        MatrixFreeOperator<VT, PT> op{ctx, w, k, o.center, *t256p, parts[0], P, cvec, Y, v_lock, v_lock + kl};
        SRX_TRY(solve(s, op, finish_round, plans));
    }
    st.d_small = d_small;
    st.info.n_iter = (uint32_t)(s.iters + o.warm);
    st.info.residual = s.resid;
    if (!s.converged)
        return fail(ctx, SRX_E_NOCONV, "pca: subspace iteration stopped at max_iter=%d with residual %.3e > tol %.3e",
                    o.max_iter, s.resid, o.tol);
    return SRX_OK;
}

// Defaults and limits of pca_inplace (dim_red/mod.rs:38-57) and of this solver.
int32_t resolve_opts(srx_ctx* ctx, const srx_pca_opts* opts, int k, uint64_t Ng, bool f32, Resolved& o, int& l_act) {
    // dim_red/mod.rs:38-41: column(0)/column(1) and slice(..5) panic when k < 2 or N < 5
    if (k < 2 || Ng < 5) return fail(ctx, SRX_E_SHAPE, "pca_inplace needs >= 2 selected features and >= 5 cells (k=%d, N=%llu)",
                                     k, (unsigned long long)Ng);
    int want = (!opts || opts->n_components < 0) ? 2 : opts->n_components;      // :52
    o.n_pc = std::min(want, k);
    o.center = (!opts || opts->center < 0) ? 1 : (opts->center != 0);           // :55
    o.scale = (!opts || opts->scale < 0) ? 1 : (opts->scale != 0);              // :56
    o.max_iter = (opts && opts->max_iter > 0) ? opts->max_iter : 0;          // default set below, once the solver is known
    o.tol = (opts && opts->tol > 0) ? opts->tol : 0.0;
    o.seed = opts ? opts->seed : 0;
    o.solver = opts ? opts->solver : 0;
    if (o.solver < 0 || o.solver > 2) return fail(ctx, SRX_E_ARG, "pca: solver must be 0 (auto), 1 (gram) or 2 (spmm)");
    // auto: the explicit Gram matrix as long as it fits (k <= 16384: 2 GB of f64).  At c2's size k = 6000 / 8000 cost
    // 13.6 / 20.5 ms per pipeline against 23.7 / 30 of the matrix-free iteration, and on a flat-tailed spectrum at
    // k = 9000 105 ms against 297 (round 6)
    if (o.solver == 0) o.solver = k <= 16384 ? 1 : 2;
    // a sweep is `power` applications of C: the same default budget of 600 applications for both solvers
    if (o.max_iter == 0) o.max_iter = o.solver == 1 ? 200 : 600;
    o.power = o.solver == 1 ? 3 : 1;
    o.warm = o.solver == 1 ? 2 : 0;
    // (Round 5, measured at c3 with the schedule overridden — warm-up sweeps x applications per sweep: 2 x 3 (this) 0.97 ms, residual
    //  1.0e-8; 1 x 6 0.90 ms, the same residuals to four digits — one CholeskyQR less, on a block of condition (theta_1 / theta_l)^6; 1 x 5
    //  0.88 ms, 4.9e-8; 1 x 4 and 2 x 2 need a third Ritz step, 1.2-1.3 ms.  The 0.07-0.1 ms are not worth a CholeskyQR on the sixth
    //  power of the spectrum's spread: kept at 2 x 3.  profiles/r05_knockouts.md)
    if (o.solver == 1 && k > 16384) return fail(ctx, SRX_E_ARG, "pca: the Gram solver holds a k x k f64 matrix; k=%d is too large", k);
    // default tolerance on the relative Ritz residual: what the arithmetic of the solver supports
    if (o.tol == 0.0) o.tol = f32 ? 1e-7 : 1e-9;
    if (o.n_pc < 1) return fail(ctx, SRX_E_ARG, "pca: n_components must be >= 1");
    if (opts && opts->block != 0 && opts->block != L) return fail(ctx, SRX_E_ARG, "pca: only block = %d is built", L);
    // Z has rank <= min(k, N - 1) (N when not centred): a block wider than that cannot stay independent under C
    const uint64_t rank_bound = std::min<uint64_t>((uint64_t)k, Ng - (o.center ? 1 : 0));
    if ((uint64_t)o.n_pc > rank_bound && !(k <= L && o.solver == 1))
        return fail(ctx, SRX_E_ARG, "pca: n_components %d exceeds the rank of the data (min(k, N%s) = %llu)", o.n_pc,
                    o.center ? " - 1" : "", (unsigned long long)rank_bound);
    l_act = (int)std::min<uint64_t>((uint64_t)L, rank_bound);
    // k <= 64 with the explicit matrix: the k x k matrix goes straight to the eigen-solver (exact for any rank)
    if (k <= L && o.solver == 1) {
        o.direct = true;
        l_act = k;
    }
    if (o.n_pc > l_act && o.solver != 1)
        return fail(ctx, SRX_E_ARG, "pca: n_components %d exceeds what the %d-column block resolves (max %d)", o.n_pc, L, l_act);
    // beyond L - 8 components the Gram solver runs deflation rounds on the explicit k x k matrix; the matrix-free
    // solver has nothing to deflate
    if (rank_bound > (uint64_t)L && o.n_pc > L - 8 && o.solver != 1)
        return fail(ctx, SRX_E_ARG, "pca: n_components %d > %d needs the Gram solver (k <= 16384, opts.solver = 1)", o.n_pc, L - 8);
    return SRX_OK;
}

// Everything the host side of the result needs stays on the device until the first fetch (pca_materialize).
static int32_t stash_results(srx_ctx* ctx, srx_pca_state& st, int k, int n_pc, const SelDev& sel) {
    st.k = (uint32_t)k;
    st.n_pc = (uint32_t)n_pc;
    const PcaResultLayout lay = result_block(st);
    double* const sm = st.d_small;
    CopySegs cs;                                           // (four runtime copies were 20 us of dispatches)
    cs.src[0] = (const uint32_t*)sel.d_mu;       cs.dst[0] = (uint32_t*)(sm + lay.mu());        cs.words[0] = (uint32_t)k * 2;
    cs.src[1] = (const uint32_t*)sel.d_sd;       cs.dst[1] = (uint32_t*)(sm + lay.sd());        cs.words[1] = (uint32_t)k * 2;
    cs.src[2] = (const uint32_t*)sel.d_trace;    cs.dst[2] = (uint32_t*)(sm + lay.trace());     cs.words[2] = 2;
    cs.src[3] = (const uint32_t*)sel.d_sel_rank; cs.dst[3] = (uint32_t*)(sm + lay.sel_rank());  cs.words[3] = (uint32_t)k;
    hipLaunchKernelGGL(k_copy_segs, dim3(16), dim3(256), 0, ctx->stream, cs);
    SRX_HIP(ctx, hipGetLastError());
    st.sel.clear();
    st.host_pending = true;
    st.valid = true;
    return SRX_OK;
}

int32_t solve_and_stash(srx_ctx* ctx, bool f32, const RowMajor* parts, int n_parts, const Tiled* t256p, double* gram_packed,
                        const Resolved& o, const SelDev& sel, int l_act, uint64_t n_cells, uint64_t nnz_selected, srx_pca_state& st,
                        const DenseSource* dense) {
    const int k = dense ? dense->k : parts[0].k;
    st.valid = false;
    st.residual = dense ? dense->route : kResidualNone;
    st.info = srx_pca_info{};
    st.info.n_cells_global = n_cells;
    st.info.k = (uint32_t)k;
    st.info.n_pc = (uint32_t)o.n_pc;
    st.info.block = L;
    st.info.nnz_selected = nnz_selected;
    st.info.solver = (uint32_t)o.solver;
    // f32 storage: f32 panels and products for the one transform of the Gram route; the matrix-free iteration runs its
    // panels in f64 (f32 products of Z W level the residuals of the small components off at ~1e-7 theta_1 / theta_i:
    // 6.6e-5 at k = 9000 on a flat-tailed matrix, however many sweeps)
    const auto run = !f32 ? run_pca<double, double> : o.solver == 2 ? run_pca<float, double> : run_pca<float, float>;
    const int32_t rc = run(ctx, parts, n_parts, t256p, gram_packed, o, sel, l_act, (double)n_cells, st, dense);
    if ((rc != SRX_OK && rc != SRX_E_NOCONV) || !st.d_small) return rc;      // d_small unset: the solve broke down early
    SRX_TRY(stash_results(ctx, st, k, o.n_pc, sel));
    return rc;
}

}  // namespace srx

using namespace srx;

extern "C" {

// Kernel-level entry point: Y = X[:, sel] * P, T = X[:, sel]^T * Y and G = X[:, sel]^T X[:, sel]
// for a caller-supplied 64-column panel (no centring / scaling).  Exists so the SpMM and Gram
// kernels can be checked against a CPU reference in isolation, and as the raw operators.
int32_t srx_spmm(srx_mat* m, const uint64_t* sel, uint64_t k64, const double* panel, double* y_out, double* t_out,
                 double* gram_out) {
    if (!m || !sel) return fail(m ? m->ctx : nullptr, SRX_E_ARG, "null argument");
    if ((y_out || t_out) && !panel) return fail(m->ctx, SRX_E_ARG, "srx_spmm: panel is required for y/t");
    if (m->csc) return fail(m->ctx, SRX_E_FORMAT, "srx_spmm walks cells: convert the CSC matrix with srx_matrix_to_csr");
    srx_ctx* ctx = m->ctx;
    SRX_HIP(ctx, hipSetDevice(ctx->device));
    const int k = (int)k64;
    for (int s = 1; s < k; ++s)
        if (sel[s] <= sel[s - 1]) return fail(ctx, SRX_E_ARG, "srx_spmm: sel must be strictly ascending");
    SelDev sd;                                     // (the bits alone: no moments, no vectors)
    SRX_TRY(select_list(m, sel, k64, 0, 0, sd, false));
    RowMajor crm;
    Tiled c256;
    SRX_TRY(compact_selection(m, sd.d_bits, sd.n_words, k, crm));
    SRX_TRY(retile(m, crm, c256));
    const size_t kl = (size_t)k * L;
    double* T;
    SRX_TRY(scratch(ctx, "pca_T", (kl + L) * 8, (void**)&T));
    auto run = [&](auto vt, auto pt) -> int32_t {
        using VT = decltype(vt);
        using PT = decltype(pt);
        if (y_out || t_out) {
            const Tiled& c = c256;
            PT *P, *Y;
            SRX_TRY(scratch(ctx, "pca_P", (kl + L) * sizeof(PT), (void**)&P));
            SRX_TRY(scratch(ctx, "pca_Y", (c.n_rows ? c.n_rows : 1) * (size_t)L * sizeof(PT), (void**)&Y));
            std::vector<PT> hp(kl + L, PT(0));
            for (size_t e = 0; e < kl; ++e) hp[e] = (PT)panel[e];
            SRX_TRY(h2d(ctx, P, hp.data(), (kl + L) * sizeof(PT)));
            // SRX_SPMM_ROWS=1 (kernel-level parity tests): the product from the row-major records — the kernel the transform
            // runs (k_spmm_rows) — instead of the tile-major view
            if (getenv("SRX_SPMM_ROWS") && atoi(getenv("SRX_SPMM_ROWS"))) {
                SRX_TRY((launch_fwd_rows<VT, PT>(ctx, crm, P, P + kl, L, (double*)nullptr, Y, L)));
            } else {
                SRX_TRY((launch_fwd<VT, PT>(ctx, c, P, P + kl, Y)));
            }
            if (y_out) {
                std::vector<PT> hy(c.n_rows * (size_t)L);
                SRX_TRY(d2h(ctx, hy.data(), Y, hy.size() * sizeof(PT)));
                for (size_t e = 0; e < hy.size(); ++e) y_out[e] = (double)hy[e];
            }
            if (t_out) {
                SRX_TRY((launch_t<VT, PT>(ctx, c, Y, T)));
                SRX_TRY(d2h(ctx, t_out, T, kl * 8));
            }
        }
        if (gram_out) {
            double *C, *Pk;
            SRX_TRY(scratch(ctx, "pca_C", (size_t)k * k * 8, (void**)&C));
            SRX_TRY(scratch(ctx, "pca_gpacked", gram_packed_count(k) * sizeof(double), (void**)&Pk));
            SRX_HIP(ctx, hipMemsetAsync(Pk, 0, gram_packed_count(k) * sizeof(double), ctx->stream));
            SRX_TRY(launch_gram<VT>(ctx, crm, Pk));
            hipLaunchKernelGGL(k_gram_expand, dim3((unsigned)(((size_t)k * k + 255) / 256)), dim3(256), 0, ctx->stream, Pk,
                               k, (const double*)nullptr, (const double*)nullptr, 0, 0.0, C);
            SRX_HIP(ctx, hipGetLastError());
            SRX_TRY(d2h(ctx, gram_out, C, (size_t)k * k * 8));
        }
        return SRX_OK;
    };
    return is_f32(m) ? run(float{}, float{}) : run(double{}, double{});
}

// Kernel-level entry point of the dense iteration (test and diagnostics: no stability promise): one operation of
// Iteration on host arrays, through the solver's own launch_* functions, in fresh device buffers of exactly the stated
// sizes (a k x 64 block: k + 8 rows, the last 8 a sentinel that must come back untouched).
namespace {
constexpr int kItTail = 8;
constexpr double kItSentinel = -7.25e77;
struct ItBufs {                                    // the device buffers of one call, freed when it returns
    std::vector<void*> p;
    ~ItBufs() {
        for (void* q : p) (void)hipFree(q);
    }
};
}  // namespace

static int32_t it_alloc(srx_ctx* ctx, ItBufs& bufs, size_t bytes, void** out) {
    SRX_HIP(ctx, hipMalloc(out, bytes));
    bufs.p.push_back(*out);
    return SRX_OK;
}
// a host array -> a fresh device buffer of `n` doubles (+ the sentinel rows of a k x 64 block)
static int32_t it_up(srx_ctx* ctx, ItBufs& bufs, const double* host, size_t n, bool block, double** dev) {
    const size_t tail = block ? (size_t)kItTail * L : 0;
    SRX_TRY(it_alloc(ctx, bufs, (n + tail) * 8, (void**)dev));
    std::vector<double> h(n + tail, kItSentinel);
    if (host) memcpy(h.data(), host, n * 8);
    else std::fill(h.begin(), h.begin() + n, 0.0);
    return h2d(ctx, *dev, h.data(), h.size() * 8);
}
static int32_t it_down(srx_ctx* ctx, double* host, const double* dev, size_t n, bool block, int32_t* touched) {
    const size_t tail = block ? (size_t)kItTail * L : 0;
    std::vector<double> h(n + tail);
    SRX_TRY(d2h(ctx, h.data(), dev, h.size() * 8));
    if (host) memcpy(host, h.data(), n * 8);
    for (size_t e = n; e < n + tail; ++e)
        if (h[e] != kItSentinel) *touched = 1;
    return SRX_OK;
}

int32_t srx_iterate_op(srx_ctx* ctx, int32_t op, srx_iterate_args* a) {
    if (!ctx || !a) return fail(ctx, SRX_E_ARG, "srx_iterate_op: null argument");
    if (a->k < 1) return fail(ctx, SRX_E_ARG, "srx_iterate_op: k must be >= 1");
    const bool needs_n = op == SRX_IT_CHOL || op == SRX_IT_EIG;
    const bool needs_l = op == SRX_IT_RITZ || op == SRX_IT_CHEB;
    if (needs_n && (a->n < 1 || a->n > L)) return fail(ctx, SRX_E_ARG, "srx_iterate_op: n must be in 1..%d", L);
    if (needs_l && (a->l_act < 1 || a->l_act > L)) return fail(ctx, SRX_E_ARG, "srx_iterate_op: l_act must be in 1..%d", L);
    if (op == SRX_IT_RITZ && (a->n_pc < 1 || a->n_pc > a->l_act)) return fail(ctx, SRX_E_ARG, "srx_iterate_op: n_pc must be in 1..l_act");
    int n_blk = 0, n_sm = 0, n_vec = 0;            // the slots the operation names: all must be given
    bool need_c = false, need_xi = false;
    switch (op) {
        case SRX_IT_APPLY: n_blk = 2; need_c = true; break;
        case SRX_IT_GRAM1: n_blk = (a->flags & SRX_IT_ALIAS_B) ? 1 : 2; n_sm = 1; break;
        case SRX_IT_GRAM2: n_blk = (a->flags & SRX_IT_ALIAS_B) ? 1 : 2; n_sm = 2; break;
        case SRX_IT_CHOL:
            if (a->variant < 0 || a->variant > 2) return fail(ctx, SRX_E_ARG, "srx_iterate_op: chol variant must be 0, 1 or 2");
            n_sm = 2; n_vec = 1; need_xi = a->variant == 2; break;
        case SRX_IT_TRSM:
            if (a->variant < 0 || a->variant > 1) return fail(ctx, SRX_E_ARG, "srx_iterate_op: trsm variant must be 0 or 1");
            n_blk = 2; n_sm = 2; n_vec = a->variant == 0 ? 1 : 0; need_xi = a->variant == 1;
            for (int i = 0; i < 3; ++i)
                if ((a->flags & (SRX_IT_Z0 << i)) && !a->blk[2 + i]) return fail(ctx, SRX_E_ARG, "srx_iterate_op: null z block");
            break;
        case SRX_IT_EIG: n_sm = 2; n_vec = 1; break;
        case SRX_IT_RITZ: n_blk = 4; n_sm = 2; n_vec = 3; break;
        case SRX_IT_CHEB:
            if (a->variant < 0 || a->variant > 3) return fail(ctx, SRX_E_ARG, "srx_iterate_op: cheb variant must be 0..3");
            n_blk = a->variant == 0 ? 2 : a->variant == 1 ? 4 : a->variant == 2 ? 3 : 1; n_vec = 1; break;
        default: return fail(ctx, SRX_E_ARG, "srx_iterate_op: unknown op %d", op);
    }
    for (int i = 0; i < n_blk; ++i)
        if (!a->blk[i]) return fail(ctx, SRX_E_ARG, "srx_iterate_op: null block %d", i);
    for (int i = (op == SRX_IT_TRSM || op == SRX_IT_RITZ ? 1 : 0); i < n_sm; ++i)      // (these two read sm[1] alone)
        if (!a->sm[i]) return fail(ctx, SRX_E_ARG, "srx_iterate_op: null matrix %d", i);
    for (int i = 0; i < n_vec; ++i)
        if (!a->vec[i]) return fail(ctx, SRX_E_ARG, "srx_iterate_op: null vector %d", i);
    if ((need_c && !a->c) || (need_xi && !a->xi)) return fail(ctx, SRX_E_ARG, "srx_iterate_op: null argument");
    SRX_HIP(ctx, hipSetDevice(ctx->device));

    const int k = a->k;
    const size_t kl = (size_t)k * L, ll = (size_t)L * L;
    ItBufs bufs;
    double *blk[5] = {nullptr, nullptr, nullptr, nullptr, nullptr}, *sm[2] = {nullptr, nullptr}, *vec[3] = {nullptr, nullptr, nullptr};
    double *c = nullptr, *xi = nullptr, *out = nullptr;
    int *status = nullptr, *status_sel = nullptr;
    a->tail_touched = 0;
    for (int i = 0; i < 5; ++i)
        if (a->blk[i]) SRX_TRY(it_up(ctx, bufs, a->blk[i], kl, true, &blk[i]));
    for (int i = 0; i < 2; ++i) SRX_TRY(it_up(ctx, bufs, a->sm[i], ll, false, &sm[i]));
    for (int i = 0; i < 3; ++i) SRX_TRY(it_up(ctx, bufs, a->vec[i], L, false, &vec[i]));
    SRX_TRY(it_up(ctx, bufs, a->xi, 4 * 16 * 16, false, &xi));
    SRX_TRY(it_up(ctx, bufs, nullptr, 8, false, &out));
    if (a->c) SRX_TRY(it_up(ctx, bufs, a->c, (size_t)k * k, false, &c));
    SRX_TRY(it_alloc(ctx, bufs, 512, (void**)&status));         // (the solver's 256-byte status block, and the selection's word)
    SRX_HIP(ctx, hipMemsetAsync(status, 0, 512, ctx->stream));
    status_sel = status + 64;

    switch (op) {
        case SRX_IT_APPLY:
            SRX_TRY(attr_dense_apply(ctx));
            launch_dense_apply(ctx, c, blk[0], k, blk[1]);
            break;
        case SRX_IT_GRAM1:
            launch_gram1(ctx, blk[0], (a->flags & SRX_IT_ALIAS_B) ? blk[0] : blk[1], k, sm[0]);
            break;
        case SRX_IT_GRAM2: {
            Work w{};
            double* hg;
            SRX_TRY(it_alloc(ctx, bufs, (size_t)kGram2Blocks * 2 * ll * 8, (void**)&w.gpart));
            SRX_TRY(it_alloc(ctx, bufs, 2 * ll * 8, (void**)&hg));
            w.dHG = hg;
            SRX_TRY(gram2(ctx, w, blk[0], (a->flags & SRX_IT_ALIAS_B) ? blk[0] : blk[1], k));
            SRX_HIP(ctx, hipMemcpyAsync(sm[0], hg, ll * 8, hipMemcpyDeviceToDevice, ctx->stream));
            SRX_HIP(ctx, hipMemcpyAsync(sm[1], hg + ll, ll * 8, hipMemcpyDeviceToDevice, ctx->stream));
            break;
        }
        case SRX_IT_CHOL:
            if (a->variant == 2) launch_chol_mfma(ctx, sm[0], a->n, sm[1], vec[0], xi, status);
            else launch_chol(ctx, sm[0], a->n, sm[1], vec[0], status, a->variant);
            break;
        case SRX_IT_TRSM: {
            double* const src = blk[0];
            double* const W = (a->flags & SRX_IT_SRC_IS_W) ? src : blk[1];
            double* z[3];
            for (int i = 0; i < 3; ++i) z[i] = (a->flags & (SRX_IT_Z0 << i)) ? blk[2 + i] : nullptr;
            if (a->flags & SRX_IT_Z0_IS_SRC) z[0] = src;
            if (a->variant == 0) launch_trsm_rows(ctx, src, sm[1], vec[0], k, W, z[0], z[1], z[2]);
            else launch_trsm_mfma(ctx, src, sm[1], xi, k, W, z[0], z[1], z[2]);
            if (W != blk[1]) SRX_HIP(ctx, hipMemcpyAsync(blk[1], W, kl * 8, hipMemcpyDeviceToDevice, ctx->stream));
            break;
        }
        case SRX_IT_EIG:
            SRX_TRY(attr_jacobi(ctx));
            launch_jacobi(ctx, sm[0], a->n, sm[1], vec[0], status, a->off_tol2, a->n_want);
            break;
        case SRX_IT_RITZ: {
            double* part;
            SRX_TRY(it_alloc(ctx, bufs, (size_t)kRitzBlocks * 3 * L * 8, (void**)&part));
            launch_ritz_post(ctx, blk[0], blk[1], sm[1], vec[0], k, blk[2], blk[3], part, (a->flags & SRX_IT_ZERO_WP) ? 1 : 0);
            launch_resid_final(ctx, part, vec[0], a->n_pc, a->l_act, status, status_sel, vec[1], vec[2], out);
            break;
        }
        case SRX_IT_CHEB:
            if (a->variant == 0) launch_cheb_first(ctx, blk[0], blk[1], vec[0], a->l_act, kl);
            else if (a->variant == 1) launch_cheb_first2(ctx, blk[0], blk[1], blk[2], blk[3], vec[0], a->l_act, kl);
            else if (a->variant == 2) launch_cheb_step(ctx, blk[0], blk[1], blk[2], vec[0], a->l_act, kl);
            else launch_cheb_scale(ctx, blk[0], vec[0], a->l_act, a->d, kl);
            break;
    }
    SRX_HIP(ctx, hipGetLastError());
    SRX_HIP(ctx, hipStreamSynchronize(ctx->stream));
    for (int i = 0; i < 5; ++i)
        if (blk[i]) SRX_TRY(it_down(ctx, a->blk[i], blk[i], kl, true, &a->tail_touched));
    for (int i = 0; i < 2; ++i) SRX_TRY(it_down(ctx, a->sm[i], sm[i], ll, false, nullptr));
    for (int i = 0; i < 3; ++i) SRX_TRY(it_down(ctx, a->vec[i], vec[i], L, false, nullptr));
    SRX_TRY(it_down(ctx, a->xi, xi, 4 * 16 * 16, false, nullptr));
    SRX_TRY(it_down(ctx, a->out, out, 8, false, nullptr));
    SRX_TRY(d2h(ctx, a->status, status, sizeof a->status));
    return SRX_OK;
}

}  // extern "C"

// Pca::transform: a fitted model applied to other cells (the forward product of the scores above, on a query)
#include "pca_model.inl"
