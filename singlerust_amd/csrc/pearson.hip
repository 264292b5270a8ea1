// pearson.hip — highly variable genes by analytic Pearson residuals (srx.h: srx_pearson_gene_variance, srx_select_hvg_pearson,
// srx_pearson_residuals).  Raw counts in, per-gene residual variances, a ranked selection or a block of residuals out.
//
// A residual exists for every (cell, gene) pair, zeros included: n x G of them (3.6e10 at 1.3 M x 28 k).  The residual of a ZERO
// entry depends on r_i and g_j alone, so the sums over all pairs are made without touching the matrix (k_pr_dense: r streamed,
// a few genes per thread in registers — the compute-bound part: one f64 division and one square root per pair), and the stored
// entries then CORRECT them by z - f and z^2 - f^2 (k_pr_sparse_csr: one pass over the matrix, the corrections of a gene in
// 64-bit fixed point: integer atomics, exact in any order).  A CSC handle stores the genes as rows: a wave per gene walks all
// cells with the stored entries merged in and evaluates every pair as defined (k_pr_gene_direct).  The order of every sum is
// fixed: cell chunks in ascending order, a CSC gene's cells by lane and butterfly.  The ranking is select.hip's
// (rank_keys_device).
#include "pearson_internal.hpp"
#include "pca_internal.hpp"

#include <algorithm>
#include <cmath>
#include <limits>

// srx.h states the order of every operation of a residual
#pragma clang fp contract(off)

namespace srx {

// The sizes the tests walk round (tests/test_pearson_gpu.py names the same numbers).
constexpr int kPrDenseThreads = 256;
constexpr int kPrGenesPerThread = 4;
constexpr int kPrGeneTile = kPrDenseThreads * kPrGenesPerThread;      // 1024 genes per workgroup of the dense pass
constexpr int kPrCellStep = 1024;            // cells staged in LDS at a time; a cell chunk is a multiple of it
constexpr int kPrMaxChunks = 128;            // cell chunks of the dense pass: partial sums of 2 x 128 x G doubles at the most
constexpr int kPrSparseThreads = 1024;       // CSR correction: a workgroup owns one (gene tile of the matrix, row block) and the LDS of its CU
constexpr int kPrSparseMinRows = 64;         // ... of at least this many rows
constexpr int kPrBlockTile = 256;            // outputs per workgroup of the block kernel
constexpr uint64_t kPrBlockBytes = 1ull << 30;

// The residual of a zero entry in the dense pass's form: f = -min(mu / sqrt(mu (1 + mu / theta)), c) from mu = r_i * (g_j / T),
// and its square.  One division and one root; the dense pass and the corrections call THIS function, so that what a stored
// entry takes off again is bit for bit what the dense pass put in.
__device__ __forceinline__ void pr_zero(double mu, double inv_theta, double clip, double& f, double& f2) {
    const double s = sqrt(mu * (1.0 + mu * inv_theta));
    double a = mu > 0.0 ? mu / s : 0.0;
    a = fmin(a, clip);
    f = -a;
    f2 = a * a;
}

// ---- totals: T = sum r_i in one fixed order, the expressed genes, the empty cells (one workgroup) ----------------------------
// small[0] = T; counts[0] = genes with g_j > 0, counts[1] = cells with r_i == 0
__global__ __launch_bounds__(1024) void k_pr_totals(const double* __restrict__ cell_sum, uint64_t n, const double* __restrict__ gene_sum,
                                                    uint64_t G, double* __restrict__ small, uint64_t* __restrict__ counts) {
    __shared__ double s_t[1024];
    __shared__ uint32_t s_e[1024], s_x[1024];
    const int t = threadIdx.x;
    double sum = 0.0;
    uint32_t empty = 0, expr = 0;
    for (uint64_t i = t; i < n; i += 1024) {
        const double r = cell_sum[i];
        sum += r;
        empty += r == 0.0 ? 1u : 0u;
    }
    for (uint64_t j = t; j < G; j += 1024) expr += gene_sum[j] > 0.0 ? 1u : 0u;
    s_t[t] = sum;
    s_e[t] = empty;
    s_x[t] = expr;
    __syncthreads();
    for (int half = 512; half > 0; half >>= 1) {
        if (t < half) {
            s_t[t] += s_t[t + half];
            s_e[t] += s_e[t + half];
            s_x[t] += s_x[t + half];
        }
        __syncthreads();
    }
    if (t == 0) {
        small[0] = s_t[0];
        counts[0] = s_x[0];
        counts[1] = s_e[0];
    }
}
// a_j = g_j / T, the per-gene factor of the dense form (0 for a gene without counts and for T == 0)
__global__ __launch_bounds__(256) void k_pr_gene_factor(const double* __restrict__ gene_sum, uint64_t G, const double* __restrict__ small,
                                                        double* __restrict__ gene_a) {
    const uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= G) return;
    const double T = small[0], g = gene_sum[j];
    gene_a[j] = (T > 0.0 && g > 0.0) ? g / T : 0.0;
}

// ---- dense pass: S1_j, S2_j over the zero-entry residual of every cell ----------------------------------------------------------
// Workgroup (x, y): genes 1024 x .. 1024 x + 1023 (thread t owns t, t + 256, t + 512, t + 768 of them: coalesced, four independent
// division / root chains) against the cells of chunk y; r comes through LDS, 1024 cells at a time (each r_i is read from memory
// once per workgroup, then broadcast).  A cell behind the chunk's end is staged as r = 0, whose residual is exactly 0.
__global__ __launch_bounds__(kPrDenseThreads) void k_pr_dense(const double* __restrict__ cell_sum, const double* __restrict__ gene_a,
                                                              uint64_t n, uint64_t G, uint64_t chunk, double inv_theta, double clip,
                                                              double* __restrict__ part1, double* __restrict__ part2) {
    __shared__ double s_r[kPrCellStep];
    const uint64_t j0 = (uint64_t)blockIdx.x * kPrGeneTile + threadIdx.x;
    double a[kPrGenesPerThread], s1[kPrGenesPerThread], s2[kPrGenesPerThread];
#pragma unroll
    for (int k = 0; k < kPrGenesPerThread; ++k) {
        const uint64_t j = j0 + (uint64_t)k * kPrDenseThreads;
        a[k] = j < G ? gene_a[j] : 0.0;
        s1[k] = 0.0;
        s2[k] = 0.0;
    }
    const uint64_t c0 = (uint64_t)blockIdx.y * chunk;
    const uint64_t c1 = c0 + chunk < n ? c0 + chunk : n;
    for (uint64_t base = c0; base < c1; base += kPrCellStep) {
        __syncthreads();
        for (int e = threadIdx.x; e < kPrCellStep; e += kPrDenseThreads) s_r[e] = base + e < c1 ? cell_sum[base + e] : 0.0;
        __syncthreads();
        const int m = c1 - base < (uint64_t)kPrCellStep ? (int)(c1 - base) : kPrCellStep;
#pragma unroll 2
        for (int i = 0; i < m; ++i) {
            const double r = s_r[i];
#pragma unroll
            for (int k = 0; k < kPrGenesPerThread; ++k) {
                double f, f2;
                pr_zero(r * a[k], inv_theta, clip, f, f2);
                s1[k] += f;
                s2[k] += f2;
            }
        }
    }
#pragma unroll
    for (int k = 0; k < kPrGenesPerThread; ++k) {
        const uint64_t j = j0 + (uint64_t)k * kPrDenseThreads;
        if (j < G) {
            part1[(uint64_t)blockIdx.y * G + j] = s1[k];
            part2[(uint64_t)blockIdx.y * G + j] = s2[k];
        }
    }
}

// ---- sparse correction, CSR handle: a scatter over genes -----------------------------------------------------------------------
// The matrix's own gene tiles (ensure_tiles: a tile's entries are one segment of every row) with two 64-bit fixed-point
// accumulators per gene in LDS; a wave per row.  Integer addition is associative: the order the atomics land in does not
// matter, in LDS or in the flush to the G x 2 global accumulators.
template <typename T>
__global__ __launch_bounds__(kPrSparseThreads) void k_pr_sparse_csr(
    const int64_t* __restrict__ indptr, const int64_t* __restrict__ tp, const int32_t* __restrict__ idx, const T* __restrict__ vals,
    uint64_t n_rows, uint64_t G, int n_tiles, int tile_genes, uint64_t rows_per_block, const double* __restrict__ cell_sum,
    const double* __restrict__ gene_sum, const double* __restrict__ gene_a, PrArgs a, double fx1, double fx2,
    unsigned long long* __restrict__ acc) {
    extern __shared__ unsigned long long s_acc[];       // 2 x tile_genes
    for (int g = threadIdx.x; g < 2 * tile_genes; g += kPrSparseThreads) s_acc[g] = 0ull;
    __syncthreads();
    const int tile = (int)(blockIdx.x % (unsigned)n_tiles);
    const uint64_t rb = blockIdx.x / (unsigned)n_tiles;
    const int32_t gbase = tile * tile_genes;
    const uint64_t r0 = rb * rows_per_block;
    const uint64_t r1 = r0 + rows_per_block < n_rows ? r0 + rows_per_block : n_rows;
    const int lane = lane_id();
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x / kWave);
    for (uint64_t r = r0 + wave; r < r1; r += kPrSparseThreads / kWave) {
        int64_t lo, hi;
        seg_bounds(indptr, tp, n_rows, n_tiles, tile, r, lo, hi);
        const double rs = cell_sum[r];
        for (int64_t e = lo + lane; e < hi; e += kWave) {
            const int32_t g = idx[e];
            const int32_t gl = g - gbase;
            if ((uint32_t)gl >= (uint32_t)tile_genes || (uint64_t)g >= G) continue;      // (never, for the cuts of a validated matrix)
            const double z = pr_resid((double)vals[e], rs, gene_sum[g], a);
            double f, f2;
            pr_zero(rs * gene_a[g], a.inv_theta, a.clip, f, f2);
            const long long q1 = __double2ll_rn((z - f) * fx1);
            const long long q2 = __double2ll_rn((z * z - f2) * fx2);
            atomicAdd(&s_acc[2 * gl], (unsigned long long)q1);
            atomicAdd(&s_acc[2 * gl + 1], (unsigned long long)q2);
        }
    }
    __syncthreads();
    for (int gl = threadIdx.x; gl < tile_genes; gl += kPrSparseThreads) {
        const uint64_t g = (uint64_t)gbase + (uint64_t)gl;
        if (g >= G) break;
        const unsigned long long q1 = s_acc[2 * gl], q2 = s_acc[2 * gl + 1];
        if (q1) atomicAdd(&acc[2 * g], q1);
        if (q2) atomicAdd(&acc[2 * g + 1], q2);
    }
}

// ---- CSC handle: the stored rows are the genes, every pair of a gene is evaluated directly -------------------------------------
// A wave per gene walks ALL n cells, 64 at a time, with the gene's stored entries (sorted by cell) merged in through LDS: the
// entries of a window of 64 cells are the next <= 64 of the list.  z as srx.h defines it for every pair, zeros included, so
// nothing is added and taken off again: a gene whose residuals are all 0 gets the variance 0.0 exactly.  Lane l sums the cells
// l, l + 64, .. in that order, the 64 partial sums meet in a butterfly: f64, no atomics, the same order wherever the gene sits.
template <typename T>
__global__ __launch_bounds__(256) void k_pr_gene_direct(const int64_t* __restrict__ indptr, const int32_t* __restrict__ idx,
                                                        const T* __restrict__ vals, uint64_t G, uint64_t n,
                                                        const double* __restrict__ cell_sum, const double* __restrict__ gene_sum,
                                                        PrArgs a, double* __restrict__ sums) {
    __shared__ double s_x[256 / kWave][kWave];
    const uint64_t j = global_wave_id();
    if (j >= G) return;                        // (a whole wave; the kernel has no workgroup barrier)
    const int lane = lane_id();
    double* const x_of = s_x[__builtin_amdgcn_readfirstlane(threadIdx.x / kWave)];
    const int64_t hi = indptr[j + 1];
    int64_t p = indptr[j];
    const double gs = gene_sum[j];
    double s1 = 0.0, s2 = 0.0;
    for (uint64_t base = 0; gs > 0.0 && base < n; base += kWave) {
        x_of[lane] = 0.0;
        wave_lds_sync();
        const int64_t e = p + lane;
        const int64_t c = e < hi ? (int64_t)idx[e] - (int64_t)base : -1;       // sorted and unique: the window's entries are a prefix
        const bool in = c >= 0 && c < kWave;
        if (in) x_of[c] = (double)vals[e];
        p += __popcll(__ballot(in));
        wave_lds_sync();
        const uint64_t i = base + lane;
        if (i < n) {
            const double z = pr_resid(x_of[lane], cell_sum[i], gs, a);
            s1 += z;
            s2 += z * z;
        }
        wave_lds_sync();
    }
    s1 = wave_sum(s1);
    s2 = wave_sum(s2);
    if (lane == 0) {
        sums[2 * j] = s1;
        sums[2 * j + 1] = s2;
    }
}

// ---- v_j and the ranking key ---------------------------------------------------------------------------------------------------
// The chunks' partial sums in ascending order, then the correction (fixed point: `acc`; else `corr`, a CSC handle's whole sums
// with n_chunks = 0).  A gene without counts:
// variance 0.0, key -inf (behind every expressed gene in the ranking); the rank table starts at 0 for k_hvg_rank's sums.
__global__ __launch_bounds__(256) void k_pr_finish(const double* __restrict__ part1, const double* __restrict__ part2, uint32_t n_chunks,
                                                   uint64_t G, const double* __restrict__ gene_sum,
                                                   const unsigned long long* __restrict__ acc, double q1, double q2,
                                                   const double* __restrict__ corr, double n_cells, double* __restrict__ var,
                                                   double* __restrict__ key, uint32_t* __restrict__ rank) {
    const uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= G) return;
    double s1 = 0.0, s2 = 0.0;
    for (uint32_t c = 0; c < n_chunks; ++c) {
        s1 += part1[(uint64_t)c * G + j];
        s2 += part2[(uint64_t)c * G + j];
    }
    if (acc) {
        s1 += (double)(long long)acc[2 * j] * q1;
        s2 += (double)(long long)acc[2 * j + 1] * q2;
    } else {
        s1 += corr[2 * j];
        s2 += corr[2 * j + 1];
    }
    const double mean = s1 / n_cells;
    const double v = s2 / n_cells - mean * mean;
    const bool expressed = gene_sum[j] > 0.0;
    var[j] = expressed ? v : 0.0;
    key[j] = expressed ? v : -INFINITY;
    rank[j] = 0u;
}

// ---- block kernel: the residuals of listed genes, a chunk of cells --------------------------------------------------------------
// One thread per output: a binary search of the column in the stored row (CSR: cell i's row for the gene; CSC: the gene's row
// for cell i), x = 0 where it is not stored, then the definition.
template <typename T>
__global__ __launch_bounds__(kPrBlockTile) void k_pr_block(const int64_t* __restrict__ indptr, const int32_t* __restrict__ idx,
                                                           const T* __restrict__ vals, int csc, const double* __restrict__ cell_sum,
                                                           const double* __restrict__ gene_sum, const uint32_t* __restrict__ genes,
                                                           uint64_t k, uint64_t row0, uint64_t rows, PrArgs a, double* __restrict__ out) {
    const uint64_t o = (uint64_t)blockIdx.x * kPrBlockTile + threadIdx.x;
    if (o >= rows * k) return;
    const uint64_t i = row0 + o / k;
    const uint32_t g = genes[o % k];
    const uint64_t row = csc ? g : i;
    const int32_t col = (int32_t)(csc ? i : g);
    int64_t lo = indptr[row], hi = indptr[row + 1];
    const int64_t end = hi;
    while (lo < hi) {
        const int64_t mid = lo + ((hi - lo) >> 1);
        if (idx[mid] < col) lo = mid + 1; else hi = mid;
    }
    const double x = (lo < end && idx[lo] == col) ? (double)vals[lo] : 0.0;
    out[o] = pr_resid(x, cell_sum[i], gene_sum[g], a);
}

// ---- host side -------------------------------------------------------------------------------------------------------------------
int32_t pr_check_args(srx_mat* m, const srx_pearson_opts* opts, const char* who, PrArgs& a, uint64_t n_cells) {
    srx_ctx* ctx = m->ctx;
    if (ctx->n_ranks > 1) return fail(ctx, SRX_E_ARG, "%s: a context with more than one rank (the sharded form is out of scope)", who);
    if (ctx->pool_on > 0) return fail(ctx, SRX_E_ARG, "%s: a backed session is open on this context (the out-of-core form is out of scope)", who);
    const double theta = opts ? opts->theta : 0.0, clip = opts ? opts->clip : 0.0;
    if (!(theta >= 0.0)) return fail(ctx, SRX_E_ARG, "%s: theta = %g (negative or NaN)", who, theta);
    if (!(clip >= 0.0)) return fail(ctx, SRX_E_ARG, "%s: clip = %g (negative or NaN)", who, clip);
    a.theta = theta == 0.0 ? 100.0 : theta;
    a.poisson = a.theta > kDblMax ? 1 : 0;
    a.inv_theta = a.poisson ? 0.0 : 1.0 / a.theta;
    a.clip = clip == 0.0 ? std::sqrt((double)n_cells) : clip;
    return SRX_OK;
}

// Everything the three calls share: the arguments, the value check, r, g, T and the counts.  One small read-back.
int32_t pr_prepare(srx_mat* m, const srx_pearson_opts* opts, const char* who, PrPrep& p) {
    srx_ctx* ctx = m->ctx;
    p.n = m->csc ? m->n_cols : m->n_rows;
    p.G = m->csc ? m->n_rows : m->n_cols;
    SRX_TRY(pr_check_args(m, opts, who, p.a, p.n));
    SRX_HIP(ctx, hipSetDevice(ctx->device));
    char* d_small;
    SRX_TRY(scratch(ctx, "pearson_small", 256, (void**)&d_small));
    double* d_total = reinterpret_cast<double*>(d_small);
    uint64_t* d_counts = reinterpret_cast<uint64_t*>(d_small + 8);
    unsigned long long* d_scan = reinterpret_cast<unsigned long long*>(d_small + 24);      // the value scan's VS_WORDS words
    SRX_HIP(ctx, hipMemsetAsync(d_small, 0, 256, ctx->stream));
    value_scan(m, d_scan);
    SRX_HIP(ctx, hipGetLastError());
    // the sums over the stored rows go to a buffer of this call (the handle's d_row_sum is the normalise pass's), those over the
    // stored columns are the handle's cached raw moments
    double *d_rows, *d_gene_a;
    SRX_TRY(scratch(ctx, "pearson_rows", at_least_one(m->n_rows) * sizeof(double), (void**)&d_rows));
    SRX_TRY(scratch(ctx, "pearson_gene_a", at_least_one(p.G) * sizeof(double), (void**)&d_gene_a));
    SRX_TRY(launch_row_sums(m, d_rows));
    SRX_TRY(ensure_moments(m));
    p.d_cell = m->csc ? m->d_sum : d_rows;
    p.d_gene = m->csc ? d_rows : m->d_sum;
    p.d_gene_a = d_gene_a;
    hipLaunchKernelGGL(k_pr_totals, dim3(1), dim3(1024), 0, ctx->stream, p.d_cell, p.n, p.d_gene, p.G, d_total, d_counts);
    hipLaunchKernelGGL(k_pr_gene_factor, dim3(grid256(p.G)), dim3(256), 0, ctx->stream, p.d_gene, p.G, (const double*)d_total, d_gene_a);
    SRX_HIP(ctx, hipGetLastError());
    unsigned char host[24 + 8 * VS_WORDS];
    SRX_TRY(d2h(ctx, host, d_small, sizeof host));
    unsigned long long scan[VS_WORDS];
    uint64_t counts[2];
    memcpy(&p.a.total, host, 8);
    memcpy(counts, host + 8, 16);
    memcpy(scan, host + 24, sizeof scan);
    if (scan[VS_FLAGS] & (kValNegative | kValNonFinite)) return fail(ctx, SRX_E_ARG, "%s: the matrix holds a negative, NaN or infinite value", who);
    p.n_expressed = counts[0];
    p.n_empty = counts[1];
    return SRX_OK;
}

void pr_info(const PrPrep& p, srx_pearson_info* info) {
    if (!info) return;
    memset(info, 0, sizeof *info);
    info->n_cells = p.n;
    info->n_genes = p.G;
    info->n_expressed = p.n_expressed;
    info->n_empty_cells = p.n_empty;
    info->total = p.a.total;
    info->theta = p.a.theta;
    info->clip = p.a.clip;
}

// T and the empty cells of another set of per-cell sums (pearson_pca.hip: the sums over the listed genes), by the kernel and in
// the order of pr_prepare
int32_t pr_totals(srx_ctx* ctx, const double* d_cell, uint64_t n, const double* d_gene, uint64_t G, double* total, uint64_t* n_empty) {
    char* d_small;
    SRX_TRY(scratch(ctx, "pearson_small2", 256, (void**)&d_small));
    SRX_HIP(ctx, hipMemsetAsync(d_small, 0, 256, ctx->stream));
    hipLaunchKernelGGL(k_pr_totals, dim3(1), dim3(1024), 0, ctx->stream, d_cell, n, d_gene, G, reinterpret_cast<double*>(d_small),
                       reinterpret_cast<uint64_t*>(d_small + 8));
    SRX_HIP(ctx, hipGetLastError());
    unsigned char host[24];
    SRX_TRY(d2h(ctx, host, d_small, sizeof host));
    memcpy(total, host, 8);
    memcpy(n_empty, host + 16, 8);
    return SRX_OK;
}

// 2^shift with 2^(61 - shift) >= bound: the fixed-point scale of a sum whose magnitude stays below `bound`
static double pr_fixed_scale(double bound) {
    int e = 0;
    if (bound > 0.0 && bound <= kDblMax) {
        (void)std::frexp(bound, &e);            // bound = m 2^e, 0.5 <= m < 1
        if (std::ldexp(1.0, e - 1) == bound) e -= 1;       // ceil(log2(bound))
    }
    return std::ldexp(1.0, std::min(61 - e, 200));
}

// The variances (and with `select` the first `n_sel` genes of the ranking) into host buffers of the caller's; nothing of the
// caller's is written before the last device call has succeeded.
static int32_t pr_variance(srx_mat* m, const srx_pearson_opts* opts, const char* who, bool select, uint64_t n_sel,
                           std::vector<double>& var, std::vector<uint64_t>& sel, PrPrep& p, srx_pearson_info* info_out) {
    srx_ctx* ctx = m->ctx;
    SRX_TRY(pr_prepare(m, opts, who, p));
    srx_pearson_info info;
    pr_info(p, &info);
    const uint64_t n = p.n, G = p.G;
    var.assign(G, 0.0);
    sel.clear();
    if (G == 0 || n == 0 || p.n_expressed == 0) {          // T == 0 included: every variance 0, nothing to select
        if (info_out) *info_out = info;
        return SRX_OK;
    }
    if (G >= 0xffffffffull) return fail(ctx, SRX_E_ARG, "%s: %llu genes", who, (unsigned long long)G);

    // dense pass (CSR handles; a CSC handle evaluates every pair in k_pr_gene_direct and has no partial sums)
    const uint64_t per = (n + kPrMaxChunks - 1) / kPrMaxChunks;
    const uint64_t chunk = std::max<uint64_t>(kPrCellStep, (per + kPrCellStep - 1) / kPrCellStep * kPrCellStep);
    const uint32_t n_chunks = m->csc ? 0u : (uint32_t)((n + chunk - 1) / chunk);
    double *d_part, *d_var, *d_key;
    uint32_t* d_rank;
    SRX_TRY(scratch(ctx, "pearson_part", 2 * (size_t)at_least_one(n_chunks) * G * sizeof(double), (void**)&d_part));
    SRX_TRY(scratch(ctx, "pearson_var", 2 * G * sizeof(double), (void**)&d_var));
    SRX_TRY(scratch(ctx, "pearson_rank", G * sizeof(uint32_t), (void**)&d_rank));
    d_key = d_var + G;
    double* d_part2 = d_part + (size_t)n_chunks * G;
    if (n_chunks) {
        StreamTimer timer(ctx, ctx->stream);
        SRX_TRY(timer.start());
        hipLaunchKernelGGL(k_pr_dense, dim3((unsigned)((G + kPrGeneTile - 1) / kPrGeneTile), n_chunks), dim3(kPrDenseThreads), 0, ctx->stream,
                           p.d_cell, (const double*)p.d_gene_a, n, G, chunk, p.a.inv_theta, p.a.clip, d_part, d_part2);
        SRX_HIP(ctx, hipGetLastError());
        SRX_TRY(timer.stop(&info.ms_dense));
    }

    // sparse correction (CSR) or the whole sums (CSC)
    unsigned long long* d_acc = nullptr;
    double* d_corr = nullptr;
    double fx1 = 0.0, fx2 = 0.0;
    StreamTimer timer_s(ctx, ctx->stream);
    if (m->csc) {
        SRX_TRY(scratch(ctx, "pearson_corr", 2 * G * sizeof(double), (void**)&d_corr));
        SRX_TRY(timer_s.start());
        auto launch = [&](auto* vals) {
            using T = std::remove_pointer_t<decltype(vals)>;
            hipLaunchKernelGGL(k_pr_gene_direct<T>, dim3((unsigned)((G + 3) / 4)), dim3(256), 0, ctx->stream, m->d_indptr, m->d_indices,
                               (const T*)vals, G, n, p.d_cell, p.d_gene, p.a, d_corr);
        };
        if (is_f32(m)) launch((float*)m->d_values); else launch((double*)m->d_values);
    } else {
        SRX_TRY(ensure_tiles(m));
        SRX_TRY(scratch(ctx, "pearson_acc", 2 * G * sizeof(unsigned long long), (void**)&d_acc));
        const double b = std::min(p.a.clip, std::sqrt(p.a.total));
        fx1 = pr_fixed_scale(2.0 * (double)n * b);
        fx2 = pr_fixed_scale((double)n * b * b);
        info.sum_quantum = 1.0 / fx1;
        info.sq_quantum = 1.0 / fx2;
        uint64_t nb = std::max<uint64_t>(1, (uint64_t)(4 * ctx->n_cus) / (uint64_t)m->n_tiles);
        nb = std::min(nb, std::max<uint64_t>(1, (n + kPrSparseMinRows - 1) / kPrSparseMinRows));
        const uint64_t rpb = (n + nb - 1) / nb;
        nb = (n + rpb - 1) / rpb;
        const size_t lds = (size_t)m->tile_genes * 16;
        SRX_TRY(timer_s.start());
        SRX_HIP(ctx, hipMemsetAsync(d_acc, 0, 2 * G * sizeof(unsigned long long), ctx->stream));
        auto launch = [&](auto* vals) -> int32_t {
            using T = std::remove_pointer_t<decltype(vals)>;
            SRX_HIP(ctx, hipFuncSetAttribute((const void*)k_pr_sparse_csr<T>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
            hipLaunchKernelGGL(k_pr_sparse_csr<T>, dim3((unsigned)(nb * m->n_tiles)), dim3(kPrSparseThreads), lds, ctx->stream, m->d_indptr,
                               m->d_tile_ptr, m->d_indices, (const T*)vals, n, G, m->n_tiles, m->tile_genes, rpb, p.d_cell, p.d_gene,
                               (const double*)p.d_gene_a, p.a, fx1, fx2, d_acc);
            return SRX_OK;
        };
        if (is_f32(m)) SRX_TRY(launch((float*)m->d_values)); else SRX_TRY(launch((double*)m->d_values));
    }
    SRX_HIP(ctx, hipGetLastError());
    SRX_TRY(timer_s.stop(&info.ms_sparse));

    // variance, key, ranking
    StreamTimer timer_r(ctx, ctx->stream);
    SRX_TRY(timer_r.start());
    hipLaunchKernelGGL(k_pr_finish, dim3(grid256(G)), dim3(256), 0, ctx->stream, (const double*)d_part, (const double*)d_part2, n_chunks, G,
                       p.d_gene, (const unsigned long long*)d_acc, info.sum_quantum, info.sq_quantum, (const double*)d_corr, (double)n,
                       d_var, d_key, d_rank);
    SRX_HIP(ctx, hipGetLastError());
    const uint64_t take = select ? std::min(n_sel, p.n_expressed) : 0;
    uint64_t* d_sel = nullptr;
    if (take) {
        SRX_TRY(scratch(ctx, "pearson_sel", take * sizeof(uint64_t), (void**)&d_sel));
        SRX_TRY(rank_keys_device(ctx, d_key, G, d_rank));
        SRX_TRY(pick_top(ctx, d_rank, G, take, d_sel));
    }
    SRX_TRY(timer_r.stop(&info.ms_rank));
    SRX_TRY(d2h(ctx, var.data(), d_var, G * sizeof(double)));
    if (take) {
        sel.resize(take);
        SRX_TRY(d2h(ctx, sel.data(), d_sel, take * sizeof(uint64_t)));
    }
    if (info_out) *info_out = info;
    return SRX_OK;
}

}  // namespace srx

using namespace srx;

extern "C" {

int32_t srx_pearson_gene_variance(srx_mat* m, const srx_pearson_opts* opts, double* var_out, srx_pearson_info* info) {
    if (!m || !var_out) return fail(m ? m->ctx : nullptr, SRX_E_ARG, "pearson_gene_variance: null argument");
    std::vector<double> var;
    std::vector<uint64_t> sel;
    PrPrep p;
    SRX_TRY(pr_variance(m, opts, "pearson_gene_variance", false, 0, var, sel, p, info));
    if (!var.empty()) memcpy(var_out, var.data(), var.size() * sizeof(double));
    return SRX_OK;
}

int32_t srx_select_hvg_pearson(srx_mat* m, uint64_t n, const srx_pearson_opts* opts, uint64_t* idx_out, uint64_t* n_out, double* var_out,
                               srx_pearson_info* info) {
    if (!m || !idx_out || !n_out) return fail(m ? m->ctx : nullptr, SRX_E_ARG, "select_hvg_pearson: null argument");
    std::vector<double> var;
    std::vector<uint64_t> sel;
    PrPrep p;
    SRX_TRY(pr_variance(m, opts, "select_hvg_pearson", true, n, var, sel, p, info));
    if (var_out && !var.empty()) memcpy(var_out, var.data(), var.size() * sizeof(double));
    if (!sel.empty()) memcpy(idx_out, sel.data(), sel.size() * sizeof(uint64_t));
    *n_out = sel.size();
    return SRX_OK;
}

int32_t srx_pearson_residuals(srx_mat* m, const uint64_t* genes, uint64_t k, const srx_pearson_opts* opts, double* out,
                              srx_pearson_info* info) {
    if (!m || !out || (!genes && k)) return fail(m ? m->ctx : nullptr, SRX_E_ARG, "pearson_residuals: null argument");
    srx_ctx* ctx = m->ctx;
    const uint64_t G = m->csc ? m->n_rows : m->n_cols;
    std::vector<uint32_t> list(k);
    for (uint64_t s = 0; s < k; ++s) {
        if (genes[s] >= G)
            return fail(ctx, SRX_E_ARG, "pearson_residuals: gene index %llu out of bounds (n_cols = %llu)", (unsigned long long)genes[s],
                        (unsigned long long)G);
        list[s] = (uint32_t)genes[s];
    }
    PrPrep p;
    SRX_TRY(pr_prepare(m, opts, "pearson_residuals", p));
    pr_info(p, info);
    if (k == 0 || p.n == 0) return SRX_OK;
    const uint64_t rows_max = std::max<uint64_t>(1, kPrBlockBytes / (k * sizeof(double)));
    const uint64_t rows_buf = std::min(rows_max, p.n);
    uint32_t* d_genes;
    double* d_out;
    SRX_TRY(scratch(ctx, "pearson_list", k * sizeof(uint32_t), (void**)&d_genes));
    SRX_TRY(scratch(ctx, "pearson_block", rows_buf * k * sizeof(double), (void**)&d_out));
    SRX_TRY(h2d(ctx, d_genes, list.data(), k * sizeof(uint32_t)));
    for (uint64_t row0 = 0; row0 < p.n; row0 += rows_buf) {
        const uint64_t rows = std::min(rows_buf, p.n - row0);
        const unsigned grid = (unsigned)((rows * k + kPrBlockTile - 1) / kPrBlockTile);
        if (is_f32(m))
            hipLaunchKernelGGL(k_pr_block<float>, dim3(grid), dim3(kPrBlockTile), 0, ctx->stream, m->d_indptr, m->d_indices,
                               (const float*)m->d_values, m->csc ? 1 : 0, p.d_cell, p.d_gene, (const uint32_t*)d_genes, k, row0, rows, p.a, d_out);
        else
            hipLaunchKernelGGL(k_pr_block<double>, dim3(grid), dim3(kPrBlockTile), 0, ctx->stream, m->d_indptr, m->d_indices,
                               (const double*)m->d_values, m->csc ? 1 : 0, p.d_cell, p.d_gene, (const uint32_t*)d_genes, k, row0, rows, p.a, d_out);
        SRX_HIP(ctx, hipGetLastError());
        SRX_TRY(d2h(ctx, out + row0 * k, d_out, rows * k * sizeof(double)));
    }
    return SRX_OK;
}

}  // extern "C"
