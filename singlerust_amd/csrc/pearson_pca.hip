// pearson_pca.hip — PCA of the clipped Pearson residuals of listed genes (srx.h: srx_pca_pearson, srx_pearson_gram): scanpy's
// experimental.pp.normalize_pearson_residuals_pca on the device.
//
// The residual matrix Z (n x k) is dense and is never held as a whole.  It is made a CHUNK of cells at a time, from the
// definition (pearson_internal.hpp: pr_resid): every pair gets the residual of a zero entry (k_pp_fill), then the stored entries
// of the chunk's rows overwrite theirs (k_pp_stored).  A chunk is sized to stay in the last-level cache (kPpChunkBytes), its row
// stride padded to whole 64-column tiles with zeros, and is read back by two products on the f64 matrix cores
// (v_mfma_f64_16x16x4, the operand layouts of iterate.inl):
//   Gram    G += Z_c^T Z_c, upper triangle in 64 x 64 tiles (k_pp_syrk), and the column sums of Z_c (k_pp_colsum);
//   scores  S_c = Z_c P - 1 c^T for the solver's k x 64 panel (k_pp_scores), written at the handle's score stride.
// Between the two the Gram solver of pca_solve.hip runs unchanged on C = G - n m m^T (DenseSource): plans A / B, deflation, the
// robust mode and the result block are shared with srx_pca.  The chunk is made twice, once for each product: keeping n x k
// doubles (20.8 GB at 1.3 M x 2000) is what this route exists to avoid.
// The two products and their host loops are shared with regress.hip (dense_pca_internal.hpp): a caller hands in what makes a chunk.
// No floating-point atomics: a tile of G has one owner per launch, the launches of the chunks follow each other on the stream
// (ascending chunk order), and where a chunk is cut into slabs their partial tiles are added in ascending slab order.
#include "pearson_internal.hpp"
#include "dense_pca_internal.hpp"

// the chunk kernels evaluate the definition and the sums of this file are stated in one order
#pragma clang fp contract(off)

namespace srx {

typedef double dvec4 __attribute__((ext_vector_type(4)));

constexpr int kPpTile = kDenseTile;             // a tile of G: 64 x 64, four waves of 32 x 32 (2 x 2 MFMA tiles each)
constexpr int kPpThreads = 256;
constexpr int kPpKU = 4;                        // MFMA K-steps (of 4 cells) whose loads are in flight together
constexpr int kPpMaxSlabs = 64;
constexpr uint64_t kPpChunkBytes = 64ull << 20; // a chunk of Z: a quarter of the 256 MB last-level cache
constexpr int kPpMaxK = kDenseMaxK;

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

// ---- a chunk of Z: rows [row0, row0 + rows) x ldz columns, columns >= k zero --------------------------------------------------------
__global__ __launch_bounds__(256) void k_pp_fill(const double* __restrict__ cell_sum, const double* __restrict__ gene_sum,
                                                 const uint32_t* __restrict__ genes, uint32_t k, uint32_t ldz, uint64_t row0,
                                                 uint64_t rows, PrArgs a, double* __restrict__ Z) {
    const uint64_t o = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (o >= rows * ldz) return;
    const uint64_t i = o / ldz;
    const uint32_t c = (uint32_t)(o - i * ldz);
    Z[o] = c < k ? pr_resid(0.0, cell_sum[row0 + i], gene_sum[genes[c]], a) : 0.0;
}
// the stored entries of the chunk's rows: a wave per row, the listed ones overwrite the zero-entry residual
template <typename T>
__global__ __launch_bounds__(256) void k_pp_stored(const int64_t* __restrict__ indptr, const int32_t* __restrict__ idx,
                                                   const T* __restrict__ vals, const double* __restrict__ cell_sum,
                                                   const double* __restrict__ gene_sum, const int32_t* __restrict__ slot_of,
                                                   uint32_t ldz, uint64_t row0, uint64_t rows, PrArgs a, double* __restrict__ Z) {
    const uint64_t i = global_wave_id();
    if (i >= rows) return;
    const uint64_t r = row0 + i;
    const double rs = cell_sum[r];
    const int64_t hi = indptr[r + 1];
    for (int64_t e = indptr[r] + lane_id(); e < hi; e += kWave) {
        const int32_t g = idx[e];
        const int32_t s = slot_of[g];
        if (s >= 0) Z[i * ldz + (uint32_t)s] = pr_resid((double)vals[e], rs, gene_sum[g], a);
    }
}

// tile pair p of the upper triangle of n_t x n_t tiles, row-major: (ti, tj), ti <= tj
__device__ __forceinline__ void pp_pair(int p, int n_t, int& ti, int& tj) {
    ti = 0;
    while (p >= n_t - ti) {
        p -= n_t - ti;
        ++ti;
    }
    tj = ti + p;
}

// ---- G += Z_c^T Z_c ------------------------------------------------------------------------------------------------------------------
// Workgroup (p, s): tile pair p against the rows of slab s.  Wave (wi, wj) owns the 32 x 32 quarter of the tile: its A fragment
// of MFMA K-step u is Z[r0 + 4 u + (lane >> 4)][I0 + 32 wi + 16 s + (lane & 15)], the B fragment the same row at the tile's
// columns — both 128 contiguous bytes per 16 lanes, straight from the chunk (L2 / last-level cache), no LDS.  A row behind the
// slab's end enters as 0.  One slab: the tile is ADDED into the packed triangle by its only owner; several: it goes to `part`
// and k_pp_syrk_reduce adds the slabs in ascending order.
__global__ __launch_bounds__(kPpThreads) void k_pp_syrk(const double* __restrict__ Z, uint32_t ldz, uint32_t rows, uint32_t slab_rows,
                                                        int n_t, int k, double* __restrict__ Gp, double* __restrict__ part) {
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int li = lane & 15, lk = lane >> 4;
    const int wi = wv >> 1, wj = wv & 1;
    int ti, tj;
    pp_pair((int)blockIdx.x, n_t, ti, tj);
    const uint32_t r_beg = blockIdx.y * slab_rows;
    const uint32_t r_end = r_beg + slab_rows < rows ? r_beg + slab_rows : rows;
    const double* za = Z + (size_t)ti * kPpTile + 32 * wi + li;
    const double* zb = Z + (size_t)tj * kPpTile + 32 * wj + li;
    dvec4 acc[2][2];
#pragma unroll
    for (int s = 0; s < 2; ++s)
#pragma unroll
        for (int t = 0; t < 2; ++t) acc[s][t] = dvec4{0.0, 0.0, 0.0, 0.0};
    for (uint32_t r0 = r_beg; r0 < r_end; r0 += 4 * kPpKU) {
        double a[kPpKU][2], b[kPpKU][2];
#pragma unroll
        for (int u = 0; u < kPpKU; ++u) {
            const uint32_t r = r0 + 4 * u + lk;
            const bool ok = r < r_end;
            const size_t off = (size_t)(ok ? r : r_beg) * ldz;
            a[u][0] = ok ? za[off] : 0.0;
            a[u][1] = ok ? za[off + 16] : 0.0;
            b[u][0] = ok ? zb[off] : 0.0;
            b[u][1] = ok ? zb[off + 16] : 0.0;
        }
#pragma unroll
        for (int u = 0; u < kPpKU; ++u)
#pragma unroll
            for (int s = 0; s < 2; ++s)
#pragma unroll
                for (int t = 0; t < 2; ++t) acc[s][t] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[u][s], b[u][t], acc[s][t], 0, 0, 0);
    }
    // C/D layout of the f64 MFMA: col = lane & 15, row = (lane >> 4) + 4 * reg
    const bool direct = gridDim.y == 1;
    double* const tile = part + ((size_t)blockIdx.y * gridDim.x + blockIdx.x) * (kPpTile * kPpTile);
#pragma unroll
    for (int s = 0; s < 2; ++s)
#pragma unroll
        for (int t = 0; t < 2; ++t)
#pragma unroll
            for (int v = 0; v < 4; ++v) {
                const int row = 32 * wi + 16 * s + lk + 4 * v, col = 32 * wj + 16 * t + li;
                if (direct) {
                    const int i = ti * kPpTile + row, j = tj * kPpTile + col;
                    if (i <= j && j < k) Gp[tri_index(i, j, k)] += acc[s][t][v];
                } else {
                    tile[row * kPpTile + col] = acc[s][t][v];
                }
            }
}
__global__ __launch_bounds__(256) void k_pp_syrk_reduce(const double* __restrict__ part, int n_pairs, int n_slabs, int n_t, int k,
                                                        double* __restrict__ Gp) {
    const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x;          // 16 workgroups per tile: the pair is uniform in a workgroup
    const int p = (int)(e / (kPpTile * kPpTile)), w = (int)(e % (kPpTile * kPpTile));
    if (p >= n_pairs) return;
    int ti, tj;
    pp_pair(p, n_t, ti, tj);
    const int i = ti * kPpTile + w / kPpTile, j = tj * kPpTile + w % kPpTile;
    if (i > j || j >= k) return;
    double s = 0.0;
    for (int sl = 0; sl < n_slabs; ++sl) s += part[((size_t)sl * n_pairs + p) * (kPpTile * kPpTile) + w];
    Gp[tri_index(i, j, k)] += s;
}

// ---- column sums of a chunk: a thread per column and slab walks the rows in order; the slabs are added in ascending order ------------
__global__ __launch_bounds__(256) void k_pp_colsum(const double* __restrict__ Z, uint32_t ldz, uint32_t rows, uint32_t slab_rows, uint32_t k,
                                                   double* __restrict__ part) {
    const uint32_t c = blockIdx.x * 256 + threadIdx.x;
    if (c >= k) return;
    const uint32_t r_beg = blockIdx.y * slab_rows;
    const uint32_t r_end = r_beg + slab_rows < rows ? r_beg + slab_rows : rows;
    double s = 0.0;
    for (uint32_t r = r_beg; r < r_end; ++r) s += Z[(size_t)r * ldz + c];
    part[(size_t)blockIdx.y * k + c] = s;
}
__global__ __launch_bounds__(256) void k_pp_colsum_reduce(const double* __restrict__ part, uint32_t n_slabs, uint32_t k,
                                                          double* __restrict__ colsum) {
    const uint32_t c = blockIdx.x * 256 + threadIdx.x;
    if (c >= k) return;
    double s = 0.0;
    for (uint32_t sl = 0; sl < n_slabs; ++sl) s += part[(size_t)sl * k + c];
    colsum[c] += s;
}

// ---- the selection's vectors: m, sd = 1, trace(C) with C = G - cen n m m^T (one workgroup, one fixed order) ---------------------------
__global__ __launch_bounds__(1024) void k_pp_finish(const double* __restrict__ Gp, const double* __restrict__ colsum, int k, double n_cells,
                                                    int center, double* __restrict__ mu, double* __restrict__ sd,
                                                    double* __restrict__ dinv, double* __restrict__ trace) {
    __shared__ double s_tr[1024];
    const int t = threadIdx.x;
    double tr = 0.0;
    for (int j = t; j < k; j += 1024) {
        const double m = center ? colsum[j] / n_cells : 0.0;
        mu[j] = m;
        sd[j] = 1.0;
        dinv[j] = 1.0;
        double ss = Gp[tri_index(j, j, k)] - n_cells * (m * m);
        if (ss < 0.0) ss = 0.0;
        tr += ss;
    }
    s_tr[t] = tr;
    __syncthreads();
    for (int half = 512; half > 0; half >>= 1) {
        if (t < half) s_tr[t] += s_tr[t + half];
        __syncthreads();
    }
    if (t == 0) {
        trace[0] = s_tr[0];
        trace[1] = 0.0;
    }
}

// ---- S_c = Z_c P - 1 c^T ---------------------------------------------------------------------------------------------------------------
// A workgroup owns 16 cells; wave (t, q) of its 16 the column tile t (16 of the panel's 64 columns; a tile at or behind n_r is
// skipped) against quarter q of the genes — a chunk has few rows (4096 at k = 2000), so the genes are what fills the device: 64
// cells per workgroup left three CUs in four idle (272 ms of score pass at 1.3 M x 2000 against 201 of Gram pass).  The sum
// over the genes may run in any order as long as both operands use the same one: lane (li, lk) reads the FOUR consecutive
// residuals Z[cell li][kk + 4 lk .. + 3] of a group of 16 genes in one 32-byte load, and K-step u of the group multiplies
// element u with P[kk + 4 lk + u][16 t + li].  Padded columns of Z are 0; a row of P at or behind k is not read.  The four
// quarters meet in LDS in accumulator-register order and are added in ascending order.
constexpr int kPpScoreWaves = 16;
__global__ __launch_bounds__(kPpScoreWaves * 64) void k_pp_scores(const double* __restrict__ Z, uint32_t ldz, uint32_t rows, uint32_t k,
                                                                 const double* __restrict__ P, const double* __restrict__ cvec, int n_r,
                                                                 double* __restrict__ out /* row 0 of the chunk, first column */, int ld) {
    __shared__ double red[kPpScoreWaves][4][64];          // [wave][accumulator register][lane]
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int li = lane & 15, lk = lane >> 4;
    const int t = wv & 3, q = wv >> 2;
    const uint32_t base = blockIdx.x * 16;
    const uint32_t row = base + li;
    const bool ok = row < rows;
    const bool active = 16 * t < n_r;                      // (wave-uniform)
    const uint32_t kper = ldz / 4;                         // ldz is a multiple of 64: whole groups of 16 genes
    const uint32_t kbeg = q * kper, kend = kbeg + kper;
    const double* zr = Z + (size_t)(ok ? row : 0) * ldz + 4 * lk;
    const double* pc = P + 16 * t + li;
    dvec4 acc = dvec4{0.0, 0.0, 0.0, 0.0};
    if (active) {
        for (uint32_t kk = kbeg; kk < kend; kk += 16) {
            const dvec4 av = ok ? *reinterpret_cast<const dvec4*>(zr + kk) : dvec4{0.0, 0.0, 0.0, 0.0};
            double b[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const uint32_t g = kk + 4 * lk + u;
                b[u] = g < k ? pc[(size_t)g * L] : 0.0;
            }
#pragma unroll
            for (int u = 0; u < 4; ++u) acc = __builtin_amdgcn_mfma_f64_16x16x4f64(av[u], b[u], acc, 0, 0, 0);
        }
    }
#pragma unroll
    for (int v = 0; v < 4; ++v) red[wv][v][lane] = acc[v];
    __syncthreads();
    if (q != 0 || !active) return;
    // C/D layout of the f64 MFMA: col = lane & 15, row = (lane >> 4) + 4 * reg
#pragma unroll
    for (int v = 0; v < 4; ++v) {
        const double s = ((red[t][v][lane] + red[4 + t][v][lane]) + red[8 + t][v][lane]) + red[12 + t][v][lane];
        const uint32_t r = base + lk + 4 * v;
        const int c = 16 * t + li;
        if (r < rows && c < n_r) out[(size_t)r * ld + c] = s - cvec[c];
    }
}

// ---- host side: the passes of dense_pca_internal.hpp ------------------------------------------------------------------------------------
int32_t dense_check_list(srx_ctx* ctx, const char* who, const uint64_t* genes, uint64_t k, uint64_t G) {
    if (k > (uint64_t)kPpMaxK) return fail(ctx, SRX_E_ARG, "%s: %llu listed genes (the k x k f64 Gram matrix is built up to k = %d)", who,
                                           (unsigned long long)k, kPpMaxK);
    std::vector<uint64_t> s(genes, genes + k);
    std::sort(s.begin(), s.end());
    for (uint64_t i = 0; i < k; ++i) {
        if (s[i] >= G) return fail(ctx, SRX_E_ARG, "%s: gene index %llu out of bounds (n_cols = %llu)", who, (unsigned long long)s[i],
                                   (unsigned long long)G);
        if (i && s[i] == s[i - 1]) return fail(ctx, SRX_E_ARG, "%s: gene index %llu appears twice", who, (unsigned long long)s[i]);
    }
    return SRX_OK;
}

int32_t dense_chunks_setup(srx_ctx* ctx, uint64_t n, uint64_t k64, uint64_t chunk_cells, DenseChunks& g) {
    g.n = n;
    g.k = (int)k64;
    g.ldz = (uint32_t)((k64 + kPpTile - 1) / kPpTile * kPpTile);
    // a chunk: what the last-level cache keeps between the kernel that makes it and the product that reads it, whole 64-row
    // groups; never more rows than a 32-bit row index and the fill kernel's grid hold
    const uint64_t row_bytes = (uint64_t)g.ldz * sizeof(double);
    uint64_t chunk = chunk_cells ? chunk_cells : std::max<uint64_t>(64, kPpChunkBytes / row_bytes / 64 * 64);
    chunk = std::min<uint64_t>(chunk, (1ull << 31) / g.ldz);
    chunk = std::max<uint64_t>(1, std::min<uint64_t>(chunk, at_least_one(n)));
    g.chunk = chunk;
    g.n_chunks = (n + chunk - 1) / chunk;
    SRX_TRY(scratch(ctx, "pp_chunk", chunk * row_bytes, (void**)&g.d_Z));
    return SRX_OK;
}

// Gp (packed upper triangle, slot order) and colsum over all chunks; both zeroed here
int32_t dense_gram_pass(srx_ctx* ctx, const DenseChunks& g, const DenseChunkFn& make, double* Gp, double* colsum, double* ms) {
    const int k = g.k, n_t = (int)(g.ldz / kPpTile), n_pairs = n_t * (n_t + 1) / 2;
    // slabs: enough workgroups for two per CU where the tile pairs alone are fewer, each slab whole groups of 64 rows
    const uint64_t groups = (g.chunk + 63) / 64;
    const int want = std::max(1, (2 * ctx->n_cus + n_pairs - 1) / n_pairs);
    const int n_slabs_max = (int)std::min<uint64_t>(std::min<uint64_t>(groups, (uint64_t)want), kPpMaxSlabs);
    const int cs_slabs_max = (int)std::min<uint64_t>(groups, kPpMaxSlabs);
    double *part = nullptr, *cs_part;
    SRX_TRY(scratch(ctx, "pp_part", (size_t)n_slabs_max * n_pairs * kPpTile * kPpTile * sizeof(double), (void**)&part));
    SRX_TRY(scratch(ctx, "pp_cs_part", (size_t)cs_slabs_max * at_least_one(k) * sizeof(double), (void**)&cs_part));
    StreamTimer timer(ctx, ctx->stream);
    SRX_TRY(timer.start());
    SRX_HIP(ctx, hipMemsetAsync(Gp, 0, gram_packed_count(k) * sizeof(double), ctx->stream));
    SRX_HIP(ctx, hipMemsetAsync(colsum, 0, (size_t)k * sizeof(double), ctx->stream));
    for (uint64_t row0 = 0; row0 < g.n; row0 += g.chunk) {
        const uint64_t rows = std::min(g.chunk, g.n - row0);
        SRX_TRY(make(row0, rows, g.d_Z));
        const uint64_t gr = (rows + 63) / 64;
        const uint32_t n_slabs = (uint32_t)std::min<uint64_t>(gr, (uint64_t)n_slabs_max);
        const uint32_t slab_rows = (uint32_t)((gr + n_slabs - 1) / n_slabs * 64);
        const uint32_t ns = (uint32_t)((rows + slab_rows - 1) / slab_rows);
        hipLaunchKernelGGL(k_pp_syrk, dim3((unsigned)n_pairs, ns), dim3(kPpThreads), 0, ctx->stream, (const double*)g.d_Z, g.ldz, (uint32_t)rows,
                           slab_rows, n_t, k, Gp, part);
        if (ns > 1)
            hipLaunchKernelGGL(k_pp_syrk_reduce, dim3((unsigned)n_pairs * 16), dim3(256), 0, ctx->stream, (const double*)part, n_pairs, (int)ns,
                               n_t, k, Gp);
        const uint32_t cs_n = (uint32_t)std::min<uint64_t>(gr, (uint64_t)cs_slabs_max);
        const uint32_t cs_rows = (uint32_t)((gr + cs_n - 1) / cs_n * 64);
        const uint32_t cs_ns = (uint32_t)((rows + cs_rows - 1) / cs_rows);
        hipLaunchKernelGGL(k_pp_colsum, dim3(grid256(k), cs_ns), dim3(256), 0, ctx->stream, (const double*)g.d_Z, g.ldz, (uint32_t)rows, cs_rows,
                           (uint32_t)k, cs_part);
        hipLaunchKernelGGL(k_pp_colsum_reduce, dim3(grid256(k)), dim3(256), 0, ctx->stream, (const double*)cs_part, cs_ns, (uint32_t)k, colsum);
        SRX_HIP(ctx, hipGetLastError());
    }
    SRX_TRY(timer.stop(ms));
    return SRX_OK;
}

int32_t dense_score_pass(srx_ctx* ctx, const DenseChunks& g, const DenseChunkFn& make, const double* P, const double* cvec, int n_r,
                         double* out, int ld, double* ms_acc) {
    StreamTimer timer(ctx, ctx->stream);
    SRX_TRY(timer.start());
    for (uint64_t row0 = 0; row0 < g.n; row0 += g.chunk) {
        const uint64_t rows = std::min(g.chunk, g.n - row0);
        SRX_TRY(make(row0, rows, g.d_Z));
        hipLaunchKernelGGL(k_pp_scores, dim3((unsigned)((rows + 15) / 16)), dim3(kPpScoreWaves * 64), 0, ctx->stream, (const double*)g.d_Z, g.ldz,
                           (uint32_t)rows, (uint32_t)g.k, P, cvec, n_r, out + row0 * (size_t)ld, ld);
        SRX_HIP(ctx, hipGetLastError());
    }
    double ms = 0.0;
    SRX_TRY(timer.stop(&ms));
    *ms_acc += ms;
    return SRX_OK;
}

int32_t dense_finish(srx_ctx* ctx, const double* Gp, const double* colsum, int k, uint64_t n, int center, const SelDev& sd) {
    hipLaunchKernelGGL(k_pp_finish, dim3(1), dim3(1024), 0, ctx->stream, Gp, colsum, k, (double)n, center, sd.d_mu, sd.d_sd, sd.d_dinv,
                       sd.d_trace);
    SRX_HIP(ctx, hipGetLastError());
    return SRX_OK;
}

// ---- host side: the Pearson calls ----------------------------------------------------------------------------------------------------------
namespace {

struct PpRun {                       // everything between the arguments and the two products
    PrPrep p;
    int k = 0;
    DenseChunks g;                   // the chunk geometry and the chunk buffer
    std::vector<uint32_t> sorted;    // the list in ascending gene order: slot s of the solver is gene sorted[s]
    std::vector<int> slot_of_pos;    // caller's position -> slot
    uint32_t* d_genes = nullptr;
    int32_t* d_slot_of = nullptr;
};

// `m` is a CSR handle.  The preparation of every Pearson call, the sums over the listed genes where asked, the list and its
// slot table on the device, the chunk size and the chunk buffer.
int32_t pp_setup(srx_mat* m, const uint64_t* genes, uint64_t k64, const srx_pearson_opts* popts, int totals, uint64_t chunk_cells,
                 const char* who, PpRun& R) {
    srx_ctx* ctx = m->ctx;
    SRX_TRY(pr_prepare(m, popts, who, R.p));
    const uint64_t n = R.p.n, G = R.p.G;
    R.k = (int)k64;
    std::vector<uint32_t> order(k64);
    std::iota(order.begin(), order.end(), 0u);
    std::sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) { return genes[a] < genes[b]; });
    R.sorted.resize(k64);
    R.slot_of_pos.resize(k64);
    std::vector<int32_t> slot_of(at_least_one(G), -1);
    for (uint64_t s = 0; s < k64; ++s) {
        R.sorted[s] = (uint32_t)genes[order[s]];
        R.slot_of_pos[order[s]] = (int)s;
        slot_of[genes[order[s]]] = (int32_t)s;
    }
    SRX_TRY(scratch(ctx, "pp_genes", at_least_one(k64) * sizeof(uint32_t), (void**)&R.d_genes));
    SRX_TRY(scratch(ctx, "pp_slot_of", at_least_one(G) * sizeof(int32_t), (void**)&R.d_slot_of));
    SRX_TRY(h2d(ctx, R.d_genes, R.sorted.data(), k64 * sizeof(uint32_t)));
    SRX_TRY(h2d(ctx, R.d_slot_of, slot_of.data(), at_least_one(G) * sizeof(int32_t)));
    if (totals == SRX_PEARSON_TOTALS_SELECTED) {
        double* d_rsel;
        SRX_TRY(scratch(ctx, "pp_rows_sel", at_least_one(n) * sizeof(double), (void**)&d_rsel));
        const unsigned grid = (unsigned)((at_least_one(n) + 3) / 4);
        if (is_f32(m))
            hipLaunchKernelGGL(k_pp_row_sums<float>, dim3(grid), dim3(256), 0, ctx->stream, m->d_indptr, m->d_indices, (const float*)m->d_values,
                               n, (const int32_t*)R.d_slot_of, d_rsel);
        else
            hipLaunchKernelGGL(k_pp_row_sums<double>, dim3(grid), dim3(256), 0, ctx->stream, m->d_indptr, m->d_indices, (const double*)m->d_values,
                               n, (const int32_t*)R.d_slot_of, d_rsel);
        SRX_HIP(ctx, hipGetLastError());
        R.p.d_cell = d_rsel;
        SRX_TRY(pr_totals(ctx, d_rsel, n, R.p.d_gene, G, &R.p.a.total, &R.p.n_empty));
    }
    SRX_TRY(dense_chunks_setup(ctx, n, k64, chunk_cells, R.g));
    return SRX_OK;
}

// rows [row0, row0 + rows) of Z into the chunk buffer
int32_t pp_make_chunk(srx_mat* m, const PpRun& R, uint64_t row0, uint64_t rows, double* Z) {
    srx_ctx* ctx = m->ctx;
    hipLaunchKernelGGL(k_pp_fill, dim3((unsigned)((rows * R.g.ldz + 255) / 256)), dim3(256), 0, ctx->stream, R.p.d_cell, R.p.d_gene,
                       (const uint32_t*)R.d_genes, (uint32_t)R.k, R.g.ldz, row0, rows, R.p.a, Z);
    const unsigned grid = (unsigned)((rows + 3) / 4);
    if (is_f32(m))
        hipLaunchKernelGGL(k_pp_stored<float>, dim3(grid), dim3(256), 0, ctx->stream, m->d_indptr, m->d_indices, (const float*)m->d_values,
                           R.p.d_cell, R.p.d_gene, (const int32_t*)R.d_slot_of, R.g.ldz, row0, rows, R.p.a, Z);
    else
        hipLaunchKernelGGL(k_pp_stored<double>, dim3(grid), dim3(256), 0, ctx->stream, m->d_indptr, m->d_indices, (const double*)m->d_values,
                           R.p.d_cell, R.p.d_gene, (const int32_t*)R.d_slot_of, R.g.ldz, row0, rows, R.p.a, Z);
    SRX_HIP(ctx, hipGetLastError());
    return SRX_OK;
}

void pp_info(const PpRun& R, srx_pearson_pca_info* info) {
    if (!info) return;
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

int32_t pp_gram_entry(srx_mat* m, const uint64_t* genes, uint64_t k, const srx_pearson_pca_opts* opts, double* gram_out, double* colsum_out,
                      srx_pearson_pca_info* info) {
    srx_ctx* ctx = m->ctx;
    SRX_HIP(ctx, hipSetDevice(ctx->device));
    if (m->csc) {                              // the chunks are made from the cells' rows: on the CSR of X (device transpose, csc.hip)
        srx_mat* t = nullptr;
        SRX_TRY(transpose_device(m, &t));
        const int32_t rc = pp_gram_entry(t, genes, k, opts, gram_out, colsum_out, info);
        srx_matrix_free(t);
        return rc;
    }
    PpRun R;
    SRX_TRY(pp_setup(m, genes, k, opts ? &opts->pearson : nullptr, opts ? opts->totals : 0, opts ? opts->chunk_cells : 0, "pearson_gram", R));
    const DenseChunkFn make = [&](uint64_t row0, uint64_t rows, double* Z) { return pp_make_chunk(m, R, row0, rows, Z); };
    srx_pearson_pca_info inf;
    pp_info(R, &inf);
    double *Gp, *colsum;
    SRX_TRY(scratch(ctx, "pp_gpacked", gram_packed_count((int)k) * sizeof(double), (void**)&Gp));
    SRX_TRY(scratch(ctx, "pp_colsum", k * sizeof(double), (void**)&colsum));
    SRX_TRY(dense_gram_pass(ctx, R.g, make, Gp, colsum, &inf.ms_gram));
    std::vector<double> hp(gram_packed_count((int)k)), hc(k);
    SRX_TRY(d2h(ctx, hp.data(), Gp, hp.size() * sizeof(double)));
    SRX_TRY(d2h(ctx, hc.data(), colsum, hc.size() * sizeof(double)));
    for (uint64_t a = 0; a < k; ++a) {        // the caller's order; (a, b) and (b, a) copy the same entry
        const int sa = R.slot_of_pos[a];
        if (colsum_out) colsum_out[a] = hc[sa];
        for (uint64_t b = 0; gram_out && b < k; ++b) {
            const int sb = R.slot_of_pos[b];
            gram_out[a * k + b] = hp[tri_index(std::min(sa, sb), std::max(sa, sb), (int)k)];
        }
    }
    if (info) *info = inf;
    return SRX_OK;
}

int32_t pp_pca(srx_mat* m, const uint64_t* genes, uint64_t k64, const srx_pearson_pca_opts* opts, srx_pearson_pca_info* info) {
    srx_ctx* ctx = m->ctx;
    SRX_HIP(ctx, hipSetDevice(ctx->device));
    if (m->csc) {
        srx_mat* t = nullptr;
        SRX_TRY(transpose_device(m, &t));
        const int32_t rc = pp_pca(t, genes, k64, opts, info);
        std::swap(m->pca, t->pca);
        srx_matrix_free(t);
        return rc;
    }
    srx_pca_state& st = m->pca;
    st.valid = false;
    const int k = (int)k64;
    // the solver's options: no scaling, the centring flag of this call
    srx_pca_opts po{};
    if (opts) po = opts->pca;
    else po.n_components = -1;
    po.scale = 0;
    po.center = (!opts || opts->center != 0) ? 1 : 0;
    Resolved o;
    int l_act = 0;
    SRX_TRY(resolve_opts(ctx, &po, k, m->n_rows, false, o, l_act));
    PpRun R;
    SRX_TRY(pp_setup(m, genes, k64, opts ? &opts->pearson : nullptr, opts ? opts->totals : 0, opts ? opts->chunk_cells : 0, "pca_pearson", R));
    const DenseChunkFn make = [&](uint64_t row0, uint64_t rows, double* Z) { return pp_make_chunk(m, R, row0, rows, Z); };
    srx_pearson_pca_info inf;
    pp_info(R, &inf);
    const uint64_t n = R.p.n;
    st.center = o.center;
    st.scale = 0;

    // the selection as the solver reads it: vectors in slot order, the list in the caller's order
    SelDev sd;
    double* d_f;
    double *Gp, *colsum;
    SRX_TRY(scratch(ctx, "pp_sel_f", (3 * (size_t)k + 8) * sizeof(double), (void**)&d_f));
    SRX_TRY(scratch(ctx, "pp_sel_rank", (size_t)k * sizeof(int32_t), (void**)&sd.d_sel_rank));
    SRX_TRY(scratch(ctx, "pp_status", 256, (void**)&sd.d_status));
    SRX_TRY(scratch(ctx, "pp_gpacked", gram_packed_count(k) * sizeof(double), (void**)&Gp));
    SRX_TRY(scratch(ctx, "pp_colsum", (size_t)k * sizeof(double), (void**)&colsum));
    sd.k = k;
    sd.d_mu = d_f;
    sd.d_sd = d_f + k;
    sd.d_dinv = d_f + 2 * (size_t)k;
    sd.d_trace = d_f + 3 * (size_t)k;
    std::vector<int32_t> list(k);
    for (int s = 0; s < k; ++s) list[s] = (int32_t)genes[s];
    SRX_TRY(h2d(ctx, sd.d_sel_rank, list.data(), (size_t)k * sizeof(int32_t)));
    SRX_HIP(ctx, hipMemsetAsync(sd.d_status, 0, 256, ctx->stream));

    SRX_TRY(dense_gram_pass(ctx, R.g, make, Gp, colsum, &inf.ms_gram));
    SRX_TRY(dense_finish(ctx, Gp, colsum, k, n, o.center, sd));

    double ms_scores = 0.0;
    DenseSource src;
    src.k = k;
    src.n_rows = n;
    src.write_scores = [&](const double* P, const double* cvec, int col0, int n_r, double* scores, int ld) -> int32_t {
        return dense_score_pass(ctx, R.g, make, P, cvec, n_r, scores + col0, ld, &ms_scores);
    };
    StreamTimer timer(ctx, ctx->stream);
    SRX_TRY(timer.start());
    const int32_t rc = solve_and_stash(ctx, false, nullptr, 0, nullptr, Gp, o, sd, l_act, n, 0, st, &src);
    double ms_all = 0.0;
    SRX_TRY(timer.stop(&ms_all));
    inf.ms_scores = ms_scores;
    inf.ms_solve = ms_all - ms_scores;
    inf.pca = st.info;
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
    return pp_gram_entry(m, genes, k, opts, gram_out, colsum_out, info);
}

int32_t srx_pca_pearson(srx_mat* m, const uint64_t* genes, uint64_t k, const srx_pearson_pca_opts* opts, double* scores, double* components,
                        double* evr, double* mean, srx_pearson_pca_info* info) {
    if (!m || !genes) return fail(m ? m->ctx : nullptr, SRX_E_ARG, "pca_pearson: null argument");
    srx_ctx* ctx = m->ctx;
    SRX_TRY(pp_check_common(m, genes, k, opts, "pca_pearson"));
    if (opts && opts->pca.scale > 0) return fail(ctx, SRX_E_ARG, "pca_pearson: pca.scale is set (the residuals are not scaled)");
    if (opts && opts->pca.solver == SRX_SOLVER_SPMM)
        return fail(ctx, SRX_E_ARG, "pca_pearson: the matrix-free solver walks sparse rows; the residuals are dense (solver 0 or 1)");
    const int32_t rc = pp_pca(m, genes, k, opts, info);
    if (rc != SRX_OK && rc != SRX_E_NOCONV) return rc;
    const int32_t rc2 = srx_result_fetch(m, scores, components, evr, mean, nullptr, nullptr);
    return rc2 != SRX_OK ? rc2 : rc;
}

}  // extern "C"
