// dense_pca.hip — the PCA of a dense n x k f64 matrix Z that is never held as a whole (dense_pca_internal.hpp): the route of
// pearson_pca.hip (the clipped Pearson residuals) and regress.hip (regressed, scaled and clipped values).
//
// A caller hands in what makes a CHUNK of cells of Z (dense_make_chunk with its element function).  A chunk is sized to stay in
// the last-level cache (kDenseChunkBytes), its row stride padded to whole 64-column tiles with zeros, and is read back by two
// products on the f64 matrix cores (v_mfma_f64_16x16x4, the operand layouts of iterate.inl):
//   Gram    G += Z_c^T Z_c, upper triangle in 64 x 64 tiles (k_dense_syrk), and the column sums of Z_c (k_dense_colsum);
//   scores  S_c = Z_c P - 1 c^T for the solver's k x 64 panel (k_dense_scores), written at the handle's score stride.
// Between the two the Gram solver of pca_solve.hip runs unchanged on C = G - n m m^T (DenseSource): plans A / B, deflation, the
// robust mode and the result block are shared with srx_pca.  The chunk is made twice, once for each product: keeping n x k
// doubles (20.8 GB at 1.3 M x 2000) is what this route exists to avoid.
// No floating-point atomics: a tile of G has one owner per launch, the launches of the chunks follow each other on the stream
// (ascending chunk order), and where a chunk is cut into slabs their partial tiles are added in ascending slab order.
#include "dense_pca_internal.hpp"

// the sums of this file are stated in one order
#pragma clang fp contract(off)

namespace srx {

typedef double dvec4 __attribute__((ext_vector_type(4)));

// kDenseTile: a tile of G, 64 x 64, four waves of 32 x 32 (2 x 2 MFMA tiles each)
constexpr int kDenseThreads = 256;
constexpr int kDenseKU = 4;                        // MFMA K-steps (of 4 cells) whose loads are in flight together
constexpr int kDenseMaxSlabs = 64;
constexpr uint64_t kDenseChunkBytes = 64ull << 20; // a chunk of Z: a quarter of the 256 MB last-level cache

// tile pair p of the upper triangle of n_t x n_t tiles, row-major: (ti, tj), ti <= tj
__device__ __forceinline__ void dense_pair(int p, int n_t, int& ti, int& tj) {
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
// and k_dense_syrk_reduce adds the slabs in ascending order.
__global__ __launch_bounds__(kDenseThreads) void k_dense_syrk(const double* __restrict__ Z, uint32_t ldz, uint32_t rows, uint32_t slab_rows,
                                                        int n_t, int k, double* __restrict__ Gp, double* __restrict__ part) {
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int li = lane & 15, lk = lane >> 4;
    const int wi = wv >> 1, wj = wv & 1;
    int ti, tj;
    dense_pair((int)blockIdx.x, n_t, ti, tj);
    const uint32_t r_beg = blockIdx.y * slab_rows;
    const uint32_t r_end = r_beg + slab_rows < rows ? r_beg + slab_rows : rows;
    const double* za = Z + (size_t)ti * kDenseTile + 32 * wi + li;
    const double* zb = Z + (size_t)tj * kDenseTile + 32 * wj + li;
    dvec4 acc[2][2];
#pragma unroll
    for (int s = 0; s < 2; ++s)
#pragma unroll
        for (int t = 0; t < 2; ++t) acc[s][t] = dvec4{0.0, 0.0, 0.0, 0.0};
    for (uint32_t r0 = r_beg; r0 < r_end; r0 += 4 * kDenseKU) {
        double a[kDenseKU][2], b[kDenseKU][2];
#pragma unroll
        for (int u = 0; u < kDenseKU; ++u) {
            const uint32_t r = r0 + 4 * u + lk;
            const bool ok = r < r_end;
            const size_t off = (size_t)(ok ? r : r_beg) * ldz;
            a[u][0] = ok ? za[off] : 0.0;
            a[u][1] = ok ? za[off + 16] : 0.0;
            b[u][0] = ok ? zb[off] : 0.0;
            b[u][1] = ok ? zb[off + 16] : 0.0;
        }
#pragma unroll
        for (int u = 0; u < kDenseKU; ++u)
#pragma unroll
            for (int s = 0; s < 2; ++s)
#pragma unroll
                for (int t = 0; t < 2; ++t) acc[s][t] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[u][s], b[u][t], acc[s][t], 0, 0, 0);
    }
    // C/D layout of the f64 MFMA: col = lane & 15, row = (lane >> 4) + 4 * reg
    const bool direct = gridDim.y == 1;
    double* const tile = part + ((size_t)blockIdx.y * gridDim.x + blockIdx.x) * (kDenseTile * kDenseTile);
#pragma unroll
    for (int s = 0; s < 2; ++s)
#pragma unroll
        for (int t = 0; t < 2; ++t)
#pragma unroll
            for (int v = 0; v < 4; ++v) {
                const int row = 32 * wi + 16 * s + lk + 4 * v, col = 32 * wj + 16 * t + li;
                if (direct) {
                    const int i = ti * kDenseTile + row, j = tj * kDenseTile + col;
                    if (i <= j && j < k) Gp[tri_index(i, j, k)] += acc[s][t][v];
                } else {
                    tile[row * kDenseTile + col] = acc[s][t][v];
                }
            }
}
__global__ __launch_bounds__(256) void k_dense_syrk_reduce(const double* __restrict__ part, int n_pairs, int n_slabs, int n_t, int k,
                                                        double* __restrict__ Gp) {
    const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x;          // 16 workgroups per tile: the pair is uniform in a workgroup
    const int p = (int)(e / (kDenseTile * kDenseTile)), w = (int)(e % (kDenseTile * kDenseTile));
    if (p >= n_pairs) return;
    int ti, tj;
    dense_pair(p, n_t, ti, tj);
    const int i = ti * kDenseTile + w / kDenseTile, j = tj * kDenseTile + w % kDenseTile;
    if (i > j || j >= k) return;
    double s = 0.0;
    for (int sl = 0; sl < n_slabs; ++sl) s += part[((size_t)sl * n_pairs + p) * (kDenseTile * kDenseTile) + w];
    Gp[tri_index(i, j, k)] += s;
}

// ---- column sums of a chunk: a thread per column and slab walks the rows in order; the slabs are added in ascending order ------------
__global__ __launch_bounds__(256) void k_dense_colsum(const double* __restrict__ Z, uint32_t ldz, uint32_t rows, uint32_t slab_rows, uint32_t k,
                                                   double* __restrict__ part) {
    const uint32_t c = blockIdx.x * 256 + threadIdx.x;
    if (c >= k) return;
    const uint32_t r_beg = blockIdx.y * slab_rows;
    const uint32_t r_end = r_beg + slab_rows < rows ? r_beg + slab_rows : rows;
    double s = 0.0;
    for (uint32_t r = r_beg; r < r_end; ++r) s += Z[(size_t)r * ldz + c];
    part[(size_t)blockIdx.y * k + c] = s;
}
__global__ __launch_bounds__(256) void k_dense_colsum_reduce(const double* __restrict__ part, uint32_t n_slabs, uint32_t k,
                                                          double* __restrict__ colsum) {
    const uint32_t c = blockIdx.x * 256 + threadIdx.x;
    if (c >= k) return;
    double s = 0.0;
    for (uint32_t sl = 0; sl < n_slabs; ++sl) s += part[(size_t)sl * k + c];
    colsum[c] += s;
}

// ---- the selection's vectors: m, sd = 1, trace(C) with C = G - cen n m m^T (one workgroup, one fixed order) ---------------------------
__global__ __launch_bounds__(1024) void k_dense_finish(const double* __restrict__ Gp, const double* __restrict__ colsum, int k, double n_cells,
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
constexpr int kDenseScoreWaves = 16;
__global__ __launch_bounds__(kDenseScoreWaves * 64) void k_dense_scores(const double* __restrict__ Z, uint32_t ldz, uint32_t rows, uint32_t k,
                                                                 const double* __restrict__ P, const double* __restrict__ cvec, int n_r,
                                                                 double* __restrict__ out /* row 0 of the chunk, first column */, int ld) {
    __shared__ double red[kDenseScoreWaves][4][64];          // [wave][accumulator register][lane]
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
    if (k > (uint64_t)kDenseMaxK) return fail(ctx, SRX_E_ARG, "%s: %llu listed genes (the k x k f64 Gram matrix is built up to k = %d)", who,
                                           (unsigned long long)k, kDenseMaxK);
    std::vector<uint64_t> s(genes, genes + k);
    std::sort(s.begin(), s.end());
    for (uint64_t i = 0; i < k; ++i) {
        if (s[i] >= G) return fail(ctx, SRX_E_ARG, "%s: gene index %llu out of bounds (n_cols = %llu)", who, (unsigned long long)s[i],
                                   (unsigned long long)G);
        if (i && s[i] == s[i - 1]) return fail(ctx, SRX_E_ARG, "%s: gene index %llu appears twice", who, (unsigned long long)s[i]);
    }
    return SRX_OK;
}

int32_t dense_slots_setup(srx_ctx* ctx, const uint64_t* genes, uint64_t k, uint64_t G, DenseSlots& s) {
    std::vector<uint32_t> order(k);
    std::iota(order.begin(), order.end(), 0u);
    std::sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) { return genes[a] < genes[b]; });
    s.k = (int)k;
    s.slot_of_pos.resize(k);
    std::vector<int32_t> slot_of(at_least_one(G), -1);
    for (uint64_t t = 0; t < k; ++t) {
        s.slot_of_pos[order[t]] = (int)t;
        slot_of[genes[order[t]]] = (int32_t)t;
    }
    SRX_TRY(scratch(ctx, "dense_slot_of", at_least_one(G) * sizeof(int32_t), (void**)&s.d_slot_of));
    return h2d(ctx, s.d_slot_of, slot_of.data(), at_least_one(G) * sizeof(int32_t));
}

int32_t dense_chunks_setup(srx_ctx* ctx, uint64_t n, uint64_t k64, uint64_t chunk_cells, DenseChunks& g) {
    g.n = n;
    g.k = (int)k64;
    g.ldz = (uint32_t)((k64 + kDenseTile - 1) / kDenseTile * kDenseTile);
    // a chunk: what the last-level cache keeps between the kernel that makes it and the product that reads it, whole 64-row
    // groups; never more rows than a 32-bit row index and the fill kernel's grid hold
    const uint64_t row_bytes = (uint64_t)g.ldz * sizeof(double);
    uint64_t chunk = chunk_cells ? chunk_cells : std::max<uint64_t>(64, kDenseChunkBytes / row_bytes / 64 * 64);
    chunk = std::min<uint64_t>(chunk, (1ull << 31) / g.ldz);
    chunk = std::max<uint64_t>(1, std::min<uint64_t>(chunk, at_least_one(n)));
    g.chunk = chunk;
    g.n_chunks = (n + chunk - 1) / chunk;
    SRX_TRY(scratch(ctx, "dense_chunk", chunk * row_bytes, (void**)&g.d_Z));
    return SRX_OK;
}

// Gp (packed upper triangle, slot order) and colsum over all chunks: the scratch buffers of every caller, zeroed here
int32_t dense_gram_pass(srx_ctx* ctx, const DenseChunks& g, const DenseChunkFn& make, double** Gp_out, double** colsum_out, double* ms) {
    const int k = g.k, n_t = (int)(g.ldz / kDenseTile), n_pairs = n_t * (n_t + 1) / 2;
    double *Gp, *colsum;
    SRX_TRY(scratch(ctx, "dense_gpacked", gram_packed_count(k) * sizeof(double), (void**)&Gp));
    SRX_TRY(scratch(ctx, "dense_colsum", (size_t)k * sizeof(double), (void**)&colsum));
    *Gp_out = Gp;
    *colsum_out = colsum;
    // slabs: enough workgroups for two per CU where the tile pairs alone are fewer, each slab whole groups of 64 rows
    const uint64_t groups = (g.chunk + 63) / 64;
    const int want = std::max(1, (2 * ctx->n_cus + n_pairs - 1) / n_pairs);
    const int n_slabs_max = (int)std::min<uint64_t>(std::min<uint64_t>(groups, (uint64_t)want), kDenseMaxSlabs);
    const int cs_slabs_max = (int)std::min<uint64_t>(groups, kDenseMaxSlabs);
    double *part = nullptr, *cs_part;
    SRX_TRY(scratch(ctx, "dense_part", (size_t)n_slabs_max * n_pairs * kDenseTile * kDenseTile * sizeof(double), (void**)&part));
    SRX_TRY(scratch(ctx, "dense_cs_part", (size_t)cs_slabs_max * at_least_one(k) * sizeof(double), (void**)&cs_part));
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
        hipLaunchKernelGGL(k_dense_syrk, dim3((unsigned)n_pairs, ns), dim3(kDenseThreads), 0, ctx->stream, (const double*)g.d_Z, g.ldz, (uint32_t)rows,
                           slab_rows, n_t, k, Gp, part);
        if (ns > 1)
            hipLaunchKernelGGL(k_dense_syrk_reduce, dim3((unsigned)n_pairs * 16), dim3(256), 0, ctx->stream, (const double*)part, n_pairs, (int)ns,
                               n_t, k, Gp);
        const uint32_t cs_n = (uint32_t)std::min<uint64_t>(gr, (uint64_t)cs_slabs_max);
        const uint32_t cs_rows = (uint32_t)((gr + cs_n - 1) / cs_n * 64);
        const uint32_t cs_ns = (uint32_t)((rows + cs_rows - 1) / cs_rows);
        hipLaunchKernelGGL(k_dense_colsum, dim3(grid256(k), cs_ns), dim3(256), 0, ctx->stream, (const double*)g.d_Z, g.ldz, (uint32_t)rows, cs_rows,
                           (uint32_t)k, cs_part);
        hipLaunchKernelGGL(k_dense_colsum_reduce, dim3(grid256(k)), dim3(256), 0, ctx->stream, (const double*)cs_part, cs_ns, (uint32_t)k, colsum);
        SRX_HIP(ctx, hipGetLastError());
    }
    SRX_TRY(timer.stop(ms));
    return SRX_OK;
}

int32_t dense_gram_fetch(srx_ctx* ctx, const DenseSlots& s, const double* Gp, const double* colsum, double* gram_out, double* colsum_out) {
    const int k = s.k;
    std::vector<double> hp(gram_packed_count(k)), hc(k);
    SRX_TRY(d2h(ctx, hp.data(), Gp, hp.size() * sizeof(double)));
    SRX_TRY(d2h(ctx, hc.data(), colsum, hc.size() * sizeof(double)));
    for (int a = 0; a < k; ++a) {             // the caller's order; (a, b) and (b, a) copy the same entry
        const int sa = s.slot_of_pos[a];
        if (colsum_out) colsum_out[a] = hc[sa];
        for (int b = 0; gram_out && b < k; ++b) {
            const int sb = s.slot_of_pos[b];
            gram_out[(size_t)a * k + b] = hp[tri_index(std::min(sa, sb), std::max(sa, sb), k)];
        }
    }
    return SRX_OK;
}

// columns [0, n_r) of S = Z P - 1 cvec^T, row i at out + i * ld; *ms_acc += the time of the pass
static int32_t dense_score_pass(srx_ctx* ctx, const DenseChunks& g, const DenseChunkFn& make, const double* P, const double* cvec, int n_r,
                         double* out, int ld, double* ms_acc) {
    StreamTimer timer(ctx, ctx->stream);
    SRX_TRY(timer.start());
    for (uint64_t row0 = 0; row0 < g.n; row0 += g.chunk) {
        const uint64_t rows = std::min(g.chunk, g.n - row0);
        SRX_TRY(make(row0, rows, g.d_Z));
        hipLaunchKernelGGL(k_dense_scores, dim3((unsigned)((rows + 15) / 16)), dim3(kDenseScoreWaves * 64), 0, ctx->stream, (const double*)g.d_Z, g.ldz,
                           (uint32_t)rows, (uint32_t)g.k, P, cvec, n_r, out + row0 * (size_t)ld, ld);
        SRX_HIP(ctx, hipGetLastError());
    }
    double ms = 0.0;
    SRX_TRY(timer.stop(&ms));
    *ms_acc += ms;
    return SRX_OK;
}

// the selection's vectors from the pass's results: mu = colsum / n (center) or 0, sd = dinv = 1, trace of G - n mu mu^T
static int32_t dense_finish(srx_ctx* ctx, const double* Gp, const double* colsum, int k, uint64_t n, int center, const SelDev& sd) {
    hipLaunchKernelGGL(k_dense_finish, dim3(1), dim3(1024), 0, ctx->stream, Gp, colsum, k, (double)n, center, sd.d_mu, sd.d_sd, sd.d_dinv,
                       sd.d_trace);
    SRX_HIP(ctx, hipGetLastError());
    return SRX_OK;
}

int32_t dense_pca_solve(srx_mat* m, const Resolved& o, int l_act, const uint64_t* genes, const DenseChunks& g, const DenseChunkFn& make_gram,
                        const DenseChunkFn& make_scores, int route, int center, const double* d_sd, DenseSolved& out) {
    srx_ctx* ctx = m->ctx;
    srx_pca_state& st = m->pca;
    const int k = g.k;
    st.center = center;
    st.scale = 0;
    // the selection as the solver reads it: vectors in slot order, the list in the caller's order
    SelDev sd;
    double* d_f;
    SRX_TRY(scratch(ctx, "dense_sel_f", (3 * (size_t)k + 8) * sizeof(double), (void**)&d_f));
    SRX_TRY(scratch(ctx, "dense_sel_rank", (size_t)k * sizeof(int32_t), (void**)&sd.d_sel_rank));
    SRX_TRY(scratch(ctx, "dense_status", 256, (void**)&sd.d_status));
    sd.k = k;
    sd.d_mu = d_f;
    sd.d_sd = d_f + k;
    sd.d_dinv = d_f + 2 * (size_t)k;
    sd.d_trace = d_f + 3 * (size_t)k;
    std::vector<int32_t> list(k);
    for (int s = 0; s < k; ++s) list[s] = (int32_t)genes[s];
    SRX_TRY(h2d(ctx, sd.d_sel_rank, list.data(), (size_t)k * sizeof(int32_t)));
    SRX_HIP(ctx, hipMemsetAsync(sd.d_status, 0, 256, ctx->stream));

    double *Gp, *colsum;
    SRX_TRY(dense_gram_pass(ctx, g, make_gram, &Gp, &colsum, &out.ms_gram));
    SRX_TRY(dense_finish(ctx, Gp, colsum, k, g.n, center, sd));
    // a Z that is scaled where it is made: the solver's factor stays 1, the result block's std is the caller's
    if (d_sd) SRX_HIP(ctx, hipMemcpyAsync(sd.d_sd, d_sd, (size_t)k * sizeof(double), hipMemcpyDeviceToDevice, ctx->stream));

    DenseSource src;
    src.k = k;
    src.n_rows = g.n;
    src.route = route;
    src.write_scores = [&](const double* P, const double* cvec, int col0, int n_r, double* scores, int ld) -> int32_t {
        return dense_score_pass(ctx, g, make_scores, P, cvec, n_r, scores + col0, ld, &out.ms_scores);
    };
    StreamTimer timer(ctx, ctx->stream);
    SRX_TRY(timer.start());
    const int32_t rc = solve_and_stash(ctx, false, nullptr, 0, nullptr, Gp, o, sd, l_act, g.n, 0, st, &src);
    double ms_all = 0.0;
    SRX_TRY(timer.stop(&ms_all));
    out.ms_solve = ms_all - out.ms_scores;
    out.pca = st.info;
    out.solved = true;
    return rc;
}

}  // namespace srx
